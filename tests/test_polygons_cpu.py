"""CPU (-m "not gpu"): the restatement of the region outlines against its own invariants, the family header against
`_ext.EXT_SIGNATURES`, the argument checks, the GeoJSON and the flags of the evaluation scripts.  No compute entry point runs."""
import ctypes as C
import json
import os
import sys
import types

import numpy as np
import pytest

import polygons_ref as PR
import regions_ref
from test_binding_cpu import parse_header, signature_errors
from visiontransformer_amd import _ext, _lib, polygons, scripts
from visiontransformer_amd.predict import predict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vitseg_polygons.h")
NAMES = ["vitseg_polygons_version", "vitseg_region_polygons_scratch_bytes", "vitseg_region_polygons"]


# ---- the restatement ----

def _holes(region, connectivity):
    """Components of the complement that are off the region's outside, under the dual connectivity (scipy)."""
    from scipy import ndimage
    comp = np.pad(~region, 1, constant_values=True)
    dual = np.ones((3, 3), bool) if connectivity == 4 else None
    lab, k = ndimage.label(comp, structure=dual)
    return k - 1   # the padding joins everything outside into one component


@pytest.mark.parametrize("connectivity", [4, 8])
def test_restatement_keeps_its_invariants_on_random_masks(connectivity):
    rs = np.random.RandomState(40 + connectivity)
    checked = 0
    for it in range(150):
        H, W = int(rs.randint(1, 14)), int(rs.randint(1, 14))
        m = ((rs.rand(H, W) < rs.choice([0.3, 0.5, 0.7])) * rs.randint(1, 4, size=(H, W))).astype(np.uint8)
        rec, polys, rings, vertices, lab = PR.region_polygons_ref(m, 0 if it % 2 else -1, connectivity)
        assert len(polys) == len(rec) and int(rings[:, 2].sum()) == len(vertices)
        assert np.array_equal(rings[:, 1], np.cumsum(rings[:, 2]) - rings[:, 2])
        starts = [tuple(vertices[o]) for o in rings[:, 1]]
        assert starts == sorted(starts)   # ring order: the raster order of the start edges
        for i, (r, rg) in enumerate(zip(rec, polys)):
            region = lab == i
            areas = [PR.ring_area(g) for g in rg]
            assert areas[0] > 0 and all(a < 0 for a in areas[1:])   # one outer ring, first; the others are holes
            assert tuple(rg[0][0]) == divmod(int(r[6]), W)   # it starts at the first pixel's corner ...
            assert rg[0][1][0] == rg[0][0][0] and rg[0][1][1] > rg[0][0][1]   # ... going E
            assert len(rg) == 1 + _holes(region, connectivity)
            assert sum(areas) == int(r[5]) == int(region.sum())
            p = np.pad(region, 1)
            sides = sum(int((p[1:-1, 1:-1] & ~np.roll(p, s, axis=a)[1:-1, 1:-1]).sum()) for s in (1, -1) for a in (0, 1))
            assert sum(PR.ring_length(g) for g in rg) == sides
            assert np.array_equal(PR.rasterize(rg, H, W), region)
            for g in rg:   # collinear corners are dropped: consecutive sides alternate between rows and columns
                d = np.roll(g, -1, axis=0) - g
                assert np.all((d[:, 0] == 0) != (d[:, 1] == 0)) and np.all((d[:, 0] == 0) != (np.roll(d, -1, axis=0)[:, 0] == 0))
            checked += 1
    assert checked > 300


def test_restatement_on_the_saddle():
    m = np.array([[1, 0], [0, 1]], np.uint8)
    rec4, polys4, *_ = PR.region_polygons_ref(m, 0, 4)
    assert len(rec4) == 2 and [len(p[0]) for p in polys4] == [4, 4]
    rec8, polys8, *_ = PR.region_polygons_ref(m, 0, 8)
    assert len(rec8) == 1 and len(polys8[0]) == 1
    assert polys8[0][0].tolist() == [[0, 0], [0, 1], [1, 1], [1, 2], [2, 2], [2, 1], [1, 1], [1, 0]]   # (1, 1) twice
    assert PR.ring_area(polys8[0][0]) == 2 and polygons.ring_area(polys8[0][0]) == 2 and polygons.ring_length(polys8[0][0]) == 8


# ---- the family header and its table ----

def _table(signatures=None):
    return {name: (restype, list(argtypes)) for name, restype, argtypes in (signatures or _ext.EXT_SIGNATURES)["polygons"][2]}


def test_family_header_is_the_table_both_ways():
    decls, structs, enums, defines = parse_header(open(HEADER).read())
    assert list(_ext.EXT_SIGNATURES) == ["polygons"] and _ext.EXT_SIGNATURES["polygons"][:2] == ("vitseg_polygons.h", "the region outlines")
    assert sorted(decls) == sorted(NAMES) == sorted(_table()) and not structs and not enums
    assert signature_errors(decls, _table()) == []
    assert decls["vitseg_region_polygons"][1][12] == ("int64_t", 0) and len(decls["vitseg_region_polygons"][1]) == 17
    assert defines == {"VITSEG_POLYGONS_VERSION": 100}
    # the comparison can fail
    tab = _table()
    tab["vitseg_region_polygons"] = (C.c_int, tab["vitseg_region_polygons"][1][:12] + [C.c_int] + tab["vitseg_region_polygons"][1][13:])
    assert signature_errors(decls, tab) == ["vitseg_region_polygons: argument 12: c_int for int64_t"]
    tab = _table()
    tab["vitseg_region_polygons_scratch_bytes"] = (C.c_int, tab["vitseg_region_polygons_scratch_bytes"][1])
    assert signature_errors(decls, tab) == ["vitseg_region_polygons_scratch_bytes: restype c_int, the header returns size_t"]
    tab = _table()
    del tab["vitseg_polygons_version"]
    assert signature_errors(decls, tab) == ["vitseg_polygons_version: declared in the header, no row in the table"]
    assert signature_errors(decls, {**_table(), "vitseg_ring_simplify": (C.c_int, [])}) == [
        "vitseg_ring_simplify: a row in the table, not declared in the header"]


def test_family_stays_beside_the_frozen_header():
    assert not set(NAMES) & set(_lib.EXPORTS)
    assert all(n not in name for n in ("polygon",) for name in _lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "vitseg.h")).read()
    assert "polygon" not in hdr.lower()
    assert '#include "vitseg.h"' in open(HEADER).read()


def test_library_exports_the_family_at_its_version():
    l = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(l, name), name
    _, _, _, defines = parse_header(open(HEADER).read())
    assert defines["VITSEG_POLYGONS_VERSION"] == _ext.POLYGONS_VERSION == _ext.ext_symbol("polygons", "vitseg_polygons_version")() == 100
    fn = _ext.ext_symbol("polygons", "vitseg_region_polygons")
    assert fn.restype is C.c_int and list(fn.argtypes) == _table()["vitseg_region_polygons"][1]
    assert _ext.ext_symbol("polygons", "vitseg_region_polygons") is fn
    assert _ext.ext_symbol("polygons", "vitseg_region_polygons_scratch_bytes").restype is C.c_size_t


def test_ext_symbol_names_the_rebuild_for_a_missing_name(monkeypatch):
    msg = r"has no vitseg_ring_simplify \(built before the region outlines\): rebuild it \(python -m visiontransformer_amd\.build\)"
    with pytest.raises(RuntimeError, match=msg):
        _ext.ext_symbol("polygons", "vitseg_ring_simplify")

    class Old:   # a library built before the region outlines
        def __getattr__(self, name):
            if "polygons" in name:
                raise AttributeError(name)
            return getattr(_lib._lib, name)
    _lib.lib()
    monkeypatch.setattr(_lib, "lib", Old)
    with pytest.raises(RuntimeError, match=r"has no vitseg_region_polygons \(built before the region outlines\): rebuild it"):
        _ext.ext_symbol("polygons", "vitseg_region_polygons")


def test_every_status_code_without_a_device():
    """The argument checks come before any launch: every address is a live host buffer that no call reaches."""
    fn = _ext.ext_symbol("polygons", "vitseg_region_polygons")
    size = _ext.ext_symbol("polygons", "vitseg_region_polygons_scratch_bytes")
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    need = size(1, 8, 8)
    assert need > 0 and size(2, 8, 8) > need
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (65536, 8, 8), (1, 16385, 1), (1, 1, 16385), (1, 16384, 32768), (1, 32768, 16384)):
        assert size(*bad) == 0, bad

    def call(mask=p, n=1, H=8, W=8, conn=4, bg=0, rc=p, gc=p, vc=p, rings=p, max_rings=4, verts=p, max_verts=16, labels=None,
             scratch=p, nbytes=need):
        return fn(mask, n, H, W, conn, bg, rc, gc, vc, rings, max_rings, verts, max_verts, labels, scratch, nbytes, None)
    for kw in (dict(mask=None), dict(rc=None), dict(gc=None), dict(vc=None), dict(scratch=None), dict(rings=None),
               dict(verts=None), dict(max_rings=-1), dict(max_verts=-1), dict(conn=6), dict(bg=-2), dict(bg=256)):
        assert call(**kw) == _lib.EINVAL, kw
        assert b"region_polygons" in _lib.lib().vitseg_last_error()
    for kw in (dict(n=0), dict(H=0), dict(W=-3), dict(n=65536), dict(H=16385, W=1), dict(H=1, W=16385), dict(H=16384, W=32768)):
        assert call(**kw) == _lib.ESHAPE, kw
        with pytest.raises(ValueError, match="region_polygons: bad shape"):
            _lib.check(_lib.ESHAPE)
    assert call(nbytes=need - 1) == _lib.EWORKSPACE
    assert bytes(buf) == bytes(4096)   # nothing was written


# ---- the Python surface ----

def test_region_polygons_and_predict_reject_bad_arguments_before_the_library(monkeypatch):
    def no_call(*a, **k):
        raise AssertionError(f"{a} requested")
    monkeypatch.setattr(_ext, "ext_symbol", no_call)
    monkeypatch.setattr(_lib, "symbol", no_call)
    ok = np.zeros((4, 4), np.uint8)
    for mask, kw in ((ok, dict(connectivity=6)), (ok, dict(background=256)), (ok, dict(background=True)), (ok.astype(np.float32), {}),
                     (np.zeros((2, 2, 2, 2), np.uint8), {}), (np.zeros((0, 4), np.uint8), {}), ("mask", {}),
                     (np.full((2, 2), 300, np.int64), {}), (np.zeros((1, 16385), np.uint8), {}), (np.zeros((16385, 1), np.uint8), {})):
        with pytest.raises(ValueError):
            polygons.region_polygons(mask, **kw)

    def boom(*a, **k):
        raise AssertionError("the model was reached")
    model = types.SimpleNamespace(cfg=types.SimpleNamespace(image_size=224), arena=None, predict_mask=boom,
                                  predict_mask_windowed=boom, predict_mask_tta=boom, _lowres_and_mask=boom)
    img = np.zeros((300, 300, 3), np.uint8)
    for kw in (dict(min_area=-1), dict(max_hole_area=-2), dict(tta="hflip", sliding=True), dict(return_scores=True, sliding=True)):
        with pytest.raises(ValueError):
            predict(img, model, return_polygons=True, **kw)


def test_geojson_of_a_ring_with_a_hole():
    outer = np.array([[0, 0], [0, 3], [3, 3], [3, 0]], np.int32)
    hole = np.array([[1, 1], [2, 1], [2, 2], [1, 2]], np.int32)
    assert polygons.ring_area(outer) == 9 and polygons.ring_area(hole) == -1
    assert polygons.ring_length(outer) == 12 and polygons.ring_length(hole) == 4
    assert np.array_equal(PR.rasterize([outer, hole], 3, 3), np.array([[1, 1, 1], [1, 0, 1], [1, 1, 1]], bool))
    rec = np.array([[2, 0, 0, 2, 2, 8, 0]], np.int32)
    g = polygons.polygons_to_geojson(rec, [[outer, hole]], pixel_size=0.5, image_id="a/0", class_names=["bg", "x", "crack"])
    assert g["type"] == "FeatureCollection" and len(g["features"]) == 1
    f = g["features"][0]
    assert f["type"] == "Feature" and f["geometry"]["type"] == "Polygon"
    assert f["geometry"]["coordinates"] == [[[0.0, 0.0], [1.5, 0.0], [1.5, 1.5], [0.0, 1.5], [0.0, 0.0]],
                                            [[0.5, 0.5], [0.5, 1.0], [1.0, 1.0], [1.0, 0.5], [0.5, 0.5]]]   # [x, y], closed
    assert f["properties"] == {"class": 2, "first": 0, "area": 2.0, "holes": 1, "image_id": "a/0", "class_name": "crack"}
    assert json.loads(json.dumps(g)) == g
    plain = polygons.polygons_to_geojson(rec, [[outer, hole]])
    assert set(plain["features"][0]["properties"]) == {"class", "first", "area", "holes", "image_id"}
    assert plain["features"][0]["properties"]["image_id"] is None and plain["features"][0]["geometry"]["coordinates"][0][1] == [3.0, 0.0]
    assert polygons.polygons_to_geojson(np.zeros((0, 7), np.int32), []) == {"type": "FeatureCollection", "features": []}
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            polygons.polygons_to_geojson(rec, [[outer, hole]], pixel_size=bad)
    with pytest.raises(ValueError):
        polygons.polygons_to_geojson(rec, [])


def _load_script(rel):
    """model/<dir>/<script>.py as a module; its `from classes import ...` resolves in its own directory."""
    import importlib.util
    path = os.path.join(ROOT, *rel.split("/"))
    sys.path.insert(0, os.path.dirname(path))
    kept = sys.modules.pop("classes", None)
    try:
        spec = importlib.util.spec_from_file_location("polygons_script_" + os.path.basename(path)[:-3], path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.dirname(path))
        sys.modules.pop("classes", None)
        if kept is not None:
            sys.modules["classes"] = kept
    return mod


@pytest.mark.parametrize("rel,trainer,batches", [("model/CE/datasetTestViTmodel.py", "LightningViTModel", "ce_batches"),
                                                ("model/PAED/ViTscriptTest.py", "PAEDTrainer", "paed_binary_batches")])
def test_evaluation_scripts_pass_the_flag_on(rel, trainer, batches, monkeypatch, tmp_path):
    mod = _load_script(rel)
    seen = []
    monkeypatch.setattr(mod, trainer, lambda *a, **k: types.SimpleNamespace(model=types.SimpleNamespace(cfg=None)))
    monkeypatch.setattr(scripts, "get_latest_checkpoint", lambda *a: None)
    monkeypatch.setattr(scripts, batches, lambda *a, **k: [])
    monkeypatch.setattr(scripts, "evaluate_to_csv", lambda *a, **k: seen.append((a, k)) or [[0.0] * 12])
    monkeypatch.chdir(tmp_path)
    base = [rel, "--ids", "1", "--num-batches", "1"]
    for extra in ([], ["--region-polygons"], ["--region-polygons", "--pixel-size", "0.25", "--region-connectivity", "8", "--min-area", "9"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        mod.main()
    assert "polygons_path" not in seen[0][1]   # without the flag nothing new is asked for
    for a, k in seen[1:]:
        assert a[3].endswith("_metrics.csv")
        assert k["polygons_path"] == a[3][:-len("_metrics.csv")] + "_region_polygons.geojson"
        assert os.path.dirname(k["polygons_path"]) == os.path.dirname(a[3])
    assert (seen[2][1]["props_pixel_size"], seen[2][1]["region_connectivity"], seen[2][1]["min_area"]) == (0.25, 8, 9)
