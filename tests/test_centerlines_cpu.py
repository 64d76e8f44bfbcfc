"""CPU (-m "not gpu"): the restatement of the crack centre-lines against literal results and its own identities, the family
header against `_ext.EXT_FAMILIES`, the argument checks, the host arithmetic, the GeoJSON and the flags of the evaluation
scripts.  No compute entry point runs."""
import ctypes as C
import json
import math
import os
import sys
import types

import numpy as np
import pytest

import centerlines_ref as CR
from test_binding_cpu import parse_header, signature_errors
from test_polygons_cpu import _load_script
from visiontransformer_amd import _ext, _lib, centerlines, scripts
from visiontransformer_amd.metrics import Evaluator
from visiontransformer_amd.predict import predict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vitseg_centerlines.h")
NAMES = ["vitseg_centerlines_version", "vitseg_centerlines_scratch_bytes", "vitseg_centerlines"]


# ---- the restatement ----

def _graph(name):
    nodes, branches, points = CR.trace_ref(CR.HAND[name])
    return nodes[:, :3].tolist(), branches[:, :7].tolist(), points[:, :2].tolist()


def test_restatement_on_hand_planes():
    """(y, x, degree) of the nodes; (start, end, offset, points, kind, orthogonal, diagonal) of the branches; (y, x)."""
    assert _graph("single") == ([[1, 1, 0]], [], [])
    assert _graph("line_1x7") == ([[0, 0, 1], [0, 6, 1]], [[0, 6, 0, 7, 0, 6, 0]], [[0, x] for x in range(7)])
    # an L corner is a path of two links, not a triangle: no junction, and no link between its two ends
    assert _graph("corner") == ([[0, 0, 1], [1, 1, 1]], [[0, 3, 0, 3, 0, 2, 0]], [[0, 0], [1, 0], [1, 1]])
    assert _graph("diagonal") == ([[0, 0, 1], [3, 3, 1]], [[0, 15, 0, 4, 0, 0, 3]], [[0, 0], [1, 1], [2, 2], [3, 3]])
    nodes, branches, points = _graph("tee")
    assert nodes == [[0, 0, 1], [0, 2, 3], [0, 4, 1], [2, 2, 1]]
    assert branches == [[0, 2, 0, 3, 0, 2, 0], [2, 4, 3, 3, 0, 2, 0], [2, 12, 6, 3, 0, 2, 0]]
    assert points == [[0, 0], [0, 1], [0, 2], [0, 2], [0, 3], [0, 4], [0, 2], [1, 2], [2, 2]]
    nodes, branches, points = _graph("plus")
    assert [2, 2, 4] in nodes and sorted(n[2] for n in nodes) == [1, 1, 1, 1, 4]
    assert branches == [[2, 12, 0, 3, 0, 2, 0], [10, 12, 3, 3, 0, 2, 0], [12, 14, 6, 3, 0, 2, 0], [12, 22, 9, 3, 0, 2, 0]]
    # a ring without a node: one closed branch from its smallest pixel toward the smaller neighbour, the start not repeated
    nodes, branches, points = _graph("ring_4x4")
    assert nodes == [] and branches == [[0, 0, 0, 12, 1, 12, 0]]
    assert points == [[0, 0], [0, 1], [0, 2], [0, 3], [1, 3], [2, 3], [3, 3], [3, 2], [3, 1], [3, 0], [2, 0], [1, 0]]
    # ring plus tail: a loop at the junction (p0 = pk), walked toward the smaller of its two ring neighbours
    nodes, branches, points = _graph("lollipop")
    assert nodes == [[2, 3, 3], [2, 6, 1]]
    assert branches == [[17, 17, 0, 9, 0, 8, 0], [17, 20, 9, 4, 0, 3, 0]]
    assert points[:9] == [[2, 3], [1, 3], [0, 3], [0, 2], [0, 1], [1, 1], [2, 1], [2, 2], [2, 3]]
    # two branches between the same two junctions: both reported, ordered by their second pixels
    nodes, branches, points = _graph("parallel")
    assert nodes == [[2, 0, 1], [2, 2, 3], [2, 4, 3], [2, 6, 1]]
    assert branches == [[14, 16, 0, 3, 0, 2, 0], [16, 18, 3, 7, 0, 6, 0], [16, 18, 10, 7, 0, 6, 0], [18, 20, 17, 3, 0, 2, 0]]
    assert points[4] == [1, 2] and points[11] == [3, 2]


def test_restatement_widths_and_the_degree_one_note():
    nodes, branches, points = CR.trace_ref(CR.HAND["line_1x7"])
    # the line fills its image: d2 is measured to the virtual pixel at (-1, 0)
    assert points[:, 2].tolist() == [1 + x * x for x in range(7)] and nodes[:, 3].tolist() == [1, 37]
    assert branches[0, 7] == sum(CR.q16(1 + x * x) for x in range(7)) and branches[0, 8] == 37 and CR.q16(4) == 131072
    # the pixel (1, 1) has the neighbours N and NE: two 8-neighbours, one link -- an end point here, not one of
    # vitseg_skeleton_stats' "exactly one set 8-neighbour" end points, of which this plane has none
    import skeleton_ref as SR
    m = CR.plane([".##", ".#."])
    nodes, branches, _ = CR.trace_ref(m)
    assert nodes[:, :3].tolist() == [[0, 2, 1], [1, 1, 1]] and SR.end_points(m) == 0 and branches[0, 3:7].tolist() == [3, 0, 2, 0]


def _identities(m):
    S = np.asarray(m) != 0
    nodes, branches, points = CR.trace_ref(m)
    links = CR.links_of(S)
    open_, closed = branches[branches[:, 4] == 0], branches[branches[:, 4] == 1]
    assert int(S.sum()) == len(nodes) + int((open_[:, 3] - 2).sum()) + int(closed[:, 3].sum())
    assert 2 * len(open_) == int(nodes[:, 2].sum())
    assert 2 * int((branches[:, 5] + branches[:, 6]).sum()) == sum(len(v) for v in links.values())
    covered = CR.rasterize(points, *S.shape)
    covered[nodes[:, 0], nodes[:, 1]] = True   # isolated pixels are on no branch
    assert np.array_equal(covered, S)
    assert np.array_equal(branches[:, 2], np.cumsum(branches[:, 3]) - branches[:, 3]) and int(branches[:, 3].sum()) == len(points)
    assert all(len(v) <= 4 for v in links.values())
    assert all((q in links and p in links[q]) for p, v in links.items() for q in v)   # the rule is symmetric
    keys = [(int(b[0]), int(points[b[2] + 1, 0]) * S.shape[1] + int(points[b[2] + 1, 1])) for b in branches]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    return len(branches)


def test_restatement_keeps_its_identities():
    total = sum(_identities(m) for m in CR.HAND.values())
    rs = np.random.RandomState(7)
    for it in range(120):
        H, W = int(rs.randint(1, 16)), int(rs.randint(1, 16))
        total += _identities((rs.rand(H, W) < rs.choice([0.2, 0.4, 0.6, 0.9])).astype(np.uint8))
    total += _identities(CR.nested_rings(16)) + _identities(CR.serpentine(16))
    assert total > 1000


# ---- the family header and its table ----

def _table():
    return {name: (restype, list(argtypes)) for name, restype, argtypes in _ext.EXT_FAMILIES["centerlines"][2]}


def test_family_header_is_the_table_both_ways():
    decls, structs, enums, defines = parse_header(open(HEADER).read())
    assert list(_ext.EXT_FAMILIES) == ["centerlines"]
    assert _ext.EXT_FAMILIES["centerlines"][:2] == ("vitseg_centerlines.h", "the crack centre-lines")
    assert sorted(decls) == sorted(NAMES) == sorted(_table()) and not structs and not enums
    assert signature_errors(decls, _table()) == []
    assert decls["vitseg_centerlines"][1][15] == ("int64_t", 0) and len(decls["vitseg_centerlines"][1]) == 19
    assert defines == {"VITSEG_CENTERLINES_VERSION": 100}
    # the comparison can fail
    tab = _table()
    tab["vitseg_centerlines"] = (C.c_int, tab["vitseg_centerlines"][1][:15] + [C.c_int] + tab["vitseg_centerlines"][1][16:])
    assert signature_errors(decls, tab) == ["vitseg_centerlines: argument 15: c_int for int64_t"]
    tab = _table()
    tab["vitseg_centerlines_scratch_bytes"] = (C.c_int, tab["vitseg_centerlines_scratch_bytes"][1])
    assert signature_errors(decls, tab) == ["vitseg_centerlines_scratch_bytes: restype c_int, the header returns size_t"]
    tab = _table()
    del tab["vitseg_centerlines_version"]
    assert signature_errors(decls, tab) == ["vitseg_centerlines_version: declared in the header, no row in the table"]
    assert signature_errors(decls, {**_table(), "vitseg_centerlines_prune": (C.c_int, [])}) == [
        "vitseg_centerlines_prune: a row in the table, not declared in the header"]


def test_family_stays_beside_the_frozen_tables():
    assert not set(NAMES) & set(_lib.EXPORTS) and "centerlines" not in _ext.EXT_SIGNATURES
    assert all("centerline" not in name for name in _lib.EXPORTS)
    assert "centerline" not in open(os.path.join(ROOT, "include", "vitseg.h")).read().lower()
    assert '#include "vitseg.h"' in open(HEADER).read()
    assert _ext.EXT_VERSIONS["centerlines"] == ("vitseg_centerlines_version", 100)


def test_library_exports_the_family_at_its_version():
    l = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(l, name), name
    _, _, _, defines = parse_header(open(HEADER).read())
    assert defines["VITSEG_CENTERLINES_VERSION"] == _ext.CENTERLINES_VERSION == 100
    assert _ext.ext_symbol("centerlines", "vitseg_centerlines_version")() == 100
    fn = _ext.ext_symbol("centerlines", "vitseg_centerlines")
    assert fn.restype is C.c_int and list(fn.argtypes) == _table()["vitseg_centerlines"][1]
    assert _ext.ext_symbol("centerlines", "vitseg_centerlines") is fn
    assert _ext.ext_symbol("centerlines", "vitseg_centerlines_scratch_bytes").restype is C.c_size_t
    assert _ext.ext_symbol("polygons", "vitseg_polygons_version")() == 100   # the first dict is still consulted


def test_ext_symbol_names_the_rebuild_for_a_missing_name(monkeypatch):
    msg = r"has no vitseg_centerlines_prune \(built before the crack centre-lines\): rebuild it \(python -m visiontransformer_amd\.build\)"
    with pytest.raises(RuntimeError, match=msg):
        _ext.ext_symbol("centerlines", "vitseg_centerlines_prune")

    class Old:   # a library built before the crack centre-lines
        def __getattr__(self, name):
            if "centerlines" in name:
                raise AttributeError(name)
            return getattr(_lib._lib, name)
    _lib.lib()
    monkeypatch.setattr(_lib, "lib", Old)
    with pytest.raises(RuntimeError, match=r"has no vitseg_centerlines \(built before the crack centre-lines\): rebuild it"):
        _ext.ext_symbol("centerlines", "vitseg_centerlines")


def test_every_status_code_without_a_device():
    """The argument checks come before any launch: every address is a live host buffer that no call reaches.  Route 2 (and
    route 0 where no device answers) needs no device to size its scratch."""
    fn = _ext.ext_symbol("centerlines", "vitseg_centerlines")
    size = _ext.ext_symbol("centerlines", "vitseg_centerlines_scratch_bytes")
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    need = size(1, 8, 8, 2)
    assert need > 0 and size(2, 8, 8, 2) > need
    for bad in ((0, 8, 8, 2), (1, 0, 8, 2), (1, 8, -1, 2), (32768, 8, 8, 2), (1, 16385, 1, 2), (1, 1, 16385, 2), (1, 16384, 32768, 2),
                (1, 32768, 16384, 2), (1, 8, 8, 3), (1, 8, 8, -1)):
        assert size(*bad) == 0, bad

    def call(mask=p, n=1, H=8, W=8, value=-1, thin=1, route=2, nc=p, bc=p, pc=p, nodes=p, max_nodes=4, branches=p, max_branches=4,
             points=p, max_points=16, scratch=p, nbytes=need):
        return fn(mask, n, H, W, value, thin, route, nc, bc, pc, nodes, max_nodes, branches, max_branches, points, max_points,
                  scratch, nbytes, None)
    for kw in (dict(mask=None), dict(nc=None), dict(bc=None), dict(pc=None), dict(scratch=None), dict(nodes=None),
               dict(branches=None), dict(points=None), dict(max_nodes=-1), dict(max_branches=-1), dict(max_points=-1),
               dict(value=-2), dict(value=256), dict(thin=2), dict(thin=-1), dict(route=3), dict(route=-1)):
        assert call(**kw) == _lib.EINVAL, kw
        assert b"centerlines" in _lib.lib().vitseg_last_error()
    for kw in (dict(n=0), dict(H=0), dict(W=-3), dict(n=32768), dict(H=16385, W=1), dict(H=1, W=16385), dict(H=16384, W=32768)):
        assert call(**kw) == _lib.ESHAPE, kw
        with pytest.raises(ValueError, match="centerlines: bad shape"):
            _lib.check(_lib.ESHAPE)
    assert call(nbytes=need - 1) == _lib.EWORKSPACE
    assert bytes(buf) == bytes(4096)   # nothing was written


# ---- the Python surface ----

def test_bad_arguments_are_refused_before_the_library_or_the_model(monkeypatch):
    def no_call(*a, **k):
        raise AssertionError(f"{a} requested")
    monkeypatch.setattr(_ext, "ext_symbol", no_call)
    monkeypatch.setattr(_lib, "symbol", no_call)
    ok = np.zeros((4, 4), np.uint8)
    for mask, kw in ((ok, dict(route="fast")), (ok, dict(thin=1)), (ok, dict(classes=[256])), (ok, dict(classes=[1, 1])),
                     (ok, dict(classes=[True])), (ok, dict(classes=[])), (ok, dict(classes="all")), (ok, dict(classes=[1.5])),
                     (ok.astype(np.float32), {}), (np.zeros((2, 2, 2, 2), np.uint8), {}), (np.zeros((0, 4), np.uint8), {}),
                     ("mask", {}), (np.full((2, 2), 300, np.int64), {}), (np.zeros((1, 16385), np.uint8), {}),
                     (np.zeros((16385, 1), np.uint8), {})):
        with pytest.raises(ValueError):
            centerlines.trace(mask, **kw)

    def boom(*a, **k):
        raise AssertionError("the model was reached")
    model = types.SimpleNamespace(cfg=types.SimpleNamespace(image_size=224), arena=None, predict_mask=boom,
                                  predict_mask_windowed=boom, predict_mask_tta=boom, _lowres_and_mask=boom)
    img = np.zeros((300, 300, 3), np.uint8)
    for kw in (dict(), dict(centerline_classes=[300]), dict(centerline_classes="all"), dict(centerline_classes=[1], min_area=-1),
               dict(centerline_classes=[1], tta="hflip", sliding=True)):
        with pytest.raises(ValueError):
            predict(img, model, return_centerlines=True, **kw)
    from visiontransformer_amd.model import ViTSegmentationModel
    for kw in (dict(classes=None), dict(classes=[256]), dict(classes=[1], route="fast")):
        with pytest.raises(ValueError):
            ViTSegmentationModel.predict_centerlines(model, None, **kw)
    ev = Evaluator.__new__(Evaluator)
    ev.device = "cpu"
    import torch
    pred = torch.zeros((1, 4, 4), dtype=torch.uint8)
    for args, kw in (((pred.long(), [1]), {}), ((pred[0], [1]), {}), ((pred, None), {}), ((pred, [1]), dict(pixel_size=0.0)),
                     ((pred, [999]), {})):
        with pytest.raises(ValueError):
            ev.crack_graph(*args, **kw)


def _hand_branches():
    """An open branch with a corner and a diagonal step, and a closed 2 x 2 ring, as `trace` returns them (W = 8)."""
    open_pts = np.array([[1, 1, 1], [1, 2, 4], [1, 3, 4], [2, 3, 1], [3, 4, 1]], np.int32)
    ring_pts = np.array([[5, 5, 1], [5, 6, 1], [6, 6, 1], [6, 5, 1]], np.int32)
    branches = np.array([[9, 28, 0, 5, 0, 3, 1, 65536 * 7, 4], [45, 45, 5, 4, 1, 4, 0, 65536 * 4, 1]], np.int64)
    return branches, [open_pts, ring_pts]


def test_branch_table_and_summary_are_host_arithmetic_on_the_integers():
    branches, points = _hand_branches()
    t = centerlines.branch_table(branches, 0.5, points)
    assert t[0] == {"start": 9, "end": 28, "closed": False, "points": 5, "length": (3 + math.sqrt(2.0)) * 0.5,
                    "chord": math.hypot(2, 3) * 0.5, "tortuosity": (3 + math.sqrt(2.0)) / math.hypot(2, 3),
                    "width_mean": (2 * 7 / 5 - 1) * 0.5, "width_max": 1.5}
    assert t[1]["closed"] and t[1]["chord"] == 0.0 and t[1]["tortuosity"] == float("inf") and t[1]["length"] == 2.0
    assert t[1]["width_mean"] == 0.5 and t[1]["width_max"] == 0.5
    plain = centerlines.branch_table(branches)
    assert math.isnan(plain[0]["chord"]) and math.isnan(plain[0]["tortuosity"]) and plain[0]["length"] == 3 + math.sqrt(2.0)
    nodes = np.array([[1, 1, 1, 1], [3, 4, 1, 1], [0, 7, 0, 1], [4, 0, 3, 2], [4, 1, 4, 2]], np.int32)
    assert centerlines.summary(nodes, branches, 2.0) == {"end_points": 2, "junctions": 2, "isolated": 1, "branches": 2,
                                                        "total_length": (7 + math.sqrt(2.0)) * 2.0}
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            centerlines.branch_table(branches, bad)
        with pytest.raises(ValueError):
            centerlines.summary(nodes, branches, bad)
    with pytest.raises(ValueError):
        centerlines.branch_table(branches[:, :8])
    with pytest.raises(ValueError):
        centerlines.branch_table(branches, 1.0, points[:1])


def test_geojson_of_an_open_and_a_closed_branch():
    branches, points = _hand_branches()
    g = centerlines.centerlines_to_geojson(branches, points, pixel_size=0.5, image_id="a/0", class_id=2,
                                           class_names=["bg", "x", "crack"])
    assert g["type"] == "FeatureCollection" and len(g["features"]) == 2
    f0, f1 = g["features"]
    assert f0["type"] == "Feature" and f0["geometry"]["type"] == "LineString"
    # [x + 0.5, y + 0.5] * pixel_size; the collinear point (1, 2) is dropped
    assert f0["geometry"]["coordinates"] == [[0.75, 0.75], [1.75, 0.75], [1.75, 1.25], [2.25, 1.75]]
    assert f0["properties"] == {"class": 2, "start": 9, "end": 28, "closed": False, "length": (3 + math.sqrt(2.0)) * 0.5,
                                "width_mean": (2 * 7 / 5 - 1) * 0.5, "width_max": 1.5, "points": 5, "image_id": "a/0",
                                "class_name": "crack"}
    # a closed branch repeats its first coordinate at the end
    assert f1["geometry"]["coordinates"] == [[2.75, 2.75], [3.25, 2.75], [3.25, 3.25], [2.75, 3.25], [2.75, 2.75]]
    assert f1["properties"]["closed"] is True and f1["properties"]["start"] == f1["properties"]["end"] == 45
    assert json.loads(json.dumps(g)) == g
    full = centerlines.centerlines_to_geojson(branches, points, drop_collinear=False)
    assert full["features"][0]["geometry"]["coordinates"] == [[1.5, 1.5], [2.5, 1.5], [3.5, 1.5], [3.5, 2.5], [4.5, 3.5]]
    assert set(full["features"][0]["properties"]) == {"class", "start", "end", "closed", "length", "width_mean", "width_max",
                                                      "points", "image_id"}
    assert full["features"][0]["properties"]["class"] is None and full["features"][0]["properties"]["image_id"] is None
    assert centerlines.centerlines_to_geojson(np.zeros((0, 9), np.int64), []) == {"type": "FeatureCollection", "features": []}
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            centerlines.centerlines_to_geojson(branches, points, pixel_size=bad)
    with pytest.raises(ValueError):
        centerlines.centerlines_to_geojson(branches, [])


def test_csv_rows_hold_a_row_per_branch_then_the_summary():
    branches, points = _hand_branches()
    table = centerlines.branch_table(branches, 1.0, points)
    summ = centerlines.summary(np.zeros((0, 4), np.int32), branches)
    rows = centerlines.csv_rows((7, "M"), 0, 1, 2, table, summ)
    assert len(rows) == 3 and all(len(r) == len(centerlines.CSV_COLUMNS) for r in rows)
    assert rows[0][:10] == [7, "M", 0, 1, 2, 0, 9, 28, 0, 5] and rows[1][5:9] == [1, 45, 45, 1]
    assert rows[2][5] == "summary" and rows[2][-5:] == [0, 0, 0, 2, 7 + math.sqrt(2.0)]


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
    for extra in ([], ["--crack-graph"], ["--crack-graph", "1,2", "--pixel-size", "0.25", "--min-area", "9"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        mod.main()
    assert not [k for k in seen[0][1] if "crack_graph" in k or "crack_branches" in k]   # without the flag nothing new is asked for
    for a, k in seen[1:]:
        stem = a[3][:-len("_metrics.csv")]
        assert a[3].endswith("_metrics.csv") and k["crack_graph_path"] == stem + "_crack_graph.geojson"
        assert k["crack_branches_csv_path"] == stem + "_crack_branches.csv"
    assert seen[1][1]["crack_graph_classes"] is True and seen[2][1]["crack_graph_classes"] == [1, 2]
    assert (seen[2][1]["props_pixel_size"], seen[2][1]["min_area"]) == (0.25, 9)
    monkeypatch.setattr(sys, "argv", base + ["--crack-graph", "one"])
    with pytest.raises(ValueError, match="--crack-graph takes"):
        mod.main()
