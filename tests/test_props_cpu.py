"""CPU: the numpy restatement of vitseg_region_props (tests/props_ref.py) against its naive second form, the committed scipy
golden and scipy directly; the host arithmetic of regions.props_from_records; the binding, the status codes of the argument
checks (nothing is launched, so they run without a device) and the Python validation."""
import csv
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import props_ref as PR
import regions_ref as RR
import skeleton_ref as SK
from visiontransformer_amd import _lib, metrics, regions, scripts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "props", "props.npz"))
CASES = PR.golden_cases()
_RESULTS = {}


def _ref(name):
    """The restatement's rows of a golden case, computed once."""
    if name not in _RESULTS:
        pytest.importorskip("scipy")   # skeleton_ref.inner_d2 is scipy's distance transform
        m, classes, bg, conn = CASES[name]
        _RESULTS[name] = PR.props_one(m, classes, bg, conn)[0]
    return _RESULTS[name]


def test_golden_holds_the_cases():
    assert regions.PROPS_FIELDS == PR.FIELDS and len(PR.FIELDS) == PR.NF == _lib.PROPS_FIELDS == 20
    for name, (m, classes, bg, conn) in CASES.items():
        assert np.array_equal(Z[f"{name}.mask"], m) and m.shape[0] <= 128 and m.shape[1] <= 128, name
        assert Z[f"{name}.classes"].tolist() == list(classes) and Z[f"{name}.params"].tolist() == [bg, conn]
        assert Z[f"{name}.props"].dtype == np.int64


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_golden_and_the_naive_form(name):
    m, classes, bg, conn = CASES[name]
    got = _ref(name)
    assert got.dtype == np.int64 and np.array_equal(got, Z[f"{name}.props"])
    assert np.array_equal(got, PR.props_naive(m, classes, bg, conn))


def test_what_the_special_cases_pin():
    sq = _ref("square2_16")[0]
    assert sq[2] == 4 and sq[12] == 8 and sq[13] == 0 and sq[14:19].tolist() == [1, 0, 0, -1, 0]
    s4, s8 = _ref("stairs_24_c4"), _ref("stairs_24_c8")
    assert len(s4) == 24 and len(s8) == 1
    # the documented difference: under connectivity 4 the 24 regions share the one plane's skeleton, a pixel each
    assert s4[:, 15].tolist() == [1] * 24 and s4[:, 16].sum() == 2 == s8[0, 16] and s8[0, 15] == 24
    assert s4[:, 18].sum() == s8[0, 18] == 24 * 65536 and s4[:, 12].sum() == s8[0, 12] == 96
    full = _ref("full_9x40")[0]
    # the whole image: d2 is the distance to the virtual point (-1, 0), (y + 1)^2 + x^2
    assert full[2] == 360 and full[12] == 98 and full[13] == 94 and full[14] == 81 + 39 * 39
    none = _ref("blobs5_none")
    assert (none[:, 14:19] == -1).all() and (none[:, 19] == 0).all()
    mixed = _ref("blobs5_c4")
    on = np.isin(mixed[:, 0], (1, 3))
    assert (mixed[~on, 14:19] == -1).all() and (mixed[on, 14] >= 1).all() and on.any() and (~on).any()


@pytest.mark.parametrize("name", ["blobs5_c4", "paths_c8", "rings_c4_nobg", "crack_33x65_c8"])
def test_restatement_equals_scipy(name):
    ndi = pytest.importorskip("scipy.ndimage")
    m, classes, bg, conn = CASES[name]
    got = _ref(name)
    H, W = m.shape
    yy, xx = np.mgrid[:H, :W].astype(np.int64)
    structure = None if conn == 4 else np.ones((3, 3), bool)
    rows = []
    for c in np.unique(m):
        if int(c) == bg:
            continue
        X = m == c
        lab, k = ndi.label(X, structure=structure)
        idx = np.arange(1, k + 1)
        sums = [np.rint(ndi.sum_labels(g, lab, idx)).astype(np.int64) for g in (yy, xx, yy * yy, xx * xx, xx * yy)]
        d2 = np.rint(ndi.distance_transform_edt(X) ** 2).astype(np.int64)
        mx = np.rint(ndi.maximum(d2, lab, idx)).astype(np.int64) if int(c) in classes else np.full(k, -1)
        area = np.rint(ndi.sum_labels(X, lab, idx)).astype(np.int64)
        rows += [[int(c), area[i], *[s[i] for s in sums], mx[i]] for i in range(k)]
    want = np.asarray(rows, np.int64)
    assert np.array_equal(got[:, [0, 2, 7, 8, 9, 10, 11, 14]], want)   # scipy numbers by first pixel within a class, as we do


# ---- props_from_records ----

def _rows_of(m, classes=(1,), conn=4):
    pytest.importorskip("scipy")
    return PR.props_one(np.asarray(m, np.uint8), classes, 0, conn)[0]


def test_lines_have_the_orientation_of_their_axis():
    k = 9
    m = np.zeros((5, 13), np.uint8)
    m[2, 2:2 + k] = 1
    (d,) = regions.props_from_records(_rows_of(m))
    assert d["orientation"] == 0.0 and d["minor_axis"] == 0.0 and d["length"] == k and d["width_mean"] == 1.0
    assert d["width_max"] == 1.0 and d["thickness_max"] == 1.0 and d["end_points"] == 2 and d["eccentricity"] == 1.0
    assert d["major_axis"] == pytest.approx(4 * math.sqrt((k * k - 1) / 12), rel=1e-12) and d["centroid"] == (2.0, 6.0)
    assert d["box"] == (2, 2, 2, 10) and d["area"] == k and d["extent"] == 1.0 and d["perimeter"] == 2 * k + 2
    assert d["touches_frame"] is False and d["class"] == 1
    (t,) = regions.props_from_records(_rows_of(m.T.copy()))
    assert t["orientation"] == pytest.approx(math.pi / 2, rel=1e-12) and t["minor_axis"] == 0.0 and t["length"] == k


def test_principal_axes_of_a_rectangle_equal_numpy_covariance():
    m = np.zeros((20, 30), np.uint8)
    m[3:10, 0:17] = 1   # 7 x 17, on the frame
    rows = _rows_of(m)
    (d,) = regions.props_from_records(rows)
    coords = np.argwhere(m == 1).astype(np.float64)
    cov = np.cov(coords.T, bias=True)   # [[v_yy, v_xy], [v_xy, v_xx]]
    lam, vec = np.linalg.eigh(cov)
    assert d["major_axis"] == pytest.approx(4 * math.sqrt(lam[1]), rel=1e-12)
    assert d["minor_axis"] == pytest.approx(4 * math.sqrt(lam[0]), rel=1e-12)
    assert d["eccentricity"] == pytest.approx(math.sqrt(1 - lam[0] / lam[1]), rel=1e-12)
    assert d["centroid"] == pytest.approx(tuple(coords.mean(axis=0)), rel=1e-12)
    assert abs(d["orientation"]) < 1e-12 and abs(vec[0, 1]) < 1e-12         # the major axis lies along the columns
    assert d["touches_frame"] is True and d["extent"] == 1.0 and d["perimeter"] == 48
    assert d["compactness"] == pytest.approx(4 * math.pi * 119 / 48 ** 2, rel=1e-12)
    # a slanted figure: the angle of the leading eigenvector, measured from the column axis towards the row axis
    s = np.zeros((40, 40), np.uint8)
    for i in range(30):
        s[5 + i // 2:8 + i // 2, 3 + i] = 1
    (e,) = regions.props_from_records(_rows_of(s))
    c2 = np.cov(np.argwhere(s == 1).astype(np.float64).T, bias=True)
    lam2, vec2 = np.linalg.eigh(c2)
    vy, vx = vec2[:, 1]
    assert e["orientation"] == pytest.approx(math.atan2(vy, vx) if vx > 0 else math.atan2(-vy, -vx), rel=1e-12)
    assert e["major_axis"] == pytest.approx(4 * math.sqrt(lam2[1]), rel=1e-12) and 0 < e["orientation"] < math.pi / 4


def test_pixel_size_scales_lengths_and_areas_and_unmeasured_is_nan():
    m = SK.crack_map(33, 65, 5)
    rows = _rows_of(m, classes=(2,), conn=8)
    one, half = regions.props_from_records(rows), regions.props_from_records(rows, pixel_size=0.5)
    assert len(one) == len(rows) and {d["class"] for d in one} == {1, 2}
    for a, b in zip(one, half):
        assert b["area"] == a["area"] / 4 and b["box"] == a["box"] and b["class"] == a["class"]
        for key in ("major_axis", "minor_axis", "perimeter"):
            assert b[key] == pytest.approx(a[key] / 2, rel=1e-12)
        assert b["centroid"] == pytest.approx((a["centroid"][0] / 2, a["centroid"][1] / 2), rel=1e-12)
        for key in ("orientation", "eccentricity", "extent", "compactness", "touches_frame"):
            assert b[key] == a[key]
        for key in ("thickness_max", "length", "width_mean", "width_max"):
            if a["class"] == 2 and not math.isnan(a[key]):
                assert b[key] == pytest.approx(a[key] / 2, rel=1e-12)
            else:
                assert math.isnan(b[key]) and (a["class"] == 1 or key in ("width_mean", "width_max"))
        assert math.isnan(a["end_points"]) == (a["class"] == 1)
    sq = regions.props_from_records(_rows_of(PR.square2(16, 16)))[0]   # measured, and its skeleton is empty
    assert sq["length"] == 0 and math.isnan(sq["width_mean"]) and math.isnan(sq["width_max"]) and sq["thickness_max"] == 1.0
    assert sq["end_points"] == 0
    r = rows[rows[:, 0] == 2][0]
    d = [x for x in one if x["class"] == 2][0]
    assert d["width_mean"] == pytest.approx(2 * (r[18] / 65536) / r[15] - 1, rel=1e-12)
    assert d["width_max"] == pytest.approx(2 * math.sqrt(r[17]) - 1, rel=1e-12)
    for bad in (0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            regions.props_from_records(rows, pixel_size=bad)
    with pytest.raises(ValueError):
        regions.props_from_records(rows[:, :7])
    assert regions.props_from_records(np.zeros((0, 20), np.int64)) == []


def test_the_moments_are_exact_for_sums_beyond_double_precision():
    # one row of 16384 pixels far from the origin: area * sum_xx and sum_x^2 are near 2^80 and differ by the variance alone
    x = np.arange(16384, dtype=object) + 0
    row = [1, 0, 16384, 7, 0, 7, 16383, 7 * 16384, int(x.sum()), 49 * 16384, int((x * x).sum()), 7 * int(x.sum()), 2 * 16384 + 2,
           16384, -1, -1, -1, -1, -1, 0]
    (d,) = regions.props_from_records(np.asarray([row], np.int64))
    assert d["major_axis"] == pytest.approx(4 * math.sqrt((16384 ** 2 - 1) / 12), rel=1e-12) and d["minor_axis"] == 0.0


# ---- the binding and the status codes ----

def test_exports_and_header():
    assert _lib.PROPS_EXPORTS == ["vitseg_region_props_scratch_bytes", "vitseg_region_props"]
    assert set(_lib.PROPS_EXPORTS) <= set(_lib._LATE_EXPORTS) <= set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "vitseg.h")).read()
    assert re.search(r"#define\s+VITSEG_VERSION\s+110\b", hdr) and _lib.VERSION == 110 == _lib.lib().vitseg_version()
    assert re.search(r"#define\s+VITSEG_PROPS_FIELDS\s+20\b", hdr)
    for name in _lib.PROPS_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert _lib.props_symbol(name) is not None


def test_scratch_size_function():
    f = _lib.props_symbol("vitseg_region_props_scratch_bytes")
    reg = _lib.region_symbol("vitseg_regions_scratch_bytes")
    for K in (0, 3):
        for route in (0, 2):
            assert f(0, 8, 8, K, route) == 0 and f(32768, 8, 8, K, route) == 0
            assert f(2, 0, 8, K, route) == 0 and f(2, 8, 16385, K, route) == 0 and f(2, 16385, 8, K, route) == 0
        assert f(2, 8, 8, K, -1) == 0 and f(2, 8, 8, K, 3) == 0
    assert f(2, 8, 8, -1, 0) == 0 and f(2, 8, 8, 257, 0) == 0
    assert f(2, 16384, 16384, 1, 1) == 0                      # no device holds such a plane in LDS
    n, H, W = 3, 70, 97
    base = f(n, H, W, 0, 0)
    assert base >= reg(n, H, W) + 4 * n * H * W                 # the labelling's scratch and the labels
    assert f(n, H, W, 0, 1) == f(n, H, W, 0, 2) == base         # without classes the route changes nothing
    assert f(n, H, W, 1, 2) >= base + 7 * n * H * W and f(n, H, W, 1, 2) == f(n, H, W, 256, 2)   # classes take turns


def test_every_status_code_without_a_device():
    """The argument checks come before anything touches a device: every address is a live host buffer no call reaches."""
    fn = _lib.props_symbol("vitseg_region_props")
    size = _lib.props_symbol("vitseg_region_props_scratch_bytes")
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    big = 1 << 40

    def call(*, mask=p, n=1, H=8, W=8, conn=4, bg=0, classes=(1, 2), null_classes=False, K=None, route=2, counts=p, props=p,
             max_regions=4, labels=None, scratch=p, nbytes=big):
        cls = None if null_classes else (ctypes.c_int32 * max(len(classes), 1))(*classes)
        rc = fn(mask, n, H, W, conn, bg, cls, len(classes) if K is None else K, route, counts, props, max_regions, labels,
                scratch, nbytes, None)
        assert rc == _lib.OK or _lib.lib().vitseg_last_error()
        return rc

    for kw in (dict(mask=None), dict(counts=None), dict(scratch=None), dict(props=None), dict(max_regions=-1),
               dict(conn=0), dict(conn=6), dict(bg=-2), dict(bg=256), dict(route=-1), dict(route=3), dict(null_classes=True),
               dict(classes=(1, 256)), dict(classes=(-1,)), dict(classes=(1, 1)), dict(classes=(0, 1)),
               dict(classes=(3, 2), bg=2)):
        assert call(**kw) == _lib.EINVAL, kw
    for kw in (dict(n=0), dict(n=32768), dict(H=0), dict(H=16385), dict(W=-1), dict(W=16385), dict(K=-1), dict(K=257),
               dict(H=16384, W=16384, route=1)):
        assert call(**kw) == _lib.ESHAPE, kw
    for kw in (dict(), dict(classes=(), null_classes=True), dict(bg=-1, classes=(0,)), dict(props=None, max_regions=0)):
        K = len(kw.get("classes", (1, 2)))
        need = size(1, 8, 8, K, 2)
        assert need > 0 and call(nbytes=need - 1, **kw) == _lib.EWORKSPACE, kw
    assert all(b == 0 for b in buf)   # and nothing wrote to the buffers


# ---- the Python surface ----

def test_region_props_checks_its_arguments_before_the_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "props_symbol", boom)
    m = np.zeros((4, 4), np.uint8)
    for kw in (dict(connectivity=6), dict(background=256), dict(background=True), dict(background=-2), dict(route="fast"),
               dict(skeleton_classes="some"), dict(skeleton_classes=[256]), dict(skeleton_classes=[-1]),
               dict(skeleton_classes=[1, 1]), dict(skeleton_classes=[0, 1]), dict(skeleton_classes=[1.5]),
               dict(skeleton_classes=[True]), dict(skeleton_classes=[2], background=2)):
        with pytest.raises(ValueError):
            regions.region_props(m, **kw)
    for bad in (np.zeros((2, 2, 2, 2), np.uint8), np.zeros((0, 4), np.uint8), np.zeros((4, 4), np.float32), [[0, 1]],
                np.full((2, 2), 256, np.int64), np.zeros((1, 16385), np.uint8)):
        with pytest.raises(ValueError):
            regions.region_props(bad)
    ev = metrics.Evaluator(3, device="cpu")
    pred = torch.zeros((1, 4, 4), dtype=torch.uint8)
    for bad in (pred.long(), pred[0], pred.numpy()):
        with pytest.raises(ValueError):
            ev.region_props(bad)
    with pytest.raises(ValueError, match="must be equal"):
        ev.region_props(pred, torch.zeros((2, 4, 4), dtype=torch.uint8))
    assert scripts.parse_props_classes(None) is None and scripts.parse_props_classes("all") == "all"
    assert scripts.parse_props_classes("1,3") == [1, 3]
    with pytest.raises(ValueError):
        scripts.parse_props_classes("cracks")


def test_csv_header_and_one_row(tmp_path):
    rows = _rows_of(SK.crack_map(33, 65, 5), classes=(1, 2), conn=8)
    dicts = regions.props_from_records(rows, pixel_size=0.25)
    path = tmp_path / "m_region_props.csv"
    regions.write_props_csv(str(path), [regions.props_csv_row("pred", (7, "m", 16, 192, 1, 3), 2, 1, r, d)
                                        for r, d in enumerate(dicts)])
    got = list(csv.reader(open(path, newline="")))
    assert got[0] == regions.PROPS_CSV_COLUMNS and got[0][:6] == ["Source", "Model_ID", "Model_Name", "Batch_Num", "Image_Idx",
                                                                 "Region"]
    assert len(got) == 1 + len(rows) and all(len(r) == len(got[0]) for r in got)
    col = {k: i for i, k in enumerate(got[0])}
    r, d = got[1], dicts[0]
    assert r[:7] == ["pred", "7", "m", "2", "1", "0", str(d["class"])]
    assert [int(r[col[k]]) for k in ("Y_Min", "X_Min", "Y_Max", "X_Max")] == list(rows[0, 3:7])
    assert float(r[col["Area"]]) == rows[0, 2] / 16 and float(r[col["Length"]]) == rows[0, 15] / 4
    assert float(r[col["Width_Mean"]]) == d["width_mean"] and r[col["Touches_Frame"]] in ("0", "1")
    assert int(r[col["End_Points"]]) == rows[0, 16]


def _load_script(rel):
    """model/<dir>/<script>.py as a module; its `from classes import ...` resolves in its own directory."""
    import importlib.util
    import sys
    path = os.path.join(ROOT, *rel.split("/"))
    sys.path.insert(0, os.path.dirname(path))
    kept = sys.modules.pop("classes", None)
    try:
        spec = importlib.util.spec_from_file_location("script_under_test_" + os.path.basename(path)[:-3], path)
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
def test_evaluation_scripts_pass_the_flags_on(rel, trainer, batches, monkeypatch, tmp_path):
    import sys
    import types
    mod = _load_script(rel)
    seen = []
    monkeypatch.setattr(mod, trainer, lambda *a, **k: types.SimpleNamespace(model=types.SimpleNamespace(cfg=None)))
    monkeypatch.setattr(scripts, "get_latest_checkpoint", lambda *a: None)
    monkeypatch.setattr(scripts, batches, lambda *a, **k: [])
    monkeypatch.setattr(scripts, "evaluate_to_csv", lambda *a, **k: seen.append(k) or [[0.0] * 12])
    monkeypatch.chdir(tmp_path)
    base = [rel, "--ids", "1", "--num-batches", "1"]
    for extra in ([], ["--region-props"], ["--region-props", "2,1", "--pixel-size", "0.25", "--region-connectivity", "8"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        mod.main()
    got = [(d["props_classes"], d["props_pixel_size"], d["region_connectivity"]) for d in seen]
    assert got == [(None, 1.0, 4), ("all", 1.0, 4), ([2, 1], 0.25, 8)]   # without the flag nothing new is asked for
