"""CPU (-m "not gpu"): the restatement of the precision-recall counts against scipy's grey dilation and distance transform, the
host arithmetic (curve, ODS, OIS, AP) against sklearn and hand-made counts, the family header against `_ext.EXT_LATER`, the
argument checks and the flags of the evaluation scripts.  No compute entry point runs."""
import argparse
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import curves_ref as CV
from test_binding_cpu import parse_header, signature_errors
from visiontransformer_amd import _ext, _lib, curves, reports, scripts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vitseg_curves.h")
NAMES = ["vitseg_curves_version", "vitseg_pr_counts_scratch_bytes", "vitseg_pr_counts"]
TOL2 = [0, 1, 2, 4, 5, 8, 25, 256]


# ---- the restatement ----

def _case(seed, H=41, W=37):
    """(q int64 [2, H, W], gt uint8 [2, H, W]) with sparse true pixels (class 1), void pixels (255) among and beside them"""
    rs = np.random.RandomState(seed)
    q = rs.randint(0, 65536, size=(2, H, W)).astype(np.int64)
    gt = (rs.rand(2, H, W) < 0.03).astype(np.uint8)
    gt[rs.rand(2, H, W) < 0.1] = 255
    gt[0, 0, 0] = gt[1, H - 1, W - 1] = 1   # true pixels in two corners
    return q, gt


@pytest.mark.parametrize("tol2", TOL2)
def test_found_plane_is_scipys_grey_dilation_by_the_disc(tol2):
    ndimage = pytest.importorskip("scipy.ndimage")
    r = int(np.sqrt(tol2))
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    foot = yy * yy + xx * xx <= tol2
    assert int(foot.sum()) == len(CV.disc(tol2)) and (tol2 != 256 or foot.shape == (33, 33))
    for ignore in (-1, 255):
        q, gt = _case(tol2)
        valid, pos, hit, best = CV.planes(q, gt, 1, tol2, ignore)
        src = np.where(valid, q, -1)
        for b in range(2):
            want = ndimage.maximum_filter(src[b], footprint=foot, mode="constant", cval=-1)
            assert np.array_equal(best[b], want)
        assert (best[pos] >= q[pos]).all() and (ignore == -1 or (best == -1).any() or tol2 > 0)


@pytest.mark.parametrize("tol2", TOL2)
def test_hit_plane_is_the_squared_distance_transform_within_tol2(tol2):
    ndimage = pytest.importorskip("scipy.ndimage")
    for ignore in (-1, 255):
        q, gt = _case(100 + tol2)
        valid, pos, hit, _ = CV.planes(q, gt, 1, tol2, ignore)
        for b in range(2):
            _, (iy, ix) = ndimage.distance_transform_edt(~pos[b], return_indices=True)
            yy, xx = np.mgrid[0:pos.shape[1], 0:pos.shape[2]]
            d2 = (iy - yy).astype(np.int64) ** 2 + (ix - xx).astype(np.int64) ** 2   # squared integers, no root
            assert np.array_equal(hit[b], valid[b] & (d2 <= tol2))
        if tol2 == 0:
            assert np.array_equal(hit, pos)


def test_counts_conserve_pixels_and_grow_with_the_tolerance():
    q, gt = _case(7)
    before = None
    for tol2 in TOL2:
        valid, pos, hit, best = CV.planes(q, gt, 1, tol2, 255)
        c = CV.counts_from_planes(q, valid, pos, hit, best, 16)
        assert np.array_equal(c[:, :, 0].sum(axis=1), valid.sum(axis=(1, 2)))
        assert np.array_equal(c[:, :, 2].sum(axis=1), pos.sum(axis=(1, 2)))
        assert tol2 or np.array_equal(c[:, :, 1], c[:, :, 2])
        cum = np.cumsum(c[:, ::-1], axis=1)[:, ::-1]
        assert before is None or ((cum[:, :, 1:] >= before[:, :, 1:]).all() and (cum[:, :, 2] > before[:, :, 2]).any())
        before = cum


# ---- the host arithmetic ----

def _plain_counts(bin_idx, y, bins):
    """the tolerance-0 table of scores that are bin indices and labels y"""
    c = np.zeros((bins, 3), np.int64)
    c[:, 0] = np.bincount(bin_idx, minlength=bins)
    c[:, 1] = c[:, 2] = np.bincount(bin_idx[y == 1], minlength=bins)
    return c


def test_ap_and_curve_at_tolerance_0_are_sklearns():
    skm = pytest.importorskip("sklearn.metrics")
    rs = np.random.RandomState(3)
    for bins, n in ((7, 400), (256, 5000), (1024, 3000)):
        y = (rs.rand(n) < 0.2).astype(np.int64)
        b = np.clip((rs.rand(n) * 0.6 + y * rs.rand(n) * 0.5) * bins, 0, bins - 1).astype(np.int64)
        c = _plain_counts(b, y, bins)
        assert abs(curves.ap(c) - skm.average_precision_score(y, b)) < 1e-12
        prec, rec, thr = skm.precision_recall_curve(y, b)
        cur = curves.curve_from_counts(c)
        assert cur["n_gt"] == int(y.sum())
        for k, p, r in zip(thr, prec, rec):   # sklearn's threshold t means score >= t: ours k = t
            k = int(k)
            assert Fraction(cur["hit"][k], cur["predicted"][k]) == Fraction(int((y[b >= k]).sum()), int((b >= k).sum()))
            assert abs(cur["precision"][k] - p) < 1e-12 and abs(cur["recall"][k] - r) < 1e-12
        # pooled by addition first: two halves give the whole
        half = _plain_counts(b[:n // 2], y[:n // 2], bins), _plain_counts(b[n // 2:], y[n // 2:], bins)
        assert curves.curve_from_counts(np.stack(half)) == cur
        assert cur["threshold"][0] == 0.0 and cur["threshold"][bins - 1] == curves.threshold_q(bins - 1, bins) / 65535
    assert [curves.threshold_q(k, 7) for k in range(7)] == [0, 9363, 18725, 28087, 37450, 46812, 56174]
    for bins in (1, 7, 256, 1024):   # q >= threshold_q(k) is bin >= k
        for k in range(bins):
            t = curves.threshold_q(k, bins)
            assert (t * bins) >> 16 >= k and (t == 0 or ((t - 1) * bins) >> 16 < k)


def test_ods_ois_ap_on_hand_made_counts():
    # image a: 4 bins; threshold k keeps bins k..: pred (10, 6, 4, 2), hit (4, 4, 3, 2), found (4, 4, 2, 2), n_gt 4
    a = np.array([[4, 0, 0], [2, 1, 2], [2, 1, 0], [2, 2, 2]], np.int64)
    cur = curves.curve_from_counts(a)
    assert cur["predicted"] == [10, 6, 4, 2] and cur["hit"] == [4, 4, 3, 2] and cur["found"] == [4, 4, 2, 2] and cur["n_gt"] == 4
    assert cur["precision"] == [0.4, 4 / 6, 0.75, 1.0] and cur["recall"] == [1.0, 1.0, 0.5, 0.5]
    f = [2 * p * r / (p + r) for p, r in zip(cur["precision"], cur["recall"])]
    assert cur["f"] == f and max(f) == f[1] == 0.8
    assert curves.ods(a) == {"f": 0.8, "k": 1, "threshold": 16384 / 65535, "precision": 4 / 6, "recall": 1.0}
    assert curves.ap(a) == (1.0 - 1.0) * 0.4 + (1.0 - 0.5) * (4 / 6) + 0.0 * 0.75 + 0.5 * 1.0
    # a tie: the smallest k among equals
    tie = np.array([[0, 0, 0], [0, 0, 0], [3, 3, 3], [0, 0, 0]], np.int64)
    assert curves.curve_from_counts(tie)["f"] == [1.0, 1.0, 1.0, 0.0] and curves.ods(tie)["k"] == 0
    # an empty threshold: nothing predicted there -- F is 0, the precision nan, and AP leaves it out
    cur = curves.curve_from_counts(tie)
    assert np.isnan(cur["precision"][3]) and cur["predicted"][3] == 0 and curves.ap(tie) == 1.0
    # an image without true pixels: every F is 0, OIS leaves it out, ODS pools it
    none = np.array([[5, 0, 0], [0, 0, 0], [2, 0, 0], [1, 0, 0]], np.int64)
    assert curves.curve_from_counts(none)["f"] == [0.0] * 4 and np.isnan(curves.curve_from_counts(none)["recall"][0])
    assert np.isnan(curves.ois(none)) and np.isnan(curves.ois(np.stack([none, none]))) and np.isnan(curves.ap(none))
    assert curves.ois(np.stack([a, none, tie])) == (0.8 + 1.0) / 2
    pooled = curves.ods(np.stack([a, none, tie]))
    assert pooled == curves.ods(a + none + tie) and pooled["f"] < curves.ois(np.stack([a, none, tie]))
    s = curves.summary(np.stack([a, tie]))
    assert s == {"ods": curves.ods(a + tie), "ois": 0.9, "ap": curves.ap(a + tie)}
    # found can reach pixels no prediction hits: P + R = 0 only when both are 0
    assert curves.curve_from_counts(np.array([[1, 0, 0], [1, 0, 1]], np.int64))["f"] == [0.0, 0.0]
    for bad in (np.zeros((4, 2), np.int64), np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int64), -np.ones((2, 3), np.int64), [1, 2, 3]):
        with pytest.raises(ValueError):
            curves.curve_from_counts(bad)
    rows = curves.csv_rows((7, "m"), np.stack([a, tie]), 1, 2.0)
    assert len(rows) == 4 + 3 and all(len(r) == len(curves.CSV_COLUMNS) for r in rows)
    assert [r[5] for r in rows] == [0, 1, 2, 3, "ODS", "OIS", "AP"] and rows[4][-1] == s["ods"]["f"] and rows[5][-1] == 0.9
    assert rows[6][-1] == s["ap"] and rows[0][:5] == [7, "m", 1, 4, 2.0]


# ---- the family header and its table ----

def _table():
    return {name: (restype, list(argtypes)) for name, restype, argtypes in _ext.EXT_LATER["curves"][2]}


def test_family_header_is_the_table_both_ways():
    decls, structs, enums, defines = parse_header(open(HEADER).read())
    assert _ext.EXT_LATER["curves"][:2] == ("vitseg_curves.h", "the precision-recall curves")
    assert sorted(decls) == sorted(NAMES) == sorted(_table()) and not structs and not enums
    assert signature_errors(decls, _table()) == []
    assert len(decls["vitseg_pr_counts"][1]) == 15 and decls["vitseg_pr_counts"][1][11] == ("int64_t", 1)
    assert defines == {"VITSEG_CURVES_VERSION": 100, "VITSEG_CURVES_MAX_BINS": curves.MAX_BINS, "VITSEG_CURVES_MAX_TOL2": 256}
    assert _ext.CURVES_VERSION == 100 and _ext.EXT_VERSIONS["curves"] == ("vitseg_curves_version", 100)
    tab = _table()
    tab["vitseg_pr_counts"] = (C.c_int, tab["vitseg_pr_counts"][1][:13] + [C.c_int] + tab["vitseg_pr_counts"][1][14:])
    assert signature_errors(decls, tab) == ["vitseg_pr_counts: argument 13: c_int for size_t"]   # the comparison can fail
    assert not set(NAMES) & set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "vitseg.h")).read()
    assert "pr_counts" not in hdr and "curves" not in hdr.lower() and '#include "vitseg.h"' in open(HEADER).read()


def test_library_exports_the_family_at_its_version():
    l = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(l, name), name
    assert _ext.ext_symbol("curves", "vitseg_curves_version")() == 100
    fn = _ext.ext_symbol("curves", "vitseg_pr_counts")
    assert fn.restype is C.c_int and list(fn.argtypes) == _table()["vitseg_pr_counts"][1]
    assert _ext.ext_symbol("curves", "vitseg_pr_counts_scratch_bytes").restype is C.c_size_t


def test_every_status_code_without_a_device():
    """The argument checks come before any launch: every address is a live host buffer that no call reaches."""
    fn = _ext.ext_symbol("curves", "vitseg_pr_counts")
    size = _ext.ext_symbol("curves", "vitseg_pr_counts_scratch_bytes")
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    need = size(1, 8, 25)

    def call(lowres=p, gt=p, n=1, Cc=2, g=2, S=8, cls=1, kind=0, bins=16, tol2=4, ignore=-1, counts=p, scratch=p, nbytes=need):
        return fn(lowres, gt, n, Cc, g, S, cls, kind, bins, tol2, ignore, counts, scratch, nbytes, None)
    for kw in (dict(lowres=None), dict(gt=None), dict(counts=None), dict(kind=2), dict(kind=-1), dict(kind=1, Cc=1, cls=0),
               dict(cls=-1), dict(cls=2), dict(bins=0), dict(bins=1025), dict(tol2=-1), dict(tol2=257), dict(ignore=-2),
               dict(ignore=256)):
        assert call(**kw) == _lib.EINVAL, kw
        assert b"pr_counts" in _lib.lib().vitseg_last_error()
    for kw in (dict(n=0), dict(n=65536), dict(Cc=0), dict(Cc=256), dict(S=0), dict(S=16385), dict(g=0), dict(g=9)):
        assert call(**kw) == _lib.ESHAPE, kw
        with pytest.raises(ValueError, match="pr_counts: bad shape"):
            _lib.check(_lib.ESHAPE)
    if need:
        assert call(nbytes=need - 1) == _lib.EWORKSPACE and call(scratch=None) == _lib.EINVAL
    assert bytes(buf) == bytes(4096)   # nothing was written


# ---- the Python surface ----

def test_pr_counts_rejects_bad_arguments_before_the_library(monkeypatch):
    def no_call(*a, **k):
        raise AssertionError(f"{a} requested")
    monkeypatch.setattr(_ext, "ext_symbol", no_call)
    low, gt = torch.zeros((2, 3, 4, 4)), torch.zeros((2, 8, 8), dtype=torch.uint8)
    for kw in (dict(cls=-1), dict(cls=True), dict(cls=1.0), dict(cls=3), dict(bins=0), dict(bins=1025), dict(bins=2.0),
               dict(tolerance=-1), dict(tolerance=16.5), dict(tolerance=float("nan")), dict(tolerance="2"), dict(tolerance=True),
               dict(ignore_label=-1), dict(ignore_label=256), dict(kind="softmax"), dict(gt=gt.float()), dict(gt=gt[0]),
               dict(gt=torch.zeros((2, 8, 9), dtype=torch.uint8)), dict(gt=torch.zeros((3, 8, 8), dtype=torch.uint8)),
               dict(gt=torch.zeros((2, 2, 2), dtype=torch.uint8)), dict(lowres=low.double()), dict(lowres=low[:, :, :3]),
               dict(lowres=low[:, :1], kind="margin", cls=0)):
        args = dict(lowres=low, gt=gt)
        args.update(kw)
        with pytest.raises(ValueError):
            curves.pr_counts(**args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        curves.pr_counts(low, gt)
    with pytest.raises(ValueError, match="gt must be"):
        curves.pr_counts(low, "gt")


def test_tolerance_becomes_the_floor_of_its_square():
    got = {t: curves.tolerance_to_tol2(t) for t in (0, 1, 1.4, 2 ** 0.5, 2, 5 ** 0.5, 2.24, 2.99, 3, 5, 16, np.float32(2.5), np.int64(4))}
    assert got == {0: 0, 1: 1, 1.4: 1, 2 ** 0.5: 2, 2: 4, 5 ** 0.5: 5, 2.24: 5, 2.99: 8, 3: 9, 5: 25, 16: 256, np.float32(2.5): 6,
                   np.int64(4): 16}
    for bad in (-0.5, 16.01, 17, float("inf"), float("nan"), None, "3", True):
        with pytest.raises(ValueError):
            curves.tolerance_to_tol2(bad)


# ---- the flags ----

CSV = "out/ID1/ID1_metrics.csv"


def _options(argv):
    ap = argparse.ArgumentParser()
    scripts.add_evaluation_arguments(ap)
    return scripts.evaluation_options(ap, ap.parse_args(argv), CSV)


def test_the_flags_add_their_keys_and_are_refused_with_tta():
    none = _options([])
    assert not any(k.startswith("pr_") for k in none)   # without the flag nothing new is asked for
    assert _options(["--pr-curve"]) == dict(none, pr_curve=1, pr_bins=256, pr_tolerance=0.0)
    got = _options(["--pr-curve", "2", "--pr-bins", "1024", "--pr-tolerance", "2.5", "--score-kind", "margin"])
    assert got == dict(none, pr_curve=2, pr_bins=1024, pr_tolerance=2.5, score_kind="margin")
    assert _options(["--pr-bins", "64", "--pr-tolerance", "3"]) == none   # the curve's options alone ask for nothing
    for argv in (["--pr-curve", "--tta", "hflip"], ["--pr-curve", "-1"], ["--pr-curve", "255"], ["--pr-curve", "--pr-bins", "0"],
                 ["--pr-curve", "--pr-bins", "1025"], ["--pr-curve", "--pr-tolerance", "17"], ["--pr-curve", "--pr-tolerance", "-1"],
                 ["--pr-curve", "x"]):
        with pytest.raises(SystemExit):
            _options(argv)
    with pytest.raises(ValueError, match="with tta"):
        reports.check_scoring("hflip", "prob", 0.5)

    def boom(*a, **k):
        raise AssertionError("the model was reached")
    import types
    model = types.SimpleNamespace(eval=boom, cfg=types.SimpleNamespace(num_classes=2))
    for kw in (dict(pr_curve=1, tta="hflip"), dict(pr_curve=1, pr_bins=0), dict(pr_curve=1, pr_tolerance=17), dict(pr_curve=2),
               dict(pr_curve=1, score_kind="softmax")):
        with pytest.raises(ValueError):
            scripts.evaluate_to_csv(model, [], (1, "m"), CSV, 2, 1, "cpu", **kw)


def test_the_report_writes_its_rows_without_a_batch(tmp_path):
    r = reports.PRCurve((7, "m"), cls=1, bins=4, tolerance=2)
    assert r.needs_lowres and r.suffix == "_pr_curve.csv"
    r.write(str(tmp_path / "m"))
    import csv
    got = list(csv.reader(open(tmp_path / "m_pr_curve.csv", newline="")))
    assert got[0] == curves.CSV_COLUMNS and [g[5] for g in got[1:]] == ["0", "1", "2", "3", "ODS", "OIS", "AP"]
    for kw in (dict(bins=0), dict(cls=-1), dict(tolerance=99)):
        with pytest.raises(ValueError):
            reports.PRCurve((7, "m"), **kw)


@pytest.mark.parametrize("rel,trainer,batches", [("model/CE/datasetTestViTmodel.py", "LightningViTModel", "ce_batches"),
                                                ("model/PAED/ViTscriptTest.py", "PAEDTrainer", "paed_binary_batches")])
def test_evaluation_scripts_pass_the_flags_on(rel, trainer, batches, monkeypatch, tmp_path):
    import sys
    import types
    from test_polygons_cpu import _load_script
    mod = _load_script(rel)
    seen = []
    monkeypatch.setattr(mod, trainer, lambda *a, **k: types.SimpleNamespace(model=types.SimpleNamespace(cfg=None)))
    monkeypatch.setattr(scripts, "get_latest_checkpoint", lambda *a: None)
    monkeypatch.setattr(scripts, batches, lambda *a, **k: [])
    monkeypatch.setattr(scripts, "evaluate_to_csv", lambda *a, **k: seen.append((a, k)) or [[0.0] * 12])
    monkeypatch.chdir(tmp_path)
    base = [rel, "--ids", "1", "--num-batches", "1"]
    for extra in ([], ["--pr-curve"], ["--pr-curve", "0", "--pr-bins", "100", "--pr-tolerance", "2", "--score-kind", "margin"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        mod.main()
    assert not any(k.startswith("pr_") for k in seen[0][1])   # without the flag nothing new is asked for
    assert {k: v for k, v in seen[1][1].items() if k.startswith("pr_")} == dict(pr_curve=1, pr_bins=256, pr_tolerance=0.0)
    assert {k: v for k, v in seen[2][1].items() if k.startswith("pr_")} == dict(pr_curve=0, pr_bins=100, pr_tolerance=2.0)
    assert seen[2][1]["score_kind"] == "margin"
    monkeypatch.setattr(sys, "argv", base + ["--pr-curve", "--tta", "hflip"])
    with pytest.raises(SystemExit):
        mod.main()
    assert len(seen) == 3   # refused when the arguments are parsed: no model was built
