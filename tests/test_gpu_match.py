"""GPU (-m gpu): region matching on the device (vitseg_region_match, Evaluator.region_metrics, --region-metrics of the
evaluation scripts) against the committed scipy goldens and the numpy restatement tests/match_ref.py.  Everything is an
integer: every comparison is bit for bit."""
import csv
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import match_ref as M
from guard import check, guarded, snapshot, unchanged
from visiontransformer_amd import _lib, metrics, regions
from visiontransformer_amd.preprocess import NEAREST_PIL, nearest_table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "match", "match.npz"))
CASES = M.match_cases()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(pred, gt, classes, fill, connectivity=4, background=0, ignore_label=-1, thr=(1, 2), cov=(1, 2), want=(True, True)):
    """One vitseg_region_match call through the C ABI on device tensors, with guarded outputs and a scratch pre-filled with
    `fill`: (stats, pred_info or None, gt_info or None) as numpy arrays."""
    n, H, W = pred.shape
    K = len(classes)
    nbytes = _lib.match_symbol("vitseg_region_match_scratch_bytes")(n, H, W)
    scratch = guarded((nbytes,), torch.uint8, name="scratch")
    scratch.fill_(fill)
    stats = guarded((n, K, 8), torch.int64, name="stats")
    pinfo = guarded((n, H, W, 2), torch.int32, name="pred_info") if want[0] else None
    ginfo = guarded((n, H, W, 2), torch.int32, name="gt_info") if want[1] else None
    snap = snapshot(pred, gt)
    cls = (ctypes.c_int32 * K)(*classes)
    _lib.check(_lib.match_symbol("vitseg_region_match")(
        pred.data_ptr(), gt.data_ptr(), n, H, W, cls, K, connectivity, background, ignore_label, *thr, *cov, stats.data_ptr(),
        None if pinfo is None else pinfo.data_ptr(), None if ginfo is None else ginfo.data_ptr(), scratch.data_ptr(),
        scratch.numel(), _stream()))
    torch.cuda.synchronize()
    check(stats, pinfo, ginfo, scratch)
    unchanged(snap)
    return tuple(None if t is None else t.cpu().numpy() for t in (stats, pinfo, ginfo))


def _on_device(c):
    return (guarded(c["pred"].shape, torch.uint8, torch.from_numpy(c["pred"]).to(DEV), name="pred"),
            guarded(c["gt"].shape, torch.uint8, torch.from_numpy(c["gt"]).to(DEV), name="gt"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_cases_through_the_c_abi(name):
    c = CASES[name]
    pred, gt = _on_device(c)
    runs = [_call(pred, gt, c["classes"], fill, **M.case_kwargs(c)) for fill in (0x00, 0xFF)]
    for stats, pinfo, ginfo in runs:
        assert np.array_equal(stats, Z[f"{name}.stats"]), (stats - Z[f"{name}.stats"]).reshape(-1, 8)
        for i in range(len(stats)):
            assert np.array_equal(M.table(pinfo[i]), Z[f"{name}.pred_table.{i}"]), i
            assert np.array_equal(M.table(ginfo[i]), Z[f"{name}.gt_table.{i}"]), i
            assert (pinfo[i][pinfo[i][..., 0] == -2][:, 1] == 0).all() and (ginfo[i][ginfo[i][..., 0] == -2][:, 1] == 0).all()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)   # a scratch word read before it is written would tell the two fills apart
    check(pred, gt)


@pytest.mark.parametrize("name", ["speckle5_97x131", "speckle5_97x131_novoid"])
def test_the_optional_planes_may_be_null(name):
    c = CASES[name]
    pred, gt = _on_device(c)
    full = _call(pred, gt, c["classes"], 0xFF, **M.case_kwargs(c))
    for want in ((False, False), (True, False), (False, True)):
        stats, pinfo, ginfo = _call(pred, gt, c["classes"], 0xFF, want=want, **M.case_kwargs(c))
        assert np.array_equal(stats, full[0]), want
        assert (pinfo is None) == (not want[0]) and (ginfo is None) == (not want[1])
        assert pinfo is None or np.array_equal(pinfo, full[1])
        assert ginfo is None or np.array_equal(ginfo, full[2])


@pytest.mark.parametrize("name", ["batch5_160x200", "batch5_160x200_c8"])
def test_batch_equals_restatement_and_images_alone(name):
    c = CASES[name]
    kw = M.case_kwargs(c)
    pred, gt = _on_device(c)
    got = _call(pred, gt, c["classes"], 0xFF, **kw)
    again = _call(pred, gt, c["classes"], 0xFF, **kw)
    for a, b in zip(got, again):
        assert np.array_equal(a, b)                           # two calls on one input: the same bits
    exp = M.match_ref(c["pred"], c["gt"], c["classes"], **kw)
    for i in range(5):
        for a, b in zip(got, exp):
            assert np.array_equal(a[i], b[i]), i
    tot = got[0].sum(axis=1)
    assert (tot[:, 2] > 0).all() and (tot[:, 1] > tot[:, 2]).all() and (tot[:, 0] > tot[:, 2]).all()   # tp, fp, fn
    assert (tot[:, 3] > tot[:, 2]).all()                      # found and not matched: every branch on every image
    for i in (0, 2, 4):
        alone = _call(pred[i:i + 1].contiguous(), gt[i:i + 1].contiguous(), c["classes"], 0x00, **kw)
        for a, b in zip(alone, got):
            assert np.array_equal(a[0], b[i]), i


def test_status_codes_and_nothing_written():
    c = CASES["seam_33x31"]
    pred, gt = torch.from_numpy(c["pred"]).to(DEV), torch.from_numpy(c["gt"]).to(DEV)
    n, H, W = pred.shape
    f = _lib.match_symbol("vitseg_region_match")
    size = _lib.match_symbol("vitseg_region_match_scratch_bytes")
    need = size(n, H, W)
    assert size(0, H, W) == 0 and size(n, 0, W) == 0 and size(32768, 4, 4) == 0 and size(1, 1 << 16, 1 << 15) == 0
    assert size(32767, 1, 1) > 0

    def refused(code, *, shape=(n, H, W), classes=(1, 2), K=None, conn=4, bg=0, ignore=255, thr=(1, 2), cov=(1, 2),
                scratch_bytes=need, null=()):
        scratch = guarded((scratch_bytes,), torch.uint8, name="scratch")
        scratch.fill_(0xA5)
        stats = guarded((n, 2, 8), torch.int64, name="stats")
        pinfo = guarded((n, H, W, 2), torch.int32, name="pred_info")
        ginfo = guarded((n, H, W, 2), torch.int32, name="gt_info")
        snap = snapshot(pred, gt, stats, pinfo, ginfo, scratch)
        cls = (ctypes.c_int32 * len(classes))(*classes)
        ptr = lambda which, t: None if which in null else t.data_ptr()
        rc = f(ptr("pred", pred), ptr("gt", gt), *shape, None if "classes" in null else cls, len(classes) if K is None else K,
               conn, bg, ignore, *thr, *cov, ptr("stats", stats), pinfo.data_ptr(), ginfo.data_ptr(), ptr("scratch", scratch),
               scratch.numel(), _stream())
        torch.cuda.synchronize()
        assert rc == code and _lib.lib().vitseg_last_error()
        check(stats, pinfo, ginfo, scratch)
        unchanged(snap)

    for which in ("pred", "gt", "classes", "stats", "scratch"):
        refused(_lib.EINVAL, null=(which,))
    for conn in (0, 6):
        refused(_lib.EINVAL, conn=conn)
    for bg in (-1, 256):
        refused(_lib.EINVAL, bg=bg)
    for ignore in (-2, 256, 0, 2):            # out of range, the background, one of the classes
        refused(_lib.EINVAL, ignore=ignore)
    for classes in ((1, 256), (-1, 2), (0, 1), (1, 1)):
        refused(_lib.EINVAL, classes=classes)
    for thr in ((1, 3), (499, 1000), (2, 2), (3, 2), (501, 1001), (0, 0), (1, 0), (-1, -2)):
        refused(_lib.EINVAL, thr=thr)
    for cov in ((0, 2), (3, 2), (1, 1001), (-1, 2), (1, 0)):
        refused(_lib.EINVAL, cov=cov)
    for shape in ((0, H, W), (n, 0, W), (n, H, -1), (32768, H, W), (n, 1 << 16, 1 << 15)):
        refused(_lib.ESHAPE, shape=shape)
    for K in (0, 257, -1):
        refused(_lib.ESHAPE, K=K)
    refused(_lib.EWORKSPACE, scratch_bytes=need - 1)


def test_region_metrics_on_a_ground_truth_of_another_size():
    S = 96
    pred, gt = M.pair_maps(41, S, S, 5, n=2)
    big = gt[:, nearest_table(S, 130, NEAREST_PIL)][:, :, nearest_table(S, 171, NEAREST_PIL)]   # a ground truth of another size
    yi, xi = nearest_table(130, S, NEAREST_PIL), nearest_table(171, S, NEAREST_PIL)
    small = big[:, yi][:, :, xi]
    ev = metrics.Evaluator(5, DEV)
    for gt_in in (small, big):
        for kw in (dict(), dict(classes=[3, 1], iou_threshold=0.6, coverage=0.25, connectivity=8, ignore_label=255),
                   dict(background=2, ignore_label=255)):
            classes = kw.get("classes", [c for c in range(5) if c != kw.get("background", 0)])
            ref_kw = dict(connectivity=kw.get("connectivity", 4), background=kw.get("background", 0),
                          ignore_label=kw.get("ignore_label") or -1)
            thr = metrics.iou_threshold_fraction(kw.get("iou_threshold", 0.5))
            cov = metrics.coverage_fraction(kw.get("coverage", 0.5))
            stats, pinfo, ginfo = M.match_ref(pred, small, classes, thr=thr, cov=cov, **ref_kw)
            got = ev.region_metrics(torch.from_numpy(pred), torch.from_numpy(gt_in), return_matches=True, **kw)
            exp_rows = metrics.matches_from_stats(stats)
            assert len(got) == 2
            for i, d in enumerate(got):
                assert list(d["per_class"]) == classes and np.array_equal(d["stats"], stats[i])
                assert all(d["per_class"][c] == pytest.approx(e, nan_ok=True) for c, e in zip(classes, exp_rows[i]))
                for key in metrics.REGION_KEYS:
                    vals = [e[key] for e in exp_rows[i]]
                    want = float("nan") if np.isnan(vals).all() else float(np.nanmean(vals))
                    assert d[key] == pytest.approx(want, rel=1e-12, nan_ok=True), key
                exp = M.joined_tables(pred[i], small[i], pinfo[i], ginfo[i], classes, **ref_kw)
                for side in ("pred", "gt"):
                    t = d["matches"][side]
                    assert t.dtype == np.int32 and np.array_equal(t, exp[side]), side
                # the rows are region_boxes' own, and the partners point at one another
                masked = np.where(small[i] == 255, ref_kw["background"], small[i]) if ref_kw["ignore_label"] >= 0 else small[i]
                for side, m in (("pred", pred[i]), ("gt", masked.astype(np.uint8))):
                    boxes = regions.region_boxes(m, background=ref_kw["background"], connectivity=ref_kw["connectivity"])
                    keep = {tuple(r) for r in boxes.tolist()}
                    assert all(tuple(r[:7]) in keep for r in d["matches"][side].tolist())
                pm, gm = d["matches"]["pred"], d["matches"]["gt"]
                for r, row in enumerate(pm):
                    assert row[7] == -1 or (gm[row[7], 7] == r and gm[row[7], 0] == row[0])
                assert (pm[:, 7] >= 0).sum() == (gm[:, 7] >= 0).sum() == stats[i, :, 2].sum() > 0
    plain = ev.region_metrics(torch.from_numpy(pred), torch.from_numpy(small))
    assert "matches" not in plain[0] and list(plain[0]["per_class"]) == [1, 2, 3, 4]


def _load_script(rel):
    """model/<dir>/<script>.py as a module; its `from classes import ...` resolves in its own directory."""
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


@pytest.mark.parametrize("rel,extra", [("model/CE/datasetTestViTmodel.py", ["--num-classes", "3"]),
                                       ("model/PAED/ViTscriptTest.py", ["--patch-size", "16", "--hidden-size", "192", "--layers",
                                                                        "1", "--heads", "3"])])
def test_evaluation_scripts_write_the_region_file(rel, extra, monkeypatch, tmp_path):
    mod = _load_script(rel)
    monkeypatch.chdir(tmp_path)
    common = [rel, "--ids", "1", "--num-batches", "2", "--batch-size", "2"] + extra
    monkeypatch.setattr(sys, "argv", common + ["--out", "plain"])
    mod.main()
    monkeypatch.setattr(sys, "argv", common + ["--out", "with", "--region-metrics", "--region-iou", "0.6", "--region-coverage", "0.25",
                                               "--region-connectivity", "8", "--min-area", "4"])
    mod.main()
    (name,) = os.listdir(tmp_path / "plain")
    assert os.listdir(tmp_path / "plain" / name) == [f"{name}_metrics.csv"]       # without the flag: the files of before
    assert sorted(os.listdir(tmp_path / "with" / name)) == [f"{name}_metrics.csv", f"{name}_region_metrics.csv"]
    rows = list(csv.reader(open(tmp_path / "with" / name / f"{name}_region_metrics.csv", newline="")))
    assert rows[0] == metrics.REGION_CSV_COLUMNS
    col = {k: i for i, k in enumerate(rows[0])}
    ints = ["N_GT", "N_Pred", "TP", "GT_Found", "Pred_Confirmed", "Sum_Q", "Sum_I", "Sum_U"]
    per_image = [r for r in rows[1:] if r[col["Batch_Num"]] != "pooled"]
    pooled = [r for r in rows[1:] if r[col["Batch_Num"]] == "pooled"]
    classes = sorted({int(r[col["Class"]]) for r in per_image})
    assert classes and len(per_image) == 4 * len(classes) and [int(r[col["Class"]]) for r in pooled] == classes
    assert all(r[col["IoU_Threshold"]] == "0.6" and r[col["Coverage"]] == "0.25" for r in rows[1:])
    stats = np.array([[[int(r[col[k]]) for k in ints] for r in per_image if int(r[col["Class"]]) == c] for c in classes])
    want = metrics.pool_region_stats([stats.transpose(1, 0, 2)])                  # [images, classes, 8]
    assert np.array_equal(want, np.array([[int(r[col[k]]) for k in ints] for r in pooled]))
    for r, m in zip(pooled, metrics.matches_from_stats(want)):
        for k, key in (("PQ", "pq"), ("SQ", "sq"), ("RQ", "rq"), ("Recall", "recall"), ("Found_Rate", "found_rate")):
            assert float(r[col[k]]) == pytest.approx(m[key], rel=1e-12, nan_ok=True)
        assert int(r[col["FP"]]) == m["fp"] and int(r[col["FN"]]) == m["fn"]
    assert want[:, 0].sum() > 0                                                   # the synthetic ground truth has regions
