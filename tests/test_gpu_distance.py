"""GPU (-m gpu): boundary-distance statistics on the device (vitseg_distance_stats, Evaluator.distance_metrics) against the
numpy restatement tests/distance_ref.py and the committed scipy goldens.  Counts, maxima and order statistics must be equal;
an fp64 sum of k roots must lie within 2 (k + 1) 2^-53 relative of numpy's (any-order summation of k non-negative doubles
and half an ulp per root, on both sides).  Every call has guarded outputs and scratch, the scratch pre-filled with 0x00 and
with 0xFF, and its inputs checked unchanged."""
import ctypes
import os

import numpy as np
import pytest
import torch

import distance_ref as R
from guard import check, guarded, snapshot, unchanged
from visiontransformer_amd import _lib, metrics
from visiontransformer_amd.preprocess import NEAREST_PIL, nearest_table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "distance", "distance.npz"))
PCTS = R.GOLDEN_PERCENTILES   # 0, 50, 95, 100


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, name):
    a = np.ascontiguousarray(a)
    return guarded(a.shape, torch.uint8, torch.from_numpy(a).to(DEV), name=name)


def _call(pred, gt, classes, mode, pct, fill):
    """One vitseg_distance_stats call through the C ABI: guarded device inputs [n, H, W] -> (stats_i, stats_f) numpy."""
    n, H, W = pred.shape
    K = len(classes)
    nbytes = _lib.distance_symbol("vitseg_distance_scratch_bytes")(n, H, W)
    assert nbytes > 0
    scratch = guarded((nbytes,), torch.uint8, name="scratch")
    scratch.fill_(fill)
    si = guarded((n, K, 6), torch.int64, name="stats_i")
    sf = guarded((n, K, 2), torch.float64, name="stats_f")
    snap = snapshot(pred, gt)
    cls = (ctypes.c_int32 * K)(*classes)
    _lib.check(_lib.distance_symbol("vitseg_distance_stats")(pred.data_ptr(), gt.data_ptr(), n, H, W, cls, K, mode, pct[0],
                                                             pct[1], si.data_ptr(), sf.data_ptr(), scratch.data_ptr(), nbytes,
                                                             _stream()))
    torch.cuda.synchronize()
    check(scratch, si, sf, pred, gt)
    unchanged(snap)
    return si.cpu().numpy(), sf.cpu().numpy()


def _assert_stats(got, exp, what):
    (gi, gf), (ei, ef) = got, exp
    assert gi.shape == ei.shape and gf.shape == ef.shape, what
    assert np.array_equal(gi, ei), (what, np.argwhere(gi != ei)[:4], gi[gi != ei][:4], ei[gi != ei][:4])
    assert np.isfinite(gf).all(), what
    tol = R.sum_bound(ei[..., :2].astype(np.float64)) * np.abs(ef)   # sumAP has n terms, sumPA m
    bad = np.abs(gf - ef) > tol
    assert not bad.any(), (what, gf[bad][:4], ef[bad][:4])


def _run_all(gt, pred, classes, route, what):
    """Both modes, the four percentiles, both scratch fills against the restatement; returns the results per (mode, pct)."""
    g, p = _dev(gt, "gt"), _dev(pred, "pred")
    out = {}
    for mode in (0, 1):
        exp = R.stats_ref_multi(gt, pred, classes, mode, PCTS, route)
        for pct in PCTS:
            for fill in (0x00, 0xFF):   # a scratch word read before it is written would tell the two fills apart
                got = _call(p, g, classes, mode, pct, fill)
                _assert_stats(got, exp[pct], (what, mode, pct, fill))
                if fill:
                    assert np.array_equal(got[0], out[mode, pct][0]) and np.array_equal(got[1], out[mode, pct][1])
                out[mode, pct] = got
    return out


@pytest.mark.parametrize("H,W", R.SIZES)
def test_every_mask_kind_at_every_size(H, W):
    """The ten mask kinds as one batch, classes 0, 1 and 7 (absent from both maps)."""
    cases = R.mask_cases(H, W, seed=H + W)
    gt = np.stack([g for g, _ in cases.values()])
    pred = np.stack([p for _, p in cases.values()])
    _run_all(gt, pred, [0, 1, 7], "brute" if H * W <= 300 else "edt", list(cases))


def test_batch_of_three_at_224_with_three_classes():
    gt = np.stack([R.class_map(20 + i, 224, 224, 3) for i in range(3)])
    pred = np.stack([R.shifted(gt[0], 3, -2), R.class_map(31, 224, 224, 3), np.where(gt[2] == 2, 0, gt[2]).astype(np.uint8)])
    _run_all(gt, pred, [0, 1, 2], "edt", "224")


@pytest.mark.parametrize("name", sorted(R.golden_cases()))
def test_golden_cases_through_the_c_abi(name):
    """The committed scipy results, with the cases whose lo and hi straddle a 10-bit bucket boundary of the select (2^10 and
    2^20) and the plateau of ties at the rank."""
    gt, pred, classes = Z[f"{name}.gt"], Z[f"{name}.pred"], [int(c) for c in Z[f"{name}.classes"]]
    g, p = _dev(gt[None], "gt"), _dev(pred[None], "pred")
    for mode in (0, 1):
        for num, den in PCTS:
            exp = Z[f"{name}.m{mode}.p{num}_{den}.i"][None], Z[f"{name}.m{mode}.p{num}_{den}.f"][None]
            for fill in (0x00, 0xFF):
                _assert_stats(_call(p, g, classes, mode, (num, den), fill), exp, (name, mode, num, den, fill))


def test_more_than_256_partials_per_plane():
    """1100 x 1000: 269 blocks per plane, so the final reduce walks its partials in more than one stride.  gt = some pixels of
    column 0, pred = the whole last column: every distance follows from the 1-D distance along the column."""
    import sdf_ref
    H, W = 1100, 1000
    rows = np.random.RandomState(8).rand(H) < 0.01
    rows[17] = True
    gt, pred = np.zeros((1, H, W), np.uint8), np.zeros((1, H, W), np.uint8)
    gt[0, rows, 0] = 1
    pred[0, :, W - 1] = 1
    g1 = sdf_ref.column_pass(rows[:, None])[:, 0]   # rows to the nearest gt row
    ap = np.full(int(rows.sum()), (W - 1) ** 2, np.int64)
    pa = (W - 1) ** 2 + g1 ** 2
    sf = np.array([np.sqrt(ap.astype(np.float64)).sum(), np.sqrt(pa.astype(np.float64)).sum()])
    g, p = _dev(gt, "gt"), _dev(pred, "pred")
    for mode in (0, 1):   # one-pixel-wide columns are their own borders
        for pct in PCTS:
            si = R.stats_of_fields((len(ap), len(pa), ap, pa, sf), *pct)[0]
            _assert_stats(_call(p, g, [1], mode, pct, 0xFF if mode else 0x00), (si[None, None], sf[None, None]), (mode, pct))


def test_an_image_gives_the_same_bits_alone_in_a_batch_and_on_every_call():
    H, W = 61, 77
    mid = (R.random_map(1, H, W, 0.3), R.random_map(2, H, W, 0.3))
    gt = np.stack([R.random_map(3, H, W, 0.7), mid[0], np.zeros((H, W), np.uint8)])
    pred = np.stack([R.random_map(4, H, W, 0.02), mid[1], R.random_map(5, H, W, 0.3)])
    g3, p3, g1, p1 = _dev(gt, "gt"), _dev(pred, "pred"), _dev(mid[0][None], "gt"), _dev(mid[1][None], "pred")
    for mode in (0, 1):
        for pct in PCTS:
            bi, bf = _call(p3, g3, [0, 1], mode, pct, 0x00)
            bi2, bf2 = _call(p3, g3, [0, 1], mode, pct, 0xFF)
            assert np.array_equal(bi, bi2) and np.array_equal(bf.view(np.int64), bf2.view(np.int64))
            ai, af = _call(p1, g1, [0, 1], mode, pct, 0xFF)
            assert np.array_equal(ai[0], bi[1]) and np.array_equal(af[0].view(np.int64), bf[1].view(np.int64))


def test_error_statuses_leave_the_outputs_untouched():
    f = _lib.distance_symbol("vitseg_distance_scratch_bytes")
    fn = _lib.distance_symbol("vitseg_distance_stats")
    assert f(0, 8, 8) == 0 and f(2, 0, 8) == 0 and f(2, 8, 16385) == 0 and f(32768, 1, 1) == 0
    m = torch.zeros(2, 8, 8, dtype=torch.uint8, device=DEV)
    si = torch.full((2, 2, 6), 7, dtype=torch.int64, device=DEV)
    sf = torch.full((2, 2, 2), 7.0, dtype=torch.float64, device=DEV)
    sc = torch.zeros(f(2, 8, 8), dtype=torch.uint8, device=DEV)
    st = _stream()
    ok, c256 = (ctypes.c_int32 * 2)(0, 1), (ctypes.c_int32 * 2)(0, 256)

    def call(pred=m, gt=m, n=2, H=8, W=8, classes=ok, K=2, mode=0, num=95, den=100, out_i=si, out_f=sf, scratch=sc, nbytes=None):
        p = lambda t: None if t is None else t.data_ptr()
        return fn(p(pred), p(gt), n, H, W, classes, K, mode, num, den, p(out_i), p(out_f), p(scratch),
                  sc.numel() if nbytes is None else nbytes, st)

    assert call(mode=2) == _lib.EINVAL and call(mode=-1) == _lib.EINVAL
    assert call(classes=c256) == _lib.EINVAL
    assert call(num=101, den=100) == _lib.EINVAL and call(num=-1) == _lib.EINVAL
    assert call(den=0, num=0) == _lib.EINVAL and call(num=1001, den=1001) == _lib.EINVAL
    assert call(pred=None) == _lib.EINVAL and call(out_f=None) == _lib.EINVAL and call(scratch=None) == _lib.EINVAL
    assert call(classes=None) == _lib.EINVAL
    assert call(n=32768) == _lib.ESHAPE and call(n=0) == _lib.ESHAPE
    assert call(H=0) == _lib.ESHAPE and call(W=16385) == _lib.ESHAPE and call(K=0) == _lib.ESHAPE and call(K=257) == _lib.ESHAPE
    assert call(nbytes=sc.numel() - 1) == _lib.EWORKSPACE   # one byte short
    torch.cuda.synchronize()
    assert (si == 7).all() and (sf == 7.0).all()   # nothing was launched
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert (si[..., :2] != 7).all()


def _approx_rows(got, exp):
    assert len(got) == len(exp)
    for a, b in zip(got, exp):
        assert a.keys() == b.keys()
        for k in a:
            assert a[k] == pytest.approx(b[k], rel=1e-12, abs=0.0, nan_ok=True), (k, a[k], b[k])


def test_evaluator_distance_metrics_end_to_end():
    num_classes, S = 3, 96
    pred = np.stack([R.class_map(40 + i, S, S, num_classes) for i in range(2)])
    big = np.stack([R.class_map(50 + i, 130, 171, num_classes) for i in range(2)])   # a ground truth of another size
    yi, xi = nearest_table(130, S, NEAREST_PIL), nearest_table(171, S, NEAREST_PIL)
    small = big[:, yi][:, :, xi]
    ev = metrics.Evaluator(num_classes, DEV)
    for gt_in, gt_ref in [(small, small), (big, small)]:
        for mode, pctile, classes in [("sets", 95, None), ("borders", 50, [2, 0]), ("sets", 99.5, [1, 5])]:
            num, den = metrics.percentile_fraction(pctile)
            cl = list(range(num_classes)) if classes is None else classes
            si, sf = R.stats_ref(gt_ref, pred, cl, R.MODES[mode], num, den, "edt")
            exp = metrics.distances_from_stats(si, sf, num, den)
            got = ev.distance_metrics(torch.from_numpy(pred), torch.from_numpy(gt_in), classes=classes, mode=mode,
                                      percentile=pctile)
            assert len(got) == 2
            for i, d in enumerate(got):
                assert list(d["per_class"]) == cl
                _approx_rows([d["per_class"][c] for c in cl], exp[i])
                for key in metrics.DISTANCE_KEYS:
                    vals = [r[key] for r in exp[i]]
                    want = float("nan") if np.isnan(vals).all() else float(np.nanmean(vals))
                    assert d[key] == pytest.approx(want, rel=1e-12, nan_ok=True), key
    with pytest.raises(ValueError):
        ev.distance_metrics(torch.from_numpy(pred), torch.from_numpy(small), mode="surface")
    with pytest.raises(ValueError):
        ev.distance_metrics(torch.from_numpy(pred), torch.from_numpy(small), classes=[256])
    with pytest.raises(ValueError):
        ev.distance_metrics(torch.from_numpy(pred), torch.from_numpy(small[:1]))


def test_evaluate_to_csv_writes_the_second_file_and_leaves_the_first(tmp_path):
    import csv
    from visiontransformer_amd import scripts
    from visiontransformer_amd.model import ViTSegmentationModel
    model = ViTSegmentationModel(3, 16, 192, 1, 3, image_size=224, device=DEV).eval()
    batches = scripts.ce_batches(model.cfg, 4, 2, seed=3)
    info = (7, "ID7P16H192A3", 16, 192, 1, 3)
    plain, both = str(tmp_path / "a" / "m_metrics.csv"), str(tmp_path / "b" / "m_metrics.csv")
    scripts.evaluate_to_csv(model, batches, info, plain, 3, 2, DEV)
    scripts.evaluate_to_csv(model, batches, info, both, 3, 2, DEV, distance_mode="borders")
    assert os.listdir(tmp_path / "a") == ["m_metrics.csv"]
    assert sorted(os.listdir(tmp_path / "b")) == ["m_distance_metrics.csv", "m_metrics.csv"]
    read = lambda p: list(csv.reader(open(p, newline="")))
    a, b = read(plain), read(both)
    t = metrics.CSV_COLUMNS.index("Inference_Time")
    assert a[0] == b[0] == metrics.CSV_COLUMNS and len(a) == 5
    assert [r[:t] + r[t + 1:] for r in a] == [r[:t] + r[t + 1:] for r in b]   # the same but for the measured time
    d = read(str(tmp_path / "b" / "m_distance_metrics.csv"))
    assert d[0] == metrics.DISTANCE_CSV_COLUMNS and len(d) == 5
    ev = metrics.Evaluator(3, DEV)
    with torch.no_grad():
        mask = model.predict_mask(batches[1][0].to(DEV))
    gt = batches[1][1].reshape(2, batches[1][1].shape[-2], batches[1][1].shape[-1])
    exp = ev.distance_metrics(mask, gt, mode="borders")
    for row, m in zip(d[3:], exp):
        assert row[:6] == ["7", "ID7P16H192A3", "1", row[3], "borders", "95"]
        for col, key in [(6, "paed"), (7, "hausdorff"), (8, "hd_percentile"), (9, "assd")]:
            assert float(row[col]) == pytest.approx(m[key], rel=1e-12, nan_ok=True)
