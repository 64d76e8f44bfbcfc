"""GPU (-m gpu): Zhang-Suen skeletons and the crack statistics on the device (vitseg_skeleton, vitseg_skeleton_stats,
skeleton.skeletonize, Evaluator.crack_metrics) against the per-pixel numpy restatement tests/skeleton_ref.py.  Skeletons and
pass counts must be bitwise equal, by the resident route and by the global one; the integers of the statistics equal, and an
fp64 sum of k roots within 2 (k + 1) 2^-53 relative of numpy's (the bound test_gpu_distance.py derives, reused here).  Every
call has guarded outputs and scratch, the scratch pre-filled with 0x00 and with 0xFF, and its inputs checked unchanged."""
import ctypes
import os

import numpy as np
import pytest
import torch

import skeleton_ref as R
from distance_ref import sum_bound
from guard import check, guarded, snapshot, unchanged
from visiontransformer_amd import _lib, metrics, skeleton
from visiontransformer_amd.preprocess import NEAREST_PIL, nearest_table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AUTO, RESIDENT, GLOBAL = 0, 1, 2
LDS_CAP = 160 * 1024   # what the resident kernel's registers are sized for (include/vitseg.h)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, name):
    a = np.ascontiguousarray(a)
    return guarded(a.shape, torch.uint8, torch.from_numpy(a).to(DEV), name=name)


def _lds_limit():
    """The resident route's budget, from the device attribute the library reads (hipDeviceAttributeMaxSharedMemoryPerBlock)."""
    return min(int(torch.cuda.get_device_properties(0).shared_memory_per_block), LDS_CAP)


def _resident_bytes(H, W):
    return 4 * ((H + 2) * ((W + 31) // 32 + 1) + 4)


def _fits(H, W):
    return _resident_bytes(H, W) <= _lds_limit()


def _call(mask, route, fill, want_passes=True):
    """One vitseg_skeleton call through the C ABI: guarded device mask [n, H, W] -> (skeleton, passes) numpy."""
    n, H, W = mask.shape
    nbytes = _lib.skeleton_symbol("vitseg_skeleton_scratch_bytes")(n, H, W, route)
    assert nbytes > 0
    scratch = guarded((nbytes,), torch.uint8, name="scratch")
    scratch.fill_(fill)
    out = guarded((n, H, W), torch.uint8, name="skeleton")
    passes = guarded((n,), torch.int32, name="passes") if want_passes else None
    snap = snapshot(mask)
    _lib.check(_lib.skeleton_symbol("vitseg_skeleton")(mask.data_ptr(), n, H, W, route, out.data_ptr(),
                                                       None if passes is None else passes.data_ptr(), scratch.data_ptr(),
                                                       nbytes, _stream()))
    torch.cuda.synchronize()
    check(scratch, out, passes, mask)
    unchanged(snap)
    return out.cpu().numpy(), None if passes is None else passes.cpu().numpy()


def _check_batch(masks, what, routes=None, exp=None):
    """Both routes (where the plane fits the resident one) and both scratch fills against the restatement."""
    masks = np.ascontiguousarray(masks)
    es, ep = R.skeleton_ref(masks) if exp is None else exp
    m = _dev(masks, "mask")
    H, W = masks.shape[1:]
    if routes is None:
        routes = (AUTO, RESIDENT, GLOBAL) if _fits(H, W) else (AUTO, GLOBAL)
    for route in routes:
        for fill in (0x00, 0xFF):   # a scratch word read before it is written would tell the two fills apart
            gs, gp = _call(m, route, fill)
            assert np.array_equal(gs, es), (what, route, fill, np.argwhere(gs != es)[:4])
            assert np.array_equal(gp, ep), (what, route, fill, gp, ep)
    return es, ep


@pytest.mark.parametrize("W", [1, 2, 31, 32, 33, 63, 64, 65, 100])
def test_every_generator_at_the_word_edges(W):
    for H in (1, 2, 3, 33):
        cases = R.all_masks(H, W, seed=H + W)
        _check_batch(np.stack(list(cases.values())), (H, W, list(cases)))


def _edge_cases(H, W):
    """Structures on the word boundaries of a row: bands and diagonals across columns 31 / 32 and 63 / 64, set pixels in the
    last column (in a partial word when W % 32 != 0) beside set pixels in column 0 of the next row, which are no neighbours."""
    out = []
    for x0 in (31, 63):
        if x0 + 1 < W:
            band = np.zeros((H, W), np.uint8)
            band[:, x0 - 1:x0 + 3] = 1             # a vertical band 4 wide with the boundary in its middle
            out.append(band)
            flat = np.zeros((H, W), np.uint8)
            flat[H // 2 - 1:H // 2 + 2, max(x0 - 8, 0):min(x0 + 10, W)] = 1   # a horizontal band across it
            out.append(flat)
            d = np.zeros((H, W), np.uint8)
            k = np.arange(min(H, 8))
            d[k, np.minimum(x0 - 3 + k, W - 1)] = 1   # a diagonal across it
            d[k, np.minimum(x0 - 2 + k, W - 1)] = 1   # two pixels wide
            out.append(d)
    last = np.zeros((H, W), np.uint8)
    last[:, W - 1] = 1                               # the last column, and column 0: the ends of consecutive rows
    last[:, 0] = 1
    out.append(last)
    wrap = np.zeros((H, W), np.uint8)
    wrap[1:H - 1:3, max(W - 3, 0):] = 1              # short bars ending in the last column ...
    wrap[2:H - 1:3, :min(3, W)] = 1                  # ... and bars starting in column 0 one row below
    out.append(wrap)
    thick = np.zeros((H, W), np.uint8)
    thick[:, max(W - 4, 0):] = 1                     # a band along the right edge
    out.append(thick)
    return np.stack(out)


@pytest.mark.parametrize("W", [32, 33, 64, 65, 100])
def test_structures_on_word_boundaries_and_in_the_last_column(W):
    _check_batch(_edge_cases(12, W), W)


def test_different_stopping_times_in_one_batch():
    """Empty and single pixel (1 pass), a thin crack (a few) and the full 80 x 80 square (41 passes: the global route reads its
    flags after 16, 32 and 48) in one call; every plane reports its own count."""
    masks = np.stack([R.empty(80, 80), R.single(80, 80), R.crack(80, 80, 4, 1), R.full(80, 80)])
    es, ep = _check_batch(masks, "stopping times")
    assert ep[0] == 1 and ep[1] == 1 and 1 < ep[2] < 8 and ep[3] == 41 and es[3].sum() == 1


def test_an_image_gives_the_same_bits_alone_and_in_a_batch():
    H, W = 61, 77
    masks = np.stack([R.noise(H, W, 1, 0.8), R.crack(H, W, 2, 2), R.blobs(H, W, 3), R.empty(H, W)])
    exp = R.skeleton_ref(masks)
    _check_batch(masks, "batch", exp=exp)
    for i in range(len(masks)):
        _check_batch(masks[i:i + 1], ("alone", i), exp=(exp[0][i:i + 1], exp[1][i:i + 1]))
    m = _dev(masks, "mask")
    gs, gp = _call(m, AUTO, 0xFF, want_passes=False)   # passes is optional
    assert gp is None and np.array_equal(gs, exp[0])


def test_the_resident_routes_limit():
    """The tallest 1024-wide plane the resident route takes on this device, and the next one up: automatic routing must give
    the restatement's bits on both sides of the limit, and route 1 must refuse the larger plane."""
    W, stride = 1024, 33
    H = (_lds_limit() // 4 - 4) // stride - 2
    assert _fits(H, W) and not _fits(H + 1, W)
    f = _lib.skeleton_symbol("vitseg_skeleton_scratch_bytes")
    g = _lib.skeleton_symbol("vitseg_skeleton_stats_scratch_bytes")
    assert f(1, H, W, RESIDENT) > 0 and f(1, H + 1, W, RESIDENT) == 0 and g(1, H + 1, W, RESIDENT) == 0
    assert f(1, H, W, AUTO) == f(1, H, W, RESIDENT) and f(1, H + 1, W, AUTO) == f(1, H + 1, W, GLOBAL) > 0
    big = R.crack(H + 1, W, 9, 2)[None]
    big[0, -1, ::7] = 1                                   # the last row counts too
    exp = R.skeleton_ref(big)
    _check_batch(big[:, :H], "largest resident", routes=(RESIDENT, AUTO), exp=R.skeleton_ref(big[:, :H]))
    _check_batch(big, "one row more", routes=(AUTO,), exp=exp)
    m = _dev(big, "mask")
    out = guarded((1, H + 1, W), torch.uint8, name="skeleton")
    out.fill_(7)
    sc = guarded((f(1, H + 1, W, GLOBAL),), torch.uint8, name="scratch")
    rc = _lib.skeleton_symbol("vitseg_skeleton")(m.data_ptr(), 1, H + 1, W, RESIDENT, out.data_ptr(), None, sc.data_ptr(),
                                                 sc.numel(), _stream())
    torch.cuda.synchronize()
    assert rc == _lib.ESHAPE and (out == 7).all()
    check(out, sc)


# ---- statistics ----

def _stats_call(pred, gt, classes, route, fill):
    n, H, W = pred.shape
    K = len(classes)
    nbytes = _lib.skeleton_symbol("vitseg_skeleton_stats_scratch_bytes")(n, H, W, route)
    assert nbytes > 0
    scratch = guarded((nbytes,), torch.uint8, name="scratch")
    scratch.fill_(fill)
    si = guarded((n, K, 10), torch.int64, name="stats_i")
    sf = guarded((n, K, 2), torch.float64, name="stats_f")
    snap = snapshot(pred, gt)
    cls = (ctypes.c_int32 * K)(*classes)
    _lib.check(_lib.skeleton_symbol("vitseg_skeleton_stats")(pred.data_ptr(), gt.data_ptr(), n, H, W, cls, K, route,
                                                             si.data_ptr(), sf.data_ptr(), scratch.data_ptr(), nbytes,
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
    tol = sum_bound(ei[..., 2:4].astype(np.float64)) * np.abs(ef)   # the sums run over the |S_G| and |S_P| skeleton pixels
    bad = np.abs(gf - ef) > tol
    assert not bad.any(), (what, gf[bad][:4], ef[bad][:4])


def _crack_maps(S):
    gt = np.stack([R.crack_map(S, S, 10 + i) for i in range(3)])
    pred = np.stack([np.roll(gt[0], 2, axis=0), R.crack_map(S, S, 21), np.where(gt[2] == 2, 0, gt[2]).astype(np.uint8)])
    return gt, pred


@pytest.mark.parametrize("S", [224, 512])
def test_stats_of_three_class_maps(S):
    """Three maps of thin structures, classes 1, 2 and 7 (absent from both maps), by both routes."""
    gt, pred = _crack_maps(S)
    classes = [1, 2, 7]
    exp = R.stats_ref(gt, pred, classes)
    assert (exp[0][:, 2, :6] == 0).all() and (exp[0][:, 2, 6:8] == -1).all() and (exp[0][:, :2, 2] > S // 2).all()
    g, p = _dev(gt, "gt"), _dev(pred, "pred")
    first = None
    for route in ((AUTO, RESIDENT, GLOBAL) if _fits(S, S) else (AUTO, GLOBAL)):
        for fill in (0x00, 0xFF):
            got = _stats_call(p, g, classes, route, fill)
            _assert_stats(got, exp, (S, route, fill))
            if first is None:
                first = got
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1].view(np.int64), first[1].view(np.int64))
    alone = _stats_call(_dev(pred[1:2], "pred"), _dev(gt[1:2], "gt"), classes, AUTO, 0xFF)
    assert np.array_equal(alone[0][0], first[0][1]) and np.array_equal(alone[1][0].view(np.int64), first[1][1].view(np.int64))


def test_stats_of_small_odd_maps_and_a_full_plane():
    """13 x 21 and 61 x 77 (partial words, more than one reduction chunk at neither; P % 4 != 0 at both), a class that fills a
    whole image (the distance to the virtual point outside) and one that is absent."""
    for H, W in [(13, 21), (61, 77)]:
        gt = np.stack([R.crack_map(H, W, 1), np.full((H, W), 3, np.uint8), (R.blobs(H, W, 5) * 3).astype(np.uint8)])
        pred = np.stack([R.crack_map(H, W, 2), np.full((H, W), 3, np.uint8), (R.noise(H, W, 6, 0.8) * 3).astype(np.uint8)])
        classes = [3, 1, 0, 9]
        exp = R.stats_ref(gt, pred, classes)
        g, p = _dev(gt, "gt"), _dev(pred, "pred")
        for route in (RESIDENT, GLOBAL):
            for fill in (0x00, 0xFF):
                _assert_stats(_stats_call(p, g, classes, route, fill), exp, (H, W, route, fill))


# ---- the Python surface ----

def test_skeletonize_and_crackseg():
    masks = np.stack([R.crack(40, 70, 1, 2), R.blobs(40, 70, 2), R.full(40, 70)])
    es, ep = R.skeleton_ref(masks)
    out = skeleton.skeletonize(masks)                                      # numpy in, numpy out
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and np.array_equal(out, es)
    out, passes = skeleton.skeletonize(masks, route="global", return_passes=True)
    assert np.array_equal(out, es) and np.array_equal(passes, ep)
    one = skeleton.skeletonize(masks[0] * 255)                             # [H, W]
    assert one.shape == (40, 70) and np.array_equal(one, es[0])
    t = torch.from_numpy(masks).to(DEV)
    tout = skeleton.skeletonize(t, route="resident")                       # a device tensor stays on the device
    assert tout.is_cuda and tout.dtype == torch.uint8 and np.array_equal(tout.cpu().numpy(), es)
    assert np.array_equal(skeleton.skeletonize(t.bool()).cpu().numpy(), es)
    assert np.array_equal(skeleton.skeletonize(t.float() * 0.25).cpu().numpy(), es)   # any other dtype: != 0
    prob = torch.from_numpy(masks[0].astype(np.float32) * 0.9 + 0.05)      # 0.05 / 0.95: thresholded at 0.5
    sk = skeleton.CrackSeg.skeletonize(prob)
    assert sk.dtype == torch.float32 and sk.device == prob.device and np.array_equal(sk.numpy(), es[0].astype(np.float32))
    sk = skeleton.CrackSeg.skeletonize(prob.to(DEV))
    assert sk.is_cuda and np.array_equal(sk.cpu().numpy(), es[0].astype(np.float32))
    with pytest.raises(ValueError):
        skeleton.skeletonize(np.zeros((1, 2000, 2000), np.uint8), route="resident")   # does not fit one workgroup's LDS


def test_evaluator_crack_metrics_end_to_end():
    S = 96
    pred = np.stack([R.crack_map(S, S, 40 + i) for i in range(2)])
    big = np.stack([R.crack_map(130, 171, 50 + i) for i in range(2)])    # a ground truth of another size
    yi, xi = nearest_table(130, S, NEAREST_PIL), nearest_table(171, S, NEAREST_PIL)
    small = big[:, yi][:, :, xi]
    ev = metrics.Evaluator(3, DEV)
    for gt_in, gt_ref in [(small, small), (big, small)]:
        for classes in ([1, 2], [2, 5, 1]):
            si, sf = R.stats_ref(gt_ref, pred, classes)
            exp = metrics.crack_from_stats(si, sf)
            gi, gf = ev.skeleton_stats(torch.from_numpy(pred), torch.from_numpy(gt_in), classes)
            _assert_stats((gi.cpu().numpy(), gf.cpu().numpy()), (si, sf), classes)
            got = ev.crack_metrics(torch.from_numpy(pred), torch.from_numpy(gt_in), classes=classes)
            assert len(got) == 2
            for i, d in enumerate(got):
                assert list(d["per_class"]) == classes
                for c, e in zip(classes, exp[i]):
                    r = d["per_class"][c]
                    assert r.keys() == e.keys()
                    for key in r:
                        assert r[key] == pytest.approx(e[key], rel=1e-12, abs=0.0, nan_ok=True), (c, key)
                for key in metrics.CRACK_KEYS:
                    vals = [float(r[key]) for r in exp[i]]
                    want = float("nan") if np.isnan(vals).all() else float(np.nanmean(vals))
                    assert d[key] == pytest.approx(want, rel=1e-12, nan_ok=True), key
    assert list(ev.crack_metrics(torch.from_numpy(pred), torch.from_numpy(small))[0]["per_class"]) == [0, 1, 2]
    with pytest.raises(ValueError):
        ev.crack_metrics(torch.from_numpy(pred), torch.from_numpy(small), classes=[256])
    with pytest.raises(ValueError):
        ev.crack_metrics(torch.from_numpy(pred), torch.from_numpy(small[:1]))


def test_evaluate_to_csv_writes_the_crack_file_and_leaves_the_first(tmp_path):
    import csv
    from visiontransformer_amd import scripts
    from visiontransformer_amd.model import ViTSegmentationModel
    model = ViTSegmentationModel(3, 16, 192, 1, 3, image_size=224, device=DEV).eval()
    batches = scripts.ce_batches(model.cfg, 4, 2, seed=3)
    info = (7, "ID7P16H192A3", 16, 192, 1, 3)
    plain, both = str(tmp_path / "a" / "m_metrics.csv"), str(tmp_path / "b" / "m_metrics.csv")
    scripts.evaluate_to_csv(model, batches, info, plain, 3, 2, DEV)
    scripts.evaluate_to_csv(model, batches, info, both, 3, 2, DEV, crack_classes=True)
    assert os.listdir(tmp_path / "a") == ["m_metrics.csv"]
    assert sorted(os.listdir(tmp_path / "b")) == ["m_crack_metrics.csv", "m_metrics.csv"]
    read = lambda p: list(csv.reader(open(p, newline="")))
    a, b = read(plain), read(both)
    t = metrics.CSV_COLUMNS.index("Inference_Time")
    assert [r[:t] + r[t + 1:] for r in a] == [r[:t] + r[t + 1:] for r in b]   # the same but for the measured time
    d = read(str(tmp_path / "b" / "m_crack_metrics.csv"))
    assert d[0] == metrics.CRACK_CSV_COLUMNS and len(d) == 5
    ev = metrics.Evaluator(3, DEV)
    with torch.no_grad():
        mask = model.predict_mask(batches[1][0].to(DEV))
    gt = batches[1][1].reshape(2, batches[1][1].shape[-2], batches[1][1].shape[-1])
    exp = ev.crack_metrics(mask, gt, classes=[1, 2])
    for row, m in zip(d[3:], exp):
        assert row[:3] == ["7", "ID7P16H192A3", "1"]
        for col, key in [(4, "cldice"), (5, "cl_precision"), (6, "cl_sensitivity"), (7, "length_gt"), (8, "length_pred")]:
            assert float(row[col]) == pytest.approx(m[key], rel=1e-12, nan_ok=True)


# ---- error codes ----

def test_error_statuses_leave_the_outputs_untouched():
    f = _lib.skeleton_symbol("vitseg_skeleton_scratch_bytes")
    fs = _lib.skeleton_symbol("vitseg_skeleton_stats_scratch_bytes")
    fn = _lib.skeleton_symbol("vitseg_skeleton")
    fns = _lib.skeleton_symbol("vitseg_skeleton_stats")
    for size in (f, fs):
        assert size(0, 8, 8, 0) == 0 and size(2, 0, 8, 0) == 0 and size(2, 8, 16385, 0) == 0 and size(32768, 1, 1, 0) == 0
        assert size(2, 8, 8, 3) == 0 and size(2, 8, 8, -1) == 0 and size(1, 4096, 4096, RESIDENT) == 0
    m = guarded((2, 8, 8), torch.uint8, "zero", name="mask")
    out = guarded((2, 8, 8), torch.uint8, name="skeleton")
    out.fill_(7)
    ps = guarded((2,), torch.int32, name="passes")
    ps.fill_(7)
    si = guarded((2, 2, 10), torch.int64, name="stats_i")
    si.fill_(7)
    sf = guarded((2, 2, 2), torch.float64, name="stats_f")
    sf.fill_(7.0)
    sc = guarded((max(f(2, 8, 8, GLOBAL), fs(2, 8, 8, GLOBAL)),), torch.uint8, name="scratch")
    need, needs = f(2, 8, 8, GLOBAL), fs(2, 8, 8, GLOBAL)
    st = _stream()
    ok, c256 = (ctypes.c_int32 * 2)(0, 1), (ctypes.c_int32 * 2)(0, 256)
    p = lambda t: None if t is None else t.data_ptr()

    def call(mask=m, n=2, H=8, W=8, route=GLOBAL, o=out, passes=ps, scratch=sc, nbytes=need):
        return fn(p(mask), n, H, W, route, p(o), p(passes), p(scratch), nbytes, st)

    def calls(pred=m, gt=m, n=2, H=8, W=8, classes=ok, K=2, route=GLOBAL, out_i=si, out_f=sf, scratch=sc, nbytes=needs):
        return fns(p(pred), p(gt), n, H, W, classes, K, route, p(out_i), p(out_f), p(scratch), nbytes, st)

    assert call(mask=None) == _lib.EINVAL and call(o=None) == _lib.EINVAL and call(scratch=None) == _lib.EINVAL
    assert call(route=3) == _lib.EINVAL and call(route=-1) == _lib.EINVAL
    assert call(n=0) == _lib.ESHAPE and call(n=32768) == _lib.ESHAPE and call(H=0) == _lib.ESHAPE and call(W=16385) == _lib.ESHAPE
    assert call(H=4096, W=4096, route=RESIDENT) == _lib.ESHAPE
    assert call(nbytes=need - 1) == _lib.EWORKSPACE   # one byte short
    assert calls(pred=None) == _lib.EINVAL and calls(gt=None) == _lib.EINVAL and calls(out_i=None) == _lib.EINVAL
    assert calls(out_f=None) == _lib.EINVAL and calls(scratch=None) == _lib.EINVAL and calls(classes=None) == _lib.EINVAL
    assert calls(route=3) == _lib.EINVAL and calls(classes=c256) == _lib.EINVAL
    assert calls(n=0) == _lib.ESHAPE and calls(n=32768) == _lib.ESHAPE and calls(H=16385) == _lib.ESHAPE and calls(W=0) == _lib.ESHAPE
    assert calls(K=0) == _lib.ESHAPE and calls(K=257) == _lib.ESHAPE and calls(H=4096, W=4096, route=RESIDENT) == _lib.ESHAPE
    assert calls(nbytes=needs - 1) == _lib.EWORKSPACE
    torch.cuda.synchronize()
    assert (out == 7).all() and (ps == 7).all() and (si == 7).all() and (sf == 7.0).all()   # nothing was launched
    check(m, out, ps, si, sf, sc)
    assert call() == _lib.OK and call(passes=None, route=RESIDENT) == _lib.OK and calls() == _lib.OK
    torch.cuda.synchronize()
    assert (out == 0).all() and (ps == 1).all() and (si[..., 0, :2] == 64).all() and (si[..., 1, :2] == 0).all()
    check(m, out, ps, si, sf, sc)
