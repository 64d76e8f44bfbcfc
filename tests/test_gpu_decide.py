"""GPU (-m gpu): a class decided by threshold, with hysteresis, on the device (vitseg_decide, decide.threshold_mask,
model.predict_threshold, the evaluation's threshold= keywords) against the CPU restatement tests/decide_ref.py.  Every output is an
integer: every comparison is bit for bit, there is no tolerance.  Inputs, outputs and the scratch live in guard-banded buffers;
the scratch is poisoned."""
import csv

import numpy as np
import pytest
import torch

import curves_ref as CV
import decide_ref as DR
from guard import check, guarded, snapshot, unchanged
from test_decide_cpu import KEPT4, KEPT8, PLANE
from visiontransformer_amd import _ext, _lib, clean, confidence, decide, scripts, synth
from visiontransformer_amd.config import ViTSegConfig
from visiontransformer_amd.metrics import Evaluator, csv_row
from visiontransformer_amd.model import ViTSegmentationModel
from visiontransformer_amd.predict import predict, preprocess

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = {"prob": 0, "margin": 1}
HQ, LQ = decide.threshold_to_q(0.6), decide.threshold_to_q(0.4)


def _size(n, S, hyst):
    return _ext.ext_symbol("decide", "vitseg_decide_scratch_bytes")(n, S, int(hyst))


def _call(z, S, cls, kind, high_q, low_q, conn=4, base=None, value=None, off=0, counts=True):
    """One vitseg_decide call through the C ABI on guarded buffers, the mask, the counts and the scratch poisoned: (mask uint8
    numpy [n, S, S], counts int64 numpy [n, 3] or None)"""
    n, C, g, _ = z.shape
    value = cls if value is None else value
    zd = guarded(z.shape, torch.float32, z.to(DEV), name="lowres")
    bd = None if base is None else guarded((n, S, S), torch.uint8, torch.as_tensor(base).to(DEV), name="base")
    out = guarded((n, S, S), torch.uint8, name="mask")
    cnt = guarded((n, 3), torch.int64, name="counts") if counts else None   # poisoned: the call zeroes it itself
    need = _size(n, S, low_q != high_q)
    assert (need == 0) == (low_q == high_q)
    scratch = guarded(max(need, 256), torch.uint8, name="scratch")
    snap = snapshot(zd, bd) + (snapshot(scratch) if need == 0 else [])   # a scratch of 0 bytes is not touched at all
    _lib.check(_ext.ext_symbol("decide", "vitseg_decide")(
        zd.data_ptr(), n, C, g, S, cls, KINDS[kind], high_q, low_q, conn, None if bd is None else bd.data_ptr(), value, off,
        out.data_ptr(), None if cnt is None else cnt.data_ptr(), scratch.data_ptr() if need else None, need,
        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    check(zd, bd, out, cnt, scratch)
    unchanged(snap)
    return out.cpu().numpy(), None if cnt is None else cnt.cpu().numpy()


def _both(z, S, cls, kind, high_q, low_q, conn=4, base=None, value=None, off=0):
    """`_call` with counts and without: the same mask"""
    mask, counts = _call(z, S, cls, kind, high_q, low_q, conn, base, value, off)
    again, none = _call(z, S, cls, kind, high_q, low_q, conn, base, value, off, counts=False)
    assert none is None and np.array_equal(again, mask)
    return mask, counts


# ---- the seams of the 32-pixel labelling tiles and of the 4096-pixel chunks ----

def _serpentines(S=96):
    """(A, B) bool [S, S]: two weak serpentines side by side, each through all nine 32 x 32 tiles and all three 4096-pixel
    chunks, nowhere 8-adjacent to one another: B runs inside A's turns on the right and around them on the left.  A ends at
    (84, 2)."""
    A, B = np.zeros((S, S), bool), np.zeros((S, S), bool)
    for k, y in enumerate(range(4, 85, 16)):       # A: rows 4, 20 .. 84 over columns 2..89, joined at 89 and at 2 in turn
        A[y, 2:90] = True
        if y + 16 < S - 8:
            A[y:y + 17, 89 if k % 2 == 0 else 2] = True
    for y in (8, 40, 72):                          # B: pairs of rows 8 / 16, 40 / 48, 72 / 80 joined at column 85
        B[y, 6:86] = B[y + 8, 6:86] = True
        B[y:y + 9, 85] = True
    for y in (16, 48):                             # ... and one pair to the next along column 0
        B[y, 0:6] = B[y + 24, 0:6] = True
        B[y:y + 25, 0] = True
    return A, B


def test_a_serpentine_through_every_tile_is_kept_by_one_strong_pixel_at_its_far_end():
    ndimage = pytest.importorskip("scipy.ndimage")
    S = 96
    A, B = _serpentines(S)
    for conn in (4, 8):   # two components, whichever way pixels hang together; every tile holds a piece of each
        lab, k = ndimage.label(A | B, structure=DR.STRUCTURE[conn])
        assert k == 2 and len(set(lab[A])) == 1 and len(set(lab[B])) == 1
    tiles = lambda m: m.reshape(3, 32, 3, 32).any(axis=(1, 3))
    assert tiles(A).all() and tiles(B).all() and A[84, 2] and A[4, 2] and int(A.sum()) > 500 and int(B.sum()) > 500
    z = torch.full((1, 2, S, S), -6.0)
    z[0, 1][torch.from_numpy(A | B)] = 0.0
    z[0, 1, 84, 2] = 2.0                       # the strong pixel: A's far end, in the last tile row
    q = CV.scores(z, S, 1, "prob")
    low_q, high_q = int(q[0, 4, 2]), int(q[0, 84, 2])
    assert int(q.min()) < low_q < high_q and int((q >= low_q).sum()) == int((A | B).sum()) and int((q >= high_q).sum()) == 1
    for conn in (4, 8):
        mask, counts = _both(z, S, 1, "prob", high_q, low_q, conn)
        assert np.array_equal(mask[0], A.astype(np.uint8)), conn              # the first kept whole, the second gone
        assert counts.tolist() == [[int((A | B).sum()), 1, int(A.sum())]]
        want, wcounts = DR.decide_q(q, high_q, low_q, conn)
        assert np.array_equal(mask, want) and np.array_equal(counts, wcounts)
        mask, counts = _both(z, S, 1, "prob", high_q + 1, low_q, conn)        # >= at the equality: one more and nothing is strong
        assert not mask.any() and counts.tolist() == [[int((A | B).sum()), 0, 0]]
        mask, counts = _both(z, S, 1, "prob", high_q, low_q + 1, conn)        # ... and one more and only the strong pixel is weak
        assert int(mask.sum()) == 1 and mask[0, 84, 2] == 1 and counts.tolist() == [[1, 1, 1]]


# ---- ragged sizes ----

# (S, g, n) x (C, kind, cls) -> the seed at which, on the restatement, every image's hysteresis mask differs from both plain cuts
MODELS = [(2, "prob", 1), (3, "margin", 2), (1, "prob", 0)]
SEEDS = {(33, 5, 1): (2, 1, 2), (70, 5, 1): (2, 0, 2), (130, 10, 3): (3, 0, 3), (1, 1, 1): (0, 0, 0), (33, 1, 1): (0, 0, 0),
         (70, 1, 1): (0, 0, 0)}
_REF = {}


def _case(shape, m):
    """(z fp32 [n, C, g, g], q int64 [n, S, S]) of a smooth random head output; computed once and left unchanged"""
    key = (shape, m)
    if key not in _REF:
        S, g, n = shape
        C, kind, cls = MODELS[m]
        gen = torch.Generator().manual_seed(SEEDS[shape][m])
        z = torch.randn((n, C, g, g), generator=gen) * 3.0
        _REF[key] = (z, CV.scores(z, S, cls, kind))
    return _REF[key]


@pytest.mark.parametrize("m", range(3), ids=["c2-prob", "c3-margin", "c1-prob"])
@pytest.mark.parametrize("shape", sorted(SEEDS), ids=lambda s: "x".join(map(str, s)))
def test_ragged_sizes_equal_the_restatement(shape, m):
    S, g, n = shape
    C, kind, cls = MODELS[m]
    value = 1 if C == 1 else cls
    z, q = _case(shape, m)
    for conn in (4, 8):
        weak, strong, kept = DR.kept_planes(q, HQ, LQ, conn)
        if g > 1:   # (one source pixel gives one score everywhere: a plane of one level has nothing for hysteresis to decide)
            for b in range(n):   # the case cannot pass by computing either plain cut
                assert (kept[b] != weak[b]).any() and (kept[b] != strong[b]).any(), (conn, b)
        want, wcounts = DR.decide_q(q, HQ, LQ, conn, value=value)
        mask, counts = _both(z, S, cls, kind, HQ, LQ, conn, value=value)
        assert np.array_equal(mask, want), conn
        assert np.array_equal(counts, wcounts), conn                                     # the counts against the restatement
        again, acounts = _call(z, S, cls, kind, HQ, LQ, conn, value=value)               # the same bits on a second call
        assert np.array_equal(again, mask) and np.array_equal(acounts, counts)
        for b in range(n if n > 1 else 0):                                               # an image alone: the batch's rows
            one, ocounts = _call(z[b:b + 1], S, cls, kind, HQ, LQ, conn, value=value)
            assert np.array_equal(one[0], mask[b]) and np.array_equal(ocounts[0], counts[b]), (conn, b)
    for hq in (HQ, LQ):   # the plain cuts
        mask, counts = _both(z, S, cls, kind, hq, hq, value=value)
        assert np.array_equal(mask, (q >= hq).astype(np.uint8) * value)
        k = (q >= hq).reshape(n, -1).sum(axis=1)
        assert np.array_equal(counts, np.stack([k, k, k], axis=1))


def test_the_python_call_takes_single_images_thresholds_either_way_and_the_global_route():
    shape = (130, 10, 3)
    z, q = _case(shape, 1)
    zd = z.to(DEV)
    want, wcounts = DR.decide_q(q, HQ, LQ, 8, value=2)
    got, counts = decide.threshold_mask(zd, 2, 0.6, 0.4, 8, "margin", size=130, return_counts=True)
    assert got.dtype == torch.uint8 and got.shape == (3, 130, 130) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want) and counts.dtype == np.int64 and np.array_equal(counts, wcounts)
    assert torch.equal(decide.threshold_mask(zd, 2, connectivity=8, kind="margin", size=130, high_q=HQ, low_q=LQ), got)
    one, c1 = decide.threshold_mask(zd[1], 2, 0.6, 0.4, 8, "margin", size=130, return_counts=True)
    assert one.shape == (130, 130) and np.array_equal(one.cpu().numpy(), want[1]) and np.array_equal(c1, wcounts[1])
    with _lib.option("upsample_global", 1):   # the taps read from global memory: the staged bits
        assert torch.equal(decide.threshold_mask(zd, 2, 0.6, 0.4, 8, "margin", size=130), got)
        assert np.array_equal(decide.threshold_mask(zd, 2, 0.6, kind="margin", size=130).cpu().numpy(), (q >= HQ) * np.uint8(2))


# ---- connectivity ----

def test_the_diagonal_chain_is_kept_at_8_and_cut_at_4():
    """the plane tests/test_decide_cpu.py answers by hand, as full-size logits of a one-class head"""
    z = torch.tensor([[{".": -6.0, "w": 0.0, "S": 2.0}[c] for c in r] for r in PLANE])[None, None]
    q = CV.scores(z, 8, 0, "prob")
    low_q, high_q = int(q[0, 0, 0]), int(q[0, 3, 3])
    assert low_q == 32768 and high_q > low_q and int((q >= low_q).sum()) == 15 and int((q >= high_q).sum()) == 4
    for conn, rows in ((4, KEPT4), (8, KEPT8)):
        want = np.array([[c != "." for c in r] for r in rows])[None]
        mask, counts = _both(z, 8, 0, "prob", high_q, low_q, conn, value=3, off=9)
        assert np.array_equal(mask, np.where(want, 3, 9)) and counts.tolist() == [[15, 4, int(want.sum())]]
    assert mask[0, 0, 0] == 3 and _call(z, 8, 0, "prob", high_q, low_q, 4, value=3, off=9)[0][0, 0, 0] == 9


# ---- degenerate thresholds ----

def test_degenerate_thresholds():
    """Against the device's own quantised map, the plane `curves.pr_counts` bins.  (At this shape, whose scale 5 / 70 is no power
    of two, vitseg_confidence's q lies one beside the restatement's on 2 and 4 of the 4900 pixels -- measured, the cause not
    traced; the cuts at the map's own extremes below are therefore taken from the map, as the header defines them.)"""
    shape = (70, 5, 1)
    for m in (0, 1):
        C, kind, cls = MODELS[m]
        z, ref = _case(shape, m)
        q = confidence.confidence_map(z.to(DEV), torch.full((1, 70, 70), cls, dtype=torch.uint8, device=DEV), kind=kind,
                                      quantised=True).cpu().numpy().astype(np.int64)
        assert int(np.abs(q - ref).max()) <= 1 and int((q != ref).sum()) <= 8
        for hq in (HQ, LQ, int(q.max()), int(q.max()) + 1, int(q.min()), 1):
            assert _size(1, 70, False) == 0
            mask, counts = _both(z, 70, cls, kind, hq, hq)
            assert np.array_equal(mask, (q >= hq).astype(np.uint8) * cls)
            assert counts.tolist() == [[int((q >= hq).sum())] * 3]
        mask, counts = _both(z, 70, cls, kind, 0, 0)              # reached by every pixel
        assert (mask == cls).all() and counts.tolist() == [[4900] * 3]
        mask, counts = _both(z, 70, cls, kind, 65536, 65536)      # reached by none
        assert not mask.any() and counts.tolist() == [[0] * 3]
        for conn in (4, 8):
            mask, counts = _both(z, 70, cls, kind, 65536, 0, conn)   # a full frame of weak pixels and no strong one
            assert not mask.any() and counts.tolist() == [[4900, 0, 0]]
            top = int(q.max())                                       # a full frame of weak pixels under the strongest
            mask, counts = _both(z, 70, cls, kind, top, 0, conn)
            assert (mask == cls).all() and counts.tolist() == [[4900, int((q >= top).sum()), 4900]]
            mask, counts = _both(z, 70, cls, kind, 65536, LQ, conn)
            assert not mask.any() and counts.tolist() == [[int((q >= LQ).sum()), 0, 0]]


# ---- base, value, off ----

def test_base_value_and_off():
    shape = (130, 10, 3)
    z, q = _case(shape, 1)   # three classes, the margin of class 2
    gen = torch.Generator().manual_seed(5)
    base = torch.randint(0, 3, (3, 130, 130), generator=gen).to(torch.uint8)
    base[0, :40] = 2          # a block that states the decided class itself
    for value, off in ((2, 0), (2, 1), (1, 0), (7, 9), (0, 255)):
        bnp = base.numpy()
        assert (bnp == value).any() == (value < 3)
        for conn in (4, 8):
            want, wcounts = DR.decide_q(q, HQ, LQ, conn, base=bnp, value=value, off=off)
            kept = DR.kept_planes(q, HQ, LQ, conn)[2]
            assert ((bnp == value) & ~kept).any() == (value < 3)   # base pixels that state the value and are dropped: to off
            mask, counts = _both(z, 130, 2, "margin", HQ, LQ, conn, base=bnp, value=value, off=off)
            assert np.array_equal(mask, want) and np.array_equal(counts, wcounts), (value, off, conn)
            assert np.array_equal(mask == value, kept)
        want, _ = DR.decide_q(q, HQ, HQ, 4, base=bnp, value=value, off=off)
        mask, _ = _both(z, 130, 2, "margin", HQ, HQ, 4, base=bnp, value=value, off=off)
        assert np.array_equal(mask, want), (value, off)
    got = decide.threshold_mask(z.to(DEV), 2, 0.6, 0.4, kind="margin", base=base, value=2, off=1)
    assert np.array_equal(got.cpu().numpy(), DR.decide_q(q, HQ, LQ, 4, base=base.numpy(), value=2, off=1)[0])
    one = decide.threshold_mask(z[2].to(DEV), 2, 0.6, 0.4, kind="margin", base=base[2].numpy())
    assert np.array_equal(one.cpu().numpy(), DR.decide_q(q[2:], HQ, LQ, 4, base=base[2:].numpy(), value=2)[0][0])


# ---- errors ----

def test_every_bad_argument_returns_its_code_and_launches_nothing():
    fn = _ext.ext_symbol("decide", "vitseg_decide")
    z = guarded((1, 2, 2, 2), torch.float32, "zero", name="lowres")
    base = guarded((1, 8, 8), torch.uint8, "zero", name="base")
    out = guarded((1, 8, 8), torch.uint8, name="mask")
    cnt = guarded((1, 3), torch.int64, name="counts")
    need = _size(1, 8, True)
    scratch = guarded(need, torch.uint8, name="scratch")
    snap = snapshot(z, base, out, cnt, scratch)

    def call(lowres=z.data_ptr(), n=1, C=2, g=2, S=8, cls=1, kind=0, high=40000, low=20000, conn=4, b=base.data_ptr(), value=1,
             off=0, mask=out.data_ptr(), counts=cnt.data_ptr(), sc=scratch.data_ptr(), nbytes=need):
        return fn(lowres, n, C, g, S, cls, kind, high, low, conn, b, value, off, mask, counts, sc, nbytes,
                  torch.cuda.current_stream().cuda_stream)
    for kw in (dict(lowres=None), dict(mask=None), dict(b=out.data_ptr()), dict(kind=2), dict(kind=-1), dict(kind=1, C=1, cls=0),
               dict(cls=-1), dict(cls=2), dict(low=-1), dict(high=65537), dict(low=40001), dict(high=19999), dict(conn=6),
               dict(conn=0), dict(value=-1), dict(value=256), dict(off=-1), dict(off=256), dict(value=5, off=5), dict(sc=None)):
        assert call(**kw) == _lib.EINVAL, kw
    for kw in (dict(n=0), dict(n=65536), dict(C=0), dict(C=256), dict(S=0), dict(S=16385), dict(g=0), dict(g=9)):
        assert call(**kw) == _lib.ESHAPE, kw
    assert call(nbytes=need - 1) == _lib.EWORKSPACE and call(nbytes=0) == _lib.EWORKSPACE
    torch.cuda.synchronize()
    check(z, base, out, cnt, scratch)
    unchanged(snap)   # the poisoned outputs still hold their poison: nothing ran, not even the zeroing
    assert call() == _lib.OK and call(high=32768, low=32768, sc=None, nbytes=0) == _lib.OK   # p = 0.5 everywhere: q = 32768
    torch.cuda.synchronize()
    check(z, base, out, cnt, scratch)
    assert (out == 1).all() and cnt.tolist() == [[64, 64, 64]]
    assert call(high=32769, low=32768) == _lib.OK
    torch.cuda.synchronize()
    assert (out == 0).all() and cnt.tolist() == [[64, 0, 0]]


# ---- end to end ----

_MODEL = {}
INFO = (7, "ID7P16H192A3", 16, 192, 1, 3)


def _tiny():
    """tiny16_224_c2's geometry (oracle/make_golden.py) with seeded weights, two images and the plane of class 1"""
    if "tiny" not in _MODEL:
        cfg = ViTSegConfig(2, 16, 192, 12, 3, image_size=224)
        model = ViTSegmentationModel(2, 16, 192, 12, 3, image_size=224, device=DEV).eval()
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=3).items()})
        x = torch.from_numpy(synth.make_images(cfg, 2, seed=1)).to(DEV)
        lowres, argmax = model._lowres_and_mask(x)
        q = confidence.confidence_map(lowres, torch.ones_like(argmax), quantised=True).cpu().numpy().astype(np.int64)
        _MODEL["tiny"] = (model, x, argmax, q)
    return _MODEL["tiny"]


def test_model_predict_threshold_is_the_cut_of_the_quantised_confidence():
    model, x, argmax, q = _tiny()
    t, tl = float(np.quantile(q, 0.7)) / 65535, float(np.quantile(q, 0.4)) / 65535   # cuts inside the scores' range
    hq, lq = decide.threshold_to_q(t), decide.threshold_to_q(tl)
    plain = (q >= hq).astype(np.uint8)
    assert plain.any() and not plain.all() and lq < hq
    got = model.predict_threshold(x, 1, t)
    assert got.dtype == torch.uint8 and got.shape == (2, 224, 224) and np.array_equal(got.cpu().numpy(), plain)
    assert torch.equal(model.predict_mask(x), argmax)
    over = model.predict_threshold(x, 1, t, over_argmax=True)
    assert np.array_equal(over.cpu().numpy(), DR.apply(plain.astype(bool), argmax.cpu().numpy(), 1))
    for conn in (4, 8):
        want = DR.decide_q(q, hq, lq, conn)[0]
        assert np.array_equal(model.predict_threshold(x, 1, t, tl, conn).cpu().numpy(), want)
    cleaned = model.predict_threshold(x, 1, t, min_area=8)
    assert torch.equal(cleaned, clean.clean_mask(got, min_area=8))
    with pytest.raises(ValueError):
        model.predict_threshold(x, 2, t)
    with pytest.raises(ValueError):
        model.predict_threshold(x, 0, t)


def test_predict_returns_the_decided_mask_and_what_is_read_from_it():
    model, _, _, _ = _tiny()
    image = np.random.RandomState(4).randint(0, 256, size=(150, 200, 3)).astype(np.uint8)
    x = preprocess(image, 224, DEV)
    lowres, argmax = model._lowres_and_mask(x)
    q = confidence.confidence_map(lowres, torch.ones_like(argmax), quantised=True).cpu().numpy()
    t, tl = float(np.quantile(q, 0.7)) / 65535, float(np.quantile(q, 0.4)) / 65535
    kw = dict(threshold=t, threshold_low=tl, threshold_connectivity=8)
    want = model.predict_threshold(x, 1, t, tl, 8)[0].cpu().numpy()
    assert want.any() and not want.all() and not np.array_equal(want, argmax[0].cpu().numpy())
    got = predict(image, model, **kw)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    mask, logits, boxes = predict(image, model, return_logits=True, return_boxes=True, **kw)   # over the full-size logits: the same
    assert np.array_equal(mask, want) and logits.shape == (2, 224, 224)
    from visiontransformer_amd.regions import boxes_by_class, region_boxes
    assert boxes == boxes_by_class(region_boxes(torch.from_numpy(want).to(DEV))) and set(boxes) == {1}
    over = predict(image, model, threshold_over_argmax=True, min_area=8, **kw)
    decided = model.predict_threshold(x, 1, t, tl, 8, over_argmax=True)
    assert np.array_equal(over, clean.clean_mask(decided, min_area=8)[0].cpu().numpy())   # (predict's clean-up is 4-connected)
    mask, scores = predict(image, model, return_scores=True, **kw)
    assert np.array_equal(mask, want) and len(scores) == sum(len(b) for b in boxes.values())


def test_the_evaluation_scores_the_decided_masks(tmp_path):
    model = ViTSegmentationModel(3, 16, 192, 1, 3, image_size=224, device=DEV).eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(model.cfg, seed=3).items()})
    batches = scripts.ce_batches(model.cfg, 4, 2, seed=3)
    lowres, argmax = model._lowres_and_mask(batches[0][0].to(DEV))
    q = confidence.confidence_map(lowres, torch.ones_like(argmax), quantised=True).cpu().numpy()
    t, tl = float(np.quantile(q, 0.8)) / 65535, float(np.quantile(q, 0.5)) / 65535
    kw = dict(threshold=t, threshold_low=tl, threshold_class=1, threshold_connectivity=8, threshold_over_argmax=True)
    path = tmp_path / "m_metrics.csv"
    rows = scripts.evaluate_to_csv(model, batches, INFO, str(path), 3, 2, DEV, **kw)
    ev = Evaluator(3, DEV)
    want, changed = [], 0
    for bn, (x, gt) in enumerate(batches):
        mask = model.predict_threshold(x.to(DEV), 1, t, tl, 8, over_argmax=True)
        changed += int((mask != model.predict_mask(x.to(DEV))).sum())
        gt = gt.reshape(gt.shape[0], gt.shape[-2], gt.shape[-1])
        want += [csv_row(INFO, bn, i, m, 0.0) for i, m in enumerate(ev.evaluate(mask, gt))]
    assert changed > 0 and len(rows) == 4   # the decided masks are not the argmax masks
    strip = lambda rs: [list(r[:11]) + list(r[12:]) for r in rs]   # (but the time per image)
    np.testing.assert_equal(strip(rows), strip(want))
    got = list(csv.reader(open(path, newline="")))
    assert len(got) == 5 and strip(got[1:]) == [[str(v) for v in r] for r in strip(want)]
    plain = scripts.evaluate_to_csv(model, batches, INFO, str(tmp_path / "plain" / "m_metrics.csv"), 3, 2, DEV)
    assert strip(plain) != strip(rows)
