"""GPU (-m gpu): the precision-recall counts on the device (vitseg_pr_counts, curves.pr_counts, model.pr_counts, the evaluation's
reports.PRCurve) against the CPU restatement tests/curves_ref.py.  Every output is an integer: every comparison is bit for bit,
there is no tolerance.  Inputs, outputs and the scratch live in guard-banded buffers."""
import csv

import numpy as np
import pytest
import torch

import curves_ref as CV
from guard import check, guarded, snapshot, unchanged
from visiontransformer_amd import _ext, _lib, confidence, curves, scripts, synth
from visiontransformer_amd.model import ViTSegmentationModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = {"prob": 0, "margin": 1}
# (S, g, C): 33: one ragged tile, g == S and one class; 70: a second, narrow tile; 96: 17 classes; 224: four tiles a side
SHAPES = [(33, 33, 1), (70, 5, 2), (96, 6, 17), (224, 14, 2)]
TOL2 = [0, 1, 2, 5, 25, 256]
BINS = [1, 7, 256, 1024]
_REF = {}


def _inputs(shape):
    """(lowres [3, C, g, g], gt uint8 [3, S, S], cls): thin true strokes of class `cls`, void pixels (255) scattered over the
    frame -- on the strokes, beside them and under their discs -- and a void block; image 2 has a true pixel in every corner"""
    if shape not in _REF:
        S, g, C = shape
        gen = torch.Generator().manual_seed(100 * S + C)
        z = torch.randn((3, C, g, g), generator=gen) * 2.0
        cls = min(1, C - 1)
        gt = torch.randint(0, max(C, 2), (3, S, S), generator=gen).to(torch.uint8)
        gt[gt == cls] = 0 if cls else 1
        for i in range(3):   # strokes: a diagonal, a row and a column of true pixels
            k = torch.arange(S)
            gt[i, k, (k * (i + 2) // 3 + 5 * i) % S] = cls
            gt[i, (S // 3 + 7 * i) % S, S // 4:] = cls
            gt[i, :S // 2, (2 * S // 3 + 3 * i) % S] = cls
        gt[torch.rand((3, S, S), generator=gen) < 0.08] = 255
        gt[1, S // 3:S // 3 + 9, S // 2:S // 2 + 9] = 255
        for y in (0, S - 1):
            for x in (0, S - 1):
                gt[2, y, x] = cls
        _REF[shape] = dict(z=z, gt=gt, cls=cls, q={}, planes={})
    return _REF[shape]


def _ref(shape, kind, tol2, ignore, bins):
    """the restatement's counts [3, bins, 3]; the scores and planes are computed once per key and left unchanged"""
    d = _inputs(shape)
    if kind not in d["q"]:
        d["q"][kind] = CV.scores(d["z"], shape[0], d["cls"], kind)
    key = (kind, tol2, ignore)
    if key not in d["planes"]:
        d["planes"][key] = CV.planes(d["q"][kind], d["gt"].numpy(), d["cls"], tol2, ignore)
    return CV.counts_from_planes(d["q"][kind], *d["planes"][key], bins)


def _call(z, gt, cls, kind, bins, tol2, ignore=-1):
    """One vitseg_pr_counts call through the C ABI on guarded buffers, the scratch poisoned: int64 numpy [n, bins, 3]"""
    n, C, g, _ = z.shape
    S = gt.shape[-1]
    zd = guarded(z.shape, torch.float32, z.to(DEV), name="lowres")
    gd = guarded(gt.shape, torch.uint8, gt.to(DEV), name="gt")
    out = guarded((n, bins, 3), torch.int64, name="counts")   # poisoned: the call zeroes it itself
    need = _ext.ext_symbol("curves", "vitseg_pr_counts_scratch_bytes")(n, S, tol2)
    scratch = guarded(max(need, 256), torch.uint8, name="scratch")
    snap = snapshot(zd, gd) + (snapshot(scratch) if need == 0 else [])   # a scratch of 0 bytes is not touched at all
    _lib.check(_ext.ext_symbol("curves", "vitseg_pr_counts")(
        zd.data_ptr(), gd.data_ptr(), n, C, g, S, cls, KINDS[kind], bins, tol2, ignore, out.data_ptr(), scratch.data_ptr(), need,
        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    check(zd, gd, out, scratch)
    unchanged(snap)
    return out.cpu().numpy()


@pytest.mark.parametrize("tol2", TOL2)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_counts_equal_the_restatement(shape, tol2):
    d = _inputs(shape)
    z, gt, cls = d["z"], d["gt"], d["cls"]
    assert int((gt == 255).sum()) > 0 and int((gt == cls).sum()) > 0
    for kind in (("prob", "margin") if shape[2] >= 2 else ("prob",)):
        for ignore in (-1, 255):
            for bins in BINS:
                want = _ref(shape, kind, tol2, ignore, bins)
                got = _call(z, gt, cls, kind, bins, tol2, ignore)
                assert np.array_equal(got, want), (kind, ignore, bins)
            # conservation: every valid pixel is predicted once, every true pixel found once
            valid = (gt.long() != ignore).sum(dim=(1, 2)).numpy()
            pos = ((gt.long() == cls) & (gt.long() != ignore)).sum(dim=(1, 2)).numpy()
            assert np.array_equal(got[:, :, 0].sum(axis=1), valid) and np.array_equal(got[:, :, 2].sum(axis=1), pos)
            if tol2 == 0:
                assert np.array_equal(got[:, :, 1], got[:, :, 2])
            # an image alone gives the bits it gives in the batch (n = 1 and n = 3), and a second call the same bits
            for i in range(3):
                assert np.array_equal(_call(z[i:i + 1], gt[i:i + 1], cls, kind, 1024, tol2, ignore)[0], got[i]), (kind, ignore, i)
            assert np.array_equal(_call(z, gt, cls, kind, 1024, tol2, ignore), got)
    if tol2 > 0:   # void pixels lay under the discs of true pixels
        assert int(CV.disc_max((gt == 255).numpy().astype(np.int64), tol2, 0)[(gt == cls).numpy()].sum()) > 0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cumulative_found_does_not_fall_as_the_tolerance_grows(shape):
    d = _inputs(shape)
    before = None
    for tol2 in TOL2:
        got = _call(d["z"], d["gt"], d["cls"], "prob", 256, tol2, 255)
        cum = np.cumsum(got[:, ::-1], axis=1)[:, ::-1]
        if before is not None:
            assert (cum[:, :, 2] >= before[:, :, 2]).all() and (cum[:, :, 1] >= before[:, :, 1]).all()
            assert np.array_equal(cum[:, :, 0], before[:, :, 0])   # what is predicted does not depend on the tolerance
        before = cum
    assert (before[:, :, 2] > np.cumsum(_call(d["z"], d["gt"], d["cls"], "prob", 256, 0, 255)[:, ::-1], axis=1)[:, ::-1][:, :, 2]).any()


def _offsets(d2):
    return [(dy, dx) for dy in range(-17, 18) for dx in range(-17, 18) if dy * dy + dx * dx == d2]


def _pairs(S, tile, tol2):
    """(true pixel, high pixel, inside) triples: the pair at every offset of squared length tol2 (inside the disc) and of the
    next squared length an integer offset has (outside), walked along the diagonal so that it straddles the tile seam at `tile`
    in x and in y, and placed at the four frame corners"""
    out_d2 = next(d for d in range(tol2 + 1, tol2 + 40) if _offsets(d))
    pairs = []
    for d2, inside in ((tol2, True), (out_d2, False)):
        for dy, dx in _offsets(d2):
            m = max(abs(dy), abs(dx))
            starts = {tile - 1, tile - (m + 1) // 2, tile - m, tile}                        # true pixel left of / above the seam
            starts |= {tile + m - 1, tile + m // 2}                                         # ... right of / below it
            found = [((p, p), (p + dy, p + dx)) for p in sorted(starts)]
            for c in ((0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1)):                      # a corner in either role
                found += [(c, (c[0] + dy, c[1] + dx)), ((c[0] + dy, c[1] + dx), c)]
            pairs += [(a, b, inside) for a, b in found if all(0 <= v < S for v in a + b)]
    return pairs


@pytest.mark.parametrize("tol2", [1, 2, 5, 25, 256])
def test_a_pair_at_the_edge_of_the_disc_across_every_seam_and_in_every_corner(tol2):
    """g == S: the scores are set per pixel.  One true pixel and one high-score pixel per image, at a squared distance of exactly
    tol2 (found and hit) or of the next larger one (neither)."""
    S, tile = 70, 64
    pairs = _pairs(S, tile, tol2)
    inside = np.array([p[2] for p in pairs])
    assert inside.any() and (~inside).any()
    corners = {(0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1)}
    assert corners <= {p[0] for p in pairs if p[2]} and corners <= {p[1] for p in pairs if p[2]}
    for axis in (0, 1):   # pairs whose two pixels lie on either side of the seam, in both orders
        assert any(p[0][axis] < tile <= p[1][axis] for p in pairs) and any(p[1][axis] < tile <= p[0][axis] for p in pairs)
    n = len(pairs)
    z = torch.full((n, 2, S, S), -6.0)
    gt = torch.zeros((n, S, S), dtype=torch.uint8)
    for i, ((py, px), (hy, hx), _) in enumerate(pairs):
        gt[i, py, px] = 1
        z[i, 1, hy, hx] = 6.0
    got = _call(z, gt, 1, "prob", 256, tol2)
    assert np.array_equal(got, CV.pr_counts(z, gt, 1, "prob", 256, tol2))
    top = got[:, 255]   # the high pixel's bin: it is predicted; hit and found only from inside the disc
    assert np.array_equal(top[:, 0], np.ones(n, np.int64))
    assert np.array_equal(top[:, 1], inside.astype(np.int64)) and np.array_equal(top[:, 2], inside.astype(np.int64))
    assert np.array_equal(got[:, 0, 2], (~inside).astype(np.int64))   # otherwise the true pixel finds a low score


def test_thresholding_the_quantised_map_reproduces_the_cumulative_counts():
    shape = (96, 6, 17)
    d = _inputs(shape)
    z, gt, cls = d["z"], d["gt"], d["cls"]
    for kind in ("prob", "margin"):
        q = confidence.confidence_map(z.to(DEV), torch.full_like(gt, cls).to(DEV), kind=kind, quantised=True).cpu().numpy().astype(np.int64)
        assert np.array_equal(q, CV.scores(z, 96, cls, kind))
        valid = (gt != 255).numpy()
        near = CV.planes(q, gt.numpy(), cls, 5, 255)[2]
        for bins in (7, 256):
            got = curves.pr_counts(z.to(DEV), gt, cls=cls, bins=bins, tolerance=5 ** 0.5, ignore_label=255, kind=kind)
            cum = np.cumsum(got[:, ::-1], axis=1)[:, ::-1]
            for k in range(bins):
                decided = (q >= curves.threshold_q(k, bins)) & valid
                assert np.array_equal(cum[:, k, 0], decided.sum(axis=(1, 2))), (kind, bins, k)
                assert np.array_equal(cum[:, k, 1], (decided & near).sum(axis=(1, 2))), (kind, bins, k)


def test_the_python_call_takes_single_images_numpy_and_the_global_route():
    shape = (70, 5, 2)
    d = _inputs(shape)
    z, gt = d["z"].to(DEV), d["gt"]
    want = _ref(shape, "margin", 25, -1, 256)
    assert np.array_equal(curves.pr_counts(z, gt, bins=256, tolerance=5, kind="margin"), want)
    one = curves.pr_counts(z[1], gt[1].numpy(), bins=256, tolerance=5, kind="margin")
    assert one.shape == (256, 3) and one.dtype == np.int64 and np.array_equal(one, want[1])
    with _lib.option("upsample_global", 1):   # the taps read from global memory: the staged bits
        assert np.array_equal(curves.pr_counts(z, gt, bins=256, tolerance=5, kind="margin"), want)
        assert np.array_equal(curves.pr_counts(z, gt, bins=256, tolerance=0, kind="margin"), _ref(shape, "margin", 0, -1, 256))


def test_every_bad_argument_returns_its_code_and_launches_nothing():
    fn = _ext.ext_symbol("curves", "vitseg_pr_counts")
    z = guarded((1, 2, 2, 2), torch.float32, "zero", name="lowres")
    gt = guarded((1, 8, 8), torch.uint8, "zero", name="gt")
    out = guarded((1, 16, 3), torch.int64, name="counts")
    scratch = guarded(256, torch.uint8, name="scratch")
    snap = snapshot(z, gt, out, scratch)
    need = _ext.ext_symbol("curves", "vitseg_pr_counts_scratch_bytes")(1, 8, 4)

    def call(lowres=z.data_ptr(), g_=gt.data_ptr(), n=1, C=2, g=2, S=8, cls=1, kind=0, bins=16, tol2=4, ignore=-1,
             counts=out.data_ptr(), nbytes=need):
        return fn(lowres, g_, n, C, g, S, cls, kind, bins, tol2, ignore, counts, scratch.data_ptr(), nbytes,
                  torch.cuda.current_stream().cuda_stream)
    for kw in (dict(lowres=None), dict(g_=None), dict(counts=None), dict(kind=2), dict(kind=1, C=1, cls=0), dict(cls=-1),
               dict(cls=2), dict(bins=0), dict(bins=1025), dict(tol2=-1), dict(tol2=257), dict(ignore=-2), dict(ignore=256)):
        assert call(**kw) == _lib.EINVAL, kw
    for kw in (dict(n=0), dict(n=65536), dict(C=0), dict(C=256), dict(S=0), dict(S=16385), dict(g=0), dict(g=9)):
        assert call(**kw) == _lib.ESHAPE, kw
    if need:
        assert call(nbytes=need - 1) == _lib.EWORKSPACE
    torch.cuda.synchronize()
    check(z, gt, out, scratch)
    unchanged(snap)   # the poisoned output still holds its poison: nothing ran, not even the zeroing
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert int(out.sum()) == 64 and int(out[0, 8, 0]) == 64   # 64 valid pixels at p = 0.5, no true one


# ---- end to end ----

_MODEL = {}
INFO = (7, "ID7P16H192A3", 16, 192, 1, 3)


def _model():
    if not _MODEL:
        model = ViTSegmentationModel(3, 16, 192, 1, 3, image_size=224, device=DEV).eval()
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(model.cfg, seed=3).items()})
        _MODEL.update(model=model, batches=scripts.ce_batches(model.cfg, 4, 2, seed=3))
    return _MODEL["model"], _MODEL["batches"]


def test_model_pr_counts_is_pr_counts_on_the_forward_lowres():
    model, batches = _model()
    x = batches[0][0].to(DEV)
    gt = torch.from_numpy(synth.make_targets(model.cfg, 2, seed=11, size=224)).to(torch.uint8)
    lowres, _ = model._lowres_and_mask(x)
    for kw, (cls, kind, bins, tol2, ignore) in ((dict(), (1, "prob", 256, 0, -1)),
                                                (dict(cls=2, bins=64, tolerance=2, ignore_label=0, kind="margin"), (2, "margin", 64, 4, 0))):
        got = model.pr_counts(x, gt, **kw)
        assert got.shape == (2, bins, 3) and int(got[:, :, 2].sum()) > 0
        assert np.array_equal(got, curves.pr_counts(lowres, gt, **kw))
        assert np.array_equal(got, CV.pr_counts(lowres.cpu(), gt, cls, kind, bins, tol2, ignore))


def test_the_evaluation_writes_the_curve_and_its_ods_row(tmp_path):
    model, batches = _model()
    base = scripts.evaluate_to_csv(model, batches, INFO, str(tmp_path / "plain" / "m_metrics.csv"), 3, 2, DEV)
    rows = scripts.evaluate_to_csv(model, batches, INFO, str(tmp_path / "m_metrics.csv"), 3, 2, DEV, pr_curve=1, pr_bins=64,
                                   pr_tolerance=2, score_kind="prob")
    strip = lambda rs: [list(r[:11]) + list(r[12:]) for r in rs]
    np.testing.assert_equal(strip(rows), strip(base))   # the metrics file's rows are what they were (but the time per image)
    ev_counts = []
    from visiontransformer_amd.metrics import Evaluator
    ev = Evaluator(3, DEV)
    for x, gt in batches:
        lowres, mask = model._lowres_and_mask(x.to(DEV))
        gt = gt.reshape(gt.shape[0], gt.shape[-2], gt.shape[-1])
        ev_counts.append(curves.pr_counts(lowres, ev.resized_gt(gt, mask), cls=1, bins=64, tolerance=2))
    counts = np.concatenate(ev_counts)
    assert counts.shape == (4, 64, 3) and int(counts[:, :, 2].sum()) > 0
    got = list(csv.reader(open(tmp_path / "m_pr_curve.csv", newline="")))
    assert got[0] == curves.CSV_COLUMNS and len(got) == 1 + 64 + 3
    want = [[str(v) for v in r] for r in curves.csv_rows(INFO, counts, 1, 2)]
    assert got[1:] == want
    o = curves.ods(counts.sum(axis=0))
    assert got[65][5] == "ODS" and got[65][-1] == str(o["f"]) and got[65][6] == str(o["threshold"])
    assert got[66][5] == "OIS" and got[66][-1] == str(curves.ois(counts)) and got[67][-1] == str(curves.ap(counts))
