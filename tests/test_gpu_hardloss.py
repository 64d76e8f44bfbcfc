"""GPU (-m gpu): the hard-pixel losses (vitseg_hard_ce_loss, vitseg_backward_hard, ViTSegmentationModel.ce_loss with
focal_gamma / ohem_*) against tests/hardloss_ref.py.  Every buffer is guard-banded; the hard options' scratch has exactly the
queried size and arrives NaN-poisoned.

Selection: checked with no tolerance.  The kernel's own `pixel_loss` plane goes through hardloss_ref.select_ref (integers and
bit patterns only), which must reproduce `stats` = {n_valid, k, |H|, bits of tau}, and the pixels with a non-zero gradient
row must be exactly H.  The plane itself is held against the fp64 CE within e_pix.

Values: given the kernel's H, loss and gradient are held against hardloss_ref.hard_closed_form (fp64) with the bounds of
tests/test_gpu_ce_options.py for the same quantities at eps = 0: e_pix + 6 u |loss| for the loss and w_max (e_pix + 20 u) / den
for a gradient entry, den = sum_H w[y].  The focal factor keeps within them on these inputs (each test prints its figures):
f = w q^gamma ce moves by m <= 1 + gamma / e per unit of ce and a handful of roundings of a value <= ce, against an e_pix of
a hundred u that the regenerated logits use a few u of."""
import ctypes as C
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ce_ref
import hardloss_ref as HR
from guard import check, guarded, snapshot, unchanged
from util import Golden
from visiontransformer_amd import _ext, _lib, synth
from visiontransformer_amd.model import ViTSegmentationModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -23   # fp32 unit roundoff (half an ulp of 1)
INF = float("inf")
SENTINEL = -1.0  # an ignored pixel's entry of the plane


def _sym(name):
    return _ext.ext_symbol("hardloss", name)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


def _fbits(v):
    return int(np.array(v, dtype=np.float32).view(np.uint32))


def _thresh(p):
    """The fp32 CE value of a probability threshold, as model.check_hard_options forms it."""
    return float(np.float32(-math.log(p) + 0.0))


def _ce_bounds(up, lse, C_):
    """Per-pixel error of the fp32 lse - z_c (test_gpu_ce_options._ce_bounds)."""
    zmax = up.abs().max().item()
    return 4 * U * lse.abs().max().item() + 8 * U * zmax + 4 * (C_ + 2) * U


def _run(z, target, C_, g, S, *, gamma=0.0, thresh=INF, min_kept=0, q16=0, ii=None, w=None, null_ce=False, want_grad=True,
         want_plane=True, want_stats=True, loss_scale=1.0):
    """One vitseg_hard_ce_loss call on guarded buffers; loss, grad, plane and stats come back on the CPU (None where not
    asked for).  null_ce: pass ce_opts = NULL (no ignore_index, no weights)."""
    B = z.shape[0]
    L = _lib.lib()
    zd = guarded(z.shape, torch.float32, z, name="lowres")
    td = guarded(target.shape, target.dtype, target, name="target")
    gd = guarded((B, C_, S, S), torch.float32, "nan", name="grad_logits") if want_grad else None
    scratch = guarded(L.vitseg_ce_scratch_bytes(B, S), torch.uint8, "nan", name="ce scratch")
    loss = guarded((1,), torch.float32, "nan", name="loss")
    plane = guarded((B, S, S), torch.float32, "nan", name="pixel_loss") if want_plane else None
    stats = guarded((4,), torch.int64, "nan", name="stats") if want_stats else None
    wd = guarded((C_,), torch.float32, torch.as_tensor(w, dtype=torch.float32), name="class_weight") if w is not None else None
    hbytes = int(_sym("vitseg_hard_loss_scratch_bytes")(B, S))
    hscr = guarded(hbytes, torch.uint8, "nan", name="hard scratch")
    h = _ext.CHardOptions(gamma, thresh, min_kept, q16, 0, hscr.data_ptr(), hbytes)
    ce, oscr = None, None
    if not null_ce:
        nbytes = int(_lib.ce_opts_symbol("vitseg_ce_options_scratch_bytes")(B, S))
        oscr = guarded(nbytes, torch.uint8, "nan", name="ce options scratch")
        o = _lib.CCEOptions(int(ii is not None), 0, 0 if ii is None else ii, wd.data_ptr() if wd is not None else None, 0.0,
                            oscr.data_ptr(), nbytes)
        ce = C.byref(o)
    else:
        assert ii is None and w is None
    snap = snapshot(zd, td, wd)
    ptr = lambda t: t.data_ptr() if t is not None else None
    _lib.check(_sym("vitseg_hard_ce_loss")(zd.data_ptr(), td.data_ptr(), int(target.dtype == torch.uint8), ptr(gd), scratch.data_ptr(),
                                           loss.data_ptr(), B, C_, g, S, ce, C.byref(h), loss_scale, ptr(plane), ptr(stats),
                                           _stream()))
    torch.cuda.synchronize()
    check(zd, td, gd, scratch, loss, plane, stats, wd, hscr, oscr)
    unchanged(snap)
    cpu = lambda t: t.cpu() if t is not None else None
    return SimpleNamespace(loss=loss.cpu()[0], grad=cpu(gd), plane=cpu(plane), stats=cpu(stats))


def _same(a, b):
    """Two runs gave the same bits in every output both hold."""
    for name in ("loss", "grad", "plane", "stats"):
        x, y = getattr(a, name), getattr(b, name)
        if x is not None and y is not None:
            x, y = (x.reshape(1), y.reshape(1)) if x.dim() == 0 else (x, y)
            if not torch.equal(_bits(x) if x.dtype == torch.float32 else x, _bits(y) if y.dtype == torch.float32 else y):
                return False
    return True


def _check(z, t, C_, g, S, *, gamma=0.0, thresh=INF, min_kept=0, q16=0, ii=None, w=None, null_ce=False, label=""):
    """Runs the call and checks the selection exactly and the values within the bounds.  Returns (run, H, k, tau bits)."""
    r = _run(z, t, C_, g, S, gamma=gamma, thresh=thresh, min_kept=min_kept, q16=q16, ii=ii, w=w, null_ce=null_ce)
    t64 = t.long()
    valid = torch.ones_like(t64, dtype=torch.bool) if ii is None else t64 != ii
    n_valid = int(valid.sum())
    plane = r.plane.numpy()
    assert (plane[~valid.numpy()] == SENTINEL).all()
    if thresh == INF and min_kept == 0 and q16 == 0:   # OHEM off: every valid pixel, tau = +0
        k, tau, H = 0, 0, valid.numpy()
    else:
        k, tau, H = HR.select_ref(plane, valid.numpy(), thresh, min_kept, q16)
    assert r.stats.tolist() == [n_valid, k, int(H.sum()), tau], (r.stats.tolist(), [n_valid, k, int(H.sum()), tau])
    Ht = torch.from_numpy(H)
    rows = (r.grad != 0).any(dim=1)
    assert torch.equal(rows, Ht), f"{int((rows != Ht).sum())} pixels differ between the non-zero gradient rows and H"
    outside = r.grad.permute(1, 0, 2, 3)[:, ~Ht]
    assert (outside == 0).all() and not torch.signbit(outside).any()   # +0.0f, every class
    # the plane against fp64, then loss and gradient over the kernel's own H
    up = ce_ref.upsample64(z, S)
    lse = torch.logsumexp(up, dim=1)
    loss_ref, grad_ref, den, ce64 = HR.hard_closed_form(up, t64, Ht, gamma, ii, w)
    e_pix = _ce_bounds(up, lse, C_)
    perr = (r.plane.double() - ce64)[valid].abs().max().item() if n_valid else 0.0
    assert perr <= e_pix, (perr, e_pix)
    wmax = 1.0 if w is None else float(torch.tensor(w, dtype=torch.float32).max())
    bound = e_pix + 6 * U * abs(float(loss_ref))
    g_bound = wmax * (e_pix + 20 * U) / float(den)
    err = abs(float(r.loss) - float(loss_ref))
    gerr = (r.grad.double() - grad_ref).abs().max().item()
    print(f"hard loss {label}: n_valid {n_valid} k {k} |H| {int(H.sum())}; plane err {perr:.2e} (e_pix {e_pix:.2e}), loss err "
          f"{err:.2e} (bound {bound:.2e}), grad err {gerr:.2e} (bound {g_bound:.2e})")
    assert torch.isfinite(r.loss) and err < bound, (err, bound)
    assert gerr < g_bound, (gerr, g_bound)
    return r, H, k, tau


def _random(B, C_, g, S, seed, scale=3.0):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C_, g, g, generator=gen).float() * scale
    t = torch.randint(0, C_, (B, S, S), generator=gen)
    return z, t, gen


def _weights(C_, gen):
    return (10.0 ** (torch.rand(C_, generator=gen) * 2.0 - 1.0)).float().tolist()


# ------------------------------------------------------------------ 1. the selection on random logits: every way to ask
# 2352 and 3200 pixels: ragged last blocks of 256 and of 1024; 9408: three blocks of pass A and of a histogram round (4096)
SHAPES = [(3, 2, 7, 28), (3, 3, 7, 28), (3, 17, 7, 28), (2, 3, 5, 40), (3, 5, 7, 56)]
OHEM = {
    "fraction": dict(q16=16384),
    "threshold only": dict(thresh=_thresh(0.7)),
    "floor only": dict(min_kept=500),
    "threshold below the floor's": dict(thresh=_thresh(0.9), min_kept=100),    # tau = the threshold
    "threshold above the floor's": dict(thresh=_thresh(1e-6), q16=32768),      # tau = ce_(k)
    "k = 1": dict(min_kept=1),
    "k = n_valid": dict(q16=65536),
    "min_kept > n_valid": dict(min_kept=10 ** 12),
}


@pytest.mark.parametrize("B,C_,g,S", SHAPES)
@pytest.mark.parametrize("how", list(OHEM))
def test_selection_and_values_on_random_logits(B, C_, g, S, how):
    kw = OHEM[how]
    z, t, gen = _random(B, C_, g, S, seed=B * 1000 + C_ * 10 + g)
    u8 = (C_ + len(how)) % 2 == 0                      # both target types over the table
    ii = 255 if C_ != 3 else None
    if ii is not None:
        t[torch.rand(t.shape, generator=gen) < 0.1] = ii
    w = _weights(C_, gen) if C_ == 17 else None
    gamma = 2.0 if C_ == 2 else 0.0
    r, H, k, tau = _check(z, t.to(torch.uint8) if u8 else t, C_, g, S, gamma=gamma, ii=ii, w=w, label=how, **kw)
    n_valid = int(r.stats[0])
    th = _fbits(kw.get("thresh", INF))
    if how == "threshold only":
        assert k == 0 and tau == th and 0 < H.sum() and (C_ == 17 or H.sum() < n_valid)   # 17 classes: hardly a pixel is easy
    elif how == "threshold below the floor's":
        assert k == 100 and tau == th and H.sum() > k
    elif how == "threshold above the floor's":
        assert tau < th and H.sum() >= k > 0
    elif how in ("k = n_valid", "min_kept > n_valid"):
        assert k == n_valid == H.sum()                 # keep_fraction = 1 with no threshold keeps every valid pixel
    elif how == "k = 1":
        assert k == 1 and H.sum() >= 1 and tau == int(r.plane.numpy().view(np.uint32)[H].max())
    else:
        assert H.sum() >= k > 0


# ------------------------------------------------------------------ 2. keys the radix rounds have to tell apart
def test_a_constant_logit_map_ties_every_pixel_and_all_are_kept():
    """Logits constant over the pixels (powers of two: the bilinear blend of equal values is then exact) and one label: every
    ce has the same bits, so asking for the single hardest pixel keeps them all."""
    B, C_, g, S = 3, 3, 7, 28
    z = torch.tensor([2.0, -1.0, 0.5]).view(1, 3, 1, 1).expand(B, C_, g, g).contiguous()
    t = torch.ones(B, S, S, dtype=torch.int64)
    r, H, k, tau = _check(z, t, C_, g, S, min_kept=1, label="ties")
    assert len(np.unique(r.plane.numpy().view(np.uint32))) == 1 and k == 1 and H.all()
    r, H, k, tau = _check(z, t.to(torch.uint8), C_, g, S, q16=1000, gamma=0.5, label="ties, focal")
    assert H.all()


def test_logits_scaled_down_leave_the_choice_to_the_last_rounds():
    """Logits of 1e-4: every ce is log C to four digits, the top 11 key bits are the same for all pixels and the first
    round picks one bin holding everything."""
    B, C_, g, S = 3, 2, 7, 28
    z, t, gen = _random(B, C_, g, S, seed=5, scale=1e-4)
    r, H, k, tau = _check(z, t.to(torch.uint8), C_, g, S, q16=16384, label="1e-4")
    bits = r.plane.numpy().view(np.uint32)
    assert len(np.unique(bits >> 20)) == 1 and len(np.unique(bits)) > 64 and k == 588 and 588 <= H.sum() < 700


def test_saturated_logits_put_most_keys_at_plus_zero():
    """A margin of 20 wherever a low-res cell's neighbours agree: lse - z_y is +0 on most pixels.  Half the pixels asked
    for reaches into the zeros: tau = +0 and every valid pixel is hard.  A quarter does not."""
    B, C_, g, S = 3, 3, 7, 28
    gen = torch.Generator().manual_seed(11)
    cls = torch.randint(0, C_, (B, g, g), generator=gen)
    cls[:, 1:, 1:] = cls[:, 1:2, 1:2]   # one class over 6 x 6 of the 7 x 7 cells
    z = 20.0 * torch.nn.functional.one_hot(cls, C_).permute(0, 3, 1, 2).float()
    t = ce_ref.upsample64(z, S).argmax(dim=1)
    t[torch.rand(t.shape, generator=gen) < 0.02] = 0   # a few wrong labels: ce = 20
    r, H, k, tau = _check(z, t, C_, g, S, q16=32768 + 16384, label="saturated, 3/4")
    zeros = float((r.plane == 0).float().mean())
    assert zeros > 0.5 and not torch.signbit(r.plane).any()   # +0, never -0
    assert tau == 0 and H.all()
    r, H, k, tau = _check(z, t, C_, g, S, q16=6554, label="saturated, 1/10")
    assert tau > 0 and k <= H.sum() < 0.5 * H.size


# ------------------------------------------------------------------ 3. ignored pixels, nothing valid, a bad label
@pytest.mark.parametrize("dtype,ii", [(torch.uint8, 255), (torch.int64, -100)])
def test_a_third_of_the_labels_ignored(dtype, ii):
    B, C_, g, S = 3, 3, 7, 28
    z, t, gen = _random(B, C_, g, S, seed=13)
    t[torch.rand(t.shape, generator=gen) < 1 / 3] = ii
    t[1, :20] = ii   # 560 pixels in a row: whole blocks without a valid pixel
    r, H, k, tau = _check(z, t.to(dtype), C_, g, S, gamma=2.0, thresh=_thresh(0.7), q16=16384, ii=ii, w=_weights(C_, gen),
                          label="a third ignored")
    assert 1000 < int(r.stats[0]) < 1400
    # nothing is read from under an ignored pixel: NaN logits under a fully ignored image change no bit
    t[0] = ii
    a = _run(z, t.to(dtype), C_, g, S, gamma=2.0, q16=16384, ii=ii)
    z2 = z.clone()
    z2[0] = float("nan")
    assert _same(a, _run(z2, t.to(dtype), C_, g, S, gamma=2.0, q16=16384, ii=ii)) and torch.isfinite(a.loss)


@pytest.mark.parametrize("kw", [dict(q16=16384, thresh=_thresh(0.7)), dict(gamma=2.0)], ids=["ohem", "focal"])
def test_everything_ignored(kw):
    B, C_, g, S = 3, 3, 7, 28
    z, t, gen = _random(B, C_, g, S, seed=17)
    t[:] = 255
    for tt in (t, t.to(torch.uint8)):
        r = _run(z, tt, C_, g, S, ii=255, **kw)
        assert torch.isnan(r.loss) and (r.grad == 0).all() and not torch.signbit(r.grad).any()
        assert (r.plane == SENTINEL).all()
        assert r.stats.tolist() == [0, 0, 0, _fbits(kw["thresh"]) if "thresh" in kw else 0]
        assert torch.isnan(_run(z, tt, C_, g, S, ii=255, want_grad=False, **kw).loss)


@pytest.mark.parametrize("dtype,ii,bad", [(torch.uint8, 255, 7), (torch.int64, -100, -5), (torch.int64, None, 3)])
def test_a_bad_label_is_nan_at_its_pixel_and_ranks_first(dtype, ii, bad):
    """NaN loss; NaN on that pixel's gradient row and nowhere else; the canonical NaN in the plane, which select_ref ranks
    above everything, so the pixel is hard under any request.  With every valid pixel kept the other rows are bit for bit
    those of a run with a valid label of weight 1 there: the bad label counts 1 in den."""
    B, C_, g, S = 3, 3, 7, 28
    z, t, gen = _random(B, C_, g, S, seed=19)
    if ii is not None:
        t[torch.rand(t.shape, generator=gen) < 0.1] = ii
    w = [0.5, 3.0, 1.0]
    t[1, 5, 9] = 2   # weight 1
    ok = _run(z, t.to(dtype), C_, g, S, gamma=2.0, q16=65536, ii=ii, w=w)
    assert torch.isfinite(ok.loss) and torch.isfinite(ok.grad).all()
    t[1, 5, 9] = bad
    valid = (torch.ones_like(t, dtype=torch.bool) if ii is None else t != ii).numpy()
    for kw in (dict(q16=65536), dict(min_kept=1), dict(thresh=_thresh(0.5))):
        r = _run(z, t.to(dtype), C_, g, S, gamma=2.0, ii=ii, w=w, **kw)
        assert torch.isnan(r.loss) and torch.isnan(r.grad[1, :, 5, 9]).all()
        assert int(r.plane.view(torch.int32)[1, 5, 9]) == 0x7fc00000
        rest = torch.ones(B, S, S, dtype=torch.bool)
        rest[1, 5, 9] = False
        assert torch.isfinite(r.grad.permute(1, 0, 2, 3)[:, rest]).all()
        k, tau, H = HR.select_ref(r.plane.numpy(), valid, kw.get("thresh", INF), kw.get("min_kept", 0), kw.get("q16", 0))
        assert r.stats.tolist() == [int(valid.sum()), k, int(H.sum()), tau] and H[1, 5, 9]
        assert torch.equal((r.grad != 0).any(dim=1), torch.from_numpy(H))
        if kw.get("q16") == 65536:
            assert torch.equal(_bits(r.grad.permute(1, 0, 2, 3)[:, rest]), _bits(ok.grad.permute(1, 0, 2, 3)[:, rest]))


# ------------------------------------------------------------------ 4. the focal factor alone
@pytest.mark.parametrize("B,C_,g,S", SHAPES)
@pytest.mark.parametrize("gamma", [0.5, 2.0, 5.0])
def test_focal_alone_against_fp64(B, C_, g, S, gamma):
    z, t, gen = _random(B, C_, g, S, seed=B * 1000 + C_ * 10 + g + int(gamma * 2))
    bare = B == 2                                     # one shape without ignore_index or weights: ce_opts = NULL
    ii = None if bare or C_ == 2 else 255
    if ii is not None:
        t[torch.rand(t.shape, generator=gen) < 0.1] = ii
    w = None if bare or C_ == 3 else _weights(C_, gen)
    r, H, k, tau = _check(z, t.to(torch.uint8) if C_ == 17 else t, C_, g, S, gamma=gamma, ii=ii, w=w, null_ce=bare,
                          label=f"focal {gamma}")
    assert k == 0 and tau == 0


def test_focal_factor_is_zero_not_nan_where_the_model_is_exactly_right():
    """q == 0 (ce = +0) with gamma > 0: f and m are 0, the row is written as zeros, nothing is NaN; the pixel is still in H
    (|H| counts it)."""
    B, C_, g, S = 3, 3, 7, 28
    z = torch.zeros(B, C_, g, g)
    z[:, 0] = 40.0
    t = torch.zeros(B, S, S, dtype=torch.int64)
    t[0, 0, :5] = 1   # five wrong labels: ce = 40
    for gamma in (0.5, 2.0):
        r = _run(z, t, C_, g, S, gamma=gamma, q16=65536)
        assert torch.isfinite(r.loss) and torch.isfinite(r.grad).all() and r.stats.tolist()[:3] == [2352, 2352, 2352]
        assert int((r.plane == 0).sum()) == 2352 - 5
        assert int((r.grad != 0).any(dim=1).sum()) == 5
        assert abs(float(r.loss) - 5 * 40.0 / 2352) < 1e-5


# ------------------------------------------------------------------ 5. the do-nothing paths, bit for bit
def _plain(z, t, C_, g, S, ii=None, w=None, use_opts=True, loss_scale=1.0):
    """vitseg_ce_loss_opts (use_opts) or vitseg_ce_loss on plain device buffers: (loss, grad) on the CPU."""
    B = z.shape[0]
    L = _lib.lib()
    zd, td = z.to(DEV), t.to(DEV)
    gd = torch.empty((B, C_, S, S), dtype=torch.float32, device=DEV)
    scratch = torch.empty(L.vitseg_ce_scratch_bytes(B, S), dtype=torch.uint8, device=DEV)
    loss = torch.empty(1, dtype=torch.float32, device=DEV)
    args = (zd.data_ptr(), td.data_ptr(), int(t.dtype == torch.uint8), gd.data_ptr(), scratch.data_ptr(), loss.data_ptr(), B, C_, g, S)
    if use_opts:
        nbytes = int(_lib.ce_opts_symbol("vitseg_ce_options_scratch_bytes")(B, S))
        oscr = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        wd = torch.tensor(w, dtype=torch.float32, device=DEV) if w is not None else None
        o = _lib.CCEOptions(int(ii is not None), 0, 0 if ii is None else ii, wd.data_ptr() if wd is not None else None, 0.0,
                            oscr.data_ptr(), nbytes)
        _lib.check(_lib.ce_opts_symbol("vitseg_ce_loss_opts")(*args, C.byref(o), loss_scale, _stream()))
    else:
        assert loss_scale == 1.0
        _lib.check(L.vitseg_ce_loss(*args, _stream()))
    torch.cuda.synchronize()
    return SimpleNamespace(loss=loss.cpu()[0], grad=gd.cpu(), plane=None, stats=None)


@pytest.mark.parametrize("B,C_,g,S", SHAPES)
def test_gamma_zero_with_ohem_off_is_the_existing_call_bitwise(B, C_, g, S):
    z, t, gen = _random(B, C_, g, S, seed=23 + C_)
    for tt in (t, t.to(torch.uint8)):   # no options either: vitseg_ce_loss
        want = _plain(z, tt, C_, g, S, use_opts=False)
        assert _same(want, _run(z, tt, C_, g, S, null_ce=True, want_plane=False, want_stats=False))
        assert _same(want, _run(z, tt, C_, g, S, want_plane=False, want_stats=False))
        got = _run(z, tt, C_, g, S, null_ce=True)   # ... and with the optional outputs, from the focal kernel at gamma = 0
        assert _same(want, got) and got.stats.tolist() == [B * S * S, 0, B * S * S, 0]
    t[torch.rand(t.shape, generator=gen) < 0.1] = 255
    w = _weights(C_, gen)
    for tt in (t, t.to(torch.uint8)):   # with ignore_index and weights: vitseg_ce_loss_opts
        want = _plain(z, tt, C_, g, S, ii=255, w=w, loss_scale=0.25)
        assert torch.isfinite(want.loss)
        assert _same(want, _run(z, tt, C_, g, S, ii=255, w=w, loss_scale=0.25, want_plane=False, want_stats=False))
        assert _same(want, _run(z, tt, C_, g, S, ii=255, w=w, loss_scale=0.25))
    # keep_fraction = 1 keeps every valid pixel: the sums run over the plane, the gradient is the plain one's
    full = _run(z, t, C_, g, S, ii=255, w=w, loss_scale=0.25, q16=65536)
    assert torch.equal(_bits(full.grad), _bits(want.grad)) and int(full.stats[2]) == int(full.stats[0]) == int((t != 255).sum())
    assert abs(float(full.loss) - float(want.loss)) <= 4 * U * abs(float(want.loss))   # another order of the same fp64 sum


# ------------------------------------------------------------------ 6. reproducibility, target types, the gradient scale
@pytest.mark.parametrize("kw", [dict(gamma=2.0), dict(gamma=2.0, q16=16384, thresh=_thresh(0.7)), dict(min_kept=300)],
                         ids=["focal", "focal+ohem", "ohem"])
def test_same_bits_on_every_call_for_both_target_types_and_any_scale(kw):
    B, C_, g, S = 2, 3, 5, 40
    z, t, gen = _random(B, C_, g, S, seed=29)
    t[torch.rand(t.shape, generator=gen) < 0.1] = 255
    w = _weights(C_, gen)
    a = _run(z, t, C_, g, S, ii=255, w=w, **kw)
    assert _same(a, _run(z, t, C_, g, S, ii=255, w=w, **kw))
    assert _same(a, _run(z, t.to(torch.uint8), C_, g, S, ii=255, w=w, **kw))
    nog = _run(z, t, C_, g, S, ii=255, w=w, want_grad=False, **kw)   # without the gradient: the same loss, plane and stats
    assert nog.grad is None and _same(a, nog)
    bare = _run(z, t, C_, g, S, ii=255, w=w, want_plane=False, want_stats=False, **kw)   # the plane in the scratch
    assert _same(a, bare)
    s = _run(z, t, C_, g, S, ii=255, w=w, loss_scale=0.25, **kw)   # a power of two: exactly
    assert torch.equal(_bits(s.loss.reshape(1)), _bits(a.loss.reshape(1))) and torch.equal(s.stats, a.stats)
    big = a.grad.abs() > 1e-30
    assert torch.equal(s.grad[big], (a.grad * 0.25)[big]) and torch.equal(s.grad == 0, a.grad == 0)


# ------------------------------------------------------------------ 7. through the model
@functools.lru_cache(maxsize=None)
def _model():
    c = Golden("tiny16_224_c2").cfg
    m = ViTSegmentationModel(c.num_classes, c.patch_size, c.hidden_size, c.num_hidden_layers, c.num_attention_heads,
                             image_size=c.image_size, intermediate_size=c.intermediate_size, device=DEV).eval()
    m.load_state_dict(Golden("tiny16_224_c2").state_dict())
    return m


def _model_batch(ii=None):
    m = _model()
    S = m.cfg.image_size
    x = torch.from_numpy(synth.make_images(m.cfg, 2, seed=0)).to(DEV)
    gen = torch.Generator().manual_seed(31)
    y = torch.randint(0, 2, (2, S, S), generator=gen)
    if ii is not None:
        y[torch.rand(y.shape, generator=gen) < 0.1] = ii
    return m, x, y.to(torch.uint8).to(DEV), S


def test_ce_loss_with_focal_and_ohem_is_the_standalone_loss_fed_through_backward():
    """model.ce_loss(..., focal_gamma=2, ohem_keep_fraction=0.25).backward() against vitseg_hard_ce_loss run standalone and
    its gradient fed through vitseg_backward's grad_logits entry: the same arena gradient bit for bit, only the source of
    the head gradient differs.  The training forward's low-res head output is not handed out; its full-size logits are (the
    bits the fused loss regenerates), and with g == S the taps are the identity, so the standalone call reads those."""
    m, x, y, S = _model_batch(ii=255)
    kw = dict(ignore_index=255, class_weight=[0.5, 2.0], focal_gamma=2.0, ohem_keep_fraction=0.25)
    m.zero_grad(set_to_none=True)
    loss, stats = m.ce_loss(x, y, return_stats=True, **kw)
    loss.backward()
    torch.cuda.synchronize()
    g1 = m.arena.grad.detach().clone()
    assert torch.isfinite(loss) and torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    n_valid, k, n_hard, tau = stats.tolist()
    assert n_valid == int((y != 255).sum()) and k == (n_valid * 16384 + 65535) >> 16 and k <= n_hard < k + 16

    logits = m._forward_train(x, True)
    B, C_ = 2, 2
    gd = guarded((B, C_, S, S), torch.float32, "nan", name="grad_logits")
    scr = torch.empty(_lib.lib().vitseg_ce_scratch_bytes(B, S), dtype=torch.uint8, device=DEV)
    oscr = torch.empty(int(_lib.ce_opts_symbol("vitseg_ce_options_scratch_bytes")(B, S)), dtype=torch.uint8, device=DEV)
    hscr = torch.empty(int(_sym("vitseg_hard_loss_scratch_bytes")(B, S)), dtype=torch.uint8, device=DEV)
    wd = torch.tensor([0.5, 2.0], device=DEV)
    o = _lib.CCEOptions(1, 0, 255, wd.data_ptr(), 0.0, oscr.data_ptr(), oscr.numel())
    h = _ext.CHardOptions(2.0, INF, 0, 16384, 0, hscr.data_ptr(), hscr.numel())
    loss2 = torch.empty(1, dtype=torch.float32, device=DEV)
    stats2 = torch.empty(4, dtype=torch.int64, device=DEV)
    _lib.check(_sym("vitseg_hard_ce_loss")(logits.data_ptr(), y.data_ptr(), 1, gd.data_ptr(), scr.data_ptr(), loss2.data_ptr(), B, C_,
                                           S, S, C.byref(o), C.byref(h), 1.0, None, stats2.data_ptr(), _stream()))
    torch.cuda.synchronize()
    check(gd)
    assert torch.equal(_bits(loss2), _bits(loss.detach().reshape(1))) and torch.equal(stats2, stats)
    g2, _ = m._backward(x, grad_logits=gd)
    torch.cuda.synchronize()
    assert torch.equal(_bits(g2), _bits(g1))
    m._release_grad_buffer(g2)
    # grad_scale scales the deposit and leaves the loss alone; the no-grad path selects the same number of pixels
    m.zero_grad(set_to_none=True)
    loss4 = m.ce_loss(x, y, grad_scale=0.25, **kw)
    loss4.backward()
    torch.cuda.synchronize()
    big = g1.abs() > 1e-30
    assert torch.equal(_bits(loss4.detach().reshape(1)), _bits(loss.detach().reshape(1)))
    assert torch.equal(m.arena.grad[big], (g1 * 0.25)[big])
    with torch.no_grad():
        loss_ng, stats_ng = m.ce_loss(x, y, return_stats=True, **kw)
    assert torch.isfinite(loss_ng) and stats_ng.tolist()[:2] == [n_valid, k]
    m.zero_grad(set_to_none=True)
    with pytest.raises(ValueError, match="label_smoothing"):
        m.ce_loss(x, y, label_smoothing=0.1, focal_gamma=2.0)


def test_ce_loss_at_the_defaults_launches_what_it_launched(monkeypatch):
    """No focal / OHEM argument: nothing asks for a symbol of the family, under autograd or without."""
    m, x, y, S = _model_batch()
    def boom(family, name):
        raise AssertionError(f"{name} requested at the defaults")
    monkeypatch.setattr(_ext, "ext_symbol", boom)
    m.zero_grad(set_to_none=True)
    loss = m.ce_loss(x, y, ignore_index=255)
    loss.backward()
    with torch.no_grad():
        m.ce_loss(x, y)
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    m.zero_grad(set_to_none=True)


def test_lightning_module_logs_train_kept_and_validates_with_ohem_off():
    from visiontransformer_amd.lightning import LightningViTModel
    m0, x, y, S = _model_batch()
    c = m0.cfg
    lm = LightningViTModel(c.num_classes, c.patch_size, c.hidden_size, c.num_hidden_layers, c.num_attention_heads,
                           image_size=c.image_size, intermediate_size=c.intermediate_size, device=DEV, focal_gamma=2.0,
                           ohem_keep_fraction=0.25)
    lm.model.load_state_dict(Golden("tiny16_224_c2").state_dict())
    lm.eval()
    y = y.long()
    lt = lm.training_step((x, y), 0)
    lt.backward()
    lv = lm.validation_step((x, y), 0)
    torch.cuda.synchronize()
    kept = float(lm.logged["train_kept"])
    assert lm.logged["train_kept"].is_cuda and 0.25 <= kept <= 1.0 and kept < 0.26
    assert torch.isfinite(lt) and torch.isfinite(lm.model.arena.grad).all()
    with torch.no_grad():
        want_v = lm.model.ce_loss(x, y, focal_gamma=2.0)                                  # OHEM off
        want_t = lm.model.ce_loss(x, y, focal_gamma=2.0, ohem_keep_fraction=0.25)
    assert torch.equal(_bits(lv.reshape(1)), _bits(want_v.reshape(1)))
    assert float(want_t) > float(want_v) and abs(float(lt.detach()) - float(want_t)) < 1e-3 * float(want_t)   # the hard quarter alone


# ------------------------------------------------------------------ 8. argument errors: nothing is launched
def test_argument_errors_leave_the_outputs_untouched():
    B, C_, g, S = 3, 3, 7, 28
    z, t, gen = _random(B, C_, g, S, seed=37)
    zd, td = z.to(DEV), t.to(torch.uint8).to(DEV)
    gd = guarded((B, C_, S, S), torch.float32, "nan", name="grad_logits")
    loss = guarded((1,), torch.float32, "nan", name="loss")
    plane = guarded((B, S, S), torch.float32, "nan", name="pixel_loss")
    stats = guarded((4,), torch.int64, "nan", name="stats")
    scr = guarded(_lib.lib().vitseg_ce_scratch_bytes(B, S), torch.uint8, "nan", name="ce scratch")
    need = int(_sym("vitseg_hard_loss_scratch_bytes")(B, S))
    hscr = guarded(need, torch.uint8, "nan", name="hard scratch")
    nbytes = int(_lib.ce_opts_symbol("vitseg_ce_options_scratch_bytes")(B, S))
    oscr = guarded(nbytes, torch.uint8, "nan", name="ce options scratch")
    fn = _sym("vitseg_hard_ce_loss")
    ok = dict(gamma=2.0, t=0.5, m=10, q=100, scr=hscr.data_ptr(), n=need)

    def call(eps=0.0, ce_scr=oscr.data_ptr(), ce_n=nbytes, null_hard=False, lowres=zd.data_ptr(), **kw):
        o = dict(ok, **kw)
        h = _ext.CHardOptions(o["gamma"], o["t"], o["m"], o["q"], 0, o["scr"], o["n"])
        ce = _lib.CCEOptions(0, 0, 0, None, eps, ce_scr, ce_n)
        return fn(lowres, td.data_ptr(), 1, gd.data_ptr(), scr.data_ptr(), loss.data_ptr(), B, C_, g, S, C.byref(ce),
                  None if null_hard else C.byref(h), 1.0, plane.data_ptr(), stats.data_ptr(), _stream())
    nan = float("nan")
    for kw in (dict(gamma=-0.5), dict(gamma=nan), dict(gamma=INF), dict(t=nan), dict(t=-1.0), dict(m=-1), dict(q=-1), dict(q=65537),
               dict(scr=None), dict(scr=hscr.data_ptr() + 4), dict(n=need - 1), dict(eps=0.1), dict(eps=1.5), dict(ce_scr=None),
               dict(ce_n=8), dict(null_hard=True), dict(lowres=None)):
        assert call(**kw) == _lib.EINVAL, kw
    torch.cuda.synchronize()
    check(gd, loss, plane, stats, scr, hscr, oscr)
    for t_ in (gd, loss, plane):
        assert torch.isnan(t_).all()
    assert (stats == -1).all() and (hscr == 255).all() and (scr == 255).all()   # the poison: not a byte was written
    assert call() == _lib.OK   # and the valid call goes through
    torch.cuda.synchronize()
    check(gd, loss, plane, stats, scr, hscr, oscr)
    assert torch.isfinite(loss).all() and torch.isfinite(gd).all() and int(stats[0]) == B * S * S


def test_backward_hard_argument_errors_and_its_null_form():
    """vitseg_backward_hard: EINVAL before any launch (not even the arena's memset) for the hard options together with
    grad_logits and for each bad option; hard == NULL is vitseg_backward_opts, bit for bit."""
    m = ViTSegmentationModel(3, 16, 64, 1, 1, image_size=64, intermediate_size=128, device=DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(m.cfg, seed=4).items()})
    m.eval()
    S = 64
    x = torch.from_numpy(synth.make_images(m.cfg, 1, seed=4)).to(DEV)
    t = torch.randint(0, 3, (1, S, S), generator=torch.Generator().manual_seed(1)).to(torch.uint8).to(DEV)
    m._forward_train(x, False)
    ws = m._train_workspace(1, S)
    grads = guarded(m.arena.shape, torch.float32, "nan", name="grads")
    loss = guarded((1,), torch.float32, "nan", name="loss")
    stats = guarded((4,), torch.int64, "nan", name="stats")
    gl = torch.zeros(1, 3, S, S, device=DEV)
    need = int(_sym("vitseg_hard_loss_scratch_bytes")(1, S))
    hscr = guarded(need, torch.uint8, "nan", name="hard scratch")
    nbytes = int(_lib.ce_opts_symbol("vitseg_ce_options_scratch_bytes")(1, S))
    oscr = guarded(nbytes, torch.uint8, "nan", name="ce options scratch")
    cfg = C.byref(_lib.CConfig.from_config(m.cfg))
    fn = _sym("vitseg_backward_hard")

    def call(h, ce=None, target=t, grad_logits=None):
        return fn(cfg, S, m.arena.data_ptr(), None, x.data_ptr(), 1, m.precision, 0.0, 0,
                  target.data_ptr() if target is not None else None, 1, grad_logits.data_ptr() if grad_logits is not None else None,
                  grads.data_ptr(), loss.data_ptr(), 1.0, None, ws.data_ptr(), ws.numel(), _stream(),
                  C.byref(ce) if ce is not None else None, C.byref(h) if h is not None else None, stats.data_ptr())
    H_ = lambda gamma=2.0, th=INF, mk=0, q=16384, scr=hscr.data_ptr(), n=need: _ext.CHardOptions(gamma, th, mk, q, 0, scr, n)
    assert call(H_(), target=None, grad_logits=gl) == _lib.EINVAL
    for h in (H_(gamma=-1.0), H_(gamma=float("nan")), H_(th=-1.0), H_(th=float("nan")), H_(mk=-1), H_(q=65537), H_(q=-1),
              H_(scr=None), H_(scr=hscr.data_ptr() + 4), H_(n=need - 1)):
        assert call(h) == _lib.EINVAL
    assert call(H_(), ce=_lib.CCEOptions(0, 0, 0, None, 0.1, oscr.data_ptr(), nbytes)) == _lib.EINVAL   # label smoothing
    torch.cuda.synchronize()
    check(grads, loss, stats, hscr, oscr)
    assert torch.isnan(grads).all() and torch.isnan(loss).all() and (stats == -1).all() and (hscr == 255).all()
    assert call(H_()) == _lib.OK
    torch.cuda.synchronize()
    check(grads, loss, stats, hscr, oscr)
    assert torch.isfinite(grads).all() and torch.isfinite(loss).all() and stats.tolist()[:2] == [S * S, S * S // 4]
    # hard == NULL: vitseg_backward_opts (stats is not touched)
    stats.fill_(-1)
    m._forward_train(x, False)
    assert call(None) == _lib.OK
    torch.cuda.synchronize()
    g0, l0 = grads.clone(), loss.clone()
    grads.fill_(float("nan"))
    m._forward_train(x, False)
    args = (m.arena.data_ptr(), None, x.data_ptr(), 1, m.precision, 0.0, 0, t.data_ptr(), 1, None, grads.data_ptr(), loss.data_ptr(),
            1.0, None, ws.data_ptr(), ws.numel(), _stream())
    _lib.check(_lib.ce_opts_symbol("vitseg_backward_opts")(cfg, S, *args, None))
    torch.cuda.synchronize()
    check(grads, loss, stats)
    assert torch.equal(_bits(grads), _bits(g0)) and torch.equal(_bits(loss), _bits(l0)) and (stats == -1).all()
