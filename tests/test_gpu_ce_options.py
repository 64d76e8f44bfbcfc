"""GPU (-m gpu): the fused cross-entropy with ignore_index, class weights and label smoothing (vitseg_ce_loss_opts,
vitseg_backward_opts, ViTSegmentationModel.ce_loss) against torch's CPU F.cross_entropy in fp64 (tests/ce_ref.py).
Every buffer is guard-banded; the options' scratch has exactly the queried size and arrives NaN-poisoned.

Tolerances (derived, not fitted).  `_ce_bounds` restates test_gpu_loss_cast.py: e_pix bounds the fp32 error of lse - z_c at
one pixel for any class c.  With K = (1 - eps) w_max + eps sum(w) / C:
  - a kept pixel's loss term (1 - eps) w[y] (lse - z_y) + (eps / C) sum_c w[c] (lse - z_c) is off by at most
    ((1 - eps) w[y] + eps sum(w) / C) e_pix; summed over the kept pixels and divided by den = sum_keep w[y] that is
    e_pix ((1 - eps) + eps (sum(w) / C) n_keep / den).  The factors (1 - eps) w[y] and eps / C are fp32 (3 roundings), the
    products and sums fp64, the result is rounded to fp32 once: every term is >= 0, so these add 6 u |loss| in all.
  - a gradient entry [(1 - eps) w[y] (p_c - 1[c = y]) + (eps / C) (p_c sum(w) - w[c])] scale / den carries the error of
    p_c (<= e_pix + 8 u as in the plain kernel: p <= 1) times at most K, plus about a dozen fp32 roundings (the two
    factors, fp32 sum(w), the products, the fma, (float) den, the division, the final product) of quantities bounded by K:
    K (e_pix + 20 u) |scale| / den.
  - den is an fp64 sum of fp32 weights, exact to one fp64 rounding per add: relative 2^-53 n, nothing at this scale."""
import ctypes as C

import pytest
import torch

import ce_ref
from guard import check, guarded, snapshot, unchanged
from visiontransformer_amd import _lib, synth
from visiontransformer_amd.model import ViTSegmentationModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -23   # fp32 unit roundoff (half an ulp of 1)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ce_bounds(up, lse, C_):
    """Per-pixel error of the fp32 lse - z_c (test_gpu_loss_cast._ce_bounds): the re-generated logit (an fmaf chain of 4
    products, <= 4 u |z|), the online log-sum-exp (<= 4 u |lse| + 4 (C + 2) u) and the picked logit."""
    zmax = up.abs().max().item()
    return 4 * U * lse.abs().max().item() + 8 * U * zmax + 4 * (C_ + 2) * U


def _opts_run(z, target, C_, g, S, ii=None, w=None, eps=0.0, want_grad=True, loss_scale=1.0, plain=False, cpu=True):
    """One vitseg_ce_loss_opts call (plain=True: vitseg_ce_loss) on guarded buffers.  Returns (loss, grad) on the CPU, or
    on the device with cpu=False."""
    B = z.shape[0]
    L = _lib.lib()
    zd = guarded(z.shape, torch.float32, z, name="lowres")
    td = guarded(target.shape, target.dtype, target, name="target")
    gd = guarded((B, C_, S, S), torch.float32, "nan", name="grad_logits") if want_grad else None
    scratch = guarded(L.vitseg_ce_scratch_bytes(B, S), torch.uint8, "nan", name="ce scratch")
    loss = guarded((1,), torch.float32, "nan", name="loss")
    wd = guarded((C_,), torch.float32, torch.as_tensor(w, dtype=torch.float32), name="class_weight") if w is not None else None
    args = (zd.data_ptr(), td.data_ptr(), int(target.dtype == torch.uint8), gd.data_ptr() if gd is not None else None,
            scratch.data_ptr(), loss.data_ptr(), B, C_, g, S)
    snap = snapshot(zd, td, wd)
    if plain:
        assert ii is None and w is None and eps == 0.0 and loss_scale == 1.0
        _lib.check(L.vitseg_ce_loss(*args, _stream()))
        oscr = None
    else:
        nbytes = int(_lib.ce_opts_symbol("vitseg_ce_options_scratch_bytes")(B, S))
        oscr = guarded(nbytes, torch.uint8, "nan", name="ce options scratch")
        o = _lib.CCEOptions(int(ii is not None), 0, 0 if ii is None else ii, wd.data_ptr() if wd is not None else None,
                            eps, oscr.data_ptr(), nbytes)
        _lib.check(_lib.ce_opts_symbol("vitseg_ce_loss_opts")(*args, C.byref(o), loss_scale, _stream()))
    torch.cuda.synchronize()
    check(zd, td, gd, scratch, loss, wd, oscr)
    unchanged(snap)
    if not cpu:
        return loss.clone(), gd
    return loss.cpu()[0], (gd.cpu() if gd is not None else None)


def _logits(B, C_, g, kind, gen):
    z = torch.randn(B, C_, g, g, generator=gen).float() * 3.0
    if kind == "big":   # logits at +-60: exp of the raw values would overflow without the running max
        z = (torch.rand(B, C_, g, g, generator=gen) * 120.0 - 60.0).float()
    elif kind == "ties":
        z[:, 1] = z[:, 0]
        z[0] = z[0, :1].expand(C_, g, g)
    return z


def _weights(C_, kind, gen):
    """span: log-uniform over 1e-3 .. 1e3 with both ends present; zero: the same with class 1 at weight 0."""
    if kind is None:
        return None
    w = 10.0 ** (torch.rand(C_, generator=gen) * 6.0 - 3.0)
    w[0], w[-1] = 1e-3, 1e3
    if kind == "zero":
        w[1 if C_ > 2 else 0] = 0.0
    return w.float().tolist()


# ------------------------------------------------------------------ 1. defaults: the plain calls, bit for bit
@pytest.mark.parametrize("B,C_,g,S,kind", [
    (2, 2, 14, 224, "randn"), (1, 17, 14, 224, "randn"), (2, 32, 32, 512, "randn"), (1, 1, 16, 64, "randn"),
    (2, 5, 7, 28, "randn"), (2, 5, 7, 28, "big"), (2, 17, 14, 224, "big"), (2, 4, 7, 28, "ties"),
    (64, 2, 32, 512, "randn"), (32, 17, 32, 512, "randn")])   # the last two: 65 536 and 32 768 partial sums
def test_default_options_equal_plain_ce_bitwise(B, C_, g, S, kind):
    """No ignored label, NULL weights, eps = 0 on valid labels: vitseg_ce_loss_opts gives vitseg_ce_loss's bits, loss and
    gradient, for uint8 and int64 targets (the shapes of test_ce_loss_against_fp64)."""
    gen = torch.Generator().manual_seed(B * 1000 + C_ * 10 + g)
    z = _logits(B, C_, g, kind, gen)
    t64 = torch.randint(0, C_, (B, S, S), generator=gen)
    for t in (t64, t64.to(torch.uint8)):
        loss_p, grad_p = _opts_run(z, t, C_, g, S, plain=True, cpu=False)
        loss_o, grad_o = _opts_run(z, t, C_, g, S, cpu=False)
        assert torch.isfinite(loss_p).all()
        assert torch.equal(_bits(loss_o), _bits(loss_p))
        assert torch.equal(_bits(grad_o), _bits(grad_p))
        del grad_p, grad_o
    # ... and with a gradient scale, against the plain kernels behind a NULL options pointer
    L = _lib.lib()
    zd, td = z.to(DEV), t64.to(DEV)
    out = []
    for use_opts in (False, True):
        gd = torch.empty((B, C_, S, S), dtype=torch.float32, device=DEV)
        scratch = torch.empty(L.vitseg_ce_scratch_bytes(B, S), dtype=torch.uint8, device=DEV)
        nbytes = int(_lib.ce_opts_symbol("vitseg_ce_options_scratch_bytes")(B, S))
        oscr = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        loss = torch.empty(1, dtype=torch.float32, device=DEV)
        o = _lib.CCEOptions(0, 0, 0, None, 0.0, oscr.data_ptr(), nbytes)
        _lib.check(_lib.ce_opts_symbol("vitseg_ce_loss_opts")(
            zd.data_ptr(), td.data_ptr(), 0, gd.data_ptr(), scratch.data_ptr(), loss.data_ptr(), B, C_, g, S,
            C.byref(o) if use_opts else None, 0.25, _stream()))
        torch.cuda.synchronize()
        out.append((loss, gd))
    assert torch.equal(_bits(out[0][0]), _bits(out[1][0])) and torch.equal(_bits(out[0][1]), _bits(out[1][1]))


def _small_model(C_=3, S=64, precision="fp32", seed=4):
    m = ViTSegmentationModel(C_, 16, 64, 1, 1, image_size=S, intermediate_size=128, precision=precision, device=DEV)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(m.cfg, seed=seed).items()}
    m.load_state_dict(sd)
    m.eval()   # no dropout: the forward is a pure function of (parameters, x)
    return m


def _raw_backward(m, x, target, opts, via_opts, loss_scale=1.0):
    """vitseg_backward (via_opts=False) or vitseg_backward_opts with `opts` (a CCEOptions or None) after a fresh training
    forward, into a guarded gradient arena.  Returns (grads, loss) on the device."""
    B, S = x.shape[0], int(x.shape[-1])
    m._forward_train(x, False, interp=S != m.cfg.image_size)
    ws = m._train_workspace(B, S)
    grads = guarded(m.arena.shape, torch.float32, "nan", name="grads")
    loss = guarded((1,), torch.float32, "nan", name="loss")
    args = (m.arena.data_ptr(), m._bf16_arena().data_ptr() if m._bf16_arena() is not None else None, x.data_ptr(), B,
            m.precision, 0.0, 0, target.data_ptr(), int(target.dtype == torch.uint8), None, grads.data_ptr(), loss.data_ptr(),
            float(loss_scale), None, ws.data_ptr(), ws.numel(), _stream())
    cfg = C.byref(_lib.CConfig.from_config(m.cfg))
    if via_opts:
        _lib.check(_lib.ce_opts_symbol("vitseg_backward_opts")(cfg, S, *args, C.byref(opts) if opts is not None else None))
    else:
        assert S == m.cfg.image_size
        _lib.check(_lib.lib().vitseg_backward(cfg, *args))
    torch.cuda.synchronize()
    check(grads, loss)
    return grads, loss


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_backward_opts_null_and_defaults_equal_backward_bitwise(precision):
    """vitseg_backward_opts(NULL) is vitseg_backward; so is a default-valued options struct: the same gradient arena."""
    m = _small_model(precision=precision)
    S = m.cfg.image_size
    x = torch.from_numpy(synth.make_images(m.cfg, 2, seed=4)).to(DEV)
    t = torch.randint(0, 3, (2, S, S), generator=torch.Generator().manual_seed(1)).to(torch.uint8).to(DEV)
    g0, l0 = _raw_backward(m, x, t, None, via_opts=False, loss_scale=0.5)
    assert torch.isfinite(g0).all() and torch.isfinite(l0).all()
    g1, l1 = _raw_backward(m, x, t, None, via_opts=True, loss_scale=0.5)
    assert torch.equal(_bits(g1), _bits(g0)) and torch.equal(_bits(l1), _bits(l0))
    nbytes = int(_lib.ce_opts_symbol("vitseg_ce_options_scratch_bytes")(2, S))
    oscr = guarded(nbytes, torch.uint8, "nan", name="ce options scratch")
    o = _lib.CCEOptions(0, 0, 0, None, 0.0, oscr.data_ptr(), nbytes)
    g2, l2 = _raw_backward(m, x, t, o, via_opts=True, loss_scale=0.5)
    check(oscr)
    assert torch.equal(_bits(g2), _bits(g0)) and torch.equal(_bits(l2), _bits(l0))


def test_backward_opts_argument_errors():
    """EINVAL before any launch: options together with grad_logits, smoothing out of range, scratch too small or null."""
    m = _small_model()
    S = m.cfg.image_size
    x = torch.from_numpy(synth.make_images(m.cfg, 1, seed=4)).to(DEV)
    t = torch.zeros(1, S, S, dtype=torch.uint8, device=DEV)
    m._forward_train(x, False)
    ws = m._train_workspace(1, S)
    grads = guarded(m.arena.shape, torch.float32, "nan", name="grads")
    loss = guarded((1,), torch.float32, "nan", name="loss")
    gl = torch.zeros(1, 3, S, S, device=DEV)
    nbytes = int(_lib.ce_opts_symbol("vitseg_ce_options_scratch_bytes")(1, S))
    oscr = guarded(nbytes, torch.uint8, "nan", name="ce options scratch")
    cfg = C.byref(_lib.CConfig.from_config(m.cfg))
    fn = _lib.ce_opts_symbol("vitseg_backward_opts")

    def call(o, target=t, grad_logits=None):
        return fn(cfg, S, m.arena.data_ptr(), None, x.data_ptr(), 1, m.precision, 0.0, 0,
                  target.data_ptr() if target is not None else None, 1, grad_logits.data_ptr() if grad_logits is not None else None,
                  grads.data_ptr(), loss.data_ptr(), 1.0, None, ws.data_ptr(), ws.numel(), _stream(), C.byref(o))
    ok = _lib.CCEOptions(1, 0, 255, None, 0.1, oscr.data_ptr(), nbytes)
    assert call(ok, target=None, grad_logits=gl) == _lib.EINVAL
    assert call(_lib.CCEOptions(1, 0, 255, None, 1.5, oscr.data_ptr(), nbytes)) == _lib.EINVAL
    assert call(_lib.CCEOptions(1, 0, 255, None, -0.1, oscr.data_ptr(), nbytes)) == _lib.EINVAL
    assert call(_lib.CCEOptions(1, 0, 255, None, float("nan"), oscr.data_ptr(), nbytes)) == _lib.EINVAL
    assert call(_lib.CCEOptions(1, 0, 255, None, 0.1, oscr.data_ptr(), nbytes - 1)) == _lib.EINVAL
    assert call(_lib.CCEOptions(1, 0, 255, None, 0.1, None, nbytes)) == _lib.EINVAL
    torch.cuda.synchronize()
    check(grads, loss, oscr)
    assert torch.isnan(grads).all() and torch.isnan(loss).all()   # nothing was launched: not even the arena's memset
    # the same checks in front of vitseg_ce_loss_opts
    z = torch.zeros(1, 3, 4, 4, device=DEV)
    scr = torch.empty(_lib.lib().vitseg_ce_scratch_bytes(1, S), dtype=torch.uint8, device=DEV)
    ce = _lib.ce_opts_symbol("vitseg_ce_loss_opts")
    for o in (_lib.CCEOptions(0, 0, 0, None, 2.0, oscr.data_ptr(), nbytes), _lib.CCEOptions(0, 0, 0, None, 0.0, oscr.data_ptr(), 8),
              _lib.CCEOptions(0, 0, 0, None, 0.0, None, nbytes)):
        assert ce(z.data_ptr(), t.data_ptr(), 1, None, scr.data_ptr(), loss.data_ptr(), 1, 3, 4, S, C.byref(o), 1.0,
                  _stream()) == _lib.EINVAL
    assert ce(None, t.data_ptr(), 1, None, scr.data_ptr(), loss.data_ptr(), 1, 3, 4, S, C.byref(ok), 1.0, _stream()) == _lib.EINVAL
    torch.cuda.synchronize()
    check(loss, oscr)
    assert torch.isnan(loss).all()
    assert call(ok) == _lib.OK   # and the valid call goes through
    torch.cuda.synchronize()
    check(grads, loss, oscr)
    assert torch.isfinite(grads).all() and torch.isfinite(loss).all()


# ------------------------------------------------------------------ 2. each option alone and all together, against fp64
def _targets(B, C_, S, ii, frac, whole_image, gen):
    t = torch.randint(0, C_, (B, S, S), generator=gen)
    if ii is not None:
        if frac > 0:
            t[torch.rand(B, S, S, generator=gen) < frac] = ii
        if whole_image is not None:
            t[whole_image] = ii
    return t


CASES = [
    # B, C, g, S, logits, ignore_index, ignored fraction, fully ignored image, weights, eps
    (2, 2, 14, 224, "randn", 255, 0.1, None, None, 0.0),      # ignore_index alone (uint8 void label)
    (2, 5, 7, 28, "randn", -100, 0.1, None, None, 0.0),       # ... torch's default
    (2, 5, 7, 28, "randn", None, 0.0, None, "span", 0.0),     # weights alone, 1e-3 .. 1e3
    (2, 5, 7, 28, "randn", None, 0.0, None, "zero", 0.0),     # ... with a zero weight
    (2, 5, 7, 28, "randn", None, 0.0, None, None, 0.1),       # smoothing alone
    (2, 5, 7, 28, "ties", None, 0.0, None, None, 1.0),        # ... eps = 1: the picked class drops out
    (2, 5, 7, 28, "randn", 255, 0.0, None, "zero", 0.1),      # an ignore_index no pixel carries (0 % ignored)
    (1, 17, 14, 224, "randn", -100, 0.1, None, "zero", 0.1),  # all together
    (2, 17, 14, 224, "big", 255, 0.1, 0, "span", 0.1),        # logits at +-60, image 0 fully ignored
    (2, 32, 32, 512, "randn", 255, 0.1, None, "zero", 1.0),
    (3, 2, 7, 28, "big", -100, 0.1, 1, "span", 1.0),          # image 1 fully ignored
]


@pytest.mark.parametrize("B,C_,g,S,kind,ii,frac,whole,wkind,eps", CASES)
def test_ce_options_against_fp64(B, C_, g, S, kind, ii, frac, whole, wkind, eps):
    gen = torch.Generator().manual_seed(B * 1000 + C_ * 10 + g + int(eps * 100))
    z = _logits(B, C_, g, kind, gen)
    w = _weights(C_, wkind, gen)
    t64 = _targets(B, C_, S, ii, frac, whole, gen)
    loss_ref, grad_ref, lse, up = ce_ref.ce_ref(z, t64, S, ii, w, eps)
    assert torch.isfinite(loss_ref)

    loss64, grad64 = _opts_run(z, t64, C_, g, S, ii, w, eps)
    loss_again, grad_again = _opts_run(z, t64, C_, g, S, ii, w, eps)
    assert torch.equal(_bits(loss_again), _bits(loss64)) and torch.equal(_bits(grad_again), _bits(grad64))
    if ii is None or 0 <= ii <= 255:   # uint8 targets: the same bits
        loss8, grad8 = _opts_run(z, t64.to(torch.uint8), C_, g, S, ii, w, eps)
        assert torch.equal(_bits(loss8), _bits(loss64)) and torch.equal(_bits(grad8), _bits(grad64))
    loss_nog, _ = _opts_run(z, t64, C_, g, S, ii, w, eps, want_grad=False)
    assert torch.equal(_bits(loss_nog), _bits(loss64))
    assert torch.isfinite(grad64).all()

    wt = torch.ones(C_, dtype=torch.float64) if w is None else torch.tensor(w, dtype=torch.float32).double()
    keep = torch.ones_like(t64, dtype=torch.bool) if ii is None else t64 != ii
    den = float(wt[t64[keep]].sum())
    e_pix = _ce_bounds(up, lse, C_)
    K = (1.0 - eps) * float(wt.max()) + eps * float(wt.sum()) / C_
    bound = e_pix * ((1.0 - eps) + eps * float(wt.sum()) / C_ * int(keep.sum()) / den) + 6 * U * abs(float(loss_ref))
    g_bound = K * (e_pix + 20 * U) / den
    err = abs(float(loss64) - float(loss_ref))
    gerr = (grad64.double() - grad_ref).abs().max().item()
    print(f"ce options loss err {err:.2e} (bound {bound:.2e}), grad err {gerr:.2e} (bound {g_bound:.2e})")
    assert err < bound, (err, bound)
    assert gerr < g_bound, (gerr, g_bound)
    # ignored pixels: exact zeros for every class
    if ii is not None:
        assert (grad64.permute(1, 0, 2, 3)[:, ~keep] == 0).all()
    # the gradient scale multiplies the gradient and leaves the loss alone (a power of two: exactly)
    loss_s, grad_s = _opts_run(z, t64, C_, g, S, ii, w, eps, loss_scale=0.25)
    assert torch.equal(_bits(loss_s), _bits(loss64))
    big = grad64.abs() > 1e-30
    assert torch.equal(grad_s[big], (grad64 * 0.25)[big])


# ------------------------------------------------------------------ 3. ignored pixels
@pytest.mark.parametrize("dtype,ii", [(torch.uint8, 255), (torch.int64, -100), (torch.int64, 255)])
def test_ignored_pixels_get_exact_zeros_and_their_logits_do_not_matter(dtype, ii):
    """A void label is not NaN (what the plain call makes of it): finite loss, G == 0.0f for every class at the ignored
    pixels, and nothing read from under them -- another set of logits under a fully ignored image changes no output bit."""
    B, C_, g, S = 2, 5, 7, 28
    gen = torch.Generator().manual_seed(23)
    z = torch.randn(B, C_, g, g, generator=gen).float()
    t = torch.randint(0, C_, (B, S, S), generator=gen)
    t[1][torch.rand(S, S, generator=gen) < 0.1] = ii
    t[0] = ii
    t = t.to(dtype)
    w = _weights(C_, "span", gen)
    loss, grad = _opts_run(z, t, C_, g, S, ii, w, 0.1)
    assert torch.isfinite(loss) and torch.isfinite(grad).all()
    ign = (t.long() == ii)
    assert int(ign[1].sum()) > 0
    g_ign = grad.permute(1, 0, 2, 3)[:, ign]
    assert (g_ign == 0).all() and not torch.signbit(g_ign).any()     # +0.0f, every class
    assert (grad.permute(1, 0, 2, 3)[:, ~ign] != 0).any()
    z2 = z.clone()
    z2[0] = -z[0] * 50.0 + 7.0
    loss2, grad2 = _opts_run(z2, t, C_, g, S, ii, w, 0.1)
    assert torch.equal(_bits(loss2), _bits(loss)) and torch.equal(_bits(grad2), _bits(grad))
    z2[0] = float("nan")
    loss3, grad3 = _opts_run(z2, t, C_, g, S, ii, w, 0.1)
    assert torch.equal(_bits(loss3), _bits(loss)) and torch.equal(_bits(grad3), _bits(grad))


# ------------------------------------------------------------------ 4. den == 0
@pytest.mark.parametrize("case", ["all ignored", "kept pixels have weight 0", "kept pixels have weight 0, smoothed"])
def test_zero_denominator_is_nan_as_in_torch(case):
    B, C_, g, S = 2, 5, 7, 28
    gen = torch.Generator().manual_seed(29)
    z = torch.randn(B, C_, g, g, generator=gen).float()
    ii, w, eps = 255, None, 0.0
    t = torch.full((B, S, S), ii, dtype=torch.int64)
    if case != "all ignored":
        t[1] = 2
        t[1, :4] = ii
        w = [1.0, 2.0, 0.0, 0.5, 3.0]
        eps = 0.1 if "smoothed" in case else 0.0
    keep = t != ii
    loss_ref, grad_ref, _, _ = ce_ref.ce_ref(z, t, S, ii, w, eps)
    assert torch.isnan(loss_ref)
    assert torch.isnan(grad_ref.permute(1, 0, 2, 3)[:, keep]).all() and (grad_ref.permute(1, 0, 2, 3)[:, ~keep] == 0).all()
    for tt in (t, t.to(torch.uint8)):
        loss, grad = _opts_run(z, tt, C_, g, S, ii, w, eps)
        assert torch.isnan(loss)
        assert torch.isnan(grad.permute(1, 0, 2, 3)[:, keep]).all()
        assert (grad.permute(1, 0, 2, 3)[:, ~keep] == 0).all()
        loss_nog, _ = _opts_run(z, tt, C_, g, S, ii, w, eps, want_grad=False)
        assert torch.isnan(loss_nog)


# ------------------------------------------------------------------ 5. a bad label that is not ignore_index
@pytest.mark.parametrize("dtype,ii,bad", [(torch.uint8, 255, 7), (torch.int64, -100, -5), (torch.int64, -100, 5),
                                          (torch.int64, 255, -100), (torch.uint8, None, 255)])
def test_bad_label_that_is_not_ignored_is_nan_at_its_pixel_only(dtype, ii, bad):
    """NaN loss and NaN gradient at that pixel (every class); every other pixel's gradient is bit for bit that of the run
    with a valid label there (one of weight 1, which is what the bad label counts in the denominator)."""
    B, C_, g, S = 2, 5, 7, 28
    gen = torch.Generator().manual_seed(31)
    z = torch.randn(B, C_, g, g, generator=gen).float()
    t = torch.randint(0, C_, (B, S, S), generator=gen)
    if ii is not None:
        t[torch.rand(B, S, S, generator=gen) < 0.1] = ii
    w = [0.5, 3.0, 1.0, 0.0, 20.0]
    t[1, 5, 9] = 2   # weight 1
    loss_ok, grad_ok = _opts_run(z, t.to(dtype), C_, g, S, ii, w, 0.1)
    assert torch.isfinite(loss_ok) and torch.isfinite(grad_ok).all()
    t[1, 5, 9] = bad
    loss, grad = _opts_run(z, t.to(dtype), C_, g, S, ii, w, 0.1)
    assert torch.isnan(loss)
    assert torch.isnan(grad[1, :, 5, 9]).all()
    keep = torch.ones(B, S, S, dtype=torch.bool)
    keep[1, 5, 9] = False
    assert torch.equal(_bits(grad.permute(1, 0, 2, 3)[:, keep]), _bits(grad_ok.permute(1, 0, 2, 3)[:, keep]))


# ------------------------------------------------------------------ 6. end to end
@pytest.mark.parametrize("precision,interp", [("fp32", False), ("bf16", False), ("fp32", True), ("bf16", True)])
def test_ce_loss_with_options_end_to_end(precision, interp):
    """ce_loss(x, y_with_255, ignore_index=255, class_weight=..., label_smoothing=0.1).backward(): finite parameter
    gradients where the plain call gives NaN; the head-bias gradient (the sum of d loss / d logits over every pixel) equals
    the sum of the fp64 reference gradient; grad_scale scales the gradient and leaves the loss value alone.
    The reference is taken on the logits the training forward itself produces (vitseg_forward_train's optional output,
    the bits the loss kernel regenerates), so the kernel bound applies unchanged.  Summation: n = B S S terms per class in
    fp32, in any order, err <= n u sum |G|, plus a few roundings per term in the upsample's adjoint."""
    C_, S0 = 3, 64
    m = _small_model(C_, S0, precision)
    S = 96 if interp else S0
    B = 2
    cfg_in = m.cfg if not interp else type(m.cfg)(C_, 16, 64, 1, 1, image_size=S, intermediate_size=128)
    x = torch.from_numpy(synth.make_images(cfg_in, B, seed=4)).to(DEV)
    gen = torch.Generator().manual_seed(37)
    y = torch.randint(0, C_, (B, S, S), generator=gen)
    y[torch.rand(B, S, S, generator=gen) < 0.1] = 255
    y = y.to(torch.uint8).to(DEV)
    w = [0.25, 4.0, 1.0]
    kw = dict(ignore_index=255, class_weight=w, label_smoothing=0.1, interpolate_pos_encoding=interp)
    off, n = _lib.param_offset(m.cfg, _lib.T_HEAD2_B)

    # today's behaviour without the option: the void label poisons the step
    m.zero_grad(set_to_none=True)
    m.ce_loss(x, y, interpolate_pos_encoding=interp).backward()
    assert torch.isnan(m.arena.grad[off:off + n]).all()

    m.zero_grad(set_to_none=True)
    loss = m.ce_loss(x, y, **kw)
    loss.backward()
    torch.cuda.synchronize()
    g1 = m.arena.grad.detach().clone()
    assert torch.isfinite(loss) and torch.isfinite(g1).all()

    logits = m._forward_train(x, True, interp=interp)
    torch.cuda.synchronize()
    up = logits.double().cpu().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(up, y.cpu().long(), weight=torch.tensor(w, dtype=torch.float64), ignore_index=255,
                                            label_smoothing=0.1)
    ref.backward()
    G = up.grad
    lse = torch.logsumexp(up.detach(), dim=1)
    e_pix = _ce_bounds(up.detach(), lse, C_)
    wt = torch.tensor(w, dtype=torch.float64)
    keep = y.cpu() != 255
    den = float(wt[y.cpu().long()[keep]].sum())
    K = 0.9 * float(wt.max()) + 0.1 * float(wt.sum()) / C_
    npx = B * S * S
    bound_l = e_pix * (0.9 + 0.1 * float(wt.sum()) / C_ * int(keep.sum()) / den) + 6 * U * abs(float(ref))
    err_l = abs(float(loss) - float(ref))
    bias_ref = G.sum(dim=(0, 2, 3))
    bound_b = npx * K * (e_pix + 20 * U) / den + (npx + 16) * U * float(G.abs().sum(dim=(0, 2, 3)).max())
    err_b = (g1[off:off + n].double().cpu() - bias_ref).abs().max().item()
    print(f"e2e {precision} interp={interp}: loss err {err_l:.2e} (bound {bound_l:.2e}), head-bias grad err {err_b:.2e} "
          f"(bound {bound_b:.2e}; |bias grad| max {bias_ref.abs().max().item():.2e})")
    assert err_l < bound_l, (err_l, bound_l)
    assert err_b < bound_b, (err_b, bound_b)

    # the no-grad path (vitseg_ce_loss_opts on the inference forward's low-res logits).  The loss is a weighted mean of
    # per-pixel terms that are 2-Lipschitz in the logits' max-norm (lse and the picked / averaged logit, 1 each), so it moves
    # by at most twice the distance between the two forwards' logits, plus each side's kernel error
    with torch.no_grad():
        loss_ng = m.ce_loss(x, y, **kw)
        logits_inf = m(x, interpolate_pos_encoding=interp)
    dist = (logits_inf - logits).abs().max().item()
    err_ng = abs(float(loss_ng) - float(loss))
    print(f"    no-grad loss differs by {err_ng:.2e} (logits differ by {dist:.2e})")
    assert torch.isfinite(loss_ng) and err_ng <= 2 * dist + 2 * bound_l

    m.zero_grad(set_to_none=True)
    loss4 = m.ce_loss(x, y, grad_scale=0.25, **kw)
    loss4.backward()
    torch.cuda.synchronize()
    g4 = m.arena.grad.detach().clone()
    assert torch.equal(_bits(loss4.reshape(1)), _bits(loss.detach().reshape(1)))
    big = g1.abs() > 1e-30   # a power of two at the gradient's source: every later product and sum scales exactly
    assert torch.equal(g4[big], (g1 * 0.25)[big])


def test_lightning_module_uses_the_options_in_both_steps():
    """LightningViTModel(ignore_index=..., class_weight=..., label_smoothing=...): training_step and validation_step give
    the loss ViTSegmentationModel.ce_loss gives with the same options; -100 keeps the targets int64."""
    from visiontransformer_amd.lightning import LightningViTModel
    C_, S = 3, 64
    gen = torch.Generator().manual_seed(41)
    for ii in (255, -100):
        lm = LightningViTModel(C_, 16, 64, 1, 1, image_size=S, intermediate_size=128, device=DEV, ignore_index=ii,
                               class_weight=[0.25, 4.0, 1.0], label_smoothing=0.1)
        sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(lm.model.cfg, seed=4).items()}
        lm.model.load_state_dict(sd)
        lm.eval()
        x = torch.from_numpy(synth.make_images(lm.model.cfg, 2, seed=4)).to(DEV)
        y = torch.randint(0, C_, (2, S, S), generator=gen)
        y[torch.rand(2, S, S, generator=gen) < 0.1] = ii
        y = y.to(DEV)
        opts = dict(ignore_index=ii, class_weight=[0.25, 4.0, 1.0], label_smoothing=0.1)
        want = lm.model.ce_loss(x, y, **opts)   # int64 targets; the steps resize to uint8 where a byte holds the label
        want.backward()
        lm.zero_grad(set_to_none=True)
        with torch.no_grad():
            want_ng = lm.model.ce_loss(x, y, **opts)
        lv = lm.validation_step((x, y), 0)
        lt = lm.training_step((x, y), 0)
        lt.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(lv) and torch.isfinite(lt) and torch.isfinite(lm.model.arena.grad).all()
        # the same kernels on the same inputs (uint8 and int64 targets give the same bits): the same value
        assert torch.equal(_bits(lt.detach().reshape(1)), _bits(want.detach().reshape(1)))
        assert torch.equal(_bits(lv.reshape(1)), _bits(want_ng.reshape(1)))


def test_tensor_class_weight_is_read_by_value_on_every_call():
    """A fresh device tensor of weights on every step (1 / frequency, recomputed): the allocator hands a freed block to the
    next tensor, so the address and `_version` of an earlier step come back with other values.  Each call's loss is, bit for
    bit, the loss the same values give when passed as a list (the same kernels on the same inputs); an in-place edit through
    `.data` is seen as well."""
    C_, S = 3, 64
    m = _small_model(C_, S).eval()
    x = torch.from_numpy(synth.make_images(m.cfg, 2, seed=4)).to(DEV)
    gen = torch.Generator().manual_seed(43)
    y = torch.randint(0, C_, (2, S, S), generator=gen).to(torch.uint8).to(DEV)
    sets = [[0.25, 4.0, 1.0], [3.0, 0.5, 2.0], [1.0, 1.0, 8.0]]
    with torch.no_grad():
        want = [m.ce_loss(x, y, class_weight=w) for w in sets]
        assert len({float(v) for v in want}) == len(sets)   # the weights matter on these inputs
        ptrs = set()
        for rep in range(4):
            for w, v in zip(sets, want):
                wt = torch.tensor(w, device=DEV)
                ptrs.add(wt.data_ptr())
                got = m.ce_loss(x, y, class_weight=wt)
                assert torch.equal(_bits(got.reshape(1)), _bits(v.reshape(1))), (rep, w)
                del wt
        wt = torch.tensor(sets[0], device=DEV)
        assert torch.equal(_bits(m.ce_loss(x, y, class_weight=wt).reshape(1)), _bits(want[0].reshape(1)))
        wt.data.copy_(torch.tensor(sets[1]))
        assert torch.equal(_bits(m.ce_loss(x, y, class_weight=wt).reshape(1)), _bits(want[1].reshape(1)))
    print(f"    {len(ptrs)} distinct addresses held the 12 weight tensors")
