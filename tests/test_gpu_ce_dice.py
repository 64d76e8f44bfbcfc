"""GPU (-m gpu): the fused CE + soft-Dice loss (vitseg_ce_dice_loss, vitseg_backward_dice, ViTSegmentationModel.ce_dice_loss,
LightningViTModel(dice_weight=...)) against torch's CPU autograd in fp64 (tests/dice_ref.py).  Every buffer is
guard-banded; both scratch buffers have exactly the queried size and arrive NaN-poisoned.

Tolerances: `dice_ref.bounds`, derived in that module's docstring from U = 2^-23 and the per-pixel bound e_pix on lse - z_c
and held against an fp32 emulation and four wrong formulas in tests/test_ce_dice_cpu.py."""
import ctypes as C

import pytest
import torch

import dice_ref
from guard import check, guarded, snapshot, unchanged
from visiontransformer_amd import _lib, synth
from visiontransformer_amd.config import ViTSegConfig
from visiontransformer_amd.model import ViTSegmentationModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = dice_ref.U


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(z, target, S, dice_weight=1.0, ce_weight=1.0, smooth=1e-6, include_background=True, ignore_index=None,
         class_weight=None, label_smoothing=0.0, want_grad=True, loss_scale=1.0, null_ce=None):
    """One vitseg_ce_dice_loss call on guarded buffers.  The CE options pointer is NULL when all three CE options are at
    their defaults (null_ce=False: a default-valued struct instead).  Returns (terms [3], grad or None) on the CPU."""
    B, C_, g = z.shape[0], z.shape[1], z.shape[2]
    L = _lib.lib()
    zd = guarded(z.shape, torch.float32, z, name="lowres")
    td = guarded(target.shape, target.dtype, target, name="target")
    gd = guarded((B, C_, S, S), torch.float32, "nan", name="grad_logits") if want_grad else None
    scratch = guarded(L.vitseg_ce_scratch_bytes(B, S), torch.uint8, "nan", name="ce scratch")
    terms = guarded((3,), torch.float32, "nan", name="terms")
    wd = guarded((C_,), torch.float32, torch.as_tensor(class_weight, dtype=torch.float32), name="class_weight") \
        if class_weight is not None else None
    if null_ce is None:
        null_ce = ignore_index is None and class_weight is None and label_smoothing == 0.0
    oscr = ce = None
    if not null_ce:
        nbytes = int(_lib.ce_opts_symbol("vitseg_ce_options_scratch_bytes")(B, S))
        oscr = guarded(nbytes, torch.uint8, "nan", name="ce options scratch")
        ce = _lib.CCEOptions(int(ignore_index is not None), 0, 0 if ignore_index is None else ignore_index,
                             wd.data_ptr() if wd is not None else None, label_smoothing, oscr.data_ptr(), nbytes)
    dbytes = int(_lib.dice_symbol("vitseg_dice_options_scratch_bytes")(B, C_, S))
    dscr = guarded(dbytes, torch.uint8, "nan", name="dice scratch")
    d = _lib.CDiceOptions(ce_weight, dice_weight, smooth, int(include_background), dscr.data_ptr(), dbytes)
    snap = snapshot(zd, td, wd)
    _lib.check(_lib.dice_symbol("vitseg_ce_dice_loss")(
        zd.data_ptr(), td.data_ptr(), int(target.dtype == torch.uint8), gd.data_ptr() if gd is not None else None,
        scratch.data_ptr(), terms.data_ptr(), B, C_, g, S, C.byref(ce) if ce is not None else None, C.byref(d),
        loss_scale, _stream()))
    torch.cuda.synchronize()
    check(zd, td, gd, scratch, terms, wd, oscr, dscr)
    unchanged(snap)
    return terms.cpu(), (gd.cpu() if gd is not None else None)


def _ce_opts_run(z, target, S, ignore_index=None, class_weight=None, label_smoothing=0.0, loss_scale=1.0, plain=False):
    """vitseg_ce_loss_opts (plain: vitseg_ce_loss) on the same inputs: (loss [1], grad) on the CPU."""
    B, C_, g = z.shape[0], z.shape[1], z.shape[2]
    L = _lib.lib()
    zd, td = z.to(DEV), target.to(DEV)
    gd = torch.full((B, C_, S, S), float("nan"), device=DEV)
    scratch = torch.empty(L.vitseg_ce_scratch_bytes(B, S), dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    args = (zd.data_ptr(), td.data_ptr(), int(target.dtype == torch.uint8), gd.data_ptr(), scratch.data_ptr(), loss.data_ptr(),
            B, C_, g, S)
    if plain:
        _lib.check(L.vitseg_ce_loss(*args, _stream()))
    else:
        wd = torch.as_tensor(class_weight, dtype=torch.float32).to(DEV) if class_weight is not None else None
        nbytes = int(_lib.ce_opts_symbol("vitseg_ce_options_scratch_bytes")(B, S))
        oscr = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        o = _lib.CCEOptions(int(ignore_index is not None), 0, 0 if ignore_index is None else ignore_index,
                            wd.data_ptr() if wd is not None else None, label_smoothing, oscr.data_ptr(), nbytes)
        _lib.check(_lib.ce_opts_symbol("vitseg_ce_loss_opts")(*args, C.byref(o), loss_scale, _stream()))
    torch.cuda.synchronize()
    return loss.cpu(), gd.cpu()


def _case_bounds(c, **over):
    loss, ce, dice, grad, up = c["ref"]
    _, _, _, _, sums = dice_ref.closed_form(up, c["target"], **c["kw"])
    return dice_ref.bounds(up, c["target"], sums, loss, ce, dice, grad.abs().max().item(), **dict(c["kw"], **over))


# ------------------------------------------------------------------ 1. the cases, against the fp64 oracle
@pytest.mark.parametrize("name", list(dice_ref.CASES))
def test_cases_against_fp64(name):
    """The C ABI against the oracle within the derived bound; twice for identical bits, with uint8 targets for the same bits,
    without grad_logits for the same terms (the 512 cases run once); ignored pixels hold exact zeros."""
    c = dice_ref.case(name)
    z, t, S, kw = c["z"], c["target"], c["S"], c["kw"]
    loss, ce, dice, grad, up = c["ref"]
    assert torch.isfinite(loss) and torch.isfinite(grad).all()
    terms, g = _run(z, t, S, **kw)
    b = _case_bounds(c)
    errs = [abs(float(terms[0]) - float(loss)), abs(float(terms[1]) - float(ce)), abs(float(terms[2]) - float(dice)),
            (g.double() - grad).abs().max().item()]
    print(f"{name}: loss err {errs[0]:.2e} (bound {b['loss']:.2e}), ce {errs[1]:.2e} ({b['ce']:.2e}), dice {errs[2]:.2e} "
          f"({b['dice']:.2e}), grad {errs[3]:.2e} ({b['grad']:.2e}; max |grad| {grad.abs().max().item():.2e})")
    assert torch.isfinite(terms).all() and torch.isfinite(g).all()
    assert errs[0] < b["loss"] and errs[1] < b["ce"] and errs[2] < b["dice"] and errs[3] < b["grad"]
    ii = kw.get("ignore_index")
    if ii is not None:
        g_ign = g.permute(1, 0, 2, 3)[:, t == ii]
        assert (g_ign == 0).all() and not torch.signbit(g_ign).any()
    if S == 512:
        return
    terms2, g2 = _run(z, t, S, **kw)
    assert torch.equal(_bits(terms2), _bits(terms)) and torch.equal(_bits(g2), _bits(g))
    if ii is None or 0 <= ii <= 255:
        terms8, g8 = _run(z, t.to(torch.uint8), S, **kw)
        assert torch.equal(_bits(terms8), _bits(terms)) and torch.equal(_bits(g8), _bits(g))
    terms_ng, _ = _run(z, t, S, want_grad=False, **kw)
    assert torch.equal(_bits(terms_ng), _bits(terms))


# ------------------------------------------------------------------ 2. ignored pixels
def test_ignored_pixels_get_exact_zeros_and_their_logits_do_not_matter():
    B, C_, g, S = 2, 5, 7, 28
    gen = torch.Generator().manual_seed(23)
    z = torch.randn(B, C_, g, g, generator=gen).float()
    t = torch.randint(0, C_, (B, S, S), generator=gen)
    t[1][torch.rand(S, S, generator=gen) < 0.1] = 255
    t[0] = 255
    kw = dict(ignore_index=255, class_weight=[0.5, 3.0, 1.0, 0.25, 20.0], label_smoothing=0.1)
    terms, grad = _run(z, t, S, **kw)
    assert torch.isfinite(terms).all() and torch.isfinite(grad).all()
    ign = t == 255
    g_ign = grad.permute(1, 0, 2, 3)[:, ign]
    assert (g_ign == 0).all() and not torch.signbit(g_ign).any()     # +0.0f, every class
    assert (grad.permute(1, 0, 2, 3)[:, ~ign] != 0).any()
    z2 = z.clone()
    z2[0] = -z[0] * 50.0 + 7.0
    terms2, grad2 = _run(z2, t, S, **kw)
    assert torch.equal(_bits(terms2), _bits(terms)) and torch.equal(_bits(grad2), _bits(grad))
    z2[0] = float("nan")
    terms3, grad3 = _run(z2, t.to(torch.uint8), S, **kw)
    assert torch.equal(_bits(terms3), _bits(terms)) and torch.equal(_bits(grad3), _bits(grad))


# ------------------------------------------------------------------ 3. everything ignored
def test_everything_ignored():
    """I = P = T = 0: dice = 1 - smooth / smooth = 0 and every gradient is 0; the total is that 0 with ce_weight = 0 (the CE
    term is not formed: not 0 * NaN) and NaN with ce_weight = 1; with smooth = 0 dice is NaN."""
    B, C_, g, S = 2, 5, 7, 28
    z = torch.randn(B, C_, g, g, generator=torch.Generator().manual_seed(29)).float()
    for t in (torch.full((B, S, S), 255, dtype=torch.int64), torch.full((B, S, S), 255, dtype=torch.uint8)):
        terms, grad = _run(z, t, S, ce_weight=0.0, ignore_index=255)
        assert terms.tolist() == [0.0, 0.0, 0.0] and (grad == 0).all()
        terms, grad = _run(z, t, S, ce_weight=1.0, ignore_index=255)
        assert torch.isnan(terms[0]) and torch.isnan(terms[1]) and float(terms[2]) == 0.0 and (grad == 0).all()
        terms, grad = _run(z, t, S, ce_weight=0.0, smooth=0.0, ignore_index=255)
        assert torch.isnan(terms[0]) and float(terms[1]) == 0.0 and torch.isnan(terms[2]) and (grad == 0).all()


# ------------------------------------------------------------------ 4. a bad label that is not ignore_index
@pytest.mark.parametrize("dtype,ii,bad", [(torch.uint8, 255, 7), (torch.int64, -100, 5), (torch.int64, None, -100)])
def test_bad_label_poisons_the_sums(dtype, ii, bad):
    """NaN loss, NaN dice and a NaN gradient at every kept pixel (the sums of every class hold its NaN); ignored pixels keep
    their zeros.  With the Dice term alone the same."""
    B, C_, g, S = 2, 5, 7, 28
    gen = torch.Generator().manual_seed(31)
    z = torch.randn(B, C_, g, g, generator=gen).float()
    t = torch.randint(0, C_, (B, S, S), generator=gen)
    if ii is not None:
        t[torch.rand(B, S, S, generator=gen) < 0.1] = ii
    t[1, 5, 9] = bad
    keep = torch.ones_like(t, dtype=torch.bool) if ii is None else t != ii
    for cw in (1.0, 0.0):
        terms, grad = _run(z, t.to(dtype), S, ce_weight=cw, ignore_index=ii, null_ce=False)
        assert torch.isnan(terms[0]) and torch.isnan(terms[2])
        assert torch.isnan(terms[1]) if cw else float(terms[1]) == 0.0
        assert torch.isnan(grad.permute(1, 0, 2, 3)[:, keep]).all()
        assert (grad.permute(1, 0, 2, 3)[:, ~keep] == 0).all()


# ------------------------------------------------------------------ 5. the gradient scale
def test_loss_scale_scales_the_gradient_exactly():
    c = dice_ref.case("smooth 1, weights 2 : 0.5")
    terms, grad = _run(c["z"], c["target"], c["S"], **c["kw"])
    terms_s, grad_s = _run(c["z"], c["target"], c["S"], loss_scale=0.25, **c["kw"])
    assert torch.equal(_bits(terms_s), _bits(terms))
    big = grad.abs() > 1e-30   # a power of two: every product and sum scales exactly
    assert torch.equal(grad_s[big], (grad * 0.25)[big])


# ------------------------------------------------------------------ 6. one weight at 0
@pytest.mark.parametrize("opts", [dict(), dict(ignore_index=255, class_weight=[0.5, 3.0, 1.0, 0.0, 20.0], label_smoothing=0.1)])
def test_dice_weight_zero_is_the_ce_call_bitwise(opts):
    """dice_weight = 0, ce_weight = 1: terms[1], terms[0] and the gradient are vitseg_ce_loss_opts's bits for the same options
    (vitseg_ce_loss's without any); terms[2] reads 0."""
    B, C_, g, S = 2, 5, 7, 28
    gen = torch.Generator().manual_seed(37)
    z = torch.randn(B, C_, g, g, generator=gen).float() * 3
    t = torch.randint(0, C_, (B, S, S), generator=gen)
    if opts:
        t[torch.rand(B, S, S, generator=gen) < 0.1] = 255
    for tt in (t, t.to(torch.uint8)):
        for scale in (1.0, 0.25):
            loss_ce, grad_ce = _ce_opts_run(z, tt, S, loss_scale=scale, plain=not opts and scale == 1.0, **opts)
            terms, grad = _run(z, tt, S, dice_weight=0.0, ce_weight=1.0, loss_scale=scale, **opts)
            assert torch.isfinite(loss_ce).all()
            assert torch.equal(_bits(terms[1:2]), _bits(loss_ce)) and torch.equal(_bits(terms[0:1]), _bits(loss_ce))
            assert float(terms[2]) == 0.0
            assert torch.equal(_bits(grad), _bits(grad_ce))
    if not opts:   # a default-valued options struct instead of NULL: the same bits once more
        terms_d, grad_d = _run(z, t, S, dice_weight=0.0, ce_weight=1.0, null_ce=False)
        loss_ce, grad_ce = _ce_opts_run(z, t, S, plain=True)
        assert torch.equal(_bits(terms_d[1:2]), _bits(loss_ce)) and torch.equal(_bits(grad_d), _bits(grad_ce))


def test_ce_weight_zero_is_the_pure_dice_of_the_oracle():
    c = dice_ref.case("ignored, weights, smoothing")
    kw = dict(c["kw"], ce_weight=0.0, dice_weight=0.75)
    loss, ce, dice, grad, up = dice_ref.ce_dice_ref_up(c["ref"][4], c["target"], **kw)
    _, _, _, _, sums = dice_ref.closed_form(up, c["target"], **kw)
    b = dice_ref.bounds(up, c["target"], sums, loss, ce, dice, grad.abs().max().item(), **kw)
    terms, g = _run(c["z"], c["target"], c["S"], **kw)
    errs = [abs(float(terms[0]) - float(loss)), abs(float(terms[2]) - float(dice)), (g.double() - grad).abs().max().item()]
    print(f"pure dice: loss err {errs[0]:.2e} (bound {b['loss']:.2e}), dice {errs[1]:.2e} ({b['dice']:.2e}), grad {errs[2]:.2e} "
          f"({b['grad']:.2e})")
    assert float(terms[1]) == 0.0 and float(ce) == 0.0
    assert errs[0] < b["loss"] and errs[1] < b["dice"] and errs[2] < b["grad"]


# ------------------------------------------------------------------ 7. vitseg_backward_dice
def _small_model(C_=3, S=64, precision="fp32", seed=4):
    m = ViTSegmentationModel(C_, 16, 64, 1, 1, image_size=S, intermediate_size=128, precision=precision, device=DEV)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(m.cfg, seed=seed).items()}
    m.load_state_dict(sd)
    m.eval()   # no dropout: the forward is a pure function of (parameters, x)
    return m


def _backward_args(m, x, target, grads, loss, loss_scale, grad_logits=None):
    B, S = x.shape[0], int(x.shape[-1])
    ws = m._train_workspace(B, S)
    return (m.arena.data_ptr(), m._bf16_arena().data_ptr() if m._bf16_arena() is not None else None, x.data_ptr(), B,
            m.precision, 0.0, 0, target.data_ptr() if target is not None else None, 1,
            grad_logits.data_ptr() if grad_logits is not None else None, grads.data_ptr(), loss.data_ptr(), float(loss_scale),
            None, ws.data_ptr(), ws.numel(), _stream())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_backward_dice_null_is_backward_opts_bitwise(precision):
    m = _small_model(precision=precision)
    S = m.cfg.image_size
    x = torch.from_numpy(synth.make_images(m.cfg, 2, seed=4)).to(DEV)
    gen = torch.Generator().manual_seed(1)
    t = torch.randint(0, 3, (2, S, S), generator=gen)
    t[torch.rand(2, S, S, generator=gen) < 0.1] = 255
    t = t.to(torch.uint8).to(DEV)
    nbytes = int(_lib.ce_opts_symbol("vitseg_ce_options_scratch_bytes")(2, S))
    cfg = C.byref(_lib.CConfig.from_config(m.cfg))
    out = []
    for via_dice in (False, True):
        m._forward_train(x, False)
        grads = guarded(m.arena.shape, torch.float32, "nan", name="grads")
        loss = guarded((1,), torch.float32, "nan", name="loss")
        terms = guarded((3,), torch.float32, "nan", name="terms")
        oscr = guarded(nbytes, torch.uint8, "nan", name="ce options scratch")
        o = _lib.CCEOptions(1, 0, 255, None, 0.1, oscr.data_ptr(), nbytes)
        args = _backward_args(m, x, t, grads, loss, 0.5)
        if via_dice:
            _lib.check(_lib.dice_symbol("vitseg_backward_dice")(cfg, S, *args, C.byref(o), None, terms.data_ptr()))
        else:
            _lib.check(_lib.ce_opts_symbol("vitseg_backward_opts")(cfg, S, *args, C.byref(o)))
        torch.cuda.synchronize()
        check(grads, loss, terms, oscr)
        assert torch.isnan(terms).all()   # not touched without the Dice options
        out.append((grads, loss))
    assert torch.isfinite(out[0][0]).all() and torch.isfinite(out[0][1]).all()
    assert torch.equal(_bits(out[1][0]), _bits(out[0][0])) and torch.equal(_bits(out[1][1]), _bits(out[0][1]))


def test_backward_dice_argument_errors_launch_nothing():
    """EINVAL before any launch (not even the arena's memset): outputs pre-filled with NaN are unchanged."""
    m = _small_model()
    S = m.cfg.image_size
    x = torch.from_numpy(synth.make_images(m.cfg, 1, seed=4)).to(DEV)
    t = torch.zeros(1, S, S, dtype=torch.uint8, device=DEV)
    m._forward_train(x, False)
    grads = guarded(m.arena.shape, torch.float32, "nan", name="grads")
    loss = guarded((1,), torch.float32, "nan", name="loss")
    terms = guarded((3,), torch.float32, "nan", name="terms")
    gl = torch.zeros(1, 3, S, S, device=DEV)
    dbytes = int(_lib.dice_symbol("vitseg_dice_options_scratch_bytes")(1, 3, S))
    dscr = guarded(dbytes, torch.uint8, "nan", name="dice scratch")
    nbytes = int(_lib.ce_opts_symbol("vitseg_ce_options_scratch_bytes")(1, S))
    oscr = guarded(nbytes, torch.uint8, "nan", name="ce options scratch")
    cfg = C.byref(_lib.CConfig.from_config(m.cfg))
    fn = _lib.dice_symbol("vitseg_backward_dice")

    def call(d, ce=None, target=t, grad_logits=None, terms_ptr=terms.data_ptr()):
        return fn(cfg, S, *_backward_args(m, x, target, grads, loss, 1.0, grad_logits), C.byref(ce) if ce is not None else None,
                  C.byref(d), terms_ptr)
    p, n = dscr.data_ptr(), dbytes
    ok = _lib.CDiceOptions(1.0, 0.5, 1e-6, 1, p, n)
    nan, inf = float("nan"), float("inf")
    assert call(ok, target=None, grad_logits=gl) == _lib.EINVAL          # the Dice options together with grad_logits
    assert call(ok, terms_ptr=None) == _lib.EINVAL
    for d in (_lib.CDiceOptions(-1.0, 0.5, 1e-6, 1, p, n), _lib.CDiceOptions(1.0, -0.5, 1e-6, 1, p, n),
              _lib.CDiceOptions(1.0, 0.5, -1e-6, 1, p, n), _lib.CDiceOptions(nan, 0.5, 1e-6, 1, p, n),
              _lib.CDiceOptions(1.0, inf, 1e-6, 1, p, n), _lib.CDiceOptions(1.0, 0.5, nan, 1, p, n),
              _lib.CDiceOptions(0.0, 0.0, 1e-6, 1, p, n), _lib.CDiceOptions(1.0, 0.5, 1e-6, 1, None, n),
              _lib.CDiceOptions(1.0, 0.5, 1e-6, 1, p + 4, n), _lib.CDiceOptions(1.0, 0.5, 1e-6, 1, p, n - 1)):
        assert call(d) == _lib.EINVAL
    assert call(ok, ce=_lib.CCEOptions(1, 0, 255, None, 1.5, oscr.data_ptr(), nbytes)) == _lib.EINVAL
    assert call(ok, ce=_lib.CCEOptions(1, 0, 255, None, 0.1, oscr.data_ptr(), nbytes - 1)) == _lib.EINVAL
    torch.cuda.synchronize()
    check(grads, loss, terms, dscr, oscr)
    assert torch.isnan(grads).all() and torch.isnan(loss).all() and torch.isnan(terms).all()
    # include_background = 0 with one class, in front of vitseg_ce_dice_loss (training needs C >= 2 anyway)
    z = torch.zeros(1, 1, 4, 4, device=DEV)
    scr = torch.empty(_lib.lib().vitseg_ce_scratch_bytes(1, S), dtype=torch.uint8, device=DEV)
    d1 = _lib.CDiceOptions(1.0, 0.5, 1e-6, 0, p, n)
    assert _lib.dice_symbol("vitseg_ce_dice_loss")(z.data_ptr(), t.data_ptr(), 1, None, scr.data_ptr(), terms.data_ptr(), 1, 1, 4, S,
                                                   None, C.byref(d1), 1.0, _stream()) == _lib.EINVAL
    torch.cuda.synchronize()
    check(terms, dscr)
    assert torch.isnan(terms).all()
    assert call(ok, ce=_lib.CCEOptions(1, 0, 255, None, 0.1, oscr.data_ptr(), nbytes)) == _lib.OK   # and the valid call goes through
    torch.cuda.synchronize()
    check(grads, loss, terms, dscr, oscr)
    assert torch.isfinite(grads).all() and torch.isfinite(terms).all()
    assert torch.equal(_bits(loss), _bits(terms[0:1]))


# ------------------------------------------------------------------ 8. end to end
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ce_dice_loss_end_to_end(precision):
    """Path one: model.ce_dice_loss(...).backward().  Path two: forward() -> the definition in torch on the device (fp64, so
    that its own rounding does not count; the gradient handed on in fp32) -> autograd -> vitseg_backward through grad_logits.
    The loss is held to the kernel bound against the oracle on the logits the training forward itself produces.
    Parameter gradients: both paths run the same backward walk on a d loss / d logits that differs by the loss kernel's
    rounding alone, so the tolerance is set from what the two paths differ by with dice_weight = 0 (pure CE, measured here
    in the same run: rel0 = max |g1 - g2| / max |g2|), scaled by how much wider the derived per-entry bound of d loss /
    d logits is with the Dice term than without, each relative to its largest entry, and doubled."""
    C_, B = 5, 2
    cfg = ViTSegConfig(C_, 16, 192, 2, 3, image_size=224)
    m = ViTSegmentationModel(C_, 16, 192, 2, 3, image_size=224, precision=precision, device=DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=3).items()})
    m.eval()
    S = 224
    x = torch.from_numpy(synth.make_images(cfg, B, seed=1)).to(DEV)
    gen = torch.Generator().manual_seed(41)
    y = torch.randint(0, C_, (B, S, S), generator=gen)
    y[torch.rand(B, S, S, generator=gen) < 0.1] = 255
    yd = y.to(torch.uint8).to(DEV)
    ce_kw = dict(ignore_index=255, class_weight=[0.25, 4.0, 1.0, 2.0, 0.5], label_smoothing=0.1)

    def two_paths(dice_weight):
        kw = dict(ce_kw, dice_weight=dice_weight, ce_weight=1.0, smooth=1e-6, include_background=False)
        m.zero_grad(set_to_none=True)
        loss1, ce1, dice1 = m.ce_dice_loss(x, yd, return_terms=True, **kw)
        loss1.backward()
        torch.cuda.synchronize()
        g1 = m.arena.grad.detach().clone()
        m.zero_grad(set_to_none=True)
        logits = m(x)
        up = logits.detach().double().requires_grad_(True)
        loss2, _, _ = dice_ref.ce_dice_torch(up, yd, **kw)
        loss2.backward()
        logits.backward(up.grad.float())
        torch.cuda.synchronize()
        g2 = m.arena.grad.detach().clone()
        ref = dice_ref.ce_dice_ref_up(logits.detach(), y, **kw)
        _, _, _, _, sums = dice_ref.closed_form(ref[4], y, **kw)
        b = dice_ref.bounds(ref[4], y, sums, ref[0], ref[1], ref[2], ref[3].abs().max().item(), **kw)
        return (loss1.detach(), ce1, dice1), g1, g2, ref, b

    (l0, c0, d0), g1_0, g2_0, ref0, b0 = two_paths(0.0)
    assert torch.isfinite(g1_0).all() and torch.isfinite(g2_0).all() and float(d0) == 0.0
    rel0 = (g1_0 - g2_0).abs().max().item() / g2_0.abs().max().item()
    (l1, c1, d1), g1, g2, ref, b = two_paths(0.5)
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all()
    widen = (b["grad"] / ref[3].abs().max().item()) / (b0["grad"] / ref0[3].abs().max().item())
    tol = 2.0 * max(widen, 1.0) * rel0
    rel = (g1 - g2).abs().max().item() / g2.abs().max().item()
    errs = [abs(float(l1) - float(ref[0])), abs(float(c1) - float(ref[1])), abs(float(d1) - float(ref[2]))]
    print(f"e2e {precision}: loss err {errs[0]:.2e} (bound {b['loss']:.2e}), ce {errs[1]:.2e} ({b['ce']:.2e}), dice {errs[2]:.2e} "
          f"({b['dice']:.2e}); parameter gradients differ by {rel:.2e} of the largest (pure CE: {rel0:.2e}, bound ratio "
          f"{widen:.2f}, tolerance {tol:.2e})")
    assert errs[0] < b["loss"] and errs[1] < b["ce"] and errs[2] < b["dice"]
    assert abs(float(l0) - float(ref0[0])) < b0["loss"]
    assert rel <= tol, (rel, tol)
    # the no-grad path reads the inference forward's low-res logits.  In the logits' max-norm CE is 2-Lipschitz (lse and the
    # picked / averaged logit) and dice 6-Lipschitz: sum over pixels and classes of |p_c (a_c - S)| <= 2 sum p_c |a_c|, where the
    # t_c = 1 entries are T_c <= D_c many of at most 2 / (|K| D_c) each and the others sum to N_c P_c / (|K| D_c^2) <= 1 / |K|
    # per class: 2 (2 + 1).  With dice_weight = 0.5 that is 2 + 3, plus each side's kernel error
    with torch.no_grad():
        l_ng = m.ce_dice_loss(x, yd, dice_weight=0.5, include_background=False, **ce_kw)
        dist = (m(x) - m._forward_train(x, True)).abs().max().item()
    assert torch.isfinite(l_ng) and abs(float(l_ng) - float(l1)) <= 5 * dist + 2 * b["loss"]
    # grad_scale scales the gradient and leaves the value alone
    m.zero_grad(set_to_none=True)
    l4 = m.ce_dice_loss(x, yd, dice_weight=0.5, include_background=False, grad_scale=0.25, **ce_kw)
    l4.backward()
    torch.cuda.synchronize()
    g4 = m.arena.grad.detach().clone()
    assert torch.equal(_bits(l4.detach().reshape(1)), _bits(l1.reshape(1)))
    big = g1.abs() > 1e-30
    assert torch.equal(g4[big], (g1 * 0.25)[big])


def test_ce_dice_loss_at_another_input_size():
    """interpolate_pos_encoding: the loss of a 96 x 96 input on a 64 x 64 model, against the oracle on the logits that
    training forward produces; finite parameter gradients; the no-grad path agrees within the two forwards' distance."""
    C_, B, S = 3, 2, 96
    m = _small_model(C_, 64)
    cfg_in = ViTSegConfig(C_, 16, 64, 1, 1, image_size=S, intermediate_size=128)
    x = torch.from_numpy(synth.make_images(cfg_in, B, seed=4)).to(DEV)
    gen = torch.Generator().manual_seed(47)
    y = torch.randint(0, C_, (B, S, S), generator=gen)
    y[torch.rand(B, S, S, generator=gen) < 0.1] = -100
    kw = dict(dice_weight=0.5, ignore_index=-100, class_weight=[0.25, 4.0, 1.0])
    m.zero_grad(set_to_none=True)
    loss, ce, dice = m.ce_dice_loss(x, y.to(DEV), interpolate_pos_encoding=True, return_terms=True, **kw)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(m.arena.grad).all() and float(m.arena.grad.abs().max()) > 0
    logits = m._forward_train(x, True, interp=True)
    ref = dice_ref.ce_dice_ref_up(logits, y, **kw)
    _, _, _, _, sums = dice_ref.closed_form(ref[4], y, **kw)
    b = dice_ref.bounds(ref[4], y, sums, ref[0], ref[1], ref[2], ref[3].abs().max().item(), **kw)
    errs = [abs(float(loss) - float(ref[0])), abs(float(ce) - float(ref[1])), abs(float(dice) - float(ref[2]))]
    print(f"96 on 64: loss err {errs[0]:.2e} (bound {b['loss']:.2e}), ce {errs[1]:.2e} ({b['ce']:.2e}), dice {errs[2]:.2e} ({b['dice']:.2e})")
    assert errs[0] < b["loss"] and errs[1] < b["ce"] and errs[2] < b["dice"]
    with torch.no_grad():
        l_ng = m.ce_dice_loss(x, y.to(DEV), interpolate_pos_encoding=True, **kw)
        dist = (m(x, interpolate_pos_encoding=True) - logits).abs().max().item()
    assert abs(float(l_ng) - float(loss)) <= 5 * dist + 2 * b["loss"]   # (2 + 0.5 * 6)-Lipschitz, as in the test above


# ------------------------------------------------------------------ 9. the Lightning module
def test_lightning_module_uses_the_dice_term_in_both_steps():
    """LightningViTModel(dice_weight=0.5): both steps give what ce_dice_loss gives with the same options and log the three
    values; with dice_weight = 0 the logged loss is, bit for bit, ce_loss's (today's)."""
    from visiontransformer_amd.lightning import LightningViTModel
    C_, S = 3, 64
    gen = torch.Generator().manual_seed(43)
    y = torch.randint(0, C_, (2, S, S), generator=gen)
    y[torch.rand(2, S, S, generator=gen) < 0.1] = 255
    y = y.to(DEV)
    for dw in (0.5, 0.0):
        lm = LightningViTModel(C_, 16, 64, 1, 1, image_size=S, intermediate_size=128, device=DEV, ignore_index=255,
                               label_smoothing=0.1, dice_weight=dw, dice_smooth=1.0, dice_include_background=False)
        lm.model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(lm.model.cfg, seed=4).items()})
        lm.eval()
        x = torch.from_numpy(synth.make_images(lm.model.cfg, 2, seed=4)).to(DEV)
        if dw:
            kw = dict(ignore_index=255, label_smoothing=0.1, dice_weight=dw, smooth=1.0, include_background=False, return_terms=True)
            want = lm.model.ce_dice_loss(x, y, **kw)
            want[0].backward()
            lm.zero_grad(set_to_none=True)
            with torch.no_grad():
                want_ng = lm.model.ce_dice_loss(x, y, **kw)
        else:
            want = (lm.model.ce_loss(x, y, ignore_index=255, label_smoothing=0.1),)
            want[0].backward()
            lm.zero_grad(set_to_none=True)
            with torch.no_grad():
                want_ng = (lm.model.ce_loss(x, y, ignore_index=255, label_smoothing=0.1),)
        lv = lm.validation_step((x, y), 0)
        lt = lm.training_step((x, y), 0)
        lt.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(lv) and torch.isfinite(lt) and torch.isfinite(lm.model.arena.grad).all()
        assert torch.equal(_bits(lm.logged["train_loss"].reshape(1)), _bits(want[0].detach().reshape(1)))
        assert torch.equal(_bits(lm.logged["valid_loss"].reshape(1)), _bits(want_ng[0].reshape(1)))
        if dw:
            assert set(lm.logged) == {"train_loss", "train_ce", "train_dice", "valid_loss", "valid_ce", "valid_dice"}
            for stage, w in (("train", want), ("valid", want_ng)):
                assert torch.equal(_bits(lm.logged[f"{stage}_ce"].reshape(1)), _bits(w[1].reshape(1)))
                assert torch.equal(_bits(lm.logged[f"{stage}_dice"].reshape(1)), _bits(w[2].reshape(1)))
                assert float(lm.logged[f"{stage}_dice"]) > 0 and float(lm.logged[f"{stage}_ce"]) > 0
        else:
            assert set(lm.logged) == {"train_loss", "valid_loss"}
