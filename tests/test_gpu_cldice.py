"""GPU (-m gpu): the soft-clDice loss (include/vitseg_cldice.h: vitseg_soft_skeleton, vitseg_soft_cldice,
vitseg_ce_cldice_loss, vitseg_backward_cldice, cldice.py, ViTSegmentationModel.ce_cldice_loss) against tests/cldice_ref.py.
Every buffer is guard-banded; every scratch has exactly the queried size and arrives NaN-poisoned.

Skeleton: no tolerance, the bits of restatement (a) in fp32 on the CPU.
Terms: 1e-6 relative against (a) in fp64 on the same fp32 planes (the project's bound for fp64-summed loss terms).
Gradient: 16 d_ref, d_ref = max |g_fp32 - g_fp64| of restatement (a) against itself on the same case (reference against
reference); every test prints its d_ref and its error.  Measured for the plane cases below at iters = 3 (d_ref, max |g|):
  (2, 33, 70): smooth 6.0e-10 / 6.2e-3, eighths 5.4e-10 / 6.2e-3, binary 1.0e-10 / 2.1e-3, clamped 6.3e-10 / 4.0e-3
  (3, 96, 96): smooth 2.4e-10 / 2.0e-3, eighths 2.4e-10 / 2.1e-3, binary 1.3e-10 / 1.2e-3, clamped 2.3e-10 / 2.1e-3
  (1, 1, 9) and (1, 9, 1): 1.4e-8 .. 5.3e-8 / 0.25 .. 0.34 (binary: 0, an exact case, where the device is exact too)
On the MI355X the device's error was 0.2 .. 2.2 times d_ref on these cases, and 7e-11 .. 6e-10 on the fused cases under
bounds of 1e-8 .. 2e-7.
A wrong tie rule moves the gradient of the quantised plane by 1e-3 .. 9e-3 (tests/test_cldice_cpu.py)."""
import ctypes as C
import functools
from types import SimpleNamespace

import pytest
import torch

import cldice_ref as R
import dice_ref
from ce_ref import upsample64
from guard import check, guarded, snapshot, unchanged
from visiontransformer_amd import _ext, _lib, cldice, synth
from visiontransformer_amd.model import ViTSegmentationModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -23


def _sym(name):
    return _ext.ext_symbol("cldice", name)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ptr(t):
    return t.data_ptr() if t is not None else None


# ------------------------------------------------------------------ 1. the skeleton, bit for bit
def _skeleton(p, iters):
    n, H, W = p.shape
    pd = guarded(p.shape, torch.float32, p, name="p")
    out = guarded(p.shape, torch.float32, "nan", name="skel")
    scr = guarded(int(_sym("vitseg_soft_skeleton_scratch_bytes")(n, H, W)), torch.uint8, "nan", name="skeleton scratch")
    snap = snapshot(pd)
    _lib.check(_sym("vitseg_soft_skeleton")(pd.data_ptr(), n, H, W, iters, out.data_ptr(), scr.data_ptr(), _stream()))
    torch.cuda.synchronize()
    check(pd, out, scr)
    unchanged(snap)
    return out.cpu()


# no tiling: one thread per pixel in blocks of 256 consecutive pixels; (2, 19, 517) puts several blocks in a row and block
# borders at every column phase, and blocks that straddle rows and planes
SHAPES = [(1, 1, 9), (1, 9, 1), (2, 33, 70), (3, 96, 96), (2, 19, 517)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["smooth", "eighths", "binary", "clamped"])
def test_skeleton_is_torch_fp32_bit_for_bit(shape, kind):
    n, H, W = shape
    t = R.line_target(n, H, W, seed=3)
    assert 0 < int(t.sum()) < t.numel()
    p = R.make_plane(kind, n, H, W, t, seed=4)
    if kind == "clamped":
        assert (p == 0).any() and (p == 1).any()
    for iters in (0, 1, 3, 10, 17):
        got, want = _skeleton(p, iters), R.soft_skel(p, iters)
        assert torch.equal(_bits(got), _bits(want)), (iters, int((_bits(got) != _bits(want)).sum()))
    got_t, want_t = _skeleton(t.float(), 3), R.soft_skel(t.float(), 3)
    assert torch.equal(_bits(got_t), _bits(want_t)) and float(want_t.sum()) > 0


def test_module_soft_skeleton():
    t = R.line_target(2, 33, 70, seed=3)
    p = R.make_plane("eighths", 2, 33, 70, t, seed=4)
    assert torch.equal(cldice.soft_skeleton(p.to(DEV), 3).cpu(), R.soft_skel(p, 3))
    assert torch.equal(cldice.soft_skeleton(p[0].to(DEV), iters=1).cpu(), R.soft_skel(p[:1], 1)[0])


# ------------------------------------------------------------------ 2. the plane loss and its gradient
def _plane(prob, truth, iters=3, smooth=1.0, grad_scale=1.0, want_grad=True):
    n, H, W = prob.shape
    pd = guarded(prob.shape, torch.float32, prob, name="prob")
    td = guarded(truth.shape, torch.uint8, truth, name="truth")
    gd = guarded(prob.shape, torch.float32, "nan", name="grad_prob") if want_grad else None
    terms = guarded((4,), torch.float32, "nan", name="terms")
    scr = guarded(int(_sym("vitseg_soft_cldice_scratch_bytes")(n, H, W, iters)), torch.uint8, "nan", name="cldice scratch")
    snap = snapshot(pd, td)
    _lib.check(_sym("vitseg_soft_cldice")(pd.data_ptr(), td.data_ptr(), n, H, W, iters, smooth, grad_scale, scr.data_ptr(),
                                          terms.data_ptr(), _ptr(gd), _stream()))
    torch.cuda.synchronize()
    check(pd, td, gd, terms, scr)
    unchanged(snap)
    return terms.cpu(), (gd.cpu() if want_grad else None)


def _truth(t, void):
    u = t.clone().to(torch.uint8)
    u[void] = 255
    return u


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


def _check_plane(p, t, void, iters, smooth=1.0, label=""):
    terms, g = _plane(p, _truth(t, void), iters, smooth)
    ref, g64 = R.cldice_autograd(p, t.float(), void, iters, smooth, torch.float64)
    _, g32 = R.cldice_autograd(p, t.float(), void, iters, smooth, torch.float32)
    d_ref = (g32.double() - g64).abs().max().item()
    err = (g.double() - g64).abs().max().item()
    rels = [_rel(float(terms[i]), ref[i]) for i in range(3)]
    print(f"{label} iters {iters}: cl {ref[0]:.6f} rel err {rels[0]:.1e} / {rels[1]:.1e} / {rels[2]:.1e}; grad err {err:.2e}, "
          f"d_ref {d_ref:.2e}, bound {16 * d_ref:.2e}, max |g| {g64.abs().max().item():.2e}, non-zero {int((g64 != 0).sum())}")
    assert max(rels) <= 1e-6 and float(terms[3]) == 0.0
    assert err <= 16 * d_ref
    gv = g[void]
    assert (gv == 0).all() and not torch.signbit(gv).any()
    return terms, g


@pytest.mark.parametrize("shape", [(2, 33, 70), (3, 96, 96), (1, 1, 9), (1, 9, 1)])
@pytest.mark.parametrize("kind", ["smooth", "eighths", "binary", "clamped"])
def test_plane_loss_and_gradient_against_fp64(shape, kind):
    n, H, W = shape
    t = R.line_target(n, H, W, seed=1)
    p = R.make_plane(kind, n, H, W, t, seed=2)
    void = R.void_mask(n, H, W, 0.2, seed=3)
    for iters in (0, 3, 10):
        terms, g = _check_plane(p, t, void, iters, label=f"{shape} {kind}")
    assert (g != 0).any()
    # without grad_prob the terms keep their bits; a second call gives the same bits
    terms_ng, _ = _plane(p, _truth(t, void), 10, want_grad=False)
    terms2, g2 = _plane(p, _truth(t, void), 10)
    assert torch.equal(_bits(terms_ng), _bits(terms)) and torch.equal(_bits(terms2), _bits(terms)) and torch.equal(_bits(g2), _bits(g))


def test_plane_loss_batch_order_scale_and_smooth():
    n, H, W = 3, 96, 96
    t = R.line_target(n, H, W, seed=5)
    p = R.make_plane("eighths", n, H, W, t, seed=6)
    void = R.void_mask(n, H, W, 0.1, seed=7)
    terms, g = _check_plane(p, t, void, 3, smooth=0.25, label="smooth 0.25")
    perm = torch.tensor([2, 0, 1])
    terms_p, g_p = _plane(p[perm].contiguous(), _truth(t, void)[perm].contiguous(), 3, 0.25)
    assert torch.equal(_bits(terms_p), _bits(terms)) and torch.equal(_bits(g_p), _bits(g[perm]))   # the order of the batch
    terms_s, g_s = _plane(p, _truth(t, void), 3, 0.25, grad_scale=0.25)
    big = g.abs() > 1e-30
    assert torch.equal(_bits(terms_s), _bits(terms)) and torch.equal(g_s[big], (g * 0.25)[big]) and torch.equal(g_s == 0, g == 0)


def test_plane_loss_everything_void_and_an_absent_class():
    n, H, W = 2, 33, 70
    t = R.line_target(n, H, W, seed=1)
    p = R.make_plane("smooth", n, H, W, t, seed=2)
    terms, g = _plane(p, torch.full((n, H, W), 255, dtype=torch.uint8), 3)
    assert terms.tolist() == [0.0, 1.0, 1.0, 0.0] and (g == 0).all() and not torch.signbit(g).any()
    # a class no target pixel carries: st = 0, tsens = s / s = 1, the gradient comes through tprec alone
    none = torch.zeros(n, H, W, dtype=torch.bool)
    terms, g = _check_plane(p, torch.zeros_like(t), none, 3, label="absent class")
    assert float(terms[2]) == 1.0 and float(terms[0]) > 0 and (g != 0).any()


def test_soft_cldice_loss_autograd_function():
    n, H, W = 2, 33, 70
    t = R.line_target(n, H, W, seed=1)
    p = R.make_plane("smooth", n, H, W, t, seed=2)
    void = R.void_mask(n, H, W, 0.2, seed=3)
    q = p.to(DEV).requires_grad_(True)
    loss = cldice.soft_cldice_loss(q, _truth(t, void).to(DEV), iters=3, smooth=1.0)
    (2.0 * loss).backward()
    ref, g64 = R.cldice_autograd(p, t.float(), void, 3, 1.0, torch.float64)
    _, g32 = R.cldice_autograd(p, t.float(), void, 3, 1.0, torch.float32)
    d_ref = (g32.double() - g64).abs().max().item()
    assert _rel(float(loss.detach()), ref[0]) <= 1e-6
    assert (q.grad.cpu().double() - 2.0 * g64).abs().max().item() <= 2.0 * 16 * d_ref
    with torch.no_grad():
        loss_b = cldice.soft_cldice_loss(p.to(DEV), (t == 1) & ~void, iters=3)   # bool: no void, the void pixels are not the class
    ref_b, _ = R.cldice_autograd(p, (t.bool() & ~void).float(), torch.zeros_like(void), 3, 1.0, torch.float64)
    assert _rel(float(loss_b), ref_b[0]) <= 1e-6


# ------------------------------------------------------------------ 3. the fused call
def _fused(z, target, S, classes, *, weight=0.5, iters=3, smooth=1.0, dice=None, ii=None, w=None, eps=0.0, null_ce=None,
           want_grad=True, loss_scale=1.0, null_cld=False, want_planes=True):
    """One vitseg_ce_cldice_loss call on guarded buffers.  dice: None (NULL) or (ce_weight, dice_weight)."""
    B, C_, g = z.shape[0], z.shape[1], z.shape[2]
    K = len(classes)
    L = _lib.lib()
    zd = guarded(z.shape, torch.float32, z, name="lowres")
    td = guarded(target.shape, target.dtype, target, name="target")
    gd = guarded((B, C_, S, S), torch.float32, "nan", name="grad_logits") if want_grad else None
    scratch = guarded(L.vitseg_ce_scratch_bytes(B, S), torch.uint8, "nan", name="ce scratch")
    terms = guarded((4,), torch.float32, "nan", name="terms")
    wd = guarded((C_,), torch.float32, torch.as_tensor(w, dtype=torch.float32), name="class_weight") if w is not None else None
    if null_ce is None:
        null_ce = ii is None and w is None and eps == 0.0
    oscr = ce = dscr = d = None
    if not null_ce:
        nbytes = int(_lib.ce_opts_symbol("vitseg_ce_options_scratch_bytes")(B, S))
        oscr = guarded(nbytes, torch.uint8, "nan", name="ce options scratch")
        ce = _lib.CCEOptions(int(ii is not None), 0, 0 if ii is None else ii, _ptr(wd), eps, oscr.data_ptr(), nbytes)
    if dice is not None:
        dbytes = int(_lib.dice_symbol("vitseg_dice_options_scratch_bytes")(B, C_, S))
        dscr = guarded(dbytes, torch.uint8, "nan", name="dice scratch")
        d = _lib.CDiceOptions(dice[0], dice[1], 1e-6, 1, dscr.data_ptr(), dbytes)
    cbytes = int(_sym("vitseg_cldice_scratch_bytes")(B, K, S, iters))
    cscr = guarded(cbytes, torch.uint8, "nan", name="cldice scratch")
    planes = guarded((K, B, S, S), torch.float32, "nan", name="prob_planes") if want_planes else None
    cterms = guarded((3 * K,), torch.float32, "nan", name="class_terms") if want_planes else None
    arr = (C.c_int32 * K)(*classes)
    c = _ext.CClDiceOptions(weight, smooth, iters, K, arr, cscr.data_ptr(), cbytes, _ptr(planes), _ptr(cterms))
    snap = snapshot(zd, td, wd)
    _lib.check(_sym("vitseg_ce_cldice_loss")(
        zd.data_ptr(), td.data_ptr(), int(target.dtype == torch.uint8), _ptr(gd), scratch.data_ptr(), terms.data_ptr(), B, C_, g, S,
        C.byref(ce) if ce is not None else None, C.byref(d) if d is not None else None, None if null_cld else C.byref(c), loss_scale,
        _stream()))
    torch.cuda.synchronize()
    check(zd, td, gd, scratch, terms, wd, oscr, dscr, cscr, planes, cterms)
    unchanged(snap)
    cpu = lambda t: t.cpu() if t is not None else None
    return SimpleNamespace(terms=terms.cpu(), grad=cpu(gd), planes=cpu(planes), cterms=cpu(cterms))


def _fused_case(B, C_, g, S, seed, ignore=0.0, ii=255, dtype=torch.uint8):
    """Logits that favour the thin lines of each class's target, so that the planes hold structure."""
    gen = torch.Generator().manual_seed(seed)
    t = torch.zeros(B, S, S, dtype=torch.int64)
    for c in range(1, C_):
        lines = R.line_target(B, S, S, seed=seed + c).bool()
        t[lines & (torch.rand(B, S, S, generator=gen) < 0.8)] = c
    z = torch.randn(B, C_, g, g, generator=gen).float() * 2.0
    if ignore > 0:
        t[torch.rand(B, S, S, generator=gen) < ignore] = ii
    return z, t.to(dtype)


def _reference(z, t, S, classes, r, *, weight, iters, smooth, dice, ii, w=None, eps=0.0, loss_scale=1.0):
    """The fp64 reference of a fused call from the kernel's own planes r.planes: (terms [4], grad, bound on grad, d_ref)."""
    B, C_ = z.shape[0], z.shape[1]
    K = len(classes)
    t64 = t.long()
    void = (t64 == ii) if ii is not None else torch.zeros_like(t64, dtype=torch.bool)
    cw, dw = dice if dice is not None else (1.0, 0.0)
    kw = dict(dice_weight=dw, ce_weight=cw, ignore_index=ii, class_weight=w, label_smoothing=eps)
    up = upsample64(z, S)
    if cw == 0.0 and dw == 0.0:
        loss0 = ce = dc = torch.zeros((), dtype=torch.float64)
        g0 = torch.zeros_like(up)
        b0 = bl = 0.0
    else:
        loss0, ce, dc, g0, _ = dice_ref.ce_dice_ref_up(up, t64, **kw)
        _, _, _, _, sums = dice_ref.closed_form(up, t64, **kw)
        b = dice_ref.bounds(up, t64, sums, loss0, ce, dc, g0.abs().max().item(), loss_scale=loss_scale, **kw)
        b0, bl = b["grad"], b["loss"]
        g0 = g0 * loss_scale
    # the term from the kernel's own planes, in fp64 and in fp32
    p64 = torch.softmax(up, dim=1)
    gs, cls, d_ref = {}, [], 0.0
    for k, c in enumerate(classes):
        y = (t64 == c).float()
        ref, g64 = R.cldice_autograd(r.planes[k], y, void, iters, smooth, torch.float64)
        _, g32 = R.cldice_autograd(r.planes[k], y, void, iters, smooth, torch.float32)
        d_ref = max(d_ref, (g32.double() - g64).abs().max().item() * weight / K * abs(loss_scale))
        gs[c] = g64 * (weight / K * loss_scale)
        cls.append(ref)
        p64[:, c] = torch.where(void, p64[:, c], r.planes[k].double())   # the kernel's own p where it handed one out
    cld = sum(x[0] for x in cls) / K
    sgp = sum(gs[c] * p64[:, c] for c in classes)
    grad = g0.clone()
    for j in range(C_):
        gj = gs.get(j, torch.zeros_like(sgp))
        grad[:, j] += torch.where(void, torch.zeros_like(sgp), p64[:, j] * (gj - sgp))
    terms = [float(cw * ce + dw * dc + weight * cld), float(ce), float(dc), cld]
    # the total: CE + Dice within their own bound (dice_ref.bounds), the term within 1e-6 relative, one rounding of the sum
    return terms, grad, b0 + 16 * d_ref, d_ref, cls, bl + 1e-6 * weight * cld + 2 * U * abs(terms[0])


def _check_fused(z, t, S, classes, label="", **kw):
    ii = kw.get("ii")
    r = _fused(z, t, S, classes, **kw)
    B, C_ = z.shape[0], z.shape[1]
    t64 = t.long()
    void = (t64 == ii) if ii is not None else torch.zeros_like(t64, dtype=torch.bool)
    # the planes against the oracle's softmax, within test_gpu_ce_options.py's bound on p (dice_ref: eps_p relative)
    up = upsample64(z, S)
    lse = torch.logsumexp(up, dim=1)
    e_pix = 4 * U * lse.abs().max().item() + 8 * U * up.abs().max().item() + 4 * (C_ + 2) * U
    p64 = torch.softmax(up, dim=1)
    for k, c in enumerate(classes):
        want = torch.where(void, torch.zeros_like(p64[:, c]), p64[:, c])
        assert ((r.planes[k].double() - want).abs() <= 1.01 * (e_pix + 8 * U) * want).all()
        assert (r.planes[k][void] == 0).all()
    rk = dict(weight=kw.get("weight", 0.5), iters=kw.get("iters", 3), smooth=kw.get("smooth", 1.0), dice=kw.get("dice"), ii=ii,
              w=kw.get("w"), eps=kw.get("eps", 0.0), loss_scale=kw.get("loss_scale", 1.0))
    terms, grad, bound, d_ref, cls, loss_b = _reference(z, t, S, classes, r, **rk)
    err = (r.grad.double() - grad).abs().max().item()
    rel3 = _rel(float(r.terms[3]), terms[3])
    print(f"{label}: terms {r.terms.tolist()} ref {terms}; cldice rel err {rel3:.1e}; grad err {err:.2e}, bound {bound:.2e} "
          f"(16 d_ref = {16 * d_ref:.2e}), max |grad| {grad.abs().max().item():.2e}")
    assert rel3 <= 1e-6
    for k in range(len(classes)):
        for i in range(3):
            assert _rel(float(r.cterms[3 * k + i]), cls[k][i]) <= 1e-6
    assert abs(float(r.terms[0]) - terms[0]) <= loss_b, (float(r.terms[0]), terms[0], loss_b)
    assert err <= bound
    g_ign = r.grad.permute(1, 0, 2, 3)[:, void]
    assert (g_ign == 0).all() and not torch.signbit(g_ign).any()
    return r


@pytest.mark.parametrize("B,C_,g,S", [(3, 2, 7, 28), (3, 3, 7, 28), (3, 17, 7, 28), (2, 3, 5, 40)])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
def test_fused_call_against_fp64(B, C_, g, S, dtype):
    z, t = _fused_case(B, C_, g, S, seed=11 + C_, ignore=1 / 3, dtype=dtype)
    full = list(range(1, C_))
    r = _check_fused(z, t, S, full, label=f"C {C_} K {C_ - 1}", ii=255, dice=(1.0, 0.5))
    r1 = _check_fused(z, t, S, [C_ - 1], label=f"C {C_} K 1", ii=255, iters=10, smooth=0.5)
    assert (r.grad != 0).any() and float(r1.terms[2]) == 0.0
    # the same bits on a second call, and without the optional outputs
    r2 = _fused(z, t, S, full, ii=255, dice=(1.0, 0.5), want_planes=False)
    assert torch.equal(_bits(r2.terms), _bits(r.terms)) and torch.equal(_bits(r2.grad), _bits(r.grad))
    r3 = _fused(z, t, S, full, ii=255, dice=(1.0, 0.5), want_grad=False)
    assert torch.equal(_bits(r3.terms), _bits(r.terms)) and torch.equal(_bits(r3.cterms), _bits(r.cterms))


def test_fused_call_targets_of_both_types_give_the_same_bits():
    z, t = _fused_case(3, 3, 7, 28, seed=5, ignore=0.2)
    a = _fused(z, t, 28, [1, 2], ii=255)
    b = _fused(z, t.long(), 28, [1, 2], ii=255)
    assert torch.equal(_bits(a.terms), _bits(b.terms)) and torch.equal(_bits(a.grad), _bits(b.grad))
    assert torch.equal(_bits(a.planes), _bits(b.planes))


def test_fused_call_term_alone_scaled_and_weighted():
    z, t = _fused_case(3, 3, 7, 28, seed=6, ignore=0.2)
    _check_fused(z, t, 28, [2, 1], label="ce_weight 0", ii=255, dice=(0.0, 0.0), weight=1.5)
    _check_fused(z, t, 28, [1], label="ce_weight 0, dice on", ii=255, dice=(0.0, 1.0))
    w = [0.5, 2.0, 1.0]
    a = _check_fused(z, t, 28, [1, 2], label="weights, smoothing", ii=255, w=w, eps=0.1, dice=(1.0, 0.25))
    s = _check_fused(z, t, 28, [1, 2], label="loss_scale", ii=255, w=w, eps=0.1, dice=(1.0, 0.25), loss_scale=0.25)
    assert torch.equal(_bits(s.terms), _bits(a.terms))   # the scale multiplies the gradient, not the reported terms


def test_fused_call_everything_ignored_and_a_bad_label():
    z, t = _fused_case(3, 3, 7, 28, seed=7)
    r = _fused(z, torch.full_like(t, 255), 28, [1, 2], ii=255, dice=(1.0, 0.5))
    assert torch.isnan(r.terms[0]) and torch.isnan(r.terms[1])          # CE is 0 / 0 as before
    assert float(r.terms[3]) == 0.0 and (r.grad == 0).all() and (r.planes == 0).all()
    r = _fused(z, torch.full_like(t, 255), 28, [1, 2], ii=255, dice=(0.0, 0.0))
    assert r.terms.tolist() == [0.0, 0.0, 0.0, 0.0] and (r.grad == 0).all()
    t2 = t.clone()
    t2[1, 5, 9] = 7   # no class and not ignored: the total is NaN through CE, the term itself stays finite
    r = _fused(z, t2, 28, [1, 2], ii=255)
    assert torch.isnan(r.terms[0]) and torch.isnan(r.terms[1]) and torch.isfinite(r.terms[3]) and float(r.terms[3]) > 0
    assert torch.isnan(r.grad[1, :, 5, 9]).all()


def _dice_call(z, t, S, dice, ii=None, w=None, eps=0.0, loss_scale=1.0):
    import test_gpu_ce_dice as TD
    return TD._run(z, t, S, dice_weight=dice[1], ce_weight=dice[0], ignore_index=ii, class_weight=w, label_smoothing=eps,
                   loss_scale=loss_scale)


@pytest.mark.parametrize("how", ["weight 0", "cld NULL"])
def test_without_the_term_the_bits_are_those_of_the_existing_calls(how):
    import test_gpu_ce_dice as TD
    z, t = _fused_case(3, 3, 7, 28, seed=8, ignore=0.2)
    off = dict(weight=0.0) if how == "weight 0" else dict(null_cld=True)
    a = _fused(z, t, 28, [1, 2], ii=255, w=[0.5, 2.0, 1.0], eps=0.1, dice=(1.0, 0.5), loss_scale=0.5, want_planes=False, **off)
    terms, grad = _dice_call(z, t, 28, (1.0, 0.5), ii=255, w=[0.5, 2.0, 1.0], eps=0.1, loss_scale=0.5)
    assert torch.equal(_bits(a.terms[:3]), _bits(terms)) and float(a.terms[3]) == 0.0 and torch.equal(_bits(a.grad), _bits(grad))
    # without the Dice options too: vitseg_ce_loss_opts
    b = _fused(z, t, 28, [1, 2], ii=255, w=[0.5, 2.0, 1.0], eps=0.1, loss_scale=0.5, want_planes=False, **off)
    loss, grad = TD._ce_opts_run(z, t, 28, ignore_index=255, class_weight=[0.5, 2.0, 1.0], label_smoothing=0.1, loss_scale=0.5)
    assert torch.equal(_bits(b.terms[:1]), _bits(loss)) and torch.equal(_bits(b.terms[1:2]), _bits(loss))
    assert b.terms[2:].tolist() == [0.0, 0.0] and torch.equal(_bits(b.grad), _bits(grad))
    # and with no option at all: vitseg_ce_loss
    z2, t2 = _fused_case(3, 3, 7, 28, seed=9)
    c = _fused(z2, t2, 28, [1, 2], want_planes=False, **off)
    loss, grad = TD._ce_opts_run(z2, t2, 28, plain=True)
    assert torch.equal(_bits(c.terms[:1]), _bits(loss)) and torch.equal(_bits(c.grad), _bits(grad))


def test_argument_errors_leave_the_outputs_untouched():
    B, C_, g, S = 3, 3, 7, 28
    z, t = _fused_case(B, C_, g, S, seed=10)
    zd, td = z.to(DEV), t.to(DEV)
    gd = guarded((B, C_, S, S), torch.float32, "nan", name="grad_logits")
    terms = guarded((4,), torch.float32, "nan", name="terms")
    scr = guarded(_lib.lib().vitseg_ce_scratch_bytes(B, S), torch.uint8, "nan", name="ce scratch")
    need = int(_sym("vitseg_cldice_scratch_bytes")(B, 2, S, 3))
    cscr = guarded(need, torch.uint8, "nan", name="cldice scratch")
    planes = guarded((2, B, S, S), torch.float32, "nan", name="prob_planes")
    fn = _sym("vitseg_ce_cldice_loss")
    ok = dict(weight=0.5, smooth=1.0, iters=3, classes=[1, 2], scr=cscr.data_ptr(), n=need)

    def call(lowres=zd.data_ptr(), terms_ptr=terms.data_ptr(), **kw):
        o = dict(ok, **kw)
        cls = o["classes"]
        arr = (C.c_int32 * max(len(cls), 1))(*cls)
        c = _ext.CClDiceOptions(o["weight"], o["smooth"], o["iters"], len(cls), arr, o["scr"], o["n"], planes.data_ptr(), None)
        return fn(lowres, td.data_ptr(), 1, gd.data_ptr(), scr.data_ptr(), terms_ptr, B, C_, g, S, None, None, C.byref(c), 1.0, _stream())
    nan, inf = float("nan"), float("inf")
    for kw in (dict(weight=-0.5), dict(weight=nan), dict(weight=inf), dict(smooth=0.0), dict(smooth=nan), dict(smooth=inf),
               dict(iters=-1), dict(iters=65), dict(classes=[]), dict(classes=[1, 1]), dict(classes=[3]), dict(classes=[0, 1, 2, 1]),
               dict(scr=None), dict(scr=cscr.data_ptr() + 4), dict(n=need - 1), dict(lowres=None), dict(terms_ptr=None)):
        assert call(**kw) == _lib.EINVAL, kw
    torch.cuda.synchronize()
    check(gd, terms, scr, cscr, planes)
    assert torch.isnan(gd).all() and torch.isnan(terms).all() and torch.isnan(planes).all()
    assert (cscr == 255).all() and (scr == 255).all()   # the poison: not a byte was written
    assert call() == _lib.OK   # and the valid call goes through
    torch.cuda.synchronize()
    check(gd, terms, scr, cscr, planes)
    assert torch.isfinite(terms).all() and torch.isfinite(gd).all() and torch.isfinite(planes).all()


# ------------------------------------------------------------------ 4. the whole path
def _small_model(C_=3, S=64, precision="fp32", seed=4):
    m = ViTSegmentationModel(C_, 16, 64, 1, 1, image_size=S, intermediate_size=128, precision=precision, device=DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(m.cfg, seed=seed).items()})
    m.eval()
    return m


@functools.lru_cache(maxsize=None)
def _batch(S=64, C_=3):
    gen = torch.Generator().manual_seed(41)
    y = torch.zeros(2, S, S, dtype=torch.int64)
    for c in range(1, C_):
        y[R.line_target(2, S, S, seed=40 + c).bool()] = c
    y[torch.rand(2, S, S, generator=gen) < 0.1] = 255
    return y.to(torch.uint8)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ce_cldice_loss_is_the_standalone_call_fed_through_backward(precision):
    """model.ce_cldice_loss(...).backward() against vitseg_ce_cldice_loss run standalone on the training forward's full-size
    logits (g == S: the taps are the identity, so it reads the bits the fused loss regenerates) and its gradient fed through
    vitseg_backward's grad_logits entry: the same arena gradient and the same terms, bit for bit."""
    m = _small_model(precision=precision)
    S, B, C_ = 64, 2, 3
    x = torch.from_numpy(synth.make_images(m.cfg, B, seed=4)).to(DEV)
    y = _batch().to(DEV)
    kw = dict(cldice_weight=0.5, cldice_classes=[1, 2], cldice_iters=3, dice_weight=0.25, ignore_index=255, class_weight=[0.5, 2.0, 1.0])
    m.zero_grad(set_to_none=True)
    loss, ce, dice, cld = m.ce_cldice_loss(x, y, return_terms=True, **kw)
    loss.backward()
    torch.cuda.synchronize()
    g1 = m.arena.grad.detach().clone()
    assert torch.isfinite(loss) and torch.isfinite(g1).all() and float(g1.abs().max()) > 0 and 0 < float(cld) < 1
    assert not ce.requires_grad and not cld.requires_grad
    assert abs(float(loss.detach()) - (float(ce) + 0.25 * float(dice) + 0.5 * float(cld))) <= 1e-6 * abs(float(loss.detach()))

    logits = m._forward_train(x, True)
    gd = guarded((B, C_, S, S), torch.float32, "nan", name="grad_logits")
    scr = torch.empty(_lib.lib().vitseg_ce_scratch_bytes(B, S), dtype=torch.uint8, device=DEV)
    oscr = torch.empty(int(_lib.ce_opts_symbol("vitseg_ce_options_scratch_bytes")(B, S)), dtype=torch.uint8, device=DEV)
    dscr = torch.empty(int(_lib.dice_symbol("vitseg_dice_options_scratch_bytes")(B, C_, S)), dtype=torch.uint8, device=DEV)
    cscr = torch.empty(int(_sym("vitseg_cldice_scratch_bytes")(B, 2, S, 3)), dtype=torch.uint8, device=DEV)
    wd = torch.tensor([0.5, 2.0, 1.0], device=DEV)
    o = _lib.CCEOptions(1, 0, 255, wd.data_ptr(), 0.0, oscr.data_ptr(), oscr.numel())
    d = _lib.CDiceOptions(1.0, 0.25, 1e-6, 1, dscr.data_ptr(), dscr.numel())
    arr = (C.c_int32 * 2)(1, 2)
    c = _ext.CClDiceOptions(0.5, 1.0, 3, 2, arr, cscr.data_ptr(), cscr.numel(), None, None)
    terms2 = torch.empty(4, dtype=torch.float32, device=DEV)
    _lib.check(_sym("vitseg_ce_cldice_loss")(logits.data_ptr(), y.data_ptr(), 1, gd.data_ptr(), scr.data_ptr(), terms2.data_ptr(), B, C_,
                                             S, S, C.byref(o), C.byref(d), C.byref(c), 1.0, _stream()))
    torch.cuda.synchronize()
    check(gd)
    assert torch.equal(_bits(terms2), _bits(torch.stack([loss.detach(), ce, dice, cld])))
    g2, _ = m._backward(x, grad_logits=gd)
    torch.cuda.synchronize()
    assert torch.equal(_bits(g2), _bits(g1))
    m._release_grad_buffer(g2)
    # grad_scale scales the deposit and leaves the loss alone; the no-grad path forms the same terms from the inference forward
    m.zero_grad(set_to_none=True)
    loss4 = m.ce_cldice_loss(x, y, grad_scale=0.25, **kw)
    loss4.backward()
    torch.cuda.synchronize()
    big = g1.abs() > 1e-30
    assert torch.equal(_bits(loss4.detach().reshape(1)), _bits(loss.detach().reshape(1)))
    assert torch.equal(m.arena.grad[big], (g1 * 0.25)[big])
    with torch.no_grad():
        t_ng = m.ce_cldice_loss(x, y, return_terms=True, **kw)
    # the inference forward is another chain of GEMMs than the training forward: fp32 sums in another order (a few 1e-6 of a
    # logit), 16-bit operands on the bf16 route (2^-8 per product)
    tol = 1e-4 if precision == "fp32" else 2e-2
    for a, b in zip(t_ng, (loss.detach(), ce, dice, cld)):
        assert abs(float(a) - float(b)) <= tol * abs(float(b))
    m.zero_grad(set_to_none=True)
    # the defaults: every class but 0, no Dice term; the term alone
    with torch.no_grad():
        la = m.ce_cldice_loss(x, y, ignore_index=255, return_terms=True)
        lb = m.ce_cldice_loss(x, y, ignore_index=255, cldice_classes=[1, 2], dice_weight=0.0, return_terms=True)
        lc = m.ce_cldice_loss(x, y, ignore_index=255, ce_weight=0.0, cldice_weight=1.0, return_terms=True)
        with pytest.raises(ValueError):
            m.ce_cldice_loss(x, y, cldice_classes=[3])
    assert torch.equal(_bits(torch.stack(la)), _bits(torch.stack(lb))) and float(la[2]) == 0.0
    assert torch.equal(_bits(lc[0].reshape(1)), _bits(lc[3].reshape(1))) and float(lc[1]) == 0.0
    m.zero_grad(set_to_none=True)


def test_backward_cldice_argument_errors_and_its_null_form():
    m = _small_model()
    S = 64
    x = torch.from_numpy(synth.make_images(m.cfg, 1, seed=4)).to(DEV)
    t = _batch()[:1].clone()
    t[t == 255] = 0   # no CE options here: nothing is ignored, so every label is a class
    t = t.contiguous().to(DEV)
    m._forward_train(x, False)
    ws = m._train_workspace(1, S)
    grads = guarded(m.arena.shape, torch.float32, "nan", name="grads")
    loss = guarded((1,), torch.float32, "nan", name="loss")
    terms = guarded((4,), torch.float32, "nan", name="terms")
    gl = torch.zeros(1, 3, S, S, device=DEV)
    need = int(_sym("vitseg_cldice_scratch_bytes")(1, 2, S, 3))
    cscr = guarded(need, torch.uint8, "nan", name="cldice scratch")
    dbytes = int(_lib.dice_symbol("vitseg_dice_options_scratch_bytes")(1, 3, S))
    dscr = guarded(dbytes, torch.uint8, "nan", name="dice scratch")
    cfg = C.byref(_lib.CConfig.from_config(m.cfg))
    fn = _sym("vitseg_backward_cldice")
    arr = (C.c_int32 * 2)(1, 2)
    bad = (C.c_int32 * 2)(1, 3)

    def call(c, d=None, target=t, grad_logits=None, terms_ptr=terms.data_ptr()):
        return fn(cfg, S, m.arena.data_ptr(), None, x.data_ptr(), 1, m.precision, 0.0, 0, _ptr(target), 1, _ptr(grad_logits),
                  grads.data_ptr(), loss.data_ptr(), 1.0, None, ws.data_ptr(), ws.numel(), _stream(), None,
                  C.byref(d) if d is not None else None, C.byref(c) if c is not None else None, terms_ptr)
    O_ = lambda w=0.5, sm=1.0, it=3, cl=arr, scr=cscr.data_ptr(), n=need: _ext.CClDiceOptions(w, sm, it, 2, cl, scr, n, None, None)
    assert call(O_(), target=None, grad_logits=gl) == _lib.EINVAL
    assert call(O_(), terms_ptr=None) == _lib.EINVAL
    for c in (O_(w=-1.0), O_(sm=0.0), O_(it=65), O_(cl=bad), O_(scr=None), O_(scr=cscr.data_ptr() + 4), O_(n=need - 1)):
        assert call(c) == _lib.EINVAL
    torch.cuda.synchronize()
    check(grads, loss, terms, cscr, dscr)
    assert torch.isnan(grads).all() and torch.isnan(loss).all() and torch.isnan(terms).all() and (cscr == 255).all()
    assert call(O_()) == _lib.OK
    torch.cuda.synchronize()
    check(grads, loss, terms, cscr, dscr)
    assert torch.isfinite(grads).all() and torch.isfinite(terms).all() and torch.equal(_bits(loss), _bits(terms[0:1]))
    assert float(terms[2]) == 0.0 and 0 < float(terms[3]) < 1
    # cld == NULL with the Dice options: vitseg_backward_dice's bits, and terms[3] = 0
    d = _lib.CDiceOptions(1.0, 0.5, 1e-6, 1, dscr.data_ptr(), dbytes)
    m._forward_train(x, False)
    assert call(None, d=d) == _lib.OK
    torch.cuda.synchronize()
    g0, t0 = grads.clone(), terms.clone()
    grads.fill_(float("nan"))
    m._forward_train(x, False)
    terms3 = guarded((3,), torch.float32, "nan", name="terms")
    _lib.check(_lib.dice_symbol("vitseg_backward_dice")(
        cfg, S, m.arena.data_ptr(), None, x.data_ptr(), 1, m.precision, 0.0, 0, t.data_ptr(), 1, None, grads.data_ptr(), loss.data_ptr(),
        1.0, None, ws.data_ptr(), ws.numel(), _stream(), None, C.byref(d), terms3.data_ptr()))
    torch.cuda.synchronize()
    check(grads, loss, terms3)
    assert torch.equal(_bits(grads), _bits(g0)) and torch.equal(_bits(terms3), _bits(t0[:3])) and float(t0[3]) == 0.0


def test_lightning_module_logs_the_term_and_validates_with_it():
    from visiontransformer_amd.lightning import LightningViTModel
    m0 = _small_model()
    c = m0.cfg
    lm = LightningViTModel(c.num_classes, c.patch_size, c.hidden_size, c.num_hidden_layers, c.num_attention_heads,
                           image_size=c.image_size, intermediate_size=c.intermediate_size, device=DEV, ignore_index=255,
                           cldice_weight=0.5, cldice_iters=2)
    lm.model.load_state_dict(m0.state_dict())
    lm.eval()
    x = torch.from_numpy(synth.make_images(c, 2, seed=4)).to(DEV)
    y = _batch().to(DEV)
    lt = lm.training_step((x, y), 0)
    lt.backward()
    lv = lm.validation_step((x, y), 0)
    torch.cuda.synchronize()
    assert {"train_loss", "train_ce", "train_dice", "train_cldice", "valid_loss", "valid_ce", "valid_dice", "valid_cldice"} <= set(lm.logged)
    assert lm.logged["train_cldice"].is_cuda and 0 < float(lm.logged["valid_cldice"]) < 1 and float(lm.logged["valid_dice"]) == 0.0
    assert torch.isfinite(lt) and torch.isfinite(lm.model.arena.grad).all()
    with torch.no_grad():
        want = lm.model.ce_cldice_loss(x, y, ignore_index=255, cldice_weight=0.5, cldice_iters=2)
    assert torch.equal(_bits(lv.reshape(1)), _bits(want.reshape(1)))
    assert abs(float(lv) - (float(lm.logged["valid_ce"]) + 0.5 * float(lm.logged["valid_cldice"]))) <= 1e-6 * abs(float(lv))
