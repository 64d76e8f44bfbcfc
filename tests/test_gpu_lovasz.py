"""GPU (-m gpu): the Lovasz-Softmax loss (include/vitseg_lovasz.h: vitseg_lovasz_planes, vitseg_ce_lovasz_loss,
vitseg_backward_lovasz, lovasz.py, ViTSegmentationModel.ce_lovasz_loss) against tests/lovasz_ref.py.  Every buffer is
guard-banded; every scratch has exactly the queried size and arrives NaN-poisoned.

The sort: `order` element for element and `grad_prob` bit for bit against restatement (b), the closed form in integers with one
stated fp64 formula.  Terms: 2^-22 relative -- non-negative fp64 products summed in fp64 (n 2^-53, whatever the order), then two
fp32 roundings.
The fused call: the kernel's own planes go through (b): `grad_planes` bit for bit, `class_terms` and `terms[3]` within 2^-22;
`grad_logits` within dice_ref.bounds(...)["grad"] for the CE / Dice part plus
(1.01 eps_p + (2 K + 4) U) max_pixel(max_j |g_j| + sum_c |g_c|): p_j within eps_p of the oracle's softmax, and 2 K + 4 fp32
roundings in p_j (g_j - sum_c g_c p_c) and its add."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dice_ref
import lovasz_ref as R
from ce_ref import upsample64
from guard import check, guarded, snapshot, unchanged
from test_gpu_cldice import _batch, _fused_case, _small_model
from visiontransformer_amd import _ext, _lib, lovasz, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -23
T = lovasz.TILE
REL = 2.0 ** -22


def _sym(name):
    return _ext.ext_symbol("lovasz", name)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _close(got, want, rel=REL):
    return abs(float(got) - float(want)) <= rel * abs(float(want))


# ------------------------------------------------------------------ 1. the sort, exactly
def _planes(prob, truth, grad_scale=1.0, want_grad=True, want_order=True):
    """One vitseg_lovasz_planes call on guarded buffers: prob fp32 [n, L], truth uint8 [n, L] (numpy)."""
    n, L = prob.shape
    pd = guarded((n, L), torch.float32, torch.from_numpy(prob), name="prob")
    td = guarded((n, L), torch.uint8, torch.from_numpy(truth), name="truth")
    gd = guarded((n, L), torch.float32, "nan", name="grad_prob") if want_grad else None
    od = guarded((n, L), torch.int32, "nan", name="order") if want_order else None
    terms = guarded((n,), torch.float32, "nan", name="terms")
    scr = guarded(int(_sym("vitseg_lovasz_planes_scratch_bytes")(n, L)), torch.uint8, "nan", name="lovasz scratch")
    snap = snapshot(pd, td)
    _lib.check(_sym("vitseg_lovasz_planes")(pd.data_ptr(), td.data_ptr(), n, L, grad_scale, scr.data_ptr(), terms.data_ptr(), _ptr(gd),
                                            _ptr(od), _stream()))
    torch.cuda.synchronize()
    check(pd, td, gd, od, terms, scr)
    unchanged(snap)
    return terms.cpu().numpy(), (gd.cpu().numpy() if want_grad else None), (od.cpu().numpy() if want_order else None)


def _check_planes(prob, truth, label, grad_scale=1.0):
    terms, grad, order = _planes(prob, truth, grad_scale)
    for s in range(prob.shape[0]):
        y, valid = truth[s] == 1, truth[s] != 255
        loss, g, o, G = R.closed_form(R.errors32(prob[s], y), y, valid, coef=np.float64(np.float32(grad_scale)))
        assert np.array_equal(order[s], o), (label, s, int((order[s] != o).sum()))
        assert np.array_equal(grad[s].view(np.int32), g.view(np.int32)), (label, s, int((grad[s].view(np.int32) != g.view(np.int32)).sum()))
        assert _close(terms[s], loss), (label, s, float(terms[s]), loss)
    return terms


LENGTHS = [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]
KINDS = ["smooth", "eighths", "constant", "sorted", "reversed", "lowest digit", "highest digit", "zeros and ones"]


@pytest.mark.parametrize("kind", KINDS)
def test_sort_order_and_gradient_are_the_closed_form_exactly(kind):
    for n in (1, 3):
        for L in LENGTHS:
            prob = R.make_plane(kind, n, L, seed=L + n)
            truth = R.make_truth(n, L, seed=2 * L + n)
            _check_planes(prob, truth, f"{kind} n {n} L {L}")
            if kind in ("lowest digit", "highest digit"):   # y = 0 everywhere: e = p, the keys differ in that digit alone
                key = R.sort_key(prob)
                if kind == "lowest digit":
                    assert len(np.unique(key >> 8)) == 1 and (L < 64 or len(np.unique(key & 255)) > 16)
                else:
                    assert len(np.unique(key & 0xFFFFFF)) == 1 and (L < 64 or len(np.unique(key >> 24)) > 16)
                terms = _check_planes(prob, np.zeros((n, L), np.uint8), f"{kind}, G = 0, n {n} L {L}")
                assert np.array_equal(terms, prob.max(axis=1))   # G = 0: the largest error
    if kind == "zeros and ones":
        assert set(np.unique(R.make_plane(kind, 3, T + 1, seed=1))) == {0.0, 1.0}


@pytest.mark.parametrize("void", ["a third", "everything"])
def test_sort_with_void_pixels(void):
    for n in (1, 3):
        for L in LENGTHS:
            for kind in ("smooth", "eighths"):
                prob = R.make_plane(kind, n, L, seed=L + n)
                truth = R.make_truth(n, L, seed=3 * L + n, void=1 / 3) if void == "a third" else np.full((n, L), 255, np.uint8)
                terms, grad, order = _planes(prob, truth)
                _check_planes(prob, truth, f"{kind}, {void} void, n {n} L {L}", grad_scale=0.25)
                gv = grad[truth == 255]
                assert (gv == 0).all() and not np.signbit(gv).any()
                assert ((order == -1).sum(axis=1) == (truth == 255).sum(axis=1)).all()
                if void == "everything":
                    assert (terms == 0).all() and (order == -1).all()


def test_sort_repeats_its_bits_and_ranks_a_nan_first():
    L, n = 3 * T + 17, 3
    prob = R.make_plane("eighths", n, L, seed=9)
    truth = R.make_truth(n, L, seed=10, void=0.2)
    a, b = _planes(prob, truth), _planes(prob, truth)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    c = _planes(prob, truth, want_grad=False, want_order=False)
    assert np.array_equal(c[0].view(np.int32), a[0].view(np.int32)) and c[1] is None
    prob[1, 5000] = np.nan
    truth[1, 5000] = 0
    terms, grad, order = _planes(prob, truth)
    assert order[1, 0] == 5000 and np.isnan(terms[1]) and np.isfinite(terms[[0, 2]]).all() and np.isfinite(grad).all()
    _, g, o, _ = R.closed_form(R.errors32(prob[1], truth[1] == 1), truth[1] == 1, truth[1] != 255)
    assert np.array_equal(order[1], o) and np.array_equal(grad[1].view(np.int32), g.view(np.int32))


def test_module_planes_function_under_autograd():
    n, L = 2, T + 5
    prob = R.make_plane("smooth", n, L, seed=3)
    truth = R.make_truth(n, L, seed=4, void=0.2)
    q = torch.from_numpy(prob).to(DEV).requires_grad_(True)
    losses = lovasz.lovasz_softmax_planes(q, torch.from_numpy(truth).to(DEV))
    (losses * torch.tensor([2.0, 0.5], device=DEV)).sum().backward()
    terms, grad, order = lovasz.sort_planes(torch.from_numpy(prob).to(DEV), torch.from_numpy(truth).to(DEV))
    for s, w in enumerate((2.0, 0.5)):
        y, valid = truth[s] == 1, truth[s] != 255
        loss, g, o, _ = R.closed_form(R.errors32(prob[s], y), y, valid)
        assert _close(losses[s].detach(), loss) and np.array_equal(order[s].cpu().numpy(), o)
        assert np.array_equal(grad[s].cpu().numpy(), g) and np.array_equal(q.grad[s].cpu().numpy(), g * np.float32(w))
    b = lovasz.lovasz_softmax_planes(torch.from_numpy(prob[0]).to(DEV), torch.from_numpy(truth[0] == 1).to(DEV))   # bool: no void
    assert _close(b[0], R.closed_form(R.errors32(prob[0], truth[0] == 1), truth[0] == 1)[0])


# ------------------------------------------------------------------ 2. the fused call
def _fused(z, target, S, classes, *, weight=0.5, per_image=0, present=1, dice=None, ii=None, w=None, eps=0.0, want_grad=True,
           loss_scale=1.0, null_lov=False, want_planes=True):
    """One vitseg_ce_lovasz_loss call on guarded buffers.  dice: None (NULL) or (ce_weight, dice_weight)."""
    B, C_, g = z.shape[0], z.shape[1], z.shape[2]
    K = len(classes)
    L = _lib.lib()
    zd = guarded(z.shape, torch.float32, z, name="lowres")
    td = guarded(target.shape, target.dtype, target, name="target")
    gd = guarded((B, C_, S, S), torch.float32, "nan", name="grad_logits") if want_grad else None
    scratch = guarded(L.vitseg_ce_scratch_bytes(B, S), torch.uint8, "nan", name="ce scratch")
    terms = guarded((4,), torch.float32, "nan", name="terms")
    wd = guarded((C_,), torch.float32, torch.as_tensor(w, dtype=torch.float32), name="class_weight") if w is not None else None
    oscr = ce = dscr = d = None
    if not (ii is None and w is None and eps == 0.0):
        nbytes = int(_lib.ce_opts_symbol("vitseg_ce_options_scratch_bytes")(B, S))
        oscr = guarded(nbytes, torch.uint8, "nan", name="ce options scratch")
        ce = _lib.CCEOptions(int(ii is not None), 0, 0 if ii is None else ii, _ptr(wd), eps, oscr.data_ptr(), nbytes)
    if dice is not None:
        dbytes = int(_lib.dice_symbol("vitseg_dice_options_scratch_bytes")(B, C_, S))
        dscr = guarded(dbytes, torch.uint8, "nan", name="dice scratch")
        d = _lib.CDiceOptions(dice[0], dice[1], 1e-6, 1, dscr.data_ptr(), dbytes)
    cbytes = int(_sym("vitseg_lovasz_scratch_bytes")(B, K, S))
    cscr = guarded(cbytes, torch.uint8, "nan", name="lovasz scratch")
    planes = guarded((K, B, S, S), torch.float32, "nan", name="prob_planes") if want_planes else None
    gplanes = guarded((K, B, S, S), torch.float32, "nan", name="grad_planes") if want_planes else None
    cterms = guarded((K * (B if per_image else 1),), torch.float32, "nan", name="class_terms") if want_planes else None
    arr = (C.c_int32 * K)(*classes)
    c = _ext.CLovaszOptions(weight, K, arr, per_image, present, cscr.data_ptr(), cbytes, _ptr(planes), _ptr(gplanes), _ptr(cterms))
    snap = snapshot(zd, td, wd)
    _lib.check(_sym("vitseg_ce_lovasz_loss")(
        zd.data_ptr(), td.data_ptr(), int(target.dtype == torch.uint8), _ptr(gd), scratch.data_ptr(), terms.data_ptr(), B, C_, g, S,
        C.byref(ce) if ce is not None else None, C.byref(d) if d is not None else None, None if null_lov else C.byref(c), loss_scale,
        _stream()))
    torch.cuda.synchronize()
    check(zd, td, gd, scratch, terms, wd, oscr, dscr, cscr, planes, gplanes, cterms)
    unchanged(snap)
    cpu = lambda t: t.cpu() if t is not None else None
    return SimpleNamespace(terms=terms.cpu(), grad=cpu(gd), planes=cpu(planes), gplanes=cpu(gplanes), cterms=cpu(cterms))


def _term_from_planes(r, t, classes, ii, per_image, present, weight, loss_scale):
    """(b) on the kernel's own planes: (the term, L_c per segment, the g planes fp32 [K, B, S, S])."""
    B = t.shape[0]
    tt = t.long().numpy().reshape(B, -1)
    valid = tt != ii if ii is not None else np.ones_like(tt, dtype=bool)
    y = np.stack([tt == c for c in classes])
    p = r.planes.numpy().reshape(len(classes), B, -1)
    e = np.stack([R.errors32(p[k], y[k]) for k in range(len(classes))])
    total, Lc, g = R.term(e, y, valid, bool(per_image), bool(present), weight, loss_scale)
    return total, Lc, g.reshape(r.planes.shape)


def _check_fused(z, t, S, classes, label="", **kw):
    ii, K = kw.get("ii"), len(classes)
    weight, loss_scale, dice = kw.get("weight", 0.5), kw.get("loss_scale", 1.0), kw.get("dice")
    per_image, present = kw.get("per_image", 0), kw.get("present", 1)
    r = _fused(z, t, S, classes, **kw)
    B, C_ = z.shape[0], z.shape[1]
    t64 = t.long()
    void = (t64 == ii) if ii is not None else torch.zeros_like(t64, dtype=torch.bool)
    # the planes against the oracle's softmax, within test_gpu_cldice.py's bound on p
    up = upsample64(z, S)
    lse = torch.logsumexp(up, dim=1)
    e_pix = 4 * U * lse.abs().max().item() + 8 * U * up.abs().max().item() + 4 * (C_ + 2) * U
    eps_p = e_pix + 8 * U
    p64 = torch.softmax(up, dim=1)
    for k, c in enumerate(classes):
        want = torch.where(void, torch.zeros_like(p64[:, c]), p64[:, c])
        assert ((r.planes[k].double() - want).abs() <= 1.01 * eps_p * want).all()
        assert (r.planes[k][void] == 0).all()
    # the kernel's own planes through (b)
    lov, Lc, g = _term_from_planes(r, t, classes, ii, per_image, present, weight, loss_scale)
    gp = r.gplanes.numpy()
    assert np.array_equal(gp.view(np.int32), g.view(np.int32)), (label, int((gp.view(np.int32) != g.view(np.int32)).sum()))
    gv = r.gplanes[:, void]
    assert (gv == 0).all() and not torch.signbit(gv).any()
    for got, want in zip(r.cterms.tolist(), np.asarray(Lc).reshape(-1).tolist()):
        assert _close(got, want), (label, got, want)
    assert _close(r.terms[3], lov), (label, float(r.terms[3]), lov)
    # the CE / Dice part in fp64 and its bound
    cw, dw = dice if dice is not None else (1.0, 0.0)
    dkw = dict(dice_weight=dw, ce_weight=cw, ignore_index=ii, class_weight=kw.get("w"), label_smoothing=kw.get("eps", 0.0))
    if cw == 0.0 and dw == 0.0:
        ce = dc = torch.zeros((), dtype=torch.float64)
        g0 = torch.zeros_like(up)
        b0 = bl = 0.0
    else:
        loss0, ce, dc, g0, _ = dice_ref.ce_dice_ref_up(up, t64, **dkw)
        _, _, _, _, sums = dice_ref.closed_form(up, t64, **dkw)
        b = dice_ref.bounds(up, t64, sums, loss0, ce, dc, g0.abs().max().item(), loss_scale=loss_scale, **dkw)
        b0, bl = b["grad"], b["loss"]
        g0 = g0 * loss_scale
    gs = {c: torch.from_numpy(g[k]).double() for k, c in enumerate(classes)}
    sgp = sum(gs[c] * p64[:, c] for c in classes)
    grad = g0.clone()
    zero = torch.zeros_like(sgp)
    for j in range(C_):
        grad[:, j] += torch.where(void, zero, p64[:, j] * (gs.get(j, zero) - sgp))
    gabs = torch.from_numpy(np.abs(g)).double()
    per_pixel = float((gabs.max(dim=0).values + gabs.sum(dim=0)).max())
    bound = b0 + (1.01 * eps_p + (2 * K + 4) * U) * per_pixel
    err = (r.grad.double() - grad).abs().max().item()
    total = float(cw * ce + dw * dc + weight * lov)
    loss_b = bl + REL * weight * abs(lov) + 2 * U * abs(total)
    print(f"{label}: terms {r.terms.tolist()} ref total {total:.7f} lovasz {lov:.7f}; grad err {err:.2e}, bound {bound:.2e} "
          f"(CE / Dice part {b0:.2e}), max |grad| {grad.abs().max().item():.2e}")
    assert err <= bound
    g_ign = r.grad.permute(1, 0, 2, 3)[:, void]
    assert (g_ign == 0).all() and not torch.signbit(g_ign).any()
    assert abs(float(r.terms[0]) - total) <= loss_b, (float(r.terms[0]), total, loss_b)
    return r


@pytest.mark.parametrize("B,C_,g,S", [(3, 2, 7, 28), (3, 3, 7, 28), (3, 17, 7, 28), (2, 3, 5, 40), (3, 3, 7, 56)])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
def test_fused_call_against_the_closed_form_and_fp64(B, C_, g, S, dtype):
    z, t = _fused_case(B, C_, g, S, seed=11 + C_, ignore=1 / 3, dtype=dtype)
    if S == 56:
        assert B * S * S > 4 * T   # the pooled segment spans several tiles
    for per_image in (0, 1):
        r = _check_fused(z, t, S, list(range(C_)), label=f"C {C_} K {C_} per_image {per_image}", ii=255, dice=(1.0, 0.5),
                         per_image=per_image)
        r1 = _check_fused(z, t, S, [C_ - 1], label=f"C {C_} K 1 per_image {per_image}", ii=255, per_image=per_image)
        assert (r.grad != 0).any() and float(r1.terms[2]) == 0.0 and 0 < float(r.terms[3]) <= 1
    # the same bits on a second call, and without the optional outputs
    r2 = _fused(z, t, S, [C_ - 1], ii=255, per_image=1, want_planes=False)
    assert torch.equal(_bits(r2.terms), _bits(r1.terms)) and torch.equal(_bits(r2.grad), _bits(r1.grad))
    r3 = _fused(z, t, S, [C_ - 1], ii=255, per_image=1, want_grad=False)
    assert torch.equal(_bits(r3.terms), _bits(r1.terms)) and torch.equal(_bits(r3.cterms), _bits(r1.cterms))
    assert torch.equal(_bits(r3.gplanes), _bits(r1.gplanes))


def test_fused_call_targets_of_both_types_give_the_same_bits():
    z, t = _fused_case(3, 3, 7, 28, seed=5, ignore=0.2)
    a = _fused(z, t, 28, [1, 2], ii=255)
    b = _fused(z, t.long(), 28, [1, 2], ii=255)
    assert torch.equal(_bits(a.terms), _bits(b.terms)) and torch.equal(_bits(a.grad), _bits(b.grad))
    assert torch.equal(_bits(a.planes), _bits(b.planes)) and torch.equal(_bits(a.gplanes), _bits(b.gplanes))


def test_per_image_segment_has_the_same_bits_alone_as_in_a_batch():
    z, t = _fused_case(3, 3, 7, 28, seed=5, ignore=0.2)
    a = _fused(z, t, 28, [1, 2], ii=255, per_image=1, present=0)
    for b in range(3):
        one = _fused(z[b:b + 1], t[b:b + 1], 28, [1, 2], ii=255, per_image=1, present=0)
        assert torch.equal(_bits(one.cterms), _bits(a.cterms.view(2, 3)[:, b]))


def test_fused_call_an_absent_listed_class():
    z, t = _fused_case(3, 3, 7, 28, seed=6, ignore=0.2)
    t[t == 2] = 0      # class 2 nowhere
    t[0][t[0] == 1] = 0   # class 1 not in image 0
    for per_image in (0, 1):
        on = _check_fused(z, t, 28, [0, 1, 2], label=f"absent, present_only, per_image {per_image}", ii=255, per_image=per_image)
        off = _check_fused(z, t, 28, [0, 1, 2], label=f"absent, all, per_image {per_image}", ii=255, per_image=per_image, present=0)
        assert (on.gplanes[2] == 0).all() and not torch.signbit(on.gplanes[2]).any() and (off.gplanes[2] != 0).any()
        assert torch.equal(_bits(on.cterms), _bits(off.cterms)) and float(on.terms[3]) != float(off.terms[3])
        if per_image:
            assert (on.gplanes[1, 0] == 0).all() and (on.gplanes[1, 1] != 0).any()
    alone = _check_fused(z, t, 28, [2], label="only an absent class", ii=255, dice=(0.0, 0.0))   # K' = 0: the term is 0
    assert alone.terms.tolist() == [0.0, 0.0, 0.0, 0.0] and (alone.grad == 0).all()


def test_fused_call_term_alone_scaled_and_weighted():
    z, t = _fused_case(3, 3, 7, 28, seed=6, ignore=0.2)
    _check_fused(z, t, 28, [2, 1], label="ce_weight 0", ii=255, dice=(0.0, 0.0), weight=1.5)
    _check_fused(z, t, 28, [1], label="ce_weight 0, dice on", ii=255, dice=(0.0, 1.0), per_image=1)
    w = [0.5, 2.0, 1.0]
    a = _check_fused(z, t, 28, [0, 1, 2], label="weights, smoothing", ii=255, w=w, eps=0.1, dice=(1.0, 0.25))
    s = _check_fused(z, t, 28, [0, 1, 2], label="loss_scale", ii=255, w=w, eps=0.1, dice=(1.0, 0.25), loss_scale=0.25)
    assert torch.equal(_bits(s.terms), _bits(a.terms))   # the scale multiplies the gradient, not the reported terms
    assert not torch.equal(_bits(s.gplanes), _bits(a.gplanes))


def test_fused_call_everything_ignored_and_a_bad_label():
    z, t = _fused_case(3, 3, 7, 28, seed=7)
    for per_image in (0, 1):
        r = _fused(z, torch.full_like(t, 255), 28, [1, 2], ii=255, dice=(1.0, 0.5), per_image=per_image)
        assert torch.isnan(r.terms[0]) and torch.isnan(r.terms[1])          # CE is 0 / 0 as before
        assert float(r.terms[3]) == 0.0 and (r.grad == 0).all() and (r.planes == 0).all() and (r.gplanes == 0).all()
        r = _fused(z, torch.full_like(t, 255), 28, [1, 2], ii=255, dice=(0.0, 0.0), per_image=per_image, present=0)
        assert r.terms.tolist() == [0.0, 0.0, 0.0, 0.0] and (r.grad == 0).all() and not torch.signbit(r.grad).any()
    t2 = t.clone()
    t2[1, 5, 9] = 7   # no class and not ignored: the total is NaN through CE; for the term it is a pixel of no listed class
    r = _fused(z, t2, 28, [1, 2], ii=255)
    assert torch.isnan(r.terms[0]) and torch.isnan(r.terms[1]) and torch.isfinite(r.terms[3]) and float(r.terms[3]) > 0
    assert torch.isnan(r.grad[1, :, 5, 9]).all()
    z2 = z.clone()
    z2[0, 1, 3, 3] = float("nan")   # a NaN logit: NaN errors rank first and poison the term and the total
    r = _fused(z2, t, 28, [1, 2], ii=255, dice=(0.0, 0.0))
    assert torch.isnan(r.terms[3]) and torch.isnan(r.terms[0])


@pytest.mark.parametrize("how", ["weight 0", "lovasz NULL"])
def test_without_the_term_the_bits_are_those_of_the_existing_calls(how):
    import test_gpu_ce_dice as TD
    z, t = _fused_case(3, 3, 7, 28, seed=8, ignore=0.2)
    off = dict(weight=0.0) if how == "weight 0" else dict(null_lov=True)
    a = _fused(z, t, 28, [1, 2], ii=255, w=[0.5, 2.0, 1.0], eps=0.1, dice=(1.0, 0.5), loss_scale=0.5, want_planes=False, **off)
    terms, grad = TD._run(z, t, 28, dice_weight=0.5, ce_weight=1.0, ignore_index=255, class_weight=[0.5, 2.0, 1.0],
                          label_smoothing=0.1, loss_scale=0.5)
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
    need = int(_sym("vitseg_lovasz_scratch_bytes")(B, 2, S))
    cscr = guarded(need, torch.uint8, "nan", name="lovasz scratch")
    planes = guarded((2, B, S, S), torch.float32, "nan", name="prob_planes")
    gplanes = guarded((2, B, S, S), torch.float32, "nan", name="grad_planes")
    fn = _sym("vitseg_ce_lovasz_loss")
    ok = dict(weight=0.5, classes=[1, 2], per_image=0, present=1, scr=cscr.data_ptr(), n=need)

    def call(lowres=zd.data_ptr(), terms_ptr=terms.data_ptr(), **kw):
        o = dict(ok, **kw)
        cls = o["classes"]
        arr = (C.c_int32 * max(len(cls), 1))(*cls)
        c = _ext.CLovaszOptions(o["weight"], len(cls), arr, o["per_image"], o["present"], o["scr"], o["n"], planes.data_ptr(),
                                gplanes.data_ptr(), None)
        return fn(lowres, td.data_ptr(), 1, gd.data_ptr(), scr.data_ptr(), terms_ptr, B, C_, g, S, None, None, C.byref(c), 1.0, _stream())
    nan, inf = float("nan"), float("inf")
    for kw in (dict(weight=-0.5), dict(weight=nan), dict(weight=inf), dict(classes=[]), dict(classes=[1, 1]), dict(classes=[3]),
               dict(classes=[0, 1, 2, 1]), dict(per_image=2), dict(present=-1), dict(scr=None), dict(scr=cscr.data_ptr() + 4),
               dict(n=need - 1), dict(lowres=None), dict(terms_ptr=None)):
        assert call(**kw) == _lib.EINVAL, kw
    # the planes call
    pl = _sym("vitseg_lovasz_planes")
    pneed = int(_sym("vitseg_lovasz_planes_scratch_bytes")(2, B * S * S))
    assert pneed <= need
    for args in ((None, td.data_ptr(), 2, 100), (planes.data_ptr(), None, 2, 100), (planes.data_ptr(), td.data_ptr(), 0, 100),
                 (planes.data_ptr(), td.data_ptr(), 2, 0), (planes.data_ptr(), td.data_ptr(), 2, 1 << 30)):
        assert pl(*args, 1.0, cscr.data_ptr(), terms.data_ptr(), gplanes.data_ptr(), None, _stream()) == _lib.EINVAL, args
    assert pl(planes.data_ptr(), td.data_ptr(), 2, 100, 1.0, cscr.data_ptr() + 4, terms.data_ptr(), None, None, _stream()) == _lib.EINVAL
    assert pl(planes.data_ptr(), td.data_ptr(), 2, 100, nan, cscr.data_ptr(), terms.data_ptr(), None, None, _stream()) == _lib.EINVAL
    torch.cuda.synchronize()
    check(gd, terms, scr, cscr, planes, gplanes)
    assert torch.isnan(gd).all() and torch.isnan(terms).all() and torch.isnan(planes).all() and torch.isnan(gplanes).all()
    assert (cscr == 255).all() and (scr == 255).all()   # the poison: not a byte was written
    assert call() == _lib.OK   # and the valid call goes through
    torch.cuda.synchronize()
    check(gd, terms, scr, cscr, planes, gplanes)
    assert torch.isfinite(terms).all() and torch.isfinite(gd).all() and torch.isfinite(planes).all() and torch.isfinite(gplanes).all()


# ------------------------------------------------------------------ 3. the whole path
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ce_lovasz_loss_is_the_standalone_call_fed_through_backward(precision):
    """model.ce_lovasz_loss(...).backward() against vitseg_ce_lovasz_loss run standalone on the training forward's full-size
    logits (g == S: the taps are the identity, so it reads the bits the fused loss regenerates) and its gradient fed through
    vitseg_backward's grad_logits entry: the same arena gradient and the same terms, bit for bit."""
    m = _small_model(precision=precision)
    S, B, C_ = 64, 2, 3
    x = torch.from_numpy(synth.make_images(m.cfg, B, seed=4)).to(DEV)
    y = _batch().to(DEV)
    kw = dict(lovasz_weight=0.5, lovasz_classes=[1, 2], lovasz_per_image=True, dice_weight=0.25, ignore_index=255,
              class_weight=[0.5, 2.0, 1.0])
    m.zero_grad(set_to_none=True)
    loss, ce, dice, lov = m.ce_lovasz_loss(x, y, return_terms=True, **kw)
    loss.backward()
    torch.cuda.synchronize()
    g1 = m.arena.grad.detach().clone()
    assert torch.isfinite(loss) and torch.isfinite(g1).all() and float(g1.abs().max()) > 0 and 0 < float(lov) < 1
    assert not ce.requires_grad and not lov.requires_grad
    assert abs(float(loss.detach()) - (float(ce) + 0.25 * float(dice) + 0.5 * float(lov))) <= 1e-6 * abs(float(loss.detach()))

    logits = m._forward_train(x, True)
    gd = guarded((B, C_, S, S), torch.float32, "nan", name="grad_logits")
    scr = torch.empty(_lib.lib().vitseg_ce_scratch_bytes(B, S), dtype=torch.uint8, device=DEV)
    oscr = torch.empty(int(_lib.ce_opts_symbol("vitseg_ce_options_scratch_bytes")(B, S)), dtype=torch.uint8, device=DEV)
    dscr = torch.empty(int(_lib.dice_symbol("vitseg_dice_options_scratch_bytes")(B, C_, S)), dtype=torch.uint8, device=DEV)
    cscr = torch.empty(int(_sym("vitseg_lovasz_scratch_bytes")(B, 2, S)), dtype=torch.uint8, device=DEV)
    wd = torch.tensor([0.5, 2.0, 1.0], device=DEV)
    o = _lib.CCEOptions(1, 0, 255, wd.data_ptr(), 0.0, oscr.data_ptr(), oscr.numel())
    d = _lib.CDiceOptions(1.0, 0.25, 1e-6, 1, dscr.data_ptr(), dscr.numel())
    arr = (C.c_int32 * 2)(1, 2)
    c = _ext.CLovaszOptions(0.5, 2, arr, 1, 1, cscr.data_ptr(), cscr.numel(), None, None, None)
    terms2 = torch.empty(4, dtype=torch.float32, device=DEV)
    _lib.check(_sym("vitseg_ce_lovasz_loss")(logits.data_ptr(), y.data_ptr(), 1, gd.data_ptr(), scr.data_ptr(), terms2.data_ptr(), B, C_,
                                             S, S, C.byref(o), C.byref(d), C.byref(c), 1.0, _stream()))
    torch.cuda.synchronize()
    check(gd)
    assert torch.equal(_bits(terms2), _bits(torch.stack([loss.detach(), ce, dice, lov])))
    g2, _ = m._backward(x, grad_logits=gd)
    torch.cuda.synchronize()
    assert torch.equal(_bits(g2), _bits(g1))
    m._release_grad_buffer(g2)
    # grad_scale scales the deposit and leaves the loss alone; the no-grad path forms the same terms from the inference forward
    m.zero_grad(set_to_none=True)
    loss4 = m.ce_lovasz_loss(x, y, grad_scale=0.25, **kw)
    loss4.backward()
    torch.cuda.synchronize()
    assert torch.equal(_bits(loss4.detach().reshape(1)), _bits(loss.detach().reshape(1)))
    scaled = m.arena.grad.detach()
    assert float((scaled - 0.25 * g1).abs().max()) <= 1e-5 * float(g1.abs().max())   # the scale enters coef before its roundings
    with torch.no_grad():
        t_ng = m.ce_lovasz_loss(x, y, return_terms=True, **kw)
    # the inference forward is another chain of GEMMs than the training forward: fp32 sums in another order (a few 1e-6 of a
    # logit), 16-bit operands on the bf16 route (2^-8 per product)
    tol = 1e-4 if precision == "fp32" else 2e-2
    for a, b in zip(t_ng, (loss.detach(), ce, dice, lov)):
        assert abs(float(a) - float(b)) <= tol * abs(float(b))
    m.zero_grad(set_to_none=True)
    # the defaults: every class, no Dice term, pooled; the term alone
    with torch.no_grad():
        la = m.ce_lovasz_loss(x, y, ignore_index=255, return_terms=True)
        lb = m.ce_lovasz_loss(x, y, ignore_index=255, lovasz_classes=[0, 1, 2], dice_weight=0.0, return_terms=True)
        lc = m.ce_lovasz_loss(x, y, ignore_index=255, ce_weight=0.0, lovasz_weight=1.0, return_terms=True)
        with pytest.raises(ValueError):
            m.ce_lovasz_loss(x, y, lovasz_classes=[3])
    assert torch.equal(_bits(torch.stack(la)), _bits(torch.stack(lb))) and float(la[2]) == 0.0
    assert torch.equal(_bits(lc[0].reshape(1)), _bits(lc[3].reshape(1))) and float(lc[1]) == 0.0
    m.zero_grad(set_to_none=True)


def test_backward_lovasz_argument_errors_and_its_null_form():
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
    need = int(_sym("vitseg_lovasz_scratch_bytes")(1, 2, S))
    cscr = guarded(need, torch.uint8, "nan", name="lovasz scratch")
    dbytes = int(_lib.dice_symbol("vitseg_dice_options_scratch_bytes")(1, 3, S))
    dscr = guarded(dbytes, torch.uint8, "nan", name="dice scratch")
    cfg = C.byref(_lib.CConfig.from_config(m.cfg))
    fn = _sym("vitseg_backward_lovasz")
    arr = (C.c_int32 * 2)(1, 2)
    bad = (C.c_int32 * 2)(1, 3)

    def call(c, d=None, target=t, grad_logits=None, terms_ptr=terms.data_ptr()):
        return fn(cfg, S, m.arena.data_ptr(), None, x.data_ptr(), 1, m.precision, 0.0, 0, _ptr(target), 1, _ptr(grad_logits),
                  grads.data_ptr(), loss.data_ptr(), 1.0, None, ws.data_ptr(), ws.numel(), _stream(), None,
                  C.byref(d) if d is not None else None, C.byref(c) if c is not None else None, terms_ptr)
    O_ = lambda w=0.5, cl=arr, pi=0, scr=cscr.data_ptr(), n=need: _ext.CLovaszOptions(w, 2, cl, pi, 1, scr, n, None, None, None)
    assert call(O_(), target=None, grad_logits=gl) == _lib.EINVAL
    assert call(O_(), terms_ptr=None) == _lib.EINVAL
    for c in (O_(w=-1.0), O_(cl=bad), O_(pi=3), O_(scr=None), O_(scr=cscr.data_ptr() + 4), O_(n=need - 1)):
        assert call(c) == _lib.EINVAL
    torch.cuda.synchronize()
    check(grads, loss, terms, cscr, dscr)
    assert torch.isnan(grads).all() and torch.isnan(loss).all() and torch.isnan(terms).all() and (cscr == 255).all()
    assert call(O_()) == _lib.OK
    torch.cuda.synchronize()
    check(grads, loss, terms, cscr, dscr)
    assert torch.isfinite(grads).all() and torch.isfinite(terms).all() and torch.equal(_bits(loss), _bits(terms[0:1]))
    assert float(terms[2]) == 0.0 and 0 < float(terms[3]) < 1
    # lovasz == NULL with the Dice options: vitseg_backward_dice's bits, and terms[3] = 0
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
                           lovasz_weight=0.5, lovasz_per_image=True)
    lm.model.load_state_dict(m0.state_dict())
    lm.eval()
    x = torch.from_numpy(synth.make_images(c, 2, seed=4)).to(DEV)
    y = _batch().to(DEV)
    lt = lm.training_step((x, y), 0)
    lt.backward()
    lv = lm.validation_step((x, y), 0)
    torch.cuda.synchronize()
    assert {"train_loss", "train_ce", "train_dice", "train_lovasz", "valid_loss", "valid_ce", "valid_dice", "valid_lovasz"} <= set(lm.logged)
    assert lm.logged["train_lovasz"].is_cuda and 0 < float(lm.logged["valid_lovasz"]) < 1 and float(lm.logged["valid_dice"]) == 0.0
    assert torch.isfinite(lt) and torch.isfinite(lm.model.arena.grad).all()
    with torch.no_grad():
        want = lm.model.ce_lovasz_loss(x, y, ignore_index=255, lovasz_weight=0.5, lovasz_per_image=True)
    assert torch.equal(_bits(lv.reshape(1)), _bits(want.reshape(1)))
