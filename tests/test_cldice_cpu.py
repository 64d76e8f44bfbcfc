"""CPU (-m "not gpu"): the two restatements of the soft-clDice loss (tests/cldice_ref.py) against each other, planes answered
by hand, the quantised plane on which ties are everywhere, the sensitivity of the gradient to each tie rule, the family header
against `_ext.EXT_LATER`, the status codes of the C entry points, the host-side option checks, the script flags and the
Lightning module.  No compute entry point runs; the argument checks of the C entry points do."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cldice_ref as R
from test_binding_cpu import STRUCTS, parse_header, signature_errors, struct_errors
from visiontransformer_amd import _ext, _lib, cldice, scripts
from visiontransformer_amd.lightning import LightningViTModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vitseg_cldice.h")
NAMES = ["vitseg_cldice_version", "vitseg_soft_skeleton_scratch_bytes", "vitseg_soft_skeleton", "vitseg_soft_cldice_scratch_bytes",
         "vitseg_soft_cldice", "vitseg_cldice_scratch_bytes", "vitseg_ce_cldice_loss", "vitseg_backward_cldice"]


def _case(kind, n=2, H=33, W=70, seed=1, void=0.2):
    t = R.line_target(n, H, W, seed)
    return R.make_plane(kind, n, H, W, t, seed + 1), t, R.void_mask(n, H, W, void, seed + 2)


# ---- (b) against (a) ----

@pytest.mark.parametrize("kind", ["smooth", "eighths", "binary", "clamped"])
@pytest.mark.parametrize("iters", [0, 1, 3, 10])
@pytest.mark.parametrize("shape", [(2, 33, 70), (1, 1, 9), (1, 9, 1)])
def test_explicit_adjoint_is_autograd_of_the_published_composition(kind, iters, shape):
    p, t, void = _case(kind, *shape)
    terms_a, g_a = R.cldice_autograd(p, t.float(), void, iters, 1.0, torch.float64)
    terms_b, g_b = R.cldice_explicit(p.numpy(), t.numpy(), void.numpy(), iters, 1.0)
    for a, b in zip(terms_a, terms_b):
        assert abs(a - b) <= 1e-14 * abs(a)
    gmax = g_a.abs().max().item()
    assert gmax > 0 and np.abs(g_b - g_a.numpy()).max() <= 1e-13 * gmax
    assert (g_b[void.numpy()] == 0).all()
    sk_a = R.soft_skel(p.double(), iters).numpy()
    sk_b, _ = R.skel_forward_np(p.double().numpy(), iters)
    assert np.array_equal(sk_a, sk_b)


# ---- answered by hand ----

def test_planes_answered_by_hand():
    band = torch.zeros(1, 5, 5)
    band[0, 1:4, :] = 1.0                      # three rows thick
    line = torch.zeros(1, 5, 5)
    line[0, 2, :] = 1.0                        # its centre line
    # a line one pixel thick erodes to nothing: it is its own skeleton at every iters
    for it in (0, 1, 3):
        assert torch.equal(R.soft_skel(line, it), line)
    # the band: open(band) = band, so skel_0 = 0; one erosion leaves the centre line, which the next round adds
    assert torch.equal(R.soft_skel(band, 0), torch.zeros(1, 5, 5))
    assert torch.equal(R.soft_skel(band, 1), line) and torch.equal(R.soft_skel(band, 4), line)
    none = torch.zeros(1, 5, 5, dtype=torch.bool)
    # prediction = the centre line, truth = the band: both skeletons are the line, tprec = tsens = 1
    cl, tp, ts = R.cldice_terms(line.double(), band.double(), none, 1, 1.0)
    assert (float(cl), float(tp), float(ts)) == (0.0, 1.0, 1.0)
    # a line one row off: no skeleton pixel meets the other plane; tprec = tsens = (0 + 1) / (5 + 1), cl = 1 - 1/6
    off = torch.zeros(1, 5, 5)
    off[0, 1, :] = 1.0
    cl, tp, ts = R.cldice_terms(off.double(), line.double(), none, 1, 1.0)
    assert abs(float(tp) - 1 / 6) < 1e-15 and abs(float(ts) - 1 / 6) < 1e-15 and abs(float(cl) - 5 / 6) < 1e-15
    # everything void: both sums are the smoothing alone, cl = 0 and no gradient
    (cl, tp, ts), g = R.cldice_explicit(off.numpy(), line.numpy(), np.ones((1, 5, 5), dtype=bool), 1, 1.0)
    assert (cl, tp, ts) == (0.0, 1.0, 1.0) and (g == 0).all()
    # 1 x 3, iters = 0, p flat: p - open(p) = 0 and relu'(0) = 0, so only the direct term gamma st is left.
    # st = y = [0, 1, 0]; tprec = 1 / 1; tsens = (0.5 + 1) / (1 + 1) = 3/4; cl = 1 - 2 (3/4) / (7/4) = 1/7;
    # d cl / d tsens = -2 / (7/4)^2 = -32/49, gamma = that / (sum st + 1) = -16/49
    p = np.full((1, 1, 3), 0.5)
    y = np.array([[[0.0, 1.0, 0.0]]])
    for fn in (lambda: R.cldice_explicit(p, y, np.zeros((1, 1, 3), dtype=bool), 0, 1.0),
               lambda: R.cldice_autograd(torch.from_numpy(p), torch.from_numpy(y), torch.zeros(1, 1, 3, dtype=torch.bool), 0, 1.0,
                                         torch.float64)):
        (cl, tp, ts), g = fn()
        assert abs(cl - 1 / 7) < 1e-15 and tp == 1.0 and ts == 0.75
        assert np.abs(np.asarray(g).reshape(3) - np.array([0.0, -16 / 49, 0.0])).max() < 1e-15


# ---- ties ----

def test_quantised_plane_fp32_is_fp64_and_carries_gradient():
    p, t, void = _case("eighths", 3, 96, 96, void=0.0)
    assert torch.equal(p * 8, torch.round(p * 8))
    for it in (0, 1, 3, 10):
        assert torch.equal(R.soft_skel(p, it).double(), R.soft_skel(p.double(), it))   # bit for bit
    _, g = R.cldice_autograd(p, t.float(), void, 3, 1.0, torch.float64)
    assert int((g != 0).sum()) > 5000
    # ties: many neighbours share a value
    assert int((p[:, :, 1:] == p[:, :, :-1]).sum()) > 5000


@pytest.mark.parametrize("wrong", [dict(pool_rule="last"), dict(min_rule="col")])
def test_each_tie_rule_moves_the_gradient_beyond_the_gpu_bound(wrong):
    """The GPU test allows 16 d_ref, d_ref = max |g_fp32 - g_fp64| of restatement (a).  A wrong rule must move the gradient on
    the quantised plane by far more, or that test would prove nothing about ties."""
    p, t, void = _case("eighths", 3, 96, 96)
    _, g32 = R.cldice_autograd(p, t.float(), void, 3, 1.0, torch.float32)
    _, g64 = R.cldice_autograd(p, t.float(), void, 3, 1.0, torch.float64)
    d_ref = (g32.double() - g64).abs().max().item()
    _, g_right = R.cldice_explicit(p.numpy(), t.numpy(), void.numpy(), 3, 1.0)
    _, g_wrong = R.cldice_explicit(p.numpy(), t.numpy(), void.numpy(), 3, 1.0, **wrong)
    moved = np.abs(g_wrong - g_right).max()
    print(f"{wrong}: d_ref = {d_ref:.2e}, bound = {16 * d_ref:.2e}, the wrong rule moves the gradient by {moved:.2e}")
    assert 0 < d_ref < 1e-7 and moved > 1000 * 16 * d_ref
    assert int((np.abs(g_wrong - g_right) > 16 * d_ref).sum()) > 100


# ---- the family header and its table ----

def _table():
    return {name: (restype, list(argtypes)) for name, restype, argtypes in _ext.EXT_LATER["cldice"][2]}


def test_family_header_is_the_table_both_ways():
    decls, structs, enums, defines = parse_header(open(HEADER).read())
    assert _ext.EXT_LATER["cldice"][:2] == ("vitseg_cldice.h", "the soft-clDice loss")
    assert sorted(decls) == sorted(NAMES) == sorted(_table()) and not enums
    known = dict(STRUCTS, vitseg_cldice_options=_ext.CClDiceOptions)
    assert signature_errors(decls, _table(), known) == []
    assert list(structs) == ["vitseg_cldice_options"] and struct_errors(structs["vitseg_cldice_options"], _ext.CClDiceOptions) == []
    assert defines == {"VITSEG_CLDICE_VERSION": 100, "VITSEG_CLDICE_MAX_ITERS": 64}
    assert _ext.CLDICE_VERSION == 100 and _ext.EXT_VERSIONS["cldice"] == ("vitseg_cldice_version", 100)
    assert cldice.MAX_ITERS == 64
    # vitseg_backward_cldice: the argument list of vitseg_backward_dice with cld in front of terms
    dice = list(_lib.symbol("vitseg_backward_dice").argtypes)
    assert _table()["vitseg_backward_cldice"][1] == dice[:-1] + [_ext.pcld, dice[-1]]
    tab = _table()
    tab["vitseg_soft_cldice"] = (C.c_int, tab["vitseg_soft_cldice"][1][:6] + [C.c_double] + tab["vitseg_soft_cldice"][1][7:])
    assert signature_errors(decls, tab, known) == ["vitseg_soft_cldice: argument 6: c_double for float"]   # it can fail
    assert not set(NAMES) & set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "vitseg.h")).read()
    assert "vitseg_soft_" not in hdr and "vitseg_cldice" not in hdr and "vitseg_ce_cldice" not in hdr and '#include "vitseg.h"' in open(HEADER).read()
    f = _ext.CClDiceOptions   # the layout on a 64-bit target
    assert [(n, getattr(f, n).offset) for n, _ in f._fields_] == [
        ("weight", 0), ("smooth", 4), ("iters", 8), ("K", 12), ("classes", 16), ("scratch", 24), ("scratch_bytes", 32),
        ("prob_planes", 40), ("class_terms", 48)]
    assert C.sizeof(f) == 56


def test_library_exports_the_family_at_its_version():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert _ext.ext_symbol("cldice", name) is getattr(_lib.lib(), name)
    assert _ext.ext_symbol("cldice", "vitseg_cldice_version")() == 100
    up = lambda v: (v + 255) // 256 * 256
    q3 = _ext.ext_symbol("cldice", "vitseg_soft_skeleton_scratch_bytes")
    assert q3(2, 33, 70) == 3 * up(4 * 2 * 33 * 70) and q3(0, 5, 5) == 0 and q3(1, 0, 5) == 0 and q3(8, 16384, 16384) == 0
    # header 256 | 4 K coefficients | 4 K totals | 4 n image sums | 4 n blocks partials | the choice codes, 2 B a pixel |
    # 2 iters + 12 planes
    q = _ext.ext_symbol("cldice", "vitseg_cldice_scratch_bytes")
    for B, K, S, it in ((3, 1, 28, 3), (2, 16, 40, 10), (32, 4, 512, 0)):
        n, nblk = K * B, (S * S + 1023) // 1024
        assert q(B, K, S, it) == 256 + up(16 * K) + up(32 * K) + up(32 * n) + up(32 * n * nblk) + up(2 * n * S * S) + (2 * it + 12) * up(4 * n * S * S)
    assert q(0, 1, 28, 3) == 0 and q(2, 0, 28, 3) == 0 and q(2, 1, 28, 65) == 0 and q(2, 1, 28, -1) == 0 and q(8, 1, 16384, 3) == 0
    qp = _ext.ext_symbol("cldice", "vitseg_soft_cldice_scratch_bytes")
    assert qp(3, 28, 28, 3) == q(3, 1, 28, 3) and qp(2, 33, 70, 65) == 0
    with pytest.raises(RuntimeError, match=r"has no vitseg_cldice_nothing \(built before the soft-clDice loss\)"):
        _ext.ext_symbol("cldice", "vitseg_cldice_nothing")


def _live_buffer():
    if torch.cuda.is_available():
        buf = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda")
        return buf, buf.data_ptr()
    buf = C.create_string_buffer(1 << 22)
    a = C.addressof(buf)
    return buf, a + (-a % 16)


def test_argument_errors_come_back_before_any_launch():
    """EINVAL from the checks in front of the launches; every address is a live buffer no call reaches."""
    buf, a = _live_buffer()
    EINVAL = _lib.EINVAL
    nan, inf = float("nan"), float("inf")
    sk = _ext.ext_symbol("cldice", "vitseg_soft_skeleton")
    assert sk(None, 1, 5, 5, 3, a, a, None) == EINVAL and sk(a, 1, 5, 5, 3, None, a, None) == EINVAL
    assert sk(a, 1, 5, 5, 3, a, None, None) == EINVAL and sk(a, 1, 5, 5, 3, a, a + 4, None) == EINVAL
    for n, H, W, it in ((0, 5, 5, 3), (1, 0, 5, 3), (1, 5, 0, 3), (8, 16384, 16384, 3), (1, 5, 5, -1), (1, 5, 5, 65)):
        assert sk(a, n, H, W, it, a, a, None) == EINVAL, (n, H, W, it)
    pl = _ext.ext_symbol("cldice", "vitseg_soft_cldice")
    ok = dict(prob=a, truth=a, n=1, H=5, W=5, iters=3, smooth=1.0, scratch=a, terms=a)

    def plane(**kw):
        o = dict(ok, **kw)
        return pl(o["prob"], o["truth"], o["n"], o["H"], o["W"], o["iters"], o["smooth"], 1.0, o["scratch"], o["terms"], None, None)
    for kw in (dict(prob=None), dict(truth=None), dict(scratch=None), dict(terms=None), dict(scratch=a + 4), dict(n=0), dict(H=0),
               dict(W=-1), dict(n=8, H=16384, W=16384), dict(iters=-1), dict(iters=65), dict(smooth=0.0), dict(smooth=-1.0),
               dict(smooth=nan), dict(smooth=inf)):
        assert plane(**kw) == EINVAL, kw
        assert b"soft_cldice" in _lib.lib().vitseg_last_error()
    fn = _ext.ext_symbol("cldice", "vitseg_ce_cldice_loss")
    need = int(_ext.ext_symbol("cldice", "vitseg_cldice_scratch_bytes")(2, 2, 28, 3))
    assert 0 < need <= 1 << 21
    okc = dict(weight=0.5, smooth=1.0, iters=3, classes=[1, 3], scr=a, n=need)

    def call(C_=5, lowres=a, target=a, terms=a, scratch=a, ce=None, dice=None, null_cld=False, **kw):
        o = dict(okc, **kw)
        cls = o["classes"]
        arr = (C.c_int32 * max(len(cls), 1))(*cls) if cls is not None else None
        c = _ext.CClDiceOptions(o["weight"], o["smooth"], o["iters"], o.get("K", len(cls) if cls is not None else 1), arr, o["scr"], o["n"],
                                None, None)
        return fn(lowres, target, 1, None, scratch, terms, 2, C_, 7, 28, ce, dice, None if null_cld else C.byref(c), 1.0, None)
    for kw in (dict(weight=-1.0), dict(weight=nan), dict(weight=inf), dict(smooth=0.0), dict(smooth=-1.0), dict(smooth=nan),
               dict(smooth=inf), dict(iters=-1), dict(iters=65), dict(classes=[]), dict(classes=[0, 1, 2, 3, 4, 0], K=6),
               dict(classes=None), dict(classes=[1, 1]), dict(classes=[5]), dict(classes=[-1]), dict(scr=None), dict(scr=a + 4),
               dict(n=need - 1), dict(n=0)):
        assert call(**kw) == EINVAL, kw
        assert b"cldice options" in _lib.lib().vitseg_last_error(), kw
    assert call(C_=256) == EINVAL and call(C_=0) == EINVAL
    for kw in (dict(lowres=None), dict(target=None), dict(terms=None), dict(scratch=None)):
        assert call(**kw) == EINVAL, kw
    # the errors of vitseg_ce_dice_loss and vitseg_ce_loss_opts
    dneed = int(_lib.symbol("vitseg_dice_options_scratch_bytes")(2, 5, 28))
    for bad in (_lib.CDiceOptions(1.0, -1.0, 1e-6, 1, a, dneed), _lib.CDiceOptions(1.0, 1.0, 1e-6, 1, None, dneed),
                _lib.CDiceOptions(1.0, 1.0, 1e-6, 1, a, dneed - 1)):
        assert call(dice=C.byref(bad)) == EINVAL
    both0 = _lib.CDiceOptions(0.0, 0.0, 1e-6, 1, a, dneed)
    assert call(dice=C.byref(both0), weight=0.0) == EINVAL   # nothing left to form (with the term on, both may be 0)
    for bad_ce in (_lib.CCEOptions(0, 0, 0, None, 0.0, None, 1 << 19), _lib.CCEOptions(0, 0, 0, None, 0.0, a, 8),
                   _lib.CCEOptions(0, 0, 0, None, 1.5, a, 1 << 19)):
        assert call(ce=C.byref(bad_ce)) == EINVAL


# ---- Python: the option checks, the flags, the modules ----

def test_check_options_takes_and_refuses_what_the_header_lists():
    assert cldice.check_options(5) == (0.5, [1, 2, 3, 4], 3, 1.0)
    assert cldice.check_options(2, 1, None, 0, 0.5) == (1.0, [1], 0, 0.5)
    assert cldice.check_options(5, 0.0, (3, 0), 64, 1e-3) == (0.0, [3, 0], 64, 1e-3)
    for kw in (dict(weight=-1), dict(weight=float("nan")), dict(weight=float("inf")), dict(weight="x"), dict(classes=[]),
               dict(classes=[1, 1]), dict(classes=[5]), dict(classes=[-1]), dict(classes=[0, 1, 2, 3, 4, 5]), dict(iters=-1),
               dict(iters=65), dict(iters=3.0), dict(iters=True), dict(smooth=0), dict(smooth=-1.0), dict(smooth=float("nan")),
               dict(smooth=float("inf"))):
        with pytest.raises(ValueError):
            cldice.check_options(5, **kw)
    with pytest.raises(ValueError, match="at least two classes"):
        cldice.check_options(1)


def test_module_refuses_host_planes_and_bad_arguments():
    p = torch.rand(2, 8, 8)
    with pytest.raises(ValueError, match="on the GPU"):
        cldice.soft_skeleton(p)
    with pytest.raises(ValueError, match="on the GPU"):
        cldice.soft_cldice_loss(p, torch.zeros(2, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="iters"):
        cldice.soft_skeleton(p, iters=65)
    with pytest.raises(ValueError, match="smooth"):
        cldice.soft_cldice_loss(p, torch.zeros(2, 8, 8, dtype=torch.uint8), smooth=0.0)


def test_scripts_map_the_flags():
    ap = argparse.ArgumentParser()
    scripts.add_ce_loss_arguments(ap)
    assert scripts.ce_loss_options(ap.parse_args([])) == {}
    a = ap.parse_args(["--cldice-weight", "0.5"])
    assert scripts.ce_loss_options(a) == dict(cldice_weight=0.5, cldice_iters=3, cldice_smooth=1.0)
    a = ap.parse_args(["--cldice-weight", "0.3", "--cldice-classes", "1,3", "--cldice-iters", "10", "--cldice-smooth", "0.5",
                       "--ignore-index", "255", "--dice-weight", "0.5"])
    assert scripts.ce_loss_options(a) == dict(ignore_index=255, dice_weight=0.5, dice_smooth=1e-6, dice_include_background=True,
                                              cldice_weight=0.3, cldice_classes=[1, 3], cldice_iters=10, cldice_smooth=0.5)
    assert scripts.ce_loss_options(ap.parse_args(["--cldice-iters", "5"])) == {}   # without a weight the term is off
    with pytest.raises(ValueError, match="--cldice-classes"):
        scripts.ce_loss_options(ap.parse_args(["--cldice-weight", "0.5", "--cldice-classes", "1;2"]))
    for script in ("createViTmodel.py", "trainCurrentViTmodel.py"):   # both training scripts take the flags from there
        src = open(os.path.join(ROOT, "model", "CE", script)).read()
        assert "scripts.add_ce_loss_arguments(ap)" in src and "**scripts.ce_loss_options(a)" in src


def test_lightning_module_takes_and_refuses_the_options(monkeypatch):
    mk = lambda **kw: LightningViTModel(5, 16, 64, 1, 1, image_size=32, intermediate_size=128, **kw)
    for hard in (dict(focal_gamma=2.0), dict(ohem_thresh=0.7), dict(ohem_min_kept=10), dict(ohem_keep_fraction=0.25)):
        with pytest.raises(ValueError, match="cldice_weight"):
            mk(cldice_weight=0.5, **hard)
    for kw in (dict(cldice_weight=-1.0), dict(cldice_weight=0.5, cldice_classes=[7]), dict(cldice_weight=0.5, cldice_iters=100),
               dict(cldice_weight=0.5, cldice_smooth=0.0), dict(cldice_classes=[1, 1])):
        with pytest.raises(ValueError):
            mk(**kw)
    lm = mk(ignore_index=255, cldice_weight=0.5, cldice_classes=[1, 2], cldice_iters=5, cldice_smooth=0.5, dice_weight=0.25)
    seen = []

    def fake(x, y, **kw):
        seen.append(kw)
        return torch.zeros(()), torch.ones(()), torch.full((), 2.0), torch.full((), 3.0)
    monkeypatch.setattr(lm.model, "ce_cldice_loss", fake)
    batch = (torch.zeros(1, 3, 32, 32), torch.zeros(1, 32, 32, dtype=torch.long))
    lm.training_step(batch, 0)
    lm.validation_step(batch, 0)
    want = dict(cldice_weight=0.5, cldice_classes=(1, 2), cldice_iters=5, cldice_smooth=0.5, dice_weight=0.25, smooth=1e-6,
                include_background=True, grad_scale=None, interpolate_pos_encoding=False, return_terms=True, ignore_index=255,
                class_weight=None, label_smoothing=0.0)
    assert seen == [want, want]   # validation forms the term too
    assert set(lm.logged) == {"train_loss", "train_ce", "train_dice", "train_cldice", "valid_loss", "valid_ce", "valid_dice",
                              "valid_cldice"}
    assert float(lm.logged["train_cldice"]) == 3.0 and float(lm.logged["valid_ce"]) == 1.0
    # at the default the steps pass what they passed before
    lm = mk(ignore_index=255)
    seen.clear()

    def fake_ce(x, y, **kw):
        seen.append(kw)
        return torch.zeros(())
    monkeypatch.setattr(lm.model, "ce_loss", fake_ce)
    lm.training_step(batch, 0)
    assert seen == [dict(grad_scale=None, ignore_index=255, class_weight=None, label_smoothing=0.0)]
    assert set(lm.logged) == {"train_loss"}
