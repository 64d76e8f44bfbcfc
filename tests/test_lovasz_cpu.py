"""CPU (-m "not gpu"): the two restatements of the Lovasz-Softmax loss (tests/lovasz_ref.py) against each other, planes answered
by hand, the family header against `_ext.EXT_LATER`, the status codes of the C entry points, the host-side option checks, the
script flags and the Lightning module.  No compute entry point runs; the argument checks of the C entry points do.

The planes of (b) against (a) lie on a 2^-16 grid, so that 1 - p is exact in fp32 and (a) in fp64 sees the very errors (b)
sorts: the two then agree on every tie, and the comparison holds to 1e-12."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lovasz_ref as R
from test_binding_cpu import STRUCTS, parse_header, signature_errors, struct_errors
from visiontransformer_amd import _ext, _lib, lovasz, scripts
from visiontransformer_amd.lightning import LightningViTModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vitseg_lovasz.h")
NAMES = ["vitseg_lovasz_version", "vitseg_lovasz_planes_scratch_bytes", "vitseg_lovasz_planes", "vitseg_lovasz_scratch_bytes",
         "vitseg_ce_lovasz_loss", "vitseg_backward_lovasz"]


# ---- (b) against (a) ----

def _softmax_case(B, C_, H, W, seed, void):
    """Probabilities on a 2^-16 grid that sum to 1 exactly in fp64, labels with some void."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.softmax(torch.randn(B, C_, H, W, generator=gen, dtype=torch.float64) * 2.0, dim=1)
    p = torch.round(p * 65536.0) / 65536.0
    t = torch.randint(0, C_, (B, H, W), generator=gen)
    t[0][t[0] == C_ - 1] = 0   # image 0 has no pixel of the last class
    if void > 0:
        t[torch.rand(B, H, W, generator=gen) < void] = 255
    return p, t


def _term_b(p, t, classes, per_image, present, ignore=255, dtype=np.float64):
    B, C_ = p.shape[0], p.shape[1]
    p32 = p.float().numpy().reshape(B, C_, -1)
    tt = t.numpy().reshape(B, -1)
    y = np.stack([tt == c for c in classes])
    e = np.stack([R.errors32(p32[:, c], y[k]) for k, c in enumerate(classes)])
    return R.term(e, y, tt != ignore, per_image, present, dtype=dtype)


@pytest.mark.parametrize("void", [0.0, 0.3])
@pytest.mark.parametrize("present", [True, False])
@pytest.mark.parametrize("per_image", [False, True])
def test_closed_form_is_autograd_of_the_published_composition(void, present, per_image):
    p, t = _softmax_case(3, 4, 9, 11, seed=5, void=void)
    classes = [0, 1, 2, 3]
    q = p.clone().requires_grad_(True)
    want = R.lovasz_softmax(q, t, "present" if present else "all", per_image, ignore=255)
    want.backward()
    got, Lc, g = _term_b(p, t, classes, per_image, present)
    assert abs(got - float(want.detach())) <= 1e-12
    gref = q.grad.permute(1, 0, 2, 3).reshape(4, 3, -1).numpy()
    assert np.abs(g - gref).max() <= 1e-12 and np.abs(gref).max() > 1e-3
    g32 = _term_b(p, t, classes, per_image, present, dtype=np.float32)[2]   # what the device writes: one rounding of the same
    assert g32.dtype == np.float32 and np.array_equal(g32, g.astype(np.float32))
    # a list of classes, filtered as 'present' filters
    sub = [3, 1]
    want2 = R.lovasz_softmax(p, t, sub, per_image, ignore=255, present=present)
    got2, _, _ = _term_b(p, t, sub, per_image, present)
    assert abs(got2 - float(want2)) <= 1e-12
    if present and per_image:   # image 0 lacks class 3: it is left out there, so the two settings differ
        assert abs(got2 - _term_b(p, t, sub, per_image, False)[0]) > 1e-3


def test_closed_form_gradient_in_fp64_is_autograd_to_1e_12():
    gen = np.random.default_rng(3)
    L = 500
    p = np.round(gen.random(L) * 65536.0) / 65536.0
    t = gen.random(L) < 0.3
    valid = gen.random(L) > 0.2
    e = R.errors32(p.astype(np.float32), t)
    loss, g, order, G = R.closed_form(e, t, valid, coef=1.0, dtype=np.float64)
    q = torch.from_numpy(p[valid]).requires_grad_(True)
    probas = torch.stack([1 - q, q], dim=1)
    want, per = R.lovasz_softmax_flat(probas, torch.from_numpy(t[valid].astype(np.int64)), [1])
    want.backward()
    assert abs(loss - float(want.detach())) <= 1e-12 and G == int((t & valid).sum())
    assert np.abs(g[valid] - q.grad.numpy()).max() <= 1e-12
    assert (g[~valid] == 0).all() and not np.signbit(g[~valid]).any()
    assert sorted(order[:valid.sum()].tolist()) == np.flatnonzero(valid).tolist() and (order[valid.sum():] == -1).all()


# ---- planes answered by hand ----

def test_planes_answered_by_hand():
    f = np.float32
    # all errors equal: the order is the pixel order, the loss is e times the sum of dJ = e times the last Jaccard loss, 1
    y = np.array([0, 1, 0, 1, 0], dtype=bool)
    loss, g, order, G = R.closed_form(np.full(5, 0.25, f), y)
    assert order.tolist() == [0, 1, 2, 3, 4] and G == 2 and abs(loss - 0.25) <= 1e-15
    # ranks: y = 0 1 0 1 0, G = 2: (F, U) = (0,3) (1,3) (1,4) (2,4) (2,5); dJ = 2/(2*3), 1/3, 1/(3*4), 1/4, 0
    assert np.allclose(g, [1 / 3, -1 / 3, 1 / 12, -1 / 4, 0.0], rtol=1e-7) and g[4] == 0
    # G = 0: the loss is the largest error, carried by its first pixel alone
    e = np.array([0.1, 0.7, 0.3, 0.7], f)
    loss, g, order, G = R.closed_form(e, np.zeros(4, bool))
    assert G == 0 and loss == float(f(0.7)) and order.tolist() == [1, 3, 2, 0] and g.tolist() == [0.0, 1.0, 0.0, 0.0]
    # G = L: every pixel has dJ = 1 / L, the loss is the mean error
    e = np.array([0.5, 0.25, 1.0, 0.0], f)
    loss, g, order, G = R.closed_form(e, np.ones(4, bool))
    assert G == 4 and loss == 0.4375 and order.tolist() == [2, 0, 1, 3] and g.tolist() == [-0.25] * 4
    # one valid pixel: the loss is its error, whatever y is
    for yy in (False, True):
        loss, g, order, G = R.closed_form(np.array([0.9, 0.6, 0.2], f), np.array([yy] * 3), np.array([False, True, False]))
        assert loss == float(f(0.6)) and order.tolist() == [1, -1, -1] and g.tolist() == [0.0, -1.0 if yy else 1.0, 0.0]
    # nothing valid: 0
    loss, g, order, G = R.closed_form(np.array([0.9, 0.6], f), np.array([True, False]), np.zeros(2, bool))
    assert loss == 0.0 and G == 0 and order.tolist() == [-1, -1] and g.tolist() == [0.0, 0.0]
    # a NaN error ranks first and poisons the loss; -0 ranks after +0; the keys are the header's
    e = np.array([0.5, np.nan, 1.0], f)
    loss, g, order, G = R.closed_form(e, np.array([True, False, False]))
    assert np.isnan(loss) and order.tolist() == [1, 2, 0]
    assert R.sort_key(np.array([np.nan, np.inf, 1.0, 0.0, -0.0, -1.0], f)).tolist() == [
        0x003FFFFF, 0x007FFFFF, 0x407FFFFF, 0x7FFFFFFF, 0x80000000, 0xBF800000]
    assert R.sort_key(np.array([-np.nan], f)).tolist() == [0x003FFFFF]   # no error has the void key


def test_term_counts_present_classes_per_segment():
    f = np.float32
    e = np.array([[[0.5, 0.25], [0.75, 0.5]], [[0.125, 0.5], [0.25, 0.25]]], f)   # K = 2, B = 2, P = 2
    y = np.array([[[1, 0], [0, 0]], [[0, 0], [0, 0]]], bool)                        # class 1 nowhere, class 0 in image 0
    valid = np.ones((2, 2), bool)
    t_all, Lc, _ = R.term(e, y, valid, False, False)
    t_pres, Lc2, g = R.term(e, y, valid, False, True)
    assert np.array_equal(Lc, Lc2) and abs(t_all - (Lc[0] + Lc[1]) / 2) <= 1e-15 and t_pres == Lc[0]
    assert Lc[1] == 0.5 and (g[1] == 0).all() and not np.signbit(g[1]).any() and (g[0] != 0).any()
    t_img, Lci, gi = R.term(e, y, valid, True, True)
    assert Lci.shape == (2, 2) and abs(t_img - (Lci[0, 0] + 0.0) / 2) <= 1e-15 and (gi[:, 1] == 0).all()   # image 1: K' = 0
    t_img_all, _, _ = R.term(e, y, valid, True, False)
    assert abs(t_img_all - ((Lci[0, 0] + Lci[1, 0]) / 2 + (Lci[0, 1] + Lci[1, 1]) / 2) / 2) <= 1e-15


# ---- the family header and its table ----

def _table():
    return {name: (restype, list(argtypes)) for name, restype, argtypes in _ext.EXT_LATER["lovasz"][2]}


def test_family_header_is_the_table_both_ways():
    decls, structs, enums, defines = parse_header(open(HEADER).read())
    assert _ext.EXT_LATER["lovasz"][:2] == ("vitseg_lovasz.h", "the Lovasz-Softmax loss")
    assert sorted(decls) == sorted(NAMES) == sorted(_table()) and not enums
    known = dict(STRUCTS, vitseg_lovasz_options=_ext.CLovaszOptions)
    assert signature_errors(decls, _table(), known) == []
    assert list(structs) == ["vitseg_lovasz_options"] and struct_errors(structs["vitseg_lovasz_options"], _ext.CLovaszOptions) == []
    assert defines == {"VITSEG_LOVASZ_VERSION": 100, "VITSEG_LOVASZ_TILE": 2048}
    assert _ext.LOVASZ_VERSION == 100 and _ext.EXT_VERSIONS["lovasz"] == ("vitseg_lovasz_version", 100)
    assert lovasz.TILE == 2048
    # vitseg_ce_lovasz_loss / vitseg_backward_lovasz: the argument lists of the clDice entries with the options swapped
    cld = {name: list(argtypes) for name, _, argtypes in _ext.EXT_LATER["cldice"][2]}
    swap = lambda args: [_ext.plov if a is _ext.pcld else a for a in args]
    assert _table()["vitseg_ce_lovasz_loss"][1] == swap(cld["vitseg_ce_cldice_loss"])
    assert _table()["vitseg_backward_lovasz"][1] == swap(cld["vitseg_backward_cldice"])
    tab = _table()
    tab["vitseg_lovasz_planes"] = (C.c_int, tab["vitseg_lovasz_planes"][1][:4] + [C.c_double] + tab["vitseg_lovasz_planes"][1][5:])
    assert signature_errors(decls, tab, known) == ["vitseg_lovasz_planes: argument 4: c_double for float"]   # it can fail
    assert not set(NAMES) & set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "vitseg.h")).read()
    assert "lovasz" not in hdr and '#include "vitseg.h"' in open(HEADER).read()
    f = _ext.CLovaszOptions   # the layout on a 64-bit target
    assert [(n, getattr(f, n).offset) for n, _ in f._fields_] == [
        ("weight", 0), ("K", 4), ("classes", 8), ("per_image", 16), ("present_only", 20), ("scratch", 24), ("scratch_bytes", 32),
        ("prob_planes", 40), ("grad_planes", 48), ("class_terms", 56)]
    assert C.sizeof(f) == 64


def _layout_bytes(n, L, groups):
    up = lambda v: (v + 255) // 256 * 256
    tiles = n * ((L + 2047) // 2048)
    return (256 + up(4 * n) + up(4 * n) + up(8 * n) + up(8 * n) + up(8 * groups) + up(1024 * n) + up(1024 * tiles) + up(4 * tiles)
            + up(8 * tiles) + 5 * up(4 * n * L))


def test_library_exports_the_family_at_its_version():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert _ext.ext_symbol("lovasz", name) is getattr(_lib.lib(), name)
    assert _ext.ext_symbol("lovasz", "vitseg_lovasz_version")() == 100
    qp = _ext.ext_symbol("lovasz", "vitseg_lovasz_planes_scratch_bytes")
    for n, L in ((1, 1), (3, 2049), (5, 6161)):
        assert qp(n, L) == _layout_bytes(n, L, 1)
    assert qp(0, 5) == 0 and qp(1, 0) == 0 and qp(2, 1 << 30) == 0 and qp((1 << 20) + 1, 1) == 0
    q = _ext.ext_symbol("lovasz", "vitseg_lovasz_scratch_bytes")
    for B, K, S in ((3, 1, 28), (2, 16, 40), (32, 4, 512)):   # the larger of the pooled and the per-image layout
        assert q(B, K, S) == max(_layout_bytes(K, B * S * S, 1), _layout_bytes(K * B, S * S, B))
    assert q(0, 1, 28) == 0 and q(2, 0, 28) == 0 and q(2, 1, 0) == 0 and q(8, 1, 16384) == 0
    with pytest.raises(RuntimeError, match=r"has no vitseg_lovasz_nothing \(built before the Lovasz-Softmax loss\)"):
        _ext.ext_symbol("lovasz", "vitseg_lovasz_nothing")


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
    pl = _ext.ext_symbol("lovasz", "vitseg_lovasz_planes")
    ok = dict(prob=a, truth=a, n=2, L=50, gs=1.0, scratch=a, terms=a)

    def plane(**kw):
        o = dict(ok, **kw)
        return pl(o["prob"], o["truth"], o["n"], o["L"], o["gs"], o["scratch"], o["terms"], None, None, None)
    for kw in (dict(prob=None), dict(truth=None), dict(scratch=None), dict(terms=None), dict(scratch=a + 4), dict(n=0), dict(L=0),
               dict(L=-1), dict(n=2, L=1 << 30), dict(n=(1 << 20) + 1, L=1), dict(gs=nan), dict(gs=inf), dict(gs=-inf)):
        assert plane(**kw) == EINVAL, kw
        assert b"lovasz_planes" in _lib.lib().vitseg_last_error()
    fn = _ext.ext_symbol("lovasz", "vitseg_ce_lovasz_loss")
    need = int(_ext.ext_symbol("lovasz", "vitseg_lovasz_scratch_bytes")(2, 2, 28))
    assert 0 < need <= 1 << 21
    okc = dict(weight=0.5, classes=[1, 3], per_image=0, present=1, scr=a, n=need)

    def call(C_=5, lowres=a, target=a, terms=a, scratch=a, ce=None, dice=None, null_lov=False, **kw):
        o = dict(okc, **kw)
        cls = o["classes"]
        arr = (C.c_int32 * max(len(cls), 1))(*cls) if cls is not None else None
        c = _ext.CLovaszOptions(o["weight"], o.get("K", len(cls) if cls is not None else 1), arr, o["per_image"], o["present"],
                                o["scr"], o["n"], None, None, None)
        return fn(lowres, target, 1, None, scratch, terms, 2, C_, 7, 28, ce, dice, None if null_lov else C.byref(c), 1.0, None)
    for kw in (dict(weight=-1.0), dict(weight=nan), dict(weight=inf), dict(classes=[]), dict(classes=[0, 1, 2, 3, 4, 0], K=6),
               dict(classes=None), dict(classes=[1, 1]), dict(classes=[5]), dict(classes=[-1]), dict(per_image=2), dict(per_image=-1),
               dict(present=2), dict(scr=None), dict(scr=a + 4), dict(n=need - 1), dict(n=0)):
        assert call(**kw) == EINVAL, kw
        assert b"lovasz options" in _lib.lib().vitseg_last_error(), kw
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
    assert lovasz.check_options(5) == (0.5, [0, 1, 2, 3, 4], 0, 1)
    assert lovasz.check_options(2, 1, [1], True, False) == (1.0, [1], 1, 0)
    assert lovasz.check_options(5, 0.0, (3, 0)) == (0.0, [3, 0], 0, 1)
    for kw in (dict(weight=-1), dict(weight=float("nan")), dict(weight=float("inf")), dict(weight="x"), dict(classes=[]),
               dict(classes=[1, 1]), dict(classes=[5]), dict(classes=[-1]), dict(classes=[0, 1, 2, 3, 4, 5]), dict(per_image=2),
               dict(per_image="yes"), dict(present=None)):
        with pytest.raises(ValueError):
            lovasz.check_options(5, **kw)


def test_module_refuses_host_planes_and_bad_arguments():
    p = torch.rand(2, 64)
    with pytest.raises(ValueError, match="on the GPU"):
        lovasz.lovasz_softmax_planes(p, torch.zeros(2, 64, dtype=torch.uint8))
    with pytest.raises(ValueError, match="on the GPU"):
        lovasz.sort_planes(p, torch.zeros(2, 64, dtype=torch.uint8))
    assert not hasattr(lovasz, "lovasz_grad_ref")   # host helpers only: no host restatement of the loss in the package


def test_scripts_map_the_flags():
    ap = argparse.ArgumentParser()
    scripts.add_ce_loss_arguments(ap)
    assert scripts.ce_loss_options(ap.parse_args([])) == {}
    a = ap.parse_args(["--lovasz-weight", "0.5"])
    assert scripts.ce_loss_options(a) == dict(lovasz_weight=0.5, lovasz_per_image=False)
    a = ap.parse_args(["--lovasz-weight", "0.3", "--lovasz-classes", "1,3", "--lovasz-per-image", "--ignore-index", "255",
                       "--dice-weight", "0.5"])
    assert scripts.ce_loss_options(a) == dict(ignore_index=255, dice_weight=0.5, dice_smooth=1e-6, dice_include_background=True,
                                              lovasz_weight=0.3, lovasz_classes=[1, 3], lovasz_per_image=True)
    assert scripts.ce_loss_options(ap.parse_args(["--lovasz-per-image", "--lovasz-classes", "1"])) == {}   # no weight: off
    assert scripts.ce_loss_options(ap.parse_args(["--cldice-weight", "0.5"])) == dict(cldice_weight=0.5, cldice_iters=3, cldice_smooth=1.0)
    with pytest.raises(ValueError, match="--lovasz-classes"):
        scripts.ce_loss_options(ap.parse_args(["--lovasz-weight", "0.5", "--lovasz-classes", "1;2"]))


def test_lightning_module_takes_and_refuses_the_options(monkeypatch):
    mk = lambda **kw: LightningViTModel(5, 16, 64, 1, 1, image_size=32, intermediate_size=128, **kw)
    for other in (dict(focal_gamma=2.0), dict(ohem_thresh=0.7), dict(ohem_min_kept=10), dict(ohem_keep_fraction=0.25),
                  dict(cldice_weight=0.5)):
        with pytest.raises(ValueError, match="lovasz_weight"):
            mk(lovasz_weight=0.5, **other)
    for kw in (dict(lovasz_weight=-1.0), dict(lovasz_weight=0.5, lovasz_classes=[7]), dict(lovasz_classes=[1, 1])):
        with pytest.raises(ValueError):
            mk(**kw)
    lm = mk(ignore_index=255, lovasz_weight=0.5, lovasz_classes=[1, 2], lovasz_per_image=True, dice_weight=0.25)
    seen = []

    def fake(x, y, **kw):
        seen.append(kw)
        return torch.zeros(()), torch.ones(()), torch.full((), 2.0), torch.full((), 3.0)
    monkeypatch.setattr(lm.model, "ce_lovasz_loss", fake)
    batch = (torch.zeros(1, 3, 32, 32), torch.zeros(1, 32, 32, dtype=torch.long))
    lm.training_step(batch, 0)
    lm.validation_step(batch, 0)
    want = dict(lovasz_weight=0.5, lovasz_classes=(1, 2), lovasz_per_image=True, dice_weight=0.25, smooth=1e-6,
                include_background=True, grad_scale=None, interpolate_pos_encoding=False, return_terms=True, ignore_index=255,
                class_weight=None, label_smoothing=0.0)
    assert seen == [want, want]   # validation forms the term too
    assert set(lm.logged) == {"train_loss", "train_ce", "train_dice", "train_lovasz", "valid_loss", "valid_ce", "valid_dice",
                              "valid_lovasz"}
    assert float(lm.logged["train_lovasz"]) == 3.0 and float(lm.logged["valid_ce"]) == 1.0
    # at the default the steps pass what they passed before
    lm = mk(ignore_index=255)
    seen.clear()

    def fake_ce(x, y, **kw):
        seen.append(kw)
        return torch.zeros(())
    monkeypatch.setattr(lm.model, "ce_loss", fake_ce)
    lm.training_step(batch, 0)
    assert seen == [dict(grad_scale=None, ignore_index=255, class_weight=None, label_smoothing=0.0)]
