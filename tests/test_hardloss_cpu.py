"""CPU (-m "not gpu"): the oracle of the hard-pixel losses (tests/hardloss_ref.py) against torch's autograd, the exact
selection on cases written out by hand, the family header against `_ext.EXT_LATER`, the host-side option checks, the script
flags and the Lightning module's refusals.  No compute entry point runs; the argument checks of the C entry points do."""
import argparse
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import ce_ref
import hardloss_ref as HR
from test_binding_cpu import STRUCTS, parse_header, signature_errors, struct_errors
from visiontransformer_amd import _ext, _lib, scripts
from visiontransformer_amd.lightning import LightningViTModel
from visiontransformer_amd.model import check_hard_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vitseg_hardloss.h")
NAMES = ["vitseg_hardloss_version", "vitseg_hard_loss_scratch_bytes", "vitseg_hard_ce_loss", "vitseg_backward_hard"]
INF = float("inf")


# ---- the closed form against autograd ----

def _case(seed, B=2, C_=5, g=7, S=28):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C_, g, g, generator=gen).float() * 3.0
    t = torch.randint(0, C_, (B, S, S), generator=gen)
    mask = torch.rand(B, S, S, generator=gen) < 0.3
    w = (10.0 ** (torch.rand(C_, generator=gen) * 4.0 - 2.0)).float().tolist()
    return z, t, mask, w, gen


@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0, 5.0])
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("ignore", [False, True])
@pytest.mark.parametrize("subset", [False, True])
def test_closed_form_is_autograd_of_the_definition(gamma, weights, ignore, subset):
    z, t, mask, w, gen = _case(int(gamma * 10) + 100 * weights + 200 * ignore + 400 * subset)
    S = t.shape[-1]
    ii = None
    if ignore:
        ii = 255
        t[torch.rand(t.shape, generator=gen) < 0.2] = ii
    kw = dict(ignore_index=ii, class_weight=w if weights else None)
    loss_a, grad_a, ce_a, up = HR.hard_ref(z, t, S, mask if subset else None, gamma, **kw)
    loss_c, grad_c, den, ce_c = HR.hard_closed_form(up, t, mask if subset else None, gamma, **kw)
    assert torch.isfinite(loss_a) and float(den) > 0
    assert abs(float(loss_c) - float(loss_a)) <= 1e-12 * abs(float(loss_a))
    assert (grad_c - grad_a).abs().max().item() <= 1e-12 * grad_a.abs().max().item()
    keep = torch.ones_like(t, dtype=torch.bool) if ii is None else t != ii
    assert (ce_c - ce_a).abs()[keep].max().item() <= 1e-12 * ce_a.abs().max().item()
    hard = keep & mask if subset else keep
    assert (grad_c.permute(1, 0, 2, 3)[:, ~hard] == 0).all() and (grad_c.permute(1, 0, 2, 3)[:, hard] != 0).any()


def test_gamma_zero_is_the_cross_entropy_of_ce_ref():
    z, t, mask, w, gen = _case(7)
    t[torch.rand(t.shape, generator=gen) < 0.2] = 255
    up = ce_ref.upsample64(z, t.shape[-1])
    loss_h, grad_h, den_h, _ = HR.hard_closed_form(up, t, None, 0.0, ignore_index=255, class_weight=w)
    loss_c, grad_c, den_c = ce_ref.ce_closed_form(up, t, ignore_index=255, class_weight=w)
    assert float(den_h) == float(den_c)
    assert abs(float(loss_h) - float(loss_c)) <= 1e-14 * abs(float(loss_c))
    assert (grad_h - grad_c).abs().max().item() <= 1e-14 * grad_c.abs().max().item()


def test_m_at_q_zero_and_at_gamma_zero():
    q = torch.tensor([0.0, 0.0, 0.5, 1.0 - 1e-9], dtype=torch.float64)
    ce = -torch.log1p(-q)
    for gamma in (0.5, 1.0, 2.0, 5.0):
        m = HR.focal_m(q, ce, gamma)
        assert m[0] == 0 and m[1] == 0 and torch.isfinite(m).all()
        want = 0.5 ** gamma + gamma * 0.5 * math.log(2.0) * 0.5 ** (gamma - 1.0)
        assert abs(float(m[2]) - want) <= 1e-15 * want
    assert torch.equal(HR.focal_m(q, ce, 0.0), torch.ones(4, dtype=torch.float64))
    # the loss itself at a pixel the model has exactly right: q == 0 gives f == 0 and a zero gradient row, not NaN
    up = torch.tensor([[[[80.0]], [[-80.0]]]], dtype=torch.float64)
    loss, grad, den, ce1 = HR.hard_closed_form(up, torch.zeros(1, 1, 1, dtype=torch.long), None, 0.5)
    assert float(ce1) == 0.0 and float(loss) == 0.0 and (grad == 0).all()


# ---- the selection ----

def _bits(v):
    return int(np.array(v, dtype=np.float32).view(np.uint32))


def test_select_ref_on_cases_written_out_by_hand():
    plane = np.array([0.5, 0.1, 2.0, 0.1, 3.0, 0.0, 0.1, 1.0], dtype=np.float32)
    valid = np.array([1, 1, 1, 1, 1, 1, 1, 0], dtype=bool)   # 7 valid; sorted down: 3, 2, .5, .1, .1, .1, 0
    sel = lambda **kw: HR.select_ref(plane, valid, kw.get("t", INF), kw.get("m", 0), kw.get("q", 0))
    k, tau, H = sel()                                    # OHEM "off" as a selection: k = 0, tau = +inf, nothing reaches it
    assert (k, tau, H.sum()) == (0, _bits(INF), 0)
    k, tau, H = sel(m=1)
    assert (k, tau, H.tolist()) == (1, _bits(3.0), [0, 0, 0, 0, 1, 0, 0, 0])
    k, tau, H = sel(m=4)                                 # the 4th largest is 0.1: all three tied pixels come along
    assert (k, tau, int(H.sum())) == (4, _bits(0.1), 6) and not H[5] and not H[7]
    k, tau, H = sel(m=7)
    assert (k, tau) == (7, 0) and np.array_equal(H, valid)
    k, tau, H = sel(m=100)                               # min_kept > n_valid
    assert (k, tau) == (7, 0) and np.array_equal(H, valid)
    k, tau, H = sel(q=65536)                             # the whole of the valid pixels
    assert (k, tau) == (7, 0) and np.array_equal(H, valid)
    k, tau, H = sel(q=1)                                 # ceil(7 / 65536) = 1
    assert (k, tau) == (1, _bits(3.0))
    k, tau, H = sel(q=65536 * 2 // 7 + 1)                # just above 2 / 7: ceil gives 3
    assert (k, tau) == (3, _bits(0.5))
    k, tau, H = sel(t=1.5)                               # threshold only
    assert (k, tau, H.tolist()) == (0, _bits(1.5), [0, 0, 1, 0, 1, 0, 0, 0])
    k, tau, H = sel(t=1.5, m=3)                          # the floor reaches below the threshold
    assert (k, tau, int(H.sum())) == (3, _bits(0.5), 3)
    k, tau, H = sel(t=0.05, m=2)                         # the threshold reaches below the floor
    assert (k, tau, int(H.sum())) == (2, _bits(0.05), 6)
    k, tau, H = sel(t=0.0)                               # probability threshold 1: everything valid
    assert (k, tau) == (0, 0) and np.array_equal(H, valid)


def test_select_ref_ties_empty_and_nan():
    plane = np.full((3, 5), 0.25, dtype=np.float32)
    valid = np.ones((3, 5), dtype=bool)
    for m in (1, 7, 15):
        k, tau, H = HR.select_ref(plane, valid, INF, m, 0)
        assert (k, tau) == (m, _bits(0.25)) and H.all()              # everything equal: everything is kept
    k, tau, H = HR.select_ref(plane, np.zeros((3, 5), dtype=bool), 0.5, 10, 65536)
    assert (k, tau, int(H.sum())) == (0, _bits(0.5), 0)              # n_valid = 0
    plane[1, 2] = np.nan                                             # the canonical quiet NaN ranks above everything
    plane[0, 0] = np.inf
    k, tau, H = HR.select_ref(plane, valid, INF, 1, 0)
    assert (k, tau, int(H.sum())) == (1, _bits(INF), 2) and H[1, 2]   # tau = min(+inf, NaN's pattern): the threshold's
    k, tau, H = HR.select_ref(plane, valid, INF, 2, 0)
    assert (k, tau, int(H.sum())) == (2, _bits(INF), 2) and H[0, 0] and H[1, 2]
    k, tau, H = HR.select_ref(plane, valid, 1.0, 0, 0)               # ... and above any threshold
    assert int(H.sum()) == 2
    plane[2, 2] = -1.0                                               # the ignored pixels' sentinel never ranks
    valid[2, 2] = False
    k, tau, H = HR.select_ref(plane, valid, INF, 0, 65536)
    assert (k, tau) == (14, _bits(0.25)) and np.array_equal(H, valid)
    with pytest.raises(AssertionError):
        HR.select_ref(plane, np.ones((3, 5), dtype=bool), INF, 0, 65536)


# ---- the family header and its table ----

def _table():
    return {name: (restype, list(argtypes)) for name, restype, argtypes in _ext.EXT_LATER["hardloss"][2]}


def test_family_header_is_the_table_both_ways():
    decls, structs, enums, defines = parse_header(open(HEADER).read())
    assert _ext.EXT_LATER["hardloss"][:2] == ("vitseg_hardloss.h", "the hard-pixel losses")
    assert sorted(decls) == sorted(NAMES) == sorted(_table()) and not enums
    known = dict(STRUCTS, vitseg_hard_options=_ext.CHardOptions)
    assert signature_errors(decls, _table(), known) == []
    assert list(structs) == ["vitseg_hard_options"] and struct_errors(structs["vitseg_hard_options"], _ext.CHardOptions) == []
    assert defines == {"VITSEG_HARDLOSS_VERSION": 100}
    assert _ext.HARDLOSS_VERSION == 100 and _ext.EXT_VERSIONS["hardloss"] == ("vitseg_hardloss_version", 100)
    # vitseg_backward_hard: the argument list of vitseg_backward_opts, then hard and stats
    assert _table()["vitseg_backward_hard"][1] == list(_lib.ce_opts_symbol("vitseg_backward_opts").argtypes) + [_ext.phard, C.c_void_p]
    assert len(decls["vitseg_hard_ce_loss"][1]) == 16 and decls["vitseg_hard_ce_loss"][1][14] == ("int64_t", 1)
    tab = _table()
    tab["vitseg_hard_ce_loss"] = (C.c_int, tab["vitseg_hard_ce_loss"][1][:12] + [C.c_double] + tab["vitseg_hard_ce_loss"][1][13:])
    assert signature_errors(decls, tab, known) == ["vitseg_hard_ce_loss: argument 12: c_double for float"]   # it can fail
    assert not set(NAMES) & set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "vitseg.h")).read()
    assert "vitseg_hard" not in hdr.lower() and '#include "vitseg.h"' in open(HEADER).read()
    f = _ext.CHardOptions   # the layout on a 64-bit target
    assert [(n, getattr(f, n).offset) for n, _ in f._fields_] == [
        ("gamma", 0), ("loss_thresh", 4), ("min_kept", 8), ("keep_q16", 16), ("reserved", 20), ("scratch", 24), ("scratch_bytes", 32)]
    assert C.sizeof(f) == 40


def test_library_exports_the_family_at_its_version():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert _ext.ext_symbol("hardloss", name) is getattr(_lib.lib(), name)
    assert _ext.ext_symbol("hardloss", "vitseg_hardloss_version")() == 100
    q = _ext.ext_symbol("hardloss", "vitseg_hard_loss_scratch_bytes")
    # state row 256 | 2048 bins | 2 + 3 partials per 1024 pixels | the plane, each part rounded up to 256 bytes
    up = lambda v: (v + 255) // 256 * 256
    for B, S in ((3, 28), (2, 40), (32, 512)):
        npx, nblk = B * S * S, (B * S * S + 1023) // 1024
        assert q(B, S) == 256 + 8192 + up(16 * nblk) + up(24 * nblk) + up(4 * npx)
    assert q(0, 28) == 0 and q(2, 0) == 0 and q(8, 16384) == 0   # 2^31 pixels
    with pytest.raises(RuntimeError, match=r"has no vitseg_hard_nothing \(built before the hard-pixel losses\)"):
        _ext.ext_symbol("hardloss", "vitseg_hard_nothing")


def test_argument_errors_come_back_before_any_launch():
    """EINVAL from the checks in front of the launches; every address is a live buffer no call reaches (host memory
    without a device, device memory where there is one)."""
    fn = _ext.ext_symbol("hardloss", "vitseg_hard_ce_loss")
    if torch.cuda.is_available():
        buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
        a = buf.data_ptr()
    else:
        buf = C.create_string_buffer(1 << 20)
        a = C.addressof(buf)
        a += -a % 16
    need = int(_ext.ext_symbol("hardloss", "vitseg_hard_loss_scratch_bytes")(2, 28))
    ok = dict(gamma=2.0, t=0.5, m=10, q=100, scr=a, n=need)

    def call(C_=5, lowres=a, target=a, loss=a, scratch=a, ce=None, null_hard=False, **kw):
        o = dict(ok, **kw)
        h = _ext.CHardOptions(o["gamma"], o["t"], o["m"], o["q"], 0, o["scr"], o["n"])
        return fn(lowres, target, 1, None, scratch, loss, 2, C_, 7, 28, ce, None if null_hard else C.byref(h), 1.0, None, None, None)
    nan = float("nan")
    for kw in (dict(gamma=-1.0), dict(gamma=nan), dict(gamma=INF), dict(t=nan), dict(t=-0.5), dict(t=-INF), dict(m=-1),
               dict(q=-1), dict(q=65537), dict(scr=None), dict(scr=a + 4), dict(n=need - 1), dict(n=0)):
        assert call(**kw) == _lib.EINVAL, kw
        assert b"hard loss" in _lib.lib().vitseg_last_error()
    assert call(C_=256) == _lib.EINVAL and call(C_=0) == _lib.EINVAL and call(null_hard=True) == _lib.EINVAL
    for kw in (dict(lowres=None), dict(target=None), dict(loss=None), dict(scratch=None)):
        assert call(**kw) == _lib.EINVAL, kw
    smooth = _lib.CCEOptions(0, 0, 0, None, 0.1, a, 1 << 19)
    assert call(ce=C.byref(smooth)) == _lib.EINVAL and b"label smoothing" in _lib.lib().vitseg_last_error()
    for bad_ce in (_lib.CCEOptions(0, 0, 0, None, 0.0, None, 1 << 19), _lib.CCEOptions(0, 0, 0, None, 0.0, a, 8)):
        assert call(ce=C.byref(bad_ce)) == _lib.EINVAL   # the errors of vitseg_ce_loss_opts


# ---- Python: the option checks, the flags, the module ----

def test_check_hard_options_takes_and_refuses_what_the_header_lists():
    f32 = lambda v: float(np.float32(v))
    assert check_hard_options() is None
    assert check_hard_options(0.0, None, 0, 0.0) is None
    assert check_hard_options(2) == (2.0, INF, 0, 0)
    assert check_hard_options(0.1) == (f32(0.1), INF, 0, 0)
    assert check_hard_options(ohem_thresh=0.7) == (0.0, f32(-math.log(0.7)), 0, 0)
    got = check_hard_options(ohem_thresh=1.0)
    assert got == (0.0, 0.0, 0, 0) and math.copysign(1.0, got[1]) == 1.0   # +0, not -log(1) = -0
    assert check_hard_options(ohem_min_kept=100000) == (0.0, INF, 100000, 0)
    assert check_hard_options(ohem_keep_fraction=0.25) == (0.0, INF, 0, 16384)
    assert check_hard_options(ohem_keep_fraction=1) == (0.0, INF, 0, 65536)
    assert check_hard_options(ohem_keep_fraction=1e-9) == (0.0, INF, 0, 0)   # rounds to 0 of 65536, but the option is on
    assert check_hard_options(ohem_keep_fraction=1.5 / 65536) == (0.0, INF, 0, 2)   # rint: half to even
    assert check_hard_options(2.0, 0.7, 5, 0.5) == (2.0, f32(-math.log(0.7)), 5, 32768)
    for kw in (dict(focal_gamma=-1), dict(focal_gamma=float("nan")), dict(focal_gamma=INF), dict(focal_gamma="2"),
               dict(focal_gamma=None), dict(focal_gamma=1e39), dict(ohem_thresh=0.0), dict(ohem_thresh=-0.1),
               dict(ohem_thresh=1.5), dict(ohem_thresh=float("nan")), dict(ohem_thresh="0.7x"), dict(ohem_thresh=True),
               dict(ohem_min_kept=-1), dict(ohem_min_kept=1.0), dict(ohem_min_kept=True), dict(ohem_min_kept=2 ** 63),
               dict(ohem_min_kept=None), dict(ohem_keep_fraction=-0.1), dict(ohem_keep_fraction=1.1),
               dict(ohem_keep_fraction=float("nan")), dict(ohem_keep_fraction=None), dict(ohem_keep_fraction=True)):
        with pytest.raises(ValueError):
            check_hard_options(**kw)


def test_scripts_map_the_flags():
    ap = argparse.ArgumentParser()
    scripts.add_ce_loss_arguments(ap)
    assert scripts.ce_loss_options(ap.parse_args([])) == {}
    a = ap.parse_args(["--focal-gamma", "2", "--ohem-thresh", "0.7", "--ohem-min-kept", "100000", "--ohem-keep-fraction", "0.25"])
    assert scripts.ce_loss_options(a) == dict(focal_gamma=2.0, ohem_thresh=0.7, ohem_min_kept=100000, ohem_keep_fraction=0.25)
    a = ap.parse_args(["--ignore-index", "255", "--ohem-keep-fraction", "0.5"])
    assert scripts.ce_loss_options(a) == dict(ignore_index=255, ohem_keep_fraction=0.5)
    assert scripts.ce_loss_options(ap.parse_args(["--focal-gamma", "0.5"])) == dict(focal_gamma=0.5)
    for script in ("createViTmodel.py", "trainCurrentViTmodel.py"):   # both training scripts take the flags from there
        src = open(os.path.join(ROOT, "model", "CE", script)).read()
        assert "scripts.add_ce_loss_arguments(ap)" in src and "**scripts.ce_loss_options(a)" in src


def test_lightning_module_takes_and_refuses_the_options(monkeypatch):
    mk = lambda **kw: LightningViTModel(5, 16, 64, 1, 1, image_size=32, intermediate_size=128, **kw)
    with pytest.raises(ValueError, match="Dice term .* out of scope"):
        mk(dice_weight=0.5, focal_gamma=2.0)
    with pytest.raises(ValueError, match="Dice term .* out of scope"):
        mk(dice_weight=0.5, ohem_keep_fraction=0.25)
    with pytest.raises(ValueError, match="label_smoothing"):
        mk(label_smoothing=0.1, ohem_thresh=0.7)
    for kw in (dict(focal_gamma=-1.0), dict(ohem_thresh=2.0), dict(ohem_min_kept=-5), dict(ohem_keep_fraction=2.0)):
        with pytest.raises(ValueError):
            mk(**kw)
    assert not mk().hard and not mk(dice_weight=0.5).hard and mk(focal_gamma=2.0).hard
    # the steps: training passes everything and logs train_kept; validation passes the focal factor alone
    lm = mk(ignore_index=255, focal_gamma=2.0, ohem_thresh=0.7, ohem_min_kept=10, ohem_keep_fraction=0.25)
    seen = []

    def fake_ce_loss(x, y, **kw):
        seen.append(kw)
        loss = torch.zeros(())
        return (loss, torch.tensor([100, 25, 40, 0])) if kw.get("return_stats") else loss
    monkeypatch.setattr(lm.model, "ce_loss", fake_ce_loss)
    batch = (torch.zeros(1, 3, 32, 32), torch.zeros(1, 32, 32, dtype=torch.long))
    lm.training_step(batch, 0)
    lm.validation_step(batch, 0)
    common = dict(grad_scale=None, interpolate_pos_encoding=False, ignore_index=255, class_weight=None, label_smoothing=0.0,
                  focal_gamma=2.0)
    assert seen[0] == dict(common, ohem_thresh=0.7, ohem_min_kept=10, ohem_keep_fraction=0.25, return_stats=True)
    assert seen[1] == common
    assert set(lm.logged) == {"train_loss", "train_kept", "valid_loss"} and float(lm.logged["train_kept"]) == 0.4
    # at the defaults the steps pass what they passed before
    lm = mk(ignore_index=255)
    seen.clear()
    monkeypatch.setattr(lm.model, "ce_loss", fake_ce_loss)
    lm.training_step(batch, 0)
    assert seen == [dict(grad_scale=None, ignore_index=255, class_weight=None, label_smoothing=0.0)]
    assert set(lm.logged) == {"train_loss"}
