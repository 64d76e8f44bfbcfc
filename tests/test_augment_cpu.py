"""CPU (-m "not gpu"): the training augmentation's host side.  The numpy restatement of vitseg_augment
(tests/augment_ref.py) on the cases whose answer is known without it, vitseg_augment_matrix (host arithmetic of the C ABI)
against its formula, the draws of Augmenter.sample, the export family and the argument errors of vitseg_augment, which come
back before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import augment_ref as R
from visiontransformer_amd import _lib
from visiontransformer_amd.augment import Augmenter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ID = np.array(R.IDENTITY, np.int64)


def _params(n=1, **kw):
    p = dict(hflip=np.zeros(n, bool), vflip=np.zeros(n, bool), quarter=np.zeros(n, np.int64), angle=np.zeros(n),
             scale=np.ones(n), tx=np.zeros(n), ty=np.zeros(n), brightness=np.ones(n), contrast=np.ones(n),
             saturation=np.ones(n))
    for k, v in kw.items():
        p[k] = np.full(n, v, dtype=p[k].dtype)
    return p


def _aug(**kw):
    return Augmenter(32, device="cpu", **kw)   # (the host side touches no device)


def _images(seed=0, H=13, W=17):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.standard_normal((3, H, W)).astype(np.float32)


# ---- the restatement on cases whose answer is known without it ----------------------------------------------------------
@pytest.mark.parametrize("border", [R.CONSTANT, R.EDGE])
def test_identity_returns_the_source(border):
    u8, f = _images()
    H, W = u8.shape[:2]
    out = R.warp_image_one(u8, ID, H, W, border, (9, 9, 9))
    want = u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    assert out.dtype == np.float32 and np.array_equal(out, want)
    assert np.array_equal(R.warp_image_one(f, ID, H, W, border, (9, 9, 9)).view(np.uint32), f.view(np.uint32))
    m = np.random.default_rng(1).integers(0, 7, (H, W)).astype(np.int64)
    assert np.array_equal(R.warp_mask_one(m, ID, H, W, border, 255, np.int64), m)
    assert np.array_equal(R.warp_mask_one(m.astype(np.uint8), ID, H, W, border, 255, np.uint8), m.astype(np.uint8))


def test_flips_are_exact():
    u8, f = _images(2)
    H, W = u8.shape[:2]
    A = _aug()
    Mh = A.matrices(_params(hflip=True), (H, W), (H, W))[0]
    Mv = A.matrices(_params(vflip=True), (H, W), (H, W))[0]
    assert list(Mh) == [-65536, 0, 65536 * W, 0, 65536, 0] and list(Mv) == [65536, 0, 0, 0, -65536, 65536 * H]
    for border in (R.CONSTANT, R.EDGE):
        assert np.array_equal(R.warp_image_one(f, Mh, H, W, border, (5, 5, 5)), f[:, :, ::-1])
        assert np.array_equal(R.warp_image_one(f, Mv, H, W, border, (5, 5, 5)), f[:, ::-1])
        assert np.array_equal(R.warp_image_one(u8, Mh, H, W, border, (5, 5, 5)),
                              u8[:, ::-1].transpose(2, 0, 1).astype(np.float32) / np.float32(255))
        m = u8[..., 0]
        assert np.array_equal(R.warp_mask_one(m, Mh, H, W, border, 255, np.uint8), m[:, ::-1])
        assert np.array_equal(R.warp_mask_one(m, Mv, H, W, border, 255, np.uint8), m[::-1])


@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("N", [1, 8, 15])
def test_quarter_turns_are_np_rot90(k, N):
    m = np.random.default_rng(k).integers(0, 200, (N, N)).astype(np.uint8)
    M = _aug(rot90=True).matrices(_params(quarter=k), (N, N), (N, N))[0]
    for border in (R.CONSTANT, R.EDGE):
        assert np.array_equal(R.warp_mask_one(m, M, N, N, border, 255, np.uint8), np.rot90(m, k))
    f = np.random.default_rng(k).standard_normal((3, N, N)).astype(np.float32)
    assert np.array_equal(R.warp_image_one(f, M, N, N, R.CONSTANT, (0, 0, 0)), np.rot90(f, k, axes=(1, 2)))


def test_null_colour_is_a_noop_and_the_clamp_holds():
    _, f = _images(3)
    H, W = f.shape[1:]
    f = f * np.float32(3)   # well outside [0, 1]
    x, _ = R.augment(f[None], ID[None], H, W, colour=None)
    assert np.array_equal(x[0].view(np.uint32), f.view(np.uint32))   # no multiply, no clamp
    ident = Augmenter.colour(_params())
    assert ident.dtype == np.float32 and np.array_equal(ident[0], np.eye(3, 4, dtype=np.float32).reshape(12))
    x, _ = R.augment(f[None], ID[None], H, W, colour=ident)
    assert np.array_equal(x[0], np.clip(f, 0, 1)) and x.min() == 0 and x.max() == 1
    wild = (np.random.default_rng(4).standard_normal((1, 12)) * 4).astype(np.float32)
    x, _ = R.augment(f[None], ID[None], H, W, colour=wild)
    assert x.min() >= 0 and x.max() <= 1 and (x == 0).any() and (x == 1).any()


def test_constant_border_fills_and_edge_border_clamps():
    u8, _ = _images(5, 6, 7)
    M = np.array([65536, 0, 65536 * 100, 0, 65536, 0], np.int64)   # every tap 100 pixels right of the frame
    out = R.warp_image_one(u8, M, 6, 7, R.CONSTANT, (10, 20, 30))
    for c, v in enumerate((10, 20, 30)):
        assert np.all(out[c] == np.float32(v) / np.float32(255))
    out = R.warp_image_one(u8, M, 6, 7, R.EDGE, (10, 20, 30))
    assert np.array_equal(out, np.repeat(u8[:, -1:], 7, 1).transpose(2, 0, 1).astype(np.float32) / np.float32(255))
    m = u8[..., 1]
    assert np.all(R.warp_mask_one(m, M, 6, 7, R.CONSTANT, 255, np.uint8) == 255)
    assert np.array_equal(R.warp_mask_one(m, M, 6, 7, R.EDGE, 255, np.uint8), np.repeat(m[:, -1:], 7, 1))
    extreme = np.array([np.iinfo(np.int64).max, np.iinfo(np.int64).min] * 3, np.int64)
    assert list(R.clamp_matrix(extreme)) == [1 << 26, -(1 << 26), 1 << 40, -(1 << 26), 1 << 26, -(1 << 40)]
    assert R.warp_image_one(u8, extreme, 6, 7, R.EDGE, (0, 0, 0)).shape == (3, 6, 7)   # no overflow, no bad index


def test_half_pixel_shift_averages_neighbours():
    f = np.arange(3 * 4 * 6, dtype=np.float32).reshape(3, 4, 6)
    M = np.array([65536, 0, 32768, 0, 65536, 0], np.int64)   # source x = x + 0.5
    out = R.warp_image_one(f, M, 4, 5, R.EDGE, (0, 0, 0))
    assert np.array_equal(out, (f[:, :, :5] + f[:, :, 1:6]) / 2)


# ---- vitseg_augment_matrix against the formula --------------------------------------------------------------------------
def test_matrix_matches_the_formula_over_a_sweep():
    fn = _lib.augment_symbol("vitseg_augment_matrix")
    rng = np.random.default_rng(7)
    out = (C.c_int64 * 6)()
    cases = 0
    for s in range(1, 65):
        for big in (224, 256, 512):
            for src, dst in (((s, big), (big, s)), ((big, s), (s, s)), ((big, big), (s, big))):
                a = rng.uniform(-2, 2, 6)
                assert fn((C.c_double * 6)(*a), src[0], src[1], dst[0], dst[1], out) == _lib.OK
                assert list(out) == list(R.matrix(a, src, dst)) == _lib.augment_matrix(a, src, dst), (a, src, dst)
                cases += 1
            for hw in ((s, s), (s, big), (big, s)):
                assert _lib.augment_matrix([1, 0, 0, 0, 1, 0], hw, hw) == list(R.IDENTITY)
                assert _lib.augment_matrix([-1, 0, 1, 0, 1, 0], hw, hw) == [-65536, 0, 65536 * hw[1], 0, 65536, 0]
                assert _lib.augment_matrix([1, 0, 0, 0, -1, 1], hw, hw) == [65536, 0, 0, 0, -65536, 65536 * hw[0]]
    assert cases == 64 * 3 * 3


@pytest.mark.parametrize("a,src,dst,word", [
    ([2000.0, 0, 0, 0, 1, 0], (8, 8), (8, 8), "2^26"), ([1, 0, 0, 0, -1025.0, 0], (8, 8), (8, 8), "2^26"),
    ([1, 0, 2.0 ** 24 + 1, 0, 1, 0], (8, 8), (8, 8), "2^40"), ([1, 0, 0, 0, 1, float("nan")], (8, 8), (8, 8), "2^40"),
    ([1, 0, 0, 0, 1, 0], (0, 8), (8, 8), "16384"), ([1, 0, 0, 0, 1, 0], (8, 8), (8, 16385), "16384")])
def test_matrix_errors_are_eshape_with_a_message_and_write_nothing(a, src, dst, word):
    out = (C.c_int64 * 6)(*[7] * 6)
    rc = _lib.augment_symbol("vitseg_augment_matrix")((C.c_double * 6)(*a), src[0], src[1], dst[0], dst[1], out)
    assert rc == _lib.ESHAPE and word in _lib.lib().vitseg_last_error().decode()
    assert list(out) == [7] * 6
    with pytest.raises(ValueError, match=re.escape(word)):
        _lib.augment_matrix(a, src, dst)
    # the bounds themselves are accepted
    assert _lib.augment_matrix([1024.0, 0, 2.0 ** 24 / 8, 0, 1, 0], (8, 8), (8, 8))[:3] == [1 << 26, 0, 1 << 40]
    assert _lib.augment_matrix([1, 0, 0, 0, 1, 0], (16384, 1), (16384, 16384)) == [4, 0, 0, 0, 65536, 0]


# ---- Augmenter.sample ---------------------------------------------------------------------------------------------------
def _same(p, q):
    return p.keys() == q.keys() and all(np.array_equal(p[k], q[k]) for k in p)


def test_sample_depends_on_seed_and_key_alone():
    kw = dict(seed=3, rot90=True, rotate=20.0, scale=(0.5, 2.0), translate=0.2, brightness=0.3, contrast=0.3, saturation=0.3)
    A, B = _aug(**kw), _aug(**kw)
    a0, a1 = A.sample(16, key=(0, 0)), A.sample(16, key=(0, 1))
    b1, b0 = B.sample(16, key=(0, 1)), B.sample(16, key=(0, 0))       # the other call order
    assert _same(a0, b0) and _same(a1, b1) and not _same(a0, a1)
    assert not _same(a0, _aug(**{**kw, "seed": 4}).sample(16, key=(0, 0)))
    assert not _same(a0, A.sample(16, key=(1, 0)))
    # the default key is (rank, calls): successive default draws differ and are the keyed draws
    assert A.calls == 0 and A.rank == 0
    d0, d1 = A.sample(16), A.sample(16)
    assert A.calls == 2 and _same(d0, a0) and _same(d1, a1)
    assert set(a0) == {"hflip", "vflip", "quarter", "angle", "scale", "tx", "ty", "brightness", "contrast", "saturation"}


def test_sample_stays_inside_its_ranges_and_honours_probabilities():
    A = _aug(seed=1, hflip=0.5, vflip=0.25, rot90=True, rotate=20.0, scale=(0.5, 2.0), translate=0.2, brightness=0.3,
             contrast=1.5, saturation=0.1)
    p = A.sample(4096, key=(0,))
    assert np.abs(p["angle"]).max() <= 20 and np.abs(p["angle"]).max() > 15
    assert p["scale"].min() >= 0.5 and p["scale"].max() <= 2.0
    assert np.abs(p["tx"]).max() <= 0.2 and np.abs(p["ty"]).max() <= 0.2
    assert 0.7 <= p["brightness"].min() and p["brightness"].max() <= 1.3
    assert 0.0 <= p["contrast"].min() and p["contrast"].max() <= 2.5 and (p["contrast"] == 0).any()   # max(0, 1 - v)
    assert 0.9 <= p["saturation"].min() and p["saturation"].max() <= 1.1
    assert set(np.unique(p["quarter"])) == {0, 1, 2, 3}
    assert 0.45 < p["hflip"].mean() < 0.55 and 0.2 < p["vflip"].mean() < 0.3
    never, always = _aug(hflip=0.0, vflip=0.0).sample(4096, key=(0,)), _aug(hflip=1.0, vflip=1.0).sample(4096, key=(0,))
    assert not never["hflip"].any() and not never["vflip"].any() and always["hflip"].all() and always["vflip"].all()
    assert not never["quarter"].any() and not never["angle"].any() and np.all(never["scale"] == 1)   # all off: the identity
    assert np.all(never["brightness"] == 1) and np.all(never["tx"] == 0)
    M = _aug().matrices(never, (32, 32), (32, 32))
    assert np.array_equal(M, np.tile(ID, (4096, 1)))


def test_augmenter_argument_errors():
    for kw in (dict(border="wrap"), dict(hflip=1.5), dict(scale=(0.0, 1.0)), dict(scale=(2.0, 1.0)), dict(rotate=-1.0),
               dict(fill=(0, 0))):
        with pytest.raises(ValueError):
            _aug(**kw)
    with pytest.raises(ValueError, match="fill_label"):   # before anything reaches the device
        _aug(border="constant").apply(np.zeros((1, 4, 4, 3), np.uint8), np.zeros((1, 4, 4), np.uint8))


# ---- the export family and the argument errors of vitseg_augment --------------------------------------------------------
def test_exports_and_header():
    assert _lib.AUGMENT_EXPORTS == ["vitseg_augment_matrix", "vitseg_augment"]
    assert set(_lib.AUGMENT_EXPORTS) <= set(_lib._LATE_EXPORTS) <= set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "vitseg.h")).read()
    for name in _lib.AUGMENT_EXPORTS:
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
        assert callable(_lib.augment_symbol(name))
    assert "#define VITSEG_VERSION 110" in hdr and _lib.lib().vitseg_version() == _lib.VERSION == 110
    assert (_lib.AUGMENT_CONSTANT, _lib.AUGMENT_EDGE, _lib.AUGMENT_U8_NHWC, _lib.AUGMENT_F32_NCHW) == (0, 1, 0, 1)
    assert re.search(r"VITSEG_AUGMENT_CONSTANT = 0, VITSEG_AUGMENT_EDGE = 1", hdr)
    assert re.search(r"VITSEG_AUGMENT_U8_NHWC = 0, VITSEG_AUGMENT_F32_NCHW = 1", hdr)
    # struct vitseg_augment_mask as include/vitseg.h lays it out on a 64-bit target
    assert C.sizeof(_lib.CAugmentMask) == 48 and _lib.CAugmentMask.src_is_i64.offset == 24 and _lib.CAugmentMask.ow.offset == 44


def _call(**kw):
    """vitseg_augment with dummy non-null pointers (never dereferenced: every case fails its checks before the launch)."""
    P = 0x1000
    mask = _lib.CAugmentMask(P, P, P, 0, 0, 8, 8, 8, 8)
    for k in [k for k in kw if k.startswith("mask_")]:
        setattr(mask, k[5:], kw.pop(k))
    d = dict(images=P, fmt=0, n=2, H=8, W=8, oh=8, ow=8, matrix=P, colour=None, out=P, masks=C.pointer(mask), num_masks=1,
             border=_lib.AUGMENT_EDGE, fill=(C.c_float * 3)(0, 0, 0), fill_label=0)
    d.update(kw)
    return int(_lib.augment_symbol("vitseg_augment")(d["images"], d["fmt"], d["n"], d["H"], d["W"], d["oh"], d["ow"], d["matrix"],
                                                     d["colour"], d["out"], d["masks"], d["num_masks"], d["border"], d["fill"],
                                                     d["fill_label"], None))


@pytest.mark.parametrize("kw,code,word", [
    (dict(n=0), _lib.ESHAPE, "samples"), (dict(n=-3), _lib.ESHAPE, "samples"),
    (dict(H=0), _lib.ESHAPE, "16384"), (dict(W=16385), _lib.ESHAPE, "16384"), (dict(oh=0), _lib.ESHAPE, "16384"),
    (dict(ow=16385), _lib.ESHAPE, "16384"), (dict(mask_h=0), _lib.ESHAPE, "mask 0"), (dict(mask_ow=16385), _lib.ESHAPE, "mask 0"),
    (dict(images=None), _lib.EINVAL, "null"), (dict(matrix=None), _lib.EINVAL, "null"), (dict(out=None), _lib.EINVAL, "null"),
    (dict(masks=None), _lib.EINVAL, "null"), (dict(mask_src=None), _lib.EINVAL, "mask 0"),
    (dict(mask_matrix=None), _lib.EINVAL, "mask 0"), (dict(mask_out=None), _lib.EINVAL, "mask 0"),
    (dict(mask_src_is_i64=2), _lib.EINVAL, "label format"), (dict(mask_out_is_i64=-1), _lib.EINVAL, "label format"),
    (dict(num_masks=3), _lib.EINVAL, "label planes"), (dict(num_masks=-1), _lib.EINVAL, "label planes"),
    (dict(border=2), _lib.EINVAL, "border"), (dict(fmt=2), _lib.EINVAL, "format"),
    (dict(border=_lib.AUGMENT_CONSTANT, fill=None), _lib.EINVAL, "fill"),
    (dict(n=1 << 30, oh=16384, ow=16384), _lib.ESHAPE, "one launch")])
def test_augment_argument_errors_come_back_before_any_launch(kw, code, word):
    assert _call(**kw) == code
    assert word in _lib.lib().vitseg_last_error().decode()
