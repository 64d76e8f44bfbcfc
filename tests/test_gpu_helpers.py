"""GPU (-m gpu): the embedding, seg-head and training helper kernels, each called through its own C-ABI entry
(csrc/op_helpers.hip: the production call site's arguments and launcher) against the fp64 references of tests/helpers_ref.py.

Every arithmetic kernel gets two kinds of input.  "exact": small signed integers, chosen so that every partial sum stays below
2^24 (asserted) -- the result is then the same in any summation order and in fp32, x3, bf16 and IEEE half, and is compared with
`==`: one wrong tap, row, pad or dropped element fails, however small.  "rounded": seeded Gaussians against the fp64 reference
with the bound of the existing test of the same kernel family (test_gpu_ops.py), or for the reductions
(depth + 2) * 2^-24 * sum |terms|, depth = the longest chain of dependent adds, read from the kernel's comment and stated next
to the bound.  Pure data movement is compared bit for bit.  Inputs are guard-banded and checked unchanged, outputs and scratch
start as NaN between guards (tests/guard.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import helpers_ref as R
from guard import check, guarded, snapshot, unchanged
from oracle import vitseg_oracle as O
from visiontransformer_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS24 = 2.0 ** -24
H16 = {"bf16": torch.bfloat16, "f16": torch.float16}
KINDS = ["exact", "rounded"]


def _fn(name):
    return _lib.helper_symbol(name)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t, dtype=None, name=None):
    return guarded(tuple(t.shape), dtype or t.dtype, t, device=DEV, name=name)


def _out(shape, dtype=torch.float32, fill="nan", name=None):
    return guarded(shape, dtype, fill, device=DEV, name=name)


def _p(t):
    return None if t is None else t.data_ptr()


def _after(snap, *outs):
    """after a call: every guard (inputs and outputs) intact, every input bitwise unchanged"""
    torch.cuda.synchronize()
    check(*[t for t, _ in snap if t is not None], *outs)
    unchanged(snap)


def _untouched(*ts):
    """a refused call launched nothing: every byte of these NaN-filled buffers is still 0xFF"""
    torch.cuda.synchronize()
    for t in ts:
        assert bool((t.contiguous().view(-1).view(torch.uint8) == 0xFF).all()), getattr(t._guard, "name", None)


def _bits(t):
    return t.contiguous().cpu().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _small_enough(*terms):
    """every partial sum of an exact case stays below 2^24 in magnitude: `terms` bound the absolute sum"""
    assert sum(float(t) for t in terms) < 2 ** 24


# ============================================================ the patch embedding: A_PATCH + EPI_POS, then cls_rows_kernel
@functools.lru_cache(maxsize=None)
def _patch_case(B, Cin, P, g, D, kind):
    S, Np, K = g * P, g * g, Cin * P * P
    if kind == "exact":
        img, Wp = R.ints(B, Cin, S, S, lo=-4, hi=4, seed=P + g), R.ints(D, K, lo=-2, hi=2, seed=D + 1)
        bp, pos, cls = R.ints(D, lo=-8, hi=8, seed=2), R.ints(Np + 1, D, lo=-8, hi=8, seed=3), R.ints(D, lo=-8, hi=8, seed=4)
    else:
        img, Wp = R.gauss(B, Cin, S, S, seed=P + g), R.gauss(D, K, seed=D + 1, scale=0.05)
        bp, pos, cls = R.gauss(D, seed=2, scale=0.1), R.gauss(Np + 1, D, seed=3, scale=0.5), R.gauss(D, seed=4)
    ref = R.patch_embed(img, Wp, bp, pos, cls, P)
    scale = R.im2col_patch(img, P).abs().double() @ Wp.abs().double().T      # the gathered operand, as test_linear_* form it
    return img, Wp, bp, pos, cls, ref, scale


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("x3", [0, 1, 2])
@pytest.mark.parametrize("B,Cin,P,g,D", R.PATCH_SHAPES)
def test_patch_embed(B, Cin, P, g, D, x3, kind):
    """gemm_tile.hip A_PATCH + EPI_POS gathered from the NCHW image, in fp32 and both x3 modes (2: weights through
    vitseg_cast_params_split), then cls_rows_kernel.  Shapes: K = 48 (no multiple of the 32-wide K step) with two images
    (m % Np); M = 144 crosses a 128-row tile; the generic patch sizes 8 and 12 (K = 432); N = 132 ends 4 columns past a tile;
    K = 3072.  A pos row off by one or a CLS row in the wrong place fails the exact case."""
    img, Wp, bp, pos, cls, ref, scale = _patch_case(B, Cin, P, g, D, kind)
    Np, K = g * g, Cin * P * P
    d = [_dev(t, name=n) for t, n in ((img, "img"), (Wp, "Wp"), (bp, "bp"), (pos, "pos"), (cls, "cls"))]
    W = d[1]
    if x3 == 2:
        W = _out((D, K), name="Wp split")
        _lib.check(_lib.lib().vitseg_cast_params_split(d[1].data_ptr(), W.data_ptr(), D * K, _stream()))
    X = _out((B * (Np + 1), D), name="X")
    snap = snapshot(*d, W)
    _lib.check(_fn("vitseg_op_patch_embed_f32")(d[0].data_ptr(), W.data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                                                X.data_ptr(), B, Cin, P, g, D, x3, _stream()))
    _after(snap, X)
    got = X.cpu()
    # cls_rows_kernel: one fp32 add, bit for bit
    assert torch.equal(_bits(got[B * Np:]), _bits((cls + pos[0]).expand(B, D)))
    if kind == "exact":
        _small_enough(K * img.abs().max() * Wp.abs().max(), bp.abs().max(), pos.abs().max())
        assert torch.equal(got.double(), ref)
        return
    err = (got.double() - ref).abs()[:B * Np]
    print(f"patch_embed x3={x3}: max err {err.max().item():.3e}, scale {scale.max().item():.3e}")
    if x3 == 0:   # test_linear_epilogues' bound
        assert err.max().item() < 4e-7 * scale.max().item() + 1e-6
    else:         # test_linear_f32x3_is_fp32_grade's bound
        assert (err / (scale + 1e-3)).max().item() < 1e-6


# ============================================================ the 3x3 conv as an implicit GEMM: A_CONV3 + EPI_RELU / EPI_BIAS
@functools.lru_cache(maxsize=4)
def _conv_case(B, g, C, N, relu, kind, rnd):
    """relu: H [M, C], W [N, 9 C], bias (seg_head.0 forward); not relu: no bias (the input-gradient form).  rnd: the 16-bit type
    the Gaussian inputs are rounded to first, so that only accumulation is compared."""
    M = B * g * g
    if kind == "exact":
        H, W = R.ints(M, C, lo=-4, hi=4, seed=g + C), R.ints(N, 9 * C, lo=-2, hi=2, seed=N + 1)
        bias = R.ints(N, lo=-8, hi=8, seed=5) if relu else None
        return H, W, bias, R.conv3x3(H, W, bias, B, g, relu), None
    H, W = R.gauss(M, C, seed=g + C), R.gauss(N, 9 * C, seed=N + 1, scale=0.05)
    if rnd is not None:
        H, W = H.to(rnd).float(), W.to(rnd).float()
    bias = R.gauss(N, seed=5, scale=0.1) if relu else None
    scale = R.im2col3x3(H.abs(), B, g).double() @ W.abs().double().T
    return H, W, bias, R.conv3x3(H, W, bias, B, g, relu), scale


def _run_conv(B, g, C, N, relu, mode, kind):
    M, K = B * g * g, 9 * C
    h16 = mode in H16
    H, W, bias, ref, scale = _conv_case(B, g, C, N, relu, kind, H16.get(mode) if kind == "rounded" else None)
    dt = H16.get(mode, torch.float32)
    Hd, Wd, bd = _dev(H, dt, name="H"), _dev(W, dt, name="W"), _dev(bias, name="bias") if relu else None
    Cd = _out((M, N), name="C")
    if h16:
        zeros = _out((256,), torch.uint8, "zero", name="zero page")
        snap = snapshot(Hd, Wd, bd, zeros)
        _lib.check(_fn("vitseg_op_conv3x3_h16")(Hd.data_ptr(), Wd.data_ptr(), _p(bd), Cd.data_ptr(), zeros.data_ptr(), B, g, C, N,
                                                int(relu), int(mode == "f16"), _stream()))
    else:
        x3 = {"f32": 0, "x3": 1, "x3w": 2}[mode]
        Wk = Wd
        if x3 == 2:
            Wk = _out((N, K), name="W split")
            _lib.check(_lib.lib().vitseg_cast_params_split(Wd.data_ptr(), Wk.data_ptr(), N * K, _stream()))
        snap = snapshot(Hd, Wd, bd, Wk)
        _lib.check(_fn("vitseg_op_conv3x3_f32")(Hd.data_ptr(), Wk.data_ptr(), _p(bd), Cd.data_ptr(), B, g, C, N, int(relu), x3,
                                                _stream()))
    _after(snap, Cd)
    got = Cd.cpu().double()
    if kind == "exact":
        _small_enough(K * H.abs().max() * W.abs().max(), 8)
        assert torch.equal(got, ref)
        return
    err = (got - ref).abs()
    print(f"conv3x3 {mode} relu={relu}: max err {err.max().item():.3e}, scale {scale.max().item():.3e}")
    if mode == "f32":     # test_linear_epilogues
        assert err.max().item() < 4e-7 * scale.max().item() + 1e-6
    elif h16:             # test_linear_bf16, fp32 output: fp32 accumulation of exact products
        assert err.max().item() < 4e-7 * scale.max().item() + 1e-5
    else:                 # test_linear_f32x3_is_fp32_grade
        assert (err / (scale + 1e-3)).max().item() < 1e-6


def _takes_large_h16_kernel(B, g, C):
    """gemm_dispatch.hip route_h16, restated: the 256x128 kernel of gemm_large.hip takes an A_CONV3 GEMM at M >= 4096 and
    K >= 2048 (bf16_tiles unforced); a conv's N = 256 or the hidden size never reaches the 256x256 kernel's M >= 8192, N >= 2048"""
    assert _lib.get_option("bf16_tiles") == 0
    return B * g * g >= 4096 and 9 * C >= 2048


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["f32", "x3", "x3w", "bf16", "f16"])
@pytest.mark.parametrize("B,g,C,N", R.CONV_SHAPES)
def test_conv3x3_relu(B, g, C, N, mode, kind):
    """seg_head.0 forward (forward.hip head_conv_gemm) in fp32, both x3 modes, bf16 and IEEE half (gemm_tile.hip; the 16-bit
    form reads its padding taps from the zero page).  g = 3: every pixel is a corner, an edge or the centre, two images;
    g = 1: only the centre tap is inside; (3, 12): M = 432, image boundaries inside a row tile -- a tap must not read the
    neighbouring image; (2, 14, 192)."""
    assert not _takes_large_h16_kernel(B, g, C)
    _run_conv(B, g, C, N, True, mode, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("B,g,C,N", R.CONV_DGRAD_SHAPES)
def test_conv3x3_dgrad_form(B, g, C, N, mode, kind):
    """A_CONV3 + EPI_BIAS without a bias over 256 channels: the input gradient of seg_head.0 (vitseg_train.hip head_dgrad:
    launch_gemm_f32_bwd in fp32, launch_gemm_bf16 on the bf16 route)"""
    assert not _takes_large_h16_kernel(B, g, C)
    _run_conv(B, g, C, N, False, mode, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("relu,mode", [(True, "bf16"), (True, "f16"), (False, "bf16")])
def test_conv3x3_h16_large_kernel(relu, mode, kind):
    """The same gather in gemm_large.hip's 256x128 kernel: M = 4096, K = 2304 is the router's threshold (asserted on the shape),
    with four image boundaries inside the row tiles."""
    B, g, C, N = R.CONV_LARGE_SHAPE
    assert _takes_large_h16_kernel(B, g, C) and B * g * g == 4096
    _run_conv(B, g, C, N, relu, mode, kind)


def test_conv_dgrad_weight_then_conv_is_the_input_gradient():
    """conv_dgrad_weight_kernel's output fed to the gradient-form conv equals torch.autograd.grad of the forward conv (exact)"""
    B, g, D = 2, 3, 64
    W0, dF = R.ints(R.MID, 9 * D, lo=-2, hi=2, seed=6), R.ints(B * g * g, R.MID, lo=-4, hi=4, seed=7)
    W0d, dFd = _dev(W0, name="W0"), _dev(dF, name="dF")
    Wd, dH = _out((D, 9 * R.MID), name="Wd"), _out((B * g * g, D), name="dH")
    snap = snapshot(W0d, dFd)
    _lib.check(_fn("vitseg_op_conv_dgrad_weight")(W0d.data_ptr(), Wd.data_ptr(), D, _stream()))
    _lib.check(_fn("vitseg_op_conv3x3_f32")(dFd.data_ptr(), Wd.data_ptr(), None, dH.data_ptr(), B, g, R.MID, D, 0, 0, _stream()))
    _after(snap, Wd, dH)
    assert torch.equal(dH.cpu().double(), R.conv3x3_input_grad(dF, W0, B, g))


@pytest.mark.parametrize("D", [64, 192, 100])
def test_conv_dgrad_weight(D):
    """Wd[d][t][o] = W0[o][8 - t][d], bit for bit"""
    W0 = R.gauss(R.MID, 9 * D, seed=D)
    W0d, Wd = _dev(W0, name="W0"), _out((D, 9 * R.MID), name="Wd")
    snap = snapshot(W0d)
    _lib.check(_fn("vitseg_op_conv_dgrad_weight")(W0d.data_ptr(), Wd.data_ptr(), D, _stream()))
    _after(snap, Wd)
    assert torch.equal(_bits(Wd), _bits(R.conv_dgrad_weight(W0)))


# ============================================================ seg_head.2 and its backward
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,Np,C", R.HEAD_SHAPES)
def test_head1x1(B, Np, C, kind):
    """head1x1_kernel.  Np = 9 with two images and Np = 5 with three (rows of an image in one block of 4 rows), 197 rows, one
    class, and 40 classes (more than training allows; the forward has no cap)."""
    if kind == "exact":
        Fm, W2, b2 = R.ints(B * Np, R.MID, lo=-4, hi=4, seed=Np), R.ints(C, R.MID, lo=-2, hi=2, seed=C), R.ints(C, lo=-8, hi=8, seed=8)
    else:
        Fm, W2, b2 = R.gauss(B * Np, R.MID, seed=Np), R.gauss(C, R.MID, seed=C, scale=0.1), R.gauss(C, seed=8)
    ref = R.head1x1(Fm, W2, b2, B, Np)
    Fd, Wd, bd = _dev(Fm, name="F"), _dev(W2, name="W2"), _dev(b2, name="b2")
    Z = _out((B, C, Np), name="Z")
    snap = snapshot(Fd, Wd, bd)
    _lib.check(_fn("vitseg_op_head1x1")(Fd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), Z.data_ptr(), B, Np, C, _stream()))
    _after(snap, Z)
    got = Z.cpu().double()
    if kind == "exact":
        _small_enough(R.MID * 4 * 2, 8)
        assert torch.equal(got, ref)
        return
    # depth 9: two adds of a lane's four products, six butterfly levels of wave_sum, the bias
    terms = (Fm.abs().double() @ W2.abs().double().T + b2.abs().double()).view(B, Np, C).permute(0, 2, 1)
    err = (got - ref).abs()
    print(f"head1x1: worst err / bound {(err / ((9 + 2) * EPS24 * terms)).max().item():.3f}")
    assert (err <= (9 + 2) * EPS24 * terms).all()


def _head_bwd_inputs(B, Np, C, kind):
    M = B * Np
    if kind == "exact":
        dZ, W2 = R.ints(B, C, Np, lo=-4, hi=4, seed=Np + C), R.ints(C, R.MID, lo=-2, hi=2, seed=C)
        Fm = R.ints(M, R.MID, lo=-2, hi=4, seed=9)                  # zeros, negatives and positives
    else:
        dZ, W2 = R.gauss(B, C, Np, seed=Np + C), R.gauss(C, R.MID, seed=C, scale=0.1)
        pre = R.gauss(M, R.MID, seed=9)
        Fm = torch.where(pre > -0.5, torch.relu(pre), pre)           # ReLU output with exact zeros, and planted negatives
    assert bool((Fm == 0).any()) and bool((Fm < 0).any()) and bool((Fm > 0).any())
    return dZ, Fm, W2


def _head_bwd_call(dZ, Fm, W2, B, Np, C):
    n = _fn("vitseg_op_head1x1_bwd_scratch_floats")(B, Np, C)
    dZd, Fd, Wd = _dev(dZ, name="dZ"), _dev(Fm, name="F"), _dev(W2, name="W2")
    dF, dW, db = _out((B * Np, R.MID), name="dFpre"), _out((C, R.MID), name="dW2"), _out((C,), name="db2")
    scratch = _out((n,), name="head1x1_bwd scratch")
    snap = snapshot(dZd, Fd, Wd)
    rc = _fn("vitseg_op_head1x1_bwd")(dZd.data_ptr(), Fd.data_ptr(), Wd.data_ptr(), dF.data_ptr(), dW.data_ptr(), db.data_ptr(),
                                      scratch.data_ptr(), B, Np, C, _stream())
    _after(snap, dF, dW, db, scratch)
    return rc, dF, dW, db, scratch


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,Np,C", R.HEAD_BWD_SHAPES)
def test_head1x1_bwd(B, Np, C, kind):
    """head1x1_bwd_kernel, its colsum_finish_kernel over the blocks, head_bias_bwd_kernel.  M = 18 and 13 are no multiples of the
    8 rows of a block; 16383 / 16384 lie either side of the switch to 64 rows per block; (2, 8200, 32): two images, the most
    classes.  F holds exact zeros and negative values: the F > 0 mask on both sides of zero and at zero."""
    M = B * Np
    dZ, Fm, W2 = _head_bwd_inputs(B, Np, C, kind)
    ref_dF, ref_dW, ref_db = R.head1x1_bwd(dZ, Fm, W2, B, Np)
    rc, dF, dW, db, _ = _head_bwd_call(dZ, Fm, W2, B, Np, C)
    _lib.check(rc)
    got = [t.cpu().double() for t in (dF, dW, db)]
    if kind == "exact":
        _small_enough(M * 4 * 4)
        assert torch.equal(got[0], ref_dF) and torch.equal(got[1], ref_dW) and torch.equal(got[2], ref_db)
        return
    rows = dZ.abs().double().permute(0, 2, 1).reshape(M, C)
    rpb = 8 if M < 16384 else 64                    # backward.hip head1x1_rpb
    blocks = (M + rpb - 1) // rpb
    # dFpre: one fmaf chain over the C classes.  dW2: a chain over the block's rpb rows, then colsum_finish_kernel over the
    # blocks (finish_column) -- per group a chain of at most blocks // 64 + 3, two adds joining its four chains, the 16 groups
    # in sequence.
    # db2: per thread a chain of ceil(n / 4096), two adds joining its four chains, a ten-level tree over 1024 threads.
    depth = {"dFpre": C, "dW2": rpb + blocks // 64 + 3 + 2 + 16, "db2": -(-M // 4096) + 2 + 10}
    terms = {"dFpre": rows @ W2.abs().double(), "dW2": rows.T @ Fm.abs().double(), "db2": rows.sum(0)}
    for name, g_, r_ in zip(("dFpre", "dW2", "db2"), got, (ref_dF, ref_dW, ref_db)):
        bound = (depth[name] + 2) * EPS24 * terms[name]
        err = (g_ - r_).abs()
        print(f"head1x1_bwd {name}: depth {depth[name]}, worst err / bound {(err / bound.clamp(min=1e-300)).max().item():.3f}")
        assert (err <= bound).all(), name
    assert not got[0][Fm <= 0].any()                               # nothing flows where F <= 0


def test_head1x1_bwd_refuses_33_classes():
    """C <= 32 (the kernel keeps a class per register): VITSEG_ESHAPE from the host, nothing launched, every output still NaN"""
    B, Np, C = 1, 13, 33
    dZ, Fm, W2 = _head_bwd_inputs(B, Np, C, "exact")
    rc, dF, dW, db, scratch = _head_bwd_call(dZ, Fm, W2, B, Np, C)
    assert rc == _lib.ESHAPE
    _untouched(dF, dW, db, scratch)


# ============================================================ column sums
def _run_colsum(M, N, ld, bf16, kind):
    dt = torch.bfloat16 if bf16 else torch.float32
    X = R.ints(M, ld, lo=-4, hi=4, seed=M + N) if kind == "exact" else R.gauss(M, ld, seed=M + N).to(dt).float()
    X[:, N:] = float("nan")                                          # the columns between N and ld are not the kernel's to read
    ref = X[:, :N].double().sum(0)
    Xd = _dev(X, dt, name="X")
    out = _out((N,), name="colsum")
    scratch = _out((_lib.lib().vitseg_op_colsum_scratch_floats(M, N),), name="colsum scratch")
    snap = snapshot(Xd)
    _lib.check(_fn("vitseg_op_colsum")(Xd.data_ptr(), int(bf16), out.data_ptr(), scratch.data_ptr(), M, N, ld, _stream()))
    _after(snap, out, scratch)
    got = out.cpu().double()
    if kind == "exact":
        _small_enough(M * 4)
        assert torch.equal(got, ref)
        return
    chunks = (M + 255) // 256
    if not bf16 and M <= 4096:
        # colsum_small_kernel: a row group's chain of ceil(M / 256) rows, two adds joining its four chains, 63 adds over the
        # 64 groups in group order
        depth = chunks + 2 + 63
    else:
        # colsum_partial_kernel: a wave's 64 rows as four chains of at most 15 + 3 (one chain of 64 on the scalar path of a
        # column block's last, partial vector), two adds joining them, two joining the four waves; then colsum_finish_kernel
        # (finish_column): a chain of at most chunks // 64 + 3, two adds joining four chains, the 16 groups in sequence
        depth = (64 if N % 4 else 18) + 2 + 2 + chunks // 64 + 3 + 2 + 16
    bound = (depth + 2) * EPS24 * X[:, :N].abs().double().sum(0)
    err = (got - ref).abs()
    print(f"colsum M={M} bf16={bf16}: depth {depth}, worst err / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,N,ld", R.COLSUM_F32_SHAPES + [(4097, 70, 72)])
def test_colsum_f32(M, N, ld, kind):
    """launch_colsum on fp32: colsum_small_kernel up to M = 4096 (one row; N no multiple of the block's 16 columns, ld > N;
    257 rows; 4096), colsum_partial_kernel<float> + colsum_finish_kernel from 4097 (17 chunks, the last with one row); 4353 rows:
    18 chunks, the last with one row, ld > N.  Added: (4097, 70, 72) -- N % 4 != 0 is the only way into the partial kernel's
    scalar branch (a column block's last vector is cut by N), which no listed shape reaches."""
    _run_colsum(M, N, ld, False, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,N,ld", R.COLSUM_BF16_SHAPES)
def test_colsum_bf16(M, N, ld, kind):
    """colsum_partial_kernel<bf16> + colsum_finish_kernel at any M: one chunk short of a row, one whole chunk with ld > N, three
    chunks over nine column blocks"""
    _run_colsum(M, N, ld, True, kind)


def test_colsum_refuses_a_misaligned_leading_dimension():
    """the kernels read four adjacent columns as one vector: ld % 4 != 0 is VITSEG_ESHAPE on the host, nothing launched"""
    M, N, ld = 63, 20, 22
    Xd = _dev(R.ints(M, ld, lo=-4, hi=4, seed=1), name="X")
    out, scratch = _out((N,), name="colsum"), _out((_lib.lib().vitseg_op_colsum_scratch_floats(M, N),), name="colsum scratch")
    assert _fn("vitseg_op_colsum")(Xd.data_ptr(), 0, out.data_ptr(), scratch.data_ptr(), M, N, ld, _stream()) == _lib.ESHAPE
    _untouched(out, scratch)


# ============================================================ embeddings backward
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,Np,D", R.EMBED_BWD_SHAPES)
def test_embed_bwd(B, Np, D, kind):
    """embed_bwd_kernel: dpos[1 + t] sums the patch rows b * Np + t, dpos[0] = dcls sums the CLS rows B * Np + b.  One image;
    three; D = 100 (a block of 256 threads spans rows of dpos)."""
    dX = R.ints(B * (Np + 1), D, lo=-4, hi=4, seed=Np) if kind == "exact" else R.gauss(B * (Np + 1), D, seed=Np)
    ref_pos, ref_cls = R.embed_bwd(dX, B, Np)
    dXd = _dev(dX, name="dX")
    dpos, dcls = _out((Np + 1, D), name="dpos"), _out((D,), name="dcls")
    snap = snapshot(dXd)
    _lib.check(_fn("vitseg_op_embed_bwd")(dXd.data_ptr(), dpos.data_ptr(), dcls.data_ptr(), B, Np, D, _stream()))
    _after(snap, dpos, dcls)
    assert torch.equal(_bits(dpos[0]), _bits(dcls))
    if kind == "exact":
        _small_enough(B * 4)
        assert torch.equal(dpos.cpu().double(), ref_pos) and torch.equal(dcls.cpu().double(), ref_cls)
        return
    # depth B: one chain over the images
    terms = torch.cat([dX[B * Np:].abs().double().sum(0, keepdim=True), dX[:B * Np].abs().double().view(B, Np, D).sum(0)])
    assert ((dpos.cpu().double() - ref_pos).abs() <= (B + 2) * EPS24 * terms).all()


# ============================================================ data movement: bit for bit
@pytest.mark.parametrize("src", ["f32", "bf16", "bf16_to_bf16"])
@pytest.mark.parametrize("B,g,D", R.IM2COL3_SHAPES)
def test_im2col3x3(B, g, D, src):
    """im2col3x3_kernel<float>, <bf16> (fp32 rows of a bf16 map) and im2col3x3_bf16_kernel: corners, edges and centre at g = 3,
    a single pixel, image boundaries inside a block at (3, 12), D = 8 and 72 (no multiple of 64)"""
    dt = torch.float32 if src == "f32" else torch.bfloat16
    H = R.gauss(B * g * g, D, seed=g + D).to(dt)
    ref = R.im2col3x3(H.float(), B, g).to(dt if src == "bf16_to_bf16" else torch.float32)
    Hd = _dev(H, name="H")
    T = _out((B * g * g, 9 * D), ref.dtype, name="T")
    snap = snapshot(Hd)
    if src == "bf16_to_bf16":
        _lib.check(_fn("vitseg_op_im2col3x3_bf16")(Hd.data_ptr(), T.data_ptr(), B, g, D, _stream()))
    else:
        _lib.check(_fn("vitseg_op_im2col3x3")(Hd.data_ptr(), int(src == "bf16"), T.data_ptr(), B, g, D, _stream()))
    _after(snap, T)
    assert torch.equal(_bits(T), _bits(ref))


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("B,Cin,P,g", R.IM2COL_PATCH_SHAPES)
def test_im2col_patch(B, Cin, P, g, bf16):
    """im2col_patch_kernel and im2col_patch_bf16_kernel (against .bfloat16(): round to nearest even, with values planted
    exactly halfway between two bf16 numbers, kept bit even and odd)"""
    S = g * P
    img = R.gauss(B, Cin, S, S, seed=P + g)
    ties = R.bf16_ties(32, seed=P)
    img.view(-1)[torch.randperm(img.numel(), generator=torch.Generator().manual_seed(P))[:32]] = ties
    ref = R.im2col_patch(img, P)
    if bf16:
        ref = ref.bfloat16()
    imgd = _dev(img, name="img")
    T = _out(tuple(ref.shape), ref.dtype, name="T")
    snap = snapshot(imgd)
    _lib.check(_fn("vitseg_op_im2col_patch_bf16" if bf16 else "vitseg_op_im2col_patch")(imgd.data_ptr(), T.data_ptr(), B, Cin, S, P,
                                                                                     _stream()))
    _after(snap, T)
    assert torch.equal(_bits(T), _bits(ref))


@pytest.mark.parametrize("Rr,C,ldin,Rpad", R.TRANSPOSE_SHAPES)
def test_transpose_bf16(Rr, C, ldin, Rpad):
    """transpose_bf16_kernel: whole 64x64 tiles; ragged in both directions with ldin > C and two tiles of padding; 197 rows
    padded to 256; 9 x 8.  The output starts as NaN: every element at r >= R must come out as bit zero."""
    x = R.gauss(Rr, ldin, seed=Rr + C).bfloat16()
    x[:, C:] = float("nan")
    xd = _dev(x, name="in")
    out = _out((C, Rpad), torch.bfloat16, name="out")
    snap = snapshot(xd)
    _lib.check(_fn("vitseg_op_transpose_bf16")(xd.data_ptr(), out.data_ptr(), Rr, C, ldin, Rpad, _stream()))
    _after(snap, out)
    assert torch.equal(_bits(out), _bits(R.transpose_pad(x, C, Rpad)))
    assert not _bits(out)[:, Rr:].any()


@pytest.mark.parametrize("L,D,I", R.TRANSPOSE_LAYERS_SHAPES)
def test_transpose_layers_bf16(L, D, I):
    """transpose_layers_bf16_kernel: [3D, D] [D, D] [I, D] [D, I] of every layer in one launch, from an arena with NaN gaps
    between the matrices and a layer stride larger than their sum, into the dense output; D = 72, I = 136: no multiples of 64"""
    Rs, Cs = [3 * D, D, I, D], [D, D, D, I]
    gap = 24
    src0, off = [], 8
    for r, c in zip(Rs, Cs):
        src0.append(off)
        off += r * c + gap
    stride = off + 40
    arena = torch.full((L * stride,), float("nan"), dtype=torch.bfloat16)
    ref = []
    for l in range(L):
        for k, (r, c) in enumerate(zip(Rs, Cs)):
            m = R.gauss(r, c, seed=10 * l + k).bfloat16()
            arena[l * stride + src0[k]: l * stride + src0[k] + r * c] = m.view(-1)
            ref.append(m.t().contiguous().view(-1))
    ref = torch.cat(ref)
    ad = _dev(arena, name="arena")
    out = _out((ref.numel(),), torch.bfloat16, name="out")
    snap = snapshot(ad)
    _lib.check(_fn("vitseg_op_transpose_layers_bf16")(ad.data_ptr(), out.data_ptr(), (ctypes.c_size_t * 4)(*src0),
                                                      (ctypes.c_int * 4)(*Rs), (ctypes.c_int * 4)(*Cs), stride, L, _stream()))
    _after(snap, out)
    assert torch.equal(_bits(out), _bits(ref))


@pytest.mark.parametrize("mode", ["in_place", "f32", "bf16"])
@pytest.mark.parametrize("rows,cols,p", R.DROPOUT_SHAPES)
def test_dropout_rows(rows, cols, p, mode):
    """dropout_rows_kernel<float> (in place and out of place) and <bf16>: the mask of tests/dropout_ref.py at (stream, row, col),
    one fp32 multiply by the scale, then for bf16 one rounding.  4100 x 1024: more than one pass of the 4096-block grid."""
    seed, stream_id = 0x1234ABCD, 11
    src = R.gauss(rows, cols, seed=rows)
    ref = torch.from_numpy(R.dropout_rows(src, p, seed, stream_id))
    keep, _, thresh = R.dropout_keep(rows, cols, p, seed, stream_id)
    sd = _dev(src, name="src")
    dst = sd if mode == "in_place" else _out((rows, cols), torch.bfloat16 if mode == "bf16" else torch.float32, name="dst")
    snap = snapshot(*([] if mode == "in_place" else [sd]))
    _lib.check(_fn("vitseg_op_dropout_rows")(sd.data_ptr(), dst.data_ptr(), int(mode == "bf16"), rows, cols, p, seed, stream_id,
                                             _stream()))
    _after(snap, dst)
    assert torch.equal(_bits(dst), _bits(ref.bfloat16() if mode == "bf16" else ref))
    # the kept fraction of the kernel's output within 5 standard deviations of 1 - thresh / 65536
    q, n = 1.0 - thresh / 65536.0, rows * cols
    assert bool((src != 0).all())
    kept = float((dst.float() != 0).sum()) / n
    assert abs(kept - q) <= 5 * (q * (1 - q) / n) ** 0.5, (kept, q)
    assert np.array_equal((dst.float() != 0).cpu().numpy(), keep)


def test_dropout_rows_refuses_p_zero():
    """p = 0 is "no dropout" at every call site, which then launches nothing: VITSEG_EINVAL, nothing launched"""
    sd, dst = _dev(R.gauss(5, 64, seed=1), name="src"), _out((5, 64), name="dst")
    assert _fn("vitseg_op_dropout_rows")(sd.data_ptr(), dst.data_ptr(), 0, 5, 64, 0.0, 1, 2, _stream()) == _lib.EINVAL
    _untouched(dst)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("rows,D", [(7, 192), (1025, 768), (33, 1024), (5, 2048), (9, 512)])
def test_layernorm_h16(rows, D, fmt):
    """layernorm_kernel<bf16 | f16>: test_layernorm's shapes, inputs and fp32 bound (5e-6), plus half a unit in the last place
    of the output type at |ref| for the one rounding"""
    dt = H16[fmt]
    x, w, b = R.gauss(rows, D, seed=1, scale=3.0) + 0.5, R.gauss(D, seed=2) + 1.0, R.gauss(D, seed=3)
    ref = O.layer_norm(x.double(), w.double(), b.double(), 1e-12)
    xd, wd, bd = _dev(x, name="x"), _dev(w, name="w"), _dev(b, name="b")
    y = _out((rows, D), dt, name="y")
    snap = snapshot(xd, wd, bd)
    _lib.check(_fn("vitseg_op_layernorm_h16")(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), rows, D, 1e-12,
                                              1 if fmt == "bf16" else 2, _stream()))
    _after(snap, y)
    err = (y.cpu().double() - ref).abs()
    assert (err <= 5e-6 + R.half_ulp(ref, dt)).all(), (err - R.half_ulp(ref, dt)).max().item()
