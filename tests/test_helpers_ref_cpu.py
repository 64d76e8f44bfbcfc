"""CPU: the fp64 references of tests/helpers_ref.py, checked among themselves at the shapes tests/test_gpu_helpers.py uses -- a
wrong reference (a tap order, a row layout, a flipped weight) is found here, without a GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers_ref as R


@pytest.mark.parametrize("B,g,C,N", R.CONV_SHAPES + R.CONV_DGRAD_SHAPES)
def test_unfold_then_matmul_is_the_conv(B, g, C, N):
    """im2col3x3 (k = (ky, kx, d)) times the [N, 9 C] weight equals conv2d: the gather, the weight layout and the token-major
    row order agree.  Integers: both sides are exact."""
    H, W, bias = R.ints(B * g * g, C, lo=-4, hi=4, seed=1), R.ints(N, 9 * C, lo=-2, hi=2, seed=2), R.ints(N, lo=-8, hi=8, seed=3)
    ref = R.conv3x3(H, W, bias, B, g, False)
    assert torch.equal(R.im2col3x3(H, B, g).double() @ W.double().T + bias.double(), ref)
    assert torch.equal(R.conv3x3(H, W, bias, B, g, True), ref.clamp(min=0))
    # the centre tap of every row is the row itself; the first tap of the first pixel of every image is padding
    T = R.im2col3x3(H, B, g).view(B, g * g, 9, C)
    assert torch.equal(T[:, :, 4].reshape(-1, C), H) and not T[:, 0, 0].any()


@pytest.mark.parametrize("B,Cin,P,g,D", R.PATCH_SHAPES)
def test_patch_rows_times_weight_is_the_patch_embedding(B, Cin, P, g, D):
    img, Wp = R.ints(B, Cin, g * P, g * P, lo=-4, hi=4, seed=4), R.ints(D, Cin * P * P, lo=-2, hi=2, seed=5)
    bp, pos, cls = R.ints(D, lo=-8, hi=8, seed=6), R.ints(g * g + 1, D, lo=-8, hi=8, seed=7), R.ints(D, lo=-8, hi=8, seed=8)
    X = R.patch_embed(img, Wp, bp, pos, cls, P)
    Np = g * g
    rows = R.im2col_patch(img, P).double() @ Wp.double().T + bp.double() + pos.double()[1:].repeat(B, 1)
    assert torch.equal(X[:B * Np], rows)
    assert torch.equal(X[B * Np:], (cls + pos[0]).double().expand(B, D))
    # patch (b, gy, gx) is row b * Np + gy * g + gx, and its first value is the image's pixel (gy P, gx P) of channel 0
    T = R.im2col_patch(img, P).view(B, g, g, -1)
    assert torch.equal(T[..., 0], img[:, 0, ::P, ::P])


@pytest.mark.parametrize("B,g,C,N", R.CONV_DGRAD_SHAPES + [(2, 3, 256, 256)])
def test_flipped_weight_conv_is_the_input_gradient(B, g, C, N):
    """(here C = the forward conv's output channels = the gradient conv's input channels, N = the hidden size)"""
    W0, dF = R.ints(C, 9 * N, lo=-2, hi=2, seed=9), R.ints(B * g * g, C, lo=-4, hi=4, seed=10)
    Wd = R.conv_dgrad_weight(W0)
    assert Wd.shape == (N, 9 * C)
    assert torch.equal(R.conv3x3(dF, Wd, None, B, g, False), R.conv3x3_input_grad(dF, W0, B, g))
    d, t, o = 3, 1, 5
    assert Wd.view(N, 9, C)[d, t, o] == W0.view(C, 9, N)[o, 8 - t, d]


@pytest.mark.parametrize("B,Np,C", R.HEAD_SHAPES + R.HEAD_BWD_SHAPES[:2])
def test_head1x1_and_its_backward(B, Np, C):
    Fm, W2, b2 = R.ints(B * Np, R.MID, lo=-3, hi=4, seed=11), R.ints(C, R.MID, lo=-2, hi=2, seed=12), R.ints(C, lo=-8, hi=8, seed=13)
    Z = R.head1x1(Fm, W2, b2, B, Np)
    manual = (Fm.double() @ W2.double().T + b2.double()).view(B, Np, C).permute(0, 2, 1)
    assert torch.equal(Z, manual)
    dZ = R.ints(B, C, Np, lo=-4, hi=4, seed=14)
    dF, dW, db = R.head1x1_bwd(dZ, Fm, W2, B, Np)
    dz_rows = dZ.double().permute(0, 2, 1).reshape(B * Np, C)
    assert torch.equal(dF, (dz_rows @ W2.double()) * (Fm > 0))
    assert torch.equal(dW, dz_rows.T @ Fm.double()) and torch.equal(db, dz_rows.sum(0))


@pytest.mark.parametrize("B,Np,D", R.EMBED_BWD_SHAPES)
def test_embed_bwd(B, Np, D):
    dX = R.ints(B * (Np + 1), D, lo=-4, hi=4, seed=15)
    dpos, dcls = R.embed_bwd(dX, B, Np)
    assert torch.equal(dcls, dX[B * Np:].double().sum(0)) and torch.equal(dpos[0], dcls)
    assert torch.equal(dpos[1:], dX[:B * Np].double().view(B, Np, D).sum(0))


def test_dropout_transpose_and_rounding_helpers():
    keep, scale, thresh = R.dropout_keep(197, 192, 0.5, 0x1234ABCD, 13)
    assert thresh == 32768 and scale == np.float32(2.0) and abs(keep.mean() - 0.5) < 5 * (0.25 / keep.size) ** 0.5
    x = R.gauss(197, 192, seed=16)
    out = R.dropout_rows(x, 0.5, 0x1234ABCD, 13)
    assert np.array_equal(out != 0, keep & (x.numpy() != 0)) and np.array_equal(out[keep], x.numpy()[keep] * np.float32(2.0))
    t = R.transpose_pad(torch.arange(12.).view(3, 4), 2, 5)
    assert t.tolist() == [[0, 4, 8, 0, 0], [1, 5, 9, 0, 0]]
    ref = torch.tensor([1.0, 1.5, 0.75, 3.0, 1e-3], dtype=torch.float64)
    assert R.half_ulp(ref, torch.bfloat16).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -9, 2.0 ** -7, 2.0 ** -18]
    assert R.half_ulp(ref, torch.float16).tolist() == [2.0 ** -11, 2.0 ** -11, 2.0 ** -12, 2.0 ** -10, 2.0 ** -21]
    for dt in (torch.bfloat16, torch.float16):     # rounding to nearest never moves a value by more than that
        v = R.gauss(4096, seed=17).double()
        assert ((v.to(dt).double() - v).abs() <= R.half_ulp(v, dt)).all()
    ties = R.bf16_ties(64, seed=18)
    up, down = (ties.view(torch.int32) + 0x8000).view(torch.float32), (ties.view(torch.int32) - 0x8000).view(torch.float32)
    got = ties.bfloat16().float()
    even_down = ((down.view(torch.int32) >> 16) & 1) == 0
    assert torch.equal(got, torch.where(even_down, down, up)) and bool(even_down.any()) and bool((~even_down).any())
