"""CPU (-m "not gpu"): the window grid of sliding-window inference (vitseg_window_count / vitseg_window_origins: host
arithmetic of the C ABI) against the formula, and the CPU restatement of the blend (tests/window_ref.py) against the two
cases whose answer is known without it."""
import ctypes as C

import pytest
import torch

import window_ref as R
from oracle import vitseg_oracle as O
from visiontransformer_amd import _lib


def _count(extent, S, stride):
    return int(_lib.window_symbol("vitseg_window_count")(extent, S, stride))


def test_window_grid_matches_the_formula_over_a_sweep():
    fo = _lib.window_symbol("vitseg_window_origins")
    buf = (C.c_int32 * 256)()
    cases = 0
    for S in (16, 64):
        for stride in range(1, S + 1):
            for extent in range(S, 201):
                n = _count(extent, S, stride)
                assert n == R.count(extent, S, stride) == 1 + (extent - S + stride - 1) // stride, (extent, S, stride)
                assert fo(extent, S, stride, buf) == _lib.OK
                o = list(buf[:n])
                assert o == R.origins(extent, S, stride) == _lib.window_origins(extent, S, stride), (extent, S, stride)
                assert o[0] == 0 and o[-1] + S == extent                         # starts at 0, the last window ends at the edge
                assert all(0 <= b - a <= stride for a, b in zip(o, o[1:]))       # successive origins differ by at most stride
                assert all(b <= a + S for a, b in zip(o, o[1:]))                 # ... so no pixel lies between two windows
                covered = [False] * extent
                for a in o:
                    covered[a:a + S] = [True] * S
                assert all(covered), (extent, S, stride)
                cases += 1
            for extent in range(1, S):                                           # shorter than the window
                assert _count(extent, S, stride) == _lib.ESHAPE
    assert cases == sum(S * (201 - S) for S in (16, 64))


@pytest.mark.parametrize("extent,S,stride,word", [(63, 64, 48, "shorter"), (100, 64, 0, "stride"), (100, 64, 65, "stride"),
                                                  (16385, 64, 48, "16384")])
def test_window_grid_errors_are_eshape_with_a_message(extent, S, stride, word):
    buf = (C.c_int32 * 4)(7, 7, 7, 7)
    for rc in (_count(extent, S, stride), int(_lib.window_symbol("vitseg_window_origins")(extent, S, stride, buf))):
        assert rc == _lib.ESHAPE
        assert word in _lib.lib().vitseg_last_error().decode()
    assert list(buf) == [7, 7, 7, 7]                                             # nothing is written on an error
    with pytest.raises(ValueError, match=word):
        _lib.window_origins(extent, S, stride)
    assert _count(16384, 64, 48) == 1 + -(-(16384 - 64) // 48)                   # the limit itself is accepted


@pytest.mark.parametrize("kind", ["uniform", "linear"])
def test_reference_blend_of_one_tile_is_the_plain_upsample(kind):
    g = torch.Generator().manual_seed(5)
    S = 64
    z = torch.randn((2, 3, 4, 4), generator=g)
    got = R.blend(z, 2, S, S, S, [0], [0], R.weights(kind, S))
    assert torch.equal(got, O.upsample_bilinear(z, (S, S)))
    assert torch.equal(R.mask(got), O.predict_mask(O.upsample_bilinear(z, (S, S))).to(torch.uint8))


def test_reference_blend_of_equal_tiles_with_uniform_weights_returns_their_value():
    """Two overlapping tiles that hold the same value v at every pixel: acc = v, then fma(1, v, v) = 2 v; ws = 2; 2 v / 2 = v.
    The maps are constant per class with values whose bilinear interpolation is exact (c * l + c * (1 - l) with l a
    multiple of 1 / 32 and c of two significant bits)."""
    S, W = 64, 96
    ox = R.origins(W, S, 32)
    assert ox == [0, 32]
    vals = torch.tensor([0.75, -1.5, 3.0])
    z = vals.view(1, 3, 1, 1).expand(2, 3, 4, 4).contiguous()
    got = R.blend(z, 1, S, W, S, [0], ox, R.weights("uniform", S))
    assert torch.equal(got, vals.view(1, 3, 1, 1).expand(1, 3, S, W))
    # the triangular window weighs the two tiles differently but normalises: the value comes back to rounding
    lin = R.blend(z, 1, S, W, S, [0], ox, R.weights("linear", S))
    assert float((lin - got).abs().max()) <= 4e-7


def test_fma_rn_rounds_once_where_the_fp64_sum_is_an_fp32_midpoint():
    """a b = 64 - 2^-40 exactly and c = 2^30 + 128 (odd significand): the fp64 sum loses the 2^-40 and lands on the midpoint
    2^30 + 192, which a second rounding takes to the even neighbour 2^30 + 256; one rounding of the exact sum, which lies
    below the midpoint, gives 2^30 + 128 -- what a hardware fma returns."""
    a = torch.tensor([8.0 * (1 + 2.0 ** -23)], dtype=torch.float32)
    b = torch.tensor([8.0 * (1 - 2.0 ** -23)], dtype=torch.float32)
    c = torch.tensor([2.0 ** 30 + 128], dtype=torch.float32)
    assert float(O._fma(a, b, c)) == 2.0 ** 30 + 256
    assert float(R.fma_rn(a, b, c)) == 2.0 ** 30 + 128
    # 64 - 2^-40 - (2^30 + 128): the fp64 sum is the midpoint -(2^30 + 64), the exact sum lies beyond it
    assert float(O._fma(a, b, -c)) == -(2.0 ** 30) and float(R.fma_rn(a, b, -c)) == -(2.0 ** 30 + 128)
    assert float(R.fma_rn(-a, b, -c)) == -(2.0 ** 30 + 128)             # mirrored
    x = torch.randn(1000, generator=torch.Generator().manual_seed(1))
    assert torch.equal(R.fma_rn(x, x.flip(0), x * 3), O._fma(x, x.flip(0), x * 3))
