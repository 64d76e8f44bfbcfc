"""CPU (-m "not gpu"): test-time augmentation -- the view algebra, the presets and the view order (visiontransformer_amd/tta.py),
the exact view matrices (vitseg_tta_affine + vitseg_augment_matrix: host arithmetic of the C ABI) through the numpy restatement
of the augmentation kernel, the CPU restatement of the merge (tests/tta_ref.py) on the cases whose answer is known without
it, and the argument errors of the Python surface."""
import ctypes as C

import numpy as np
import pytest
import torch

import augment_ref as A
import tta_ref as R
from oracle import vitseg_oracle as O
from visiontransformer_amd import _lib, tta
from visiontransformer_amd.model import ViTSegmentationModel


def test_unview_inverts_view_for_all_eight_ops():
    x = torch.arange(25.0).view(1, 1, 5, 5) ** 2 + torch.arange(5.0)      # no symmetry under any flip or turn
    seen = set()
    for op in range(8):
        v = R.view(x, op)
        assert torch.equal(R.unview(v, op), x) and torch.equal(R.view(R.unview(x, op), op), x)
        seen.add(tuple(v.flatten().tolist()))
    assert len(seen) == 8                                                 # eight different views: the whole group
    assert torch.equal(R.view(x, 4), torch.flip(x, [-1]))                 # op 4 the horizontal flip,
    assert torch.equal(R.view(x, 6), torch.flip(x, [-2]))                 # op 6 the vertical flip,
    assert torch.equal(R.view(x, 2), torch.flip(x, [-2, -1]))             # op 2 the half turn


def test_presets_and_view_order():
    assert tta.parse_ops("none") == (0,) and tta.parse_ops("hflip") == (0, 4)
    assert tta.parse_ops("flip") == (0, 2, 4, 6) and tta.parse_ops("d4") == tuple(range(8))
    assert tta.parse_ops((6, 1, 1)) == (1, 6) and tta.parse_ops(3) == (3,)
    assert tta.view_list("hflip", None, None, 224, 16) == [(0, 224, 1.0), (4, 224, 1.0)]
    # size-major in the order given, ops increasing within a size, one weight per size
    assert tta.view_list("hflip", (224, 160), (1, 0.5), 224, 16) == [(0, 224, 1.0), (4, 224, 1.0), (0, 160, 0.5), (4, 160, 0.5)]
    assert len(tta.view_list("d4", (160, 224), None, 224, 16)) == 16
    assert tta.parse_sizes("160,224") == (160, 224) and tta.parse_sizes(None) is None and tta.parse_sizes("") is None


def _matrix(op, src, dst):
    aff = (C.c_double * 6)()
    assert _lib.tta_symbol("vitseg_tta_affine")(op, aff) == _lib.OK
    assert list(aff) == _lib.tta_affine(op)
    return np.array(_lib.augment_matrix(list(aff), (src, src), (dst, dst)), np.int64)


@pytest.mark.parametrize("S", [8, 12])
@pytest.mark.parametrize("op", range(8))
def test_view_matrices_are_bit_exact_permutations_in_both_source_formats(op, S):
    M = _matrix(op, S, S)
    assert all(int(v) % 65536 in (0, 32768) for v in M)                   # whole pixels (the offsets: half pixels)
    rng = np.random.RandomState(10 * S + op)
    x = rng.rand(2, 3, S, S).astype(np.float32)
    u8 = rng.randint(0, 256, (2, S, S, 3)).astype(np.uint8)
    tab = np.stack([M, M])
    got, _ = A.augment(x, tab, S, S, border=A.EDGE)
    assert np.array_equal(got.view(np.int32), R.view(torch.from_numpy(x), op).numpy().view(np.int32))
    got8, _ = A.augment(u8, tab, S, S, border=A.EDGE)
    # what vitseg_preprocess_u8 ends with: one correctly rounded division by 255
    exp8 = R.view(torch.from_numpy(u8).permute(0, 3, 1, 2).float().div(255), op).numpy()
    assert np.array_equal(got8.view(np.int32), exp8.view(np.int32))


def test_tta_affine_refuses_a_bad_op_and_writes_nothing():
    aff = (C.c_double * 6)(*[7.0] * 6)
    for op in (-1, 8):
        assert _lib.tta_symbol("vitseg_tta_affine")(op, aff) == _lib.EINVAL
        assert "op" in _lib.lib().vitseg_last_error().decode()
        with pytest.raises(ValueError, match="op"):
            _lib.tta_affine(op)
    assert list(aff) == [7.0] * 6
    assert _lib.tta_symbol("vitseg_tta_affine")(0, None) == _lib.EINVAL


@pytest.mark.parametrize("mode", [R.LOGITS, R.PROBS])
def test_reference_with_one_identity_view_is_the_plain_upsample(mode):
    z = torch.randn((2, 3, 4, 4), generator=torch.Generator().manual_seed(5))
    up = O.upsample_bilinear(z, (64, 64))
    got = R.blend([(z, 0, 0.37)], 64, mode)                               # (the weight of a single view plays no part)
    assert torch.equal(got, up if mode == R.LOGITS else O.sigmoid_aten(up))
    assert torch.equal(R.mask(got, mode), O.predict_mask(up).to(torch.uint8))


def test_reference_of_a_view_and_its_own_unview_returns_the_value():
    """Two views that hold the same picture: z in the image's frame and view(z, op) in the view's frame upsample to the same
    values wherever the bilinear taps are symmetric; with constant class planes every tap is exact, so the weighted mean of
    equal values v with the weights 1, 2, 1 is fma(1, v, fma(2, v, v)) / 4 = v exactly."""
    vals = torch.tensor([0.75, -1.5, 3.0])
    z = vals.view(1, 3, 1, 1).expand(2, 3, 4, 4).contiguous()
    for op in range(8):
        got = R.blend([(z, 0, 1.0), (R.view(z, op).contiguous(), op, 2.0), (z, op, 1.0)], 64, R.LOGITS)
        assert torch.equal(got, vals.view(1, 3, 1, 1).expand(2, 3, 64, 64))
    assert float(R.weight_sum([1.0, 0.5, 2.0, 3.0])) == 6.5


def test_exports():
    assert _lib.TTA_EXPORTS == ["vitseg_tta_affine", "vitseg_tta_blend"]
    assert set(_lib.TTA_EXPORTS) <= set(_lib.EXPORTS)
    for name in _lib.TTA_EXPORTS:
        assert _lib.tta_symbol(name) is not None
    assert C.sizeof(_lib.CTTAView) == 24                                  # pointer, two int32, float, padded to 8


def test_value_errors_of_the_python_surface():
    m = ViTSegmentationModel(2, 16, 64, 1, 1, image_size=32, intermediate_size=128).eval()
    x = torch.zeros((1, 3, 32, 32))
    for bad, word in ((dict(x=torch.zeros((1, 3, 32, 48))), "square"),
                      (dict(x=torch.zeros((1, 32, 48, 3), dtype=torch.uint8)), "square"),
                      (dict(sizes=(40,)), "patch size"), (dict(sizes=(0,)), "patch size"), (dict(sizes=(-16,)), "patch size"),
                      (dict(x=torch.zeros((1, 3, 40, 40))), "patch size"),     # the default size is the input's own
                      (dict(tta="d8"), "preset"), (dict(tta=(0, 8)), "op"), (dict(tta=(-1,)), "op"),
                      (dict(weights=(0.0,)), "weight"), (dict(weights=(-1.0,)), "weight"),
                      (dict(weights=(float("nan"),)), "weight"), (dict(sizes=(32, 16), weights=(1.0,)), "weights"),
                      (dict(tta="d4", sizes=(16, 32, 48)), "views"), (dict(merge="mean"), "merge")):
        kw = dict(x=x)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            m.predict_mask_tta(**kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):             # valid arguments: only the device is missing
        m.predict_mask_tta(x, tta="hflip", sizes=(16, 32), weights=(1, 2))


def test_predict_refuses_tta_inside_sliding_windows():
    from visiontransformer_amd.predict import predict
    m = ViTSegmentationModel(2, 16, 64, 1, 1, image_size=32, intermediate_size=128).eval()
    with pytest.raises(ValueError, match="sliding"):
        predict(np.zeros((40, 40, 3), np.uint8), m, tta="flip", sliding=True)
