"""GPU (-m gpu): test-time augmentation -- vitseg_tta_blend through the C ABI on guard-banded buffers, bit for bit against the
CPU restatement tests/tta_ref.py; the view images of the augmentation launch against torch's flips and turns; and
ViTSegmentationModel.predict_mask_tta / predict(..., tta=...) against predict_mask, the restatement and the oracle."""
import functools

import numpy as np
import pytest
import torch

import augment_ref as A
import tta_ref as R
from guard import check, guarded, snapshot, unchanged
from oracle import vitseg_oracle as O
from test_gpu_forward import TOL_LOGITS
from util import Golden
from visiontransformer_amd import _lib
from visiontransformer_amd.model import ViTSegmentationModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 2
MODES = [R.LOGITS, R.PROBS]


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ----------------------------------------------------------------------------------------------------------------- blend
def _descs(views):
    return (_lib.CTTAView * len(views))(*[_lib.CTTAView(z.data_ptr(), int(z.shape[-1]), op, w) for z, op, w in views])


def _blend(views, Cc, S, mode, want_merged, want_mask):
    merged = guarded((N, Cc, S, S), name="merged") if want_merged else None
    mask = guarded((N, S, S), torch.uint8, name="mask") if want_mask else None
    _lib.check(_lib.tta_symbol("vitseg_tta_blend")(_descs(views), len(views), N, Cc, S, mode,
                                                   None if merged is None else merged.data_ptr(),
                                                   None if mask is None else mask.data_ptr(), _stream()))
    torch.cuda.synchronize()
    check(merged, mask)
    return merged, mask


def _maps(spec, Cc, seed):
    """spec: [(g, op, weight)] -> [(lowres fp32 [N, C, g, g] on the CPU, op, weight)]"""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for g, op, w in spec:
        out.append((torch.randn((N, Cc, g, g), generator=gen), op, w))
    return out


def _blend_case(cpu_views, Cc, S, mode, label):
    ref = R.blend(cpu_views, S, mode)
    ref_mask = R.mask(ref, mode)
    views = [(guarded(z.shape, fill=z.to(DEV), name=f"lowres {k}"), op, w) for k, (z, op, w) in enumerate(cpu_views)]
    snap = snapshot(*[v[0] for v in views])
    merged, mask = _blend(views, Cc, S, mode, True, True)
    check(*[v[0] for v in views])
    unchanged(snap)
    bad = int((merged.cpu().view(torch.int32) != ref.view(torch.int32)).sum())
    print(f"{label} mode {mode}: {bad} of {ref.numel()} merged values differ from the reference in bits, "
          f"{int((mask.cpu() != ref_mask).sum())} mask pixels differ")
    assert bad == 0
    assert torch.equal(mask.cpu(), ref_mask)
    only_m, _ = _blend(views, Cc, S, mode, True, False)
    _, only_k = _blend(views, Cc, S, mode, False, True)
    assert torch.equal(only_m.view(torch.int32), merged.view(torch.int32)) and torch.equal(only_k, mask)
    return ref


W4 = (1.0, 0.5, 2.0, 3.0)
CASES = {
    # (a) all eight ops on one grid, S a multiple of 4: the 16-byte store path
    "a_eight_ops": (3, 48, [(3, op, 1.0) for op in range(8)]),
    # (b) g does not divide S, S % 4 != 0 (element stores, a partly filled block), three grids x four ops, unequal weights
    "b_mixed_grids": (3, 37, [(g, op, w) for g in (2, 3, 5) for op, w in zip((0, 4, 1, 6), W4)]),
    # (c) one class and seventeen (five class chunks, the last one short)
    "c_one_class": (1, 32, [(2, op, w) for op, w in zip((0, 3, 4, 6), W4)]),
    "c_seventeen_classes": (17, 32, [(2, op, w) for op, w in zip((0, 3, 4, 6), W4)]),
    # (e) the most views one launch takes
    "e_sixteen_views": (2, 32, [(g, op, 1.0 + 0.25 * op) for g in (2, 4) for op in range(8)]),
    # more than one block along x: a second, partly filled block on either store path, and the 256-thread-wide block
    "f_two_blocks_vec": (2, 260, [(4, op, w) for op, w in zip((0, 1, 4, 7), W4)]),
    "f_two_blocks_scalar": (2, 257, [(4, op, w) for op, w in zip((0, 1, 4, 7), W4)]),
    "f_wide_block": (2, 1028, [(4, 1, 1.0), (6, 6, 2.0)]),
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_blend_matches_the_reference_bit_for_bit(case, mode):
    Cc, S, spec = CASES[case]
    _blend_case(_maps(spec, Cc, 7 + len(spec) + S), Cc, S, mode, case)


@pytest.mark.parametrize("mode", MODES)
def test_blend_of_one_view_for_every_op(mode):
    """(d) K = 1: the view's own value, the weight plays no part."""
    for op in range(8):
        ref = _blend_case(_maps([(5, op, 0.37)], 3, 40 + op), 3, 40, mode, f"d_single_op{op}")
        z = _maps([(5, op, 0.37)], 3, 40 + op)[0][0]
        up = R.unview(O.upsample_bilinear(z, (40, 40)), op)
        assert torch.equal(ref, up if mode == R.LOGITS else O.sigmoid_aten(up))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["twin_planes", "zeros", "saturated"])
def test_blend_ties_and_saturation_give_the_first_index(kind, mode):
    spec = [(3, op, w) for op, w in zip((0, 5, 2, 6), W4)]
    views = _maps(spec, 3, 99)
    if kind == "twin_planes":      # classes 1 and 2 hold the same numbers in every view: wherever they lead, 1 must win
        for z, _, _ in views:
            z[:, 2] = z[:, 1]
    elif kind == "zeros":
        views = [(torch.zeros_like(z), op, w) for z, op, w in views]
    elif kind == "saturated":      # +-120: the fp32 sigmoid is exactly 1 or 0, whole planes tie
        views = [(torch.where(z > 0, 120.0, -120.0), op, w) for z, op, w in views]
    ref = _blend_case(views, 3, 48, mode, kind)
    dec = O.sigmoid_aten(ref) if mode == R.LOGITS else ref
    ties = int(((dec == dec.max(dim=1, keepdim=True).values).sum(dim=1) > 1).sum())
    print(f"{kind}: {ties} pixels with a tied decision value")
    assert ties >= 1, "the input is there to produce ties"
    if kind == "zeros":
        assert int(R.mask(ref, mode).max()) == 0


def test_blend_refuses_bad_arguments_before_any_launch():
    z = torch.zeros((N, 2, 4, 4), device=DEV)
    f = _lib.tta_symbol("vitseg_tta_blend")
    merged, mask = guarded((N, 2, 32, 32), name="merged"), guarded((N, 32, 32), torch.uint8, name="mask")
    good = [(z, 0, 1.0), (z, 4, 1.0)]

    def call(views=good, K=None, n=N, Cc=2, S=32, mode=0, mg=merged.data_ptr(), mk=mask.data_ptr(), descs=None):
        d = _descs(views) if descs is None else descs
        return f(d, len(views) if K is None else K, n, Cc, S, mode, mg, mk, _stream())

    null_map = (_lib.CTTAView * 2)(_lib.CTTAView(z.data_ptr(), 4, 0, 1.0), _lib.CTTAView(None, 4, 4, 1.0))
    bad_g = lambda g: (_lib.CTTAView * 2)(_lib.CTTAView(z.data_ptr(), 4, 0, 1.0), _lib.CTTAView(z.data_ptr(), g, 4, 1.0))
    einval = [dict(mg=None, mk=None), dict(descs=null_map), dict(K=0), dict(K=17), dict(views=[(z, 8, 1.0)]),
              dict(views=[(z, -1, 1.0)]), dict(views=[(z, 0, 0.0)]), dict(views=[(z, 0, -1.0)]),
              dict(views=[(z, 0, float("inf"))]), dict(views=[(z, 0, float("nan"))]), dict(mode=2), dict(mode=-1)]
    for bad in einval:
        assert call(**bad) == _lib.EINVAL, bad
        assert _lib.lib().vitseg_last_error().decode().startswith("tta_blend"), bad
    assert f(None, 2, N, 2, 32, 0, merged.data_ptr(), mask.data_ptr(), _stream()) == _lib.EINVAL
    eshape = [dict(Cc=0), dict(Cc=256), dict(S=0), dict(S=4097), dict(descs=bad_g(0)), dict(descs=bad_g(4097)), dict(n=0),
              dict(n=65536)]
    for bad in eshape:
        assert call(**bad) == _lib.ESHAPE, bad
        assert _lib.lib().vitseg_last_error().decode().startswith("tta_blend"), bad
    torch.cuda.synchronize()
    check(merged, mask)
    assert bool(torch.isnan(merged).all()) and bool((mask == 255).all())     # untouched
    assert call() == _lib.OK                                                  # the same call with good arguments runs
    torch.cuda.synchronize()
    check(merged, mask)
    assert bool((merged == 0).all()) and bool((mask == 0).all())


# ----------------------------------------------------------------------------------------------------------- the tiny model
@functools.lru_cache(maxsize=None)
def _golden():
    return Golden("tiny16_224_c2")


@functools.lru_cache(maxsize=None)
def _model():
    g = _golden()
    c = g.cfg
    m = ViTSegmentationModel(c.num_classes, c.patch_size, c.hidden_size, c.num_hidden_layers, c.num_attention_heads,
                             image_size=c.image_size, intermediate_size=c.intermediate_size, device=DEV).eval()
    m.load_state_dict(g.state_dict())
    return m


@functools.lru_cache(maxsize=None)
def _images():
    from visiontransformer_amd import synth
    return torch.from_numpy(synth.make_images(_golden().cfg, N, seed=0))


def test_view_images_are_torch_flips_and_turns_bit_for_bit():
    m = _model()
    gen = torch.Generator().manual_seed(3)
    x = torch.rand((2, 3, 32, 32), generator=gen)
    u8 = torch.randint(0, 256, (2, 32, 32, 3), generator=gen, dtype=torch.uint8)
    from8 = u8.permute(0, 3, 1, 2).float().div(255)       # what vitseg_preprocess_u8 ends with
    xd = guarded(x.shape, fill=x.to(DEV), name="images")
    ud = guarded(u8.shape, torch.uint8, fill=u8.to(DEV), name="bytes")
    snap = snapshot(xd, ud)
    for op in range(8):
        for src, u8_src, exp in ((xd, False, R.view(x, op)), (ud, True, R.view(from8, op))):
            out = guarded((2, 3, 32, 32), name="view")
            got = m._tta_view_image(src, u8_src, op, 32, out)
            torch.cuda.synchronize()
            check(out, src)
            assert torch.equal(got.cpu().view(torch.int32), exp.contiguous().view(torch.int32)), (op, u8_src)
            assert (got is src) == (op == 0 and not u8_src)     # the fp32 identity view is the batch itself
    unchanged(snap)
    # a rescale is the augmentation kernel's two-tap bilinear warp
    for op in (0, 5):
        M = np.array(_lib.augment_matrix(_lib.tta_affine(op), (32, 32), (48, 48)), np.int64)
        for src, u8_src, host in ((xd, False, x.numpy()), (ud, True, u8.numpy())):
            out = guarded((2, 3, 48, 48), name="view")
            m._tta_view_image(src, u8_src, op, 48, out)
            torch.cuda.synchronize()
            check(out)
            exp, _ = A.augment(host, np.stack([M, M]), 48, 48, border=A.EDGE)
            assert np.array_equal(out.cpu().numpy().view(np.int32), exp.view(np.int32)), (op, u8_src)


def test_a_single_identity_view_is_predict_mask():
    m, x = _model(), _images().to(DEV)
    mask, logits = m.predict_mask(x, return_logits=True)
    tm, tl = m.predict_mask_tta(x, tta="none", return_merged=True)
    assert torch.equal(tm, mask) and torch.equal(tl.view(torch.int32), logits.view(torch.int32))
    assert torch.equal(m.predict_mask_tta(x, tta="none"), mask)
    pm, probs = m.predict_mask_tta(x, tta="none", merge="probs", return_merged=True)
    assert torch.equal(pm, mask)
    assert torch.equal(probs.cpu(), O.sigmoid_aten(logits.cpu()))
    # decoded bytes: the same views as the fp32 image ToTensor makes of them
    u8 = torch.randint(0, 256, (N, 224, 224, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).to(DEV)
    f32 = u8.permute(0, 3, 1, 2).float().div(255).contiguous()
    assert torch.equal(m.predict_mask_tta(u8, tta="hflip"), m.predict_mask_tta(f32, tta="hflip"))
    assert torch.equal(m.predict_mask_tta(u8, tta="none"), m.predict_mask(f32))


@pytest.mark.parametrize("kw", [dict(tta="d4"), dict(tta="hflip", sizes=(160, 224), weights=(1.0, 2.0))],
                         ids=["d4", "two_sizes_hflip"])
def test_chain_is_the_reference_merge_of_the_device_low_res_maps(kw):
    m, x = _model(), _images().to(DEV)
    plan = m._tta_lowres(x, kw["tta"], kw.get("sizes"), kw.get("weights"))
    P = m.cfg.patch_size
    exp_views = [(op, s) for s in kw.get("sizes", (224,)) for op in ((0, 4) if kw["tta"] == "hflip" else range(8))]
    assert [(op, g * P) for _, g, op, _ in plan["views"]] == exp_views
    cpu_views = [(low.cpu(), op, w) for low, _, op, w in plan["views"]]
    for merge, mode in (("logits", R.LOGITS), ("probs", R.PROBS)):
        ref = R.blend(cpu_views, 224, mode)
        mask, merged = m._tta_blend(plan, merge, True, True)
        assert torch.equal(merged.cpu().view(torch.int32), ref.view(torch.int32))
        assert torch.equal(mask.cpu(), R.mask(ref, mode))
        pm, pmerged = m.predict_mask_tta(x, merge=merge, return_merged=True, **kw)      # the public call: the same bits
        assert torch.equal(pm, mask) and torch.equal(pmerged.view(torch.int32), merged.view(torch.int32))


def test_d4_merge_matches_the_oracle_view_by_view():
    """Reference: O.forward on view(x, op) for each of the eight ops, unview, mean in fp32.  A weighted mean of values each
    within e of theirs is within e, so the merged logits answer to the forward's own fp32 gate."""
    g, m, x = _golden(), _model(), _images()
    sd = g.state_dict()
    with torch.no_grad():
        ref = torch.stack([R.unview(O.forward(R.view(x, op).contiguous(), sd, g.cfg), op) for op in range(8)]).mean(dim=0)
    mask, merged = m.predict_mask_tta(x.to(DEV), tta="d4", merge="logits", return_merged=True)
    err = float((merged.cpu() - ref).abs().max())
    stable = O.mask_stable(ref, 2.0 * err + 1e-7)
    differ = mask.cpu().long() != O.predict_mask(ref)
    print(f"max |merged - oracle| = {err:.3e}; unstable share {float((~stable).float().mean()):.3e}, "
          f"mismatch share {float(differ.float().mean()):.3e}, mismatches at stable pixels {int((differ & stable).sum())}")
    assert err <= TOL_LOGITS * max(1.0, g.head_gain), err
    assert int((differ & stable).sum()) == 0
    assert float((~stable).float().mean()) < 2e-3 and float(differ.float().mean()) < 2e-3


def test_predict_with_tta_returns_the_merged_mask():
    from visiontransformer_amd.predict import predict, preprocess
    m = _model()
    img = (np.random.RandomState(3).rand(150, 100, 3) * 255).astype(np.uint8)
    x = preprocess(img, 224, DEV)
    exp, exp_merged = m.predict_mask_tta(x, tta="flip", return_merged=True)
    mask = predict(img, m, tta="flip")
    assert mask.shape == (224, 224) and mask.dtype == np.uint8
    assert np.array_equal(mask, exp[0].cpu().numpy())
    m2, lg = predict(img, m, tta="flip", return_logits=True)
    assert np.array_equal(m2, mask) and np.array_equal(lg, exp_merged[0].cpu().numpy())
    assert np.array_equal(predict(img, m, tta="hflip", tta_sizes=(160, 224), tta_merge="probs"),
                          m.predict_mask_tta(x, tta="hflip", sizes=(160, 224), merge="probs")[0].cpu().numpy())
    assert np.array_equal(predict(img, m), m.predict_mask(x)[0].cpu().numpy())       # without the keyword: as before
    with pytest.raises(ValueError, match="sliding"):
        predict(img, m, tta="flip", sliding=True)
