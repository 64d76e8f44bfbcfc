"""GPU (-m gpu): the training augmentation -- vitseg_augment through the C ABI on guard-banded buffers, Augmenter.apply /
paed_binary and the two trainers' `augment=` path -- bit for bit against the numpy restatement tests/augment_ref.py.
Every comparison is array_equal: the feature has no tolerances."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import augment_ref as R
import sdf_ref
from guard import check, guarded, snapshot, unchanged
from visiontransformer_amd import _lib, synth
from visiontransformer_amd.augment import Augmenter

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I64 = np.iinfo(np.int64)
FILL, FILL_LABEL = (10.0, 20.0, 30.0), 255


def _params(n, **kw):
    p = dict(hflip=np.zeros(n, bool), vflip=np.zeros(n, bool), quarter=np.zeros(n, np.int64), angle=np.zeros(n),
             scale=np.ones(n), tx=np.zeros(n), ty=np.zeros(n), brightness=np.ones(n), contrast=np.ones(n),
             saturation=np.ones(n))
    for k, v in kw.items():
        p[k] = np.asarray(v, dtype=p[k].dtype)
    return p


def _call(img, M, colour, out, planes, border, fill=FILL, fill_label=FILL_LABEL):
    """planes: [(src, matrices, out)] device tensors."""
    u8 = img.dtype == torch.uint8
    n = img.shape[0]
    H, W = (img.shape[1], img.shape[2]) if u8 else (img.shape[2], img.shape[3])
    descs = (_lib.CAugmentMask * max(len(planes), 1))()
    for i, (src, Mm, dst) in enumerate(planes):
        descs[i] = _lib.CAugmentMask(src.data_ptr(), Mm.data_ptr(), dst.data_ptr(), int(src.dtype == torch.long),
                                     int(dst.dtype == torch.long), src.shape[1], src.shape[2], dst.shape[1], dst.shape[2])
    _lib.check(_lib.augment_symbol("vitseg_augment")(
        img.data_ptr(), int(not u8), n, H, W, out.shape[2], out.shape[3], M.data_ptr(),
        None if colour is None else colour.data_ptr(), out.data_ptr(), descs, len(planes), border, (C.c_float * 3)(*fill),
        fill_label, torch.cuda.current_stream().cuda_stream))


def _g(a, name):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return guarded(t.shape, t.dtype, t.to(DEV), name=name)


def _same_bits(got, want, what):
    """array_equal on the bit patterns, naming the first element that differs."""
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a, b = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {a.size} elements differ, first at {i}: got {got[i]!r} ({a[i]:#x}), "
                             f"want {want[i]!r} ({b[i]:#x}); samples hit: {sorted(set(bad[:, 0].tolist()))}")


# ------------------------------------------------------------------------------------------------ the direct C-ABI call
N, IH, IW, OH, OW, MH, MW = 4, 37, 53, 32, 48, 40, 40
M2H, M2W, O2H, O2W = 19, 23, 9, 50     # the second label plane: another source size, another output size


@functools.lru_cache(maxsize=None)
def _direct_inputs():
    rng = np.random.default_rng(0)
    A = Augmenter(OH, device="cpu")
    par = _params(3, hflip=[False, True, False], angle=[0, 33.0, 0], scale=[1, 0.7, 1], tx=[0, 0.08, 0.9],
                  ty=[0, -0.05, 0.2])
    extreme = np.array([[I64.max, I64.min, I64.max, I64.min, I64.max, I64.min]], np.int64)

    def table(src_hw, dst_hw):
        M = A.matrices(par, src_hw, dst_hw)
        M[0] = R.IDENTITY
        return np.concatenate([M, extreme])

    return dict(
        u8=rng.integers(0, 256, (N, IH, IW, 3), dtype=np.uint8),
        f32=rng.standard_normal((N, 3, IH, IW)).astype(np.float32),
        mask=rng.integers(0, 17, (N, MH, MW)).astype(np.int64),
        mask2=rng.integers(0, 17, (N, M2H, M2W)).astype(np.int64),
        M=table((IH, IW), (OH, OW)), Mm=table((MH, MW), (OH, OW)), Mm2=table((M2H, M2W), (O2H, O2W)),
        colour=(np.tile(np.eye(3, 4, dtype=np.float32).reshape(12), (N, 1))
                + rng.uniform(-0.4, 0.4, (N, 12)).astype(np.float32)))


@functools.lru_cache(maxsize=None)
def _direct_reference(fmt, border, wide, coloured):
    d = _direct_inputs()
    dt, dt2 = (np.int64, np.uint8) if wide else (np.uint8, np.int64)
    return R.augment(d[fmt], d["M"], OH, OW, colour=d["colour"] if coloured else None, border=border, fill=FILL,
                     masks=[(d["mask"].astype(dt), d["Mm"], OH, OW, dt), (d["mask2"].astype(dt2), d["Mm2"], O2H, O2W, dt)],
                     fill_label=FILL_LABEL)


def test_direct_cases_reach_every_branch():
    """From the restatement alone: the share of output pixels whose four taps are all in frame, all outside and
    straddling the edge, per matrix (0.47 / 0.49 / 0.04 for the rotation, 0.07 / 0.92 / 0.02 for the shift); the two warped
    samples together hold at least 2 % of their pixels in each, so a change of inputs cannot quietly skip a branch."""
    d = _direct_inputs()
    cov = np.array([R.coverage(M, IH, IW, OH, OW) for M in d["M"]])
    print("coverage (inside, outside, straddling) per matrix:\n", cov.round(3))
    assert tuple(cov[0]) == (1.0, 0.0, 0.0)                       # the identity crops the source's corner
    assert np.all(cov[1:3] > 0)                                   # the rotation and the shift each reach all three
    assert np.all(cov[1:3].mean(0) >= 0.02)                       # ... and hold 2 % of their pixels in every branch
    for M in d["M"][1:3]:                                         # ... with non-zero fractions nearly everywhere
        U, V = R.coords(M, OH, OW)
        assert (((U & 0xFFFF) >> 8 != 0) & ((V & 0xFFFF) >> 8 != 0)).mean() > 0.9
    assert list(R.clamp_matrix(d["M"][3])) != list(d["M"][3])     # the last table is only valid through the clamp


@pytest.mark.parametrize("coloured", [True, False], ids=["colour", "nocolour"])
@pytest.mark.parametrize("wide", [False, True], ids=["mask_u8", "mask_i64"])
@pytest.mark.parametrize("border", [R.CONSTANT, R.EDGE], ids=["constant", "edge"])
@pytest.mark.parametrize("fmt", ["u8", "f32"])
def test_direct_call_matches_the_restatement(fmt, border, wide, coloured):
    d = _direct_inputs()
    want_x, (want_y, want_y2) = _direct_reference(fmt, border, wide, coloured)
    dt, dt2 = (np.int64, np.uint8) if wide else (np.uint8, np.int64)
    img, M, Mm, Mm2 = _g(d[fmt], "image"), _g(d["M"], "matrices"), _g(d["Mm"], "mask matrices"), _g(d["Mm2"], "mask2 matrices")
    mask, mask2 = _g(d["mask"].astype(dt), "mask"), _g(d["mask2"].astype(dt2), "mask2")
    col = _g(d["colour"], "colour") if coloured else None
    tdt = torch.long if wide else torch.uint8
    x = guarded((N, 3, OH, OW), name="x")
    y, y2 = guarded((N, OH, OW), tdt, name="y"), guarded((N, O2H, O2W), tdt, name="y2")
    snap = snapshot(img, M, Mm, Mm2, mask, mask2, col)
    _call(img, M, col, x, [(mask, Mm, y), (mask2, Mm2, y2)], border)
    torch.cuda.synchronize()
    check(x, y, y2, img, M, Mm, Mm2, mask, mask2, col)
    unchanged(snap)
    _same_bits(x, want_x, "x")
    _same_bits(y, want_y, "y")
    _same_bits(y2, want_y2, "y2")
    if border == R.CONSTANT:
        assert (want_y == FILL_LABEL).mean() > 0.3


# ---------------------------------------------------------------------------------------------------- further GPU cases
def _rotated(n, src_hw, dst_hw, seed):
    rng = np.random.default_rng(seed)
    par = _params(n, hflip=rng.random(n) < 0.5, angle=rng.uniform(-40, 40, n), scale=rng.uniform(0.6, 1.4, n),
                  tx=rng.uniform(-0.2, 0.2, n), ty=rng.uniform(-0.2, 0.2, n))
    return Augmenter(8, device="cpu").matrices(par, src_hw, dst_hw)


@pytest.mark.parametrize("n,H,W,oh,ow", [(1, 5, 9, 6, 1),        # one column: every run is a scalar tail
                                         (3, 11, 13, 23, 45),    # odd width, two partly filled tiles per sample
                                         (2, 30, 50, 37, 150),   # 3 x 3 tiles of 16 rows x 64 pixels, the last ones partial
                                         (2, 1, 1, 3, 7),        # a one-pixel source
                                         (1, 24, 40, 16, 512)])  # whole runs: every store is 16 bytes
@pytest.mark.parametrize("fmt", ["u8", "f32"])
def test_sizes_tails_and_one_sample(n, H, W, oh, ow, fmt):
    rng = np.random.default_rng(n * 1000 + ow)
    src = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8) if fmt == "u8" else rng.random((n, 3, H, W), dtype=np.float32)
    m = rng.integers(0, 200, (n, H, W), dtype=np.uint8)
    Mt = _rotated(n, (H, W), (oh, ow), ow)
    col = rng.uniform(-1, 1, (n, 12)).astype(np.float32)
    for border in (R.CONSTANT, R.EDGE):
        want_x, (want_y,) = R.augment(src, Mt, oh, ow, colour=col, border=border, fill=(0.25, 0.5, 0.75),
                                      masks=[(m, Mt, oh, ow, np.uint8)], fill_label=7)
        img, M, c, mask = _g(src, "image"), _g(Mt, "matrices"), _g(col, "colour"), _g(m, "mask")
        x, y = guarded((n, 3, oh, ow), name="x"), guarded((n, oh, ow), torch.uint8, name="y")
        snap = snapshot(img, M, c, mask)
        _call(img, M, c, x, [(mask, M, y)], border, fill=(0.25, 0.5, 0.75), fill_label=7)
        torch.cuda.synchronize()
        check(x, y, img, M, c, mask)
        unchanged(snap)
        _same_bits(x, want_x, "x")
        _same_bits(y, want_y, "y")


def test_no_masks_and_an_unaligned_output():
    """Zero label planes; the output starts 4 bytes past a 16-byte boundary, so no run of a 4-multiple width is aligned."""
    n, H, W, oh, ow = 2, 9, 14, 8, 12
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    Mt = _rotated(n, (H, W), (oh, ow), 5)
    want_x, _ = R.augment(src, Mt, oh, ow, border=R.EDGE)
    img, M = _g(src, "image"), _g(Mt, "matrices")
    buf = guarded(n * 3 * oh * ow + 1, name="x")
    x = buf[1:].view(n, 3, oh, ow)
    assert x.data_ptr() % 16 == 4
    _call(img, M, None, x, [], R.EDGE)
    torch.cuda.synchronize()
    check(buf, img, M)
    _same_bits(x, want_x, "x")
    assert buf[:1].cpu().numpy().view(np.uint32)[0] == 0xFFFFFFFF   # the element before the output is untouched


def test_two_calls_give_identical_bits():
    d = _direct_inputs()
    img, M, col = _g(d["f32"], "image"), _g(d["M"], "matrices"), _g(d["colour"], "colour")
    mask, Mm = _g(d["mask"], "mask"), _g(d["Mm"], "mask matrices")
    outs = []
    for _ in range(2):
        x, y = guarded((N, 3, OH, OW), name="x"), guarded((N, OH, OW), torch.long, name="y")
        _call(img, M, col, x, [(mask, Mm, y)], R.CONSTANT)
        torch.cuda.synchronize()
        check(x, y)
        outs.append((x.cpu().numpy().view(np.uint32), y.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_identity_is_the_existing_preprocessing():
    from visiontransformer_amd.preprocess import Preprocessor
    img = torch.randint(0, 256, (2, 64, 64, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).to(DEV)
    want = Preprocessor(64, device=DEV).images(img)
    A = Augmenter(64, device=DEV, hflip=0.0)
    x, y = A.apply(img)
    assert y is None and torch.equal(x.view(torch.int32), want.view(torch.int32))
    M = _g(np.tile(np.array(R.IDENTITY, np.int64), (2, 1)), "matrices")
    x2 = guarded((2, 3, 64, 64), name="x")
    _call(img, M, None, x2, [], R.CONSTANT)
    torch.cuda.synchronize()
    check(x2, M)
    assert torch.equal(x2.view(torch.int32), want.view(torch.int32))


# -------------------------------------------------------------------------------------------------------- the Augmenter
FULL = dict(seed=5, hflip=0.5, vflip=0.5, rot90=True, rotate=25.0, scale=(0.7, 1.3), translate=0.15, brightness=0.3,
            contrast=0.3, saturation=0.3)


def _binary_masks(H, W):
    """Two masks: blobs of 0 / 1 and cracks of 0 / 255 (a decoded 'L' mask)."""
    return np.stack([sdf_ref.kind_mask("blobs", 3, H, W), sdf_ref.kind_mask("cracks", 4, H, W) * 255]).astype(np.uint8)


def _restate(A, params, images, masks, mask_hw, mask_dtype):
    """What Augmenter.apply computes, from the restatement fed A.matrices() / A.colour()."""
    u8 = images.dtype == np.uint8
    src_hw = images.shape[1:3] if u8 else images.shape[2:4]
    border = R.CONSTANT if A.border == "constant" else R.EDGE
    fill = [v * (255.0 if u8 else 1.0) for v in A.fill]
    planes = [] if masks is None else [(masks, A.matrices(params, masks.shape[1:], mask_hw), mask_hw[0], mask_hw[1], mask_dtype)]
    x, ys = R.augment(images, A.matrices(params, src_hw, (A.S, A.S)), A.S, A.S, colour=A.colour(params) if A.has_colour else None,
                      border=border, fill=fill, masks=planes, fill_label=A.fill_label or 0)
    return x, (ys[0] if ys else None)


@pytest.mark.parametrize("fmt", ["u8", "f32"])
@pytest.mark.parametrize("border", ["edge", "constant"])
def test_apply_with_explicit_params_matches_the_restatement(fmt, border):
    rng = np.random.default_rng(9)
    n = 3
    images = rng.integers(0, 256, (n, 50, 70, 3), dtype=np.uint8) if fmt == "u8" else rng.random((n, 3, 50, 70), dtype=np.float32)
    masks = rng.integers(0, 5, (n, 40, 40)).astype(np.int64)
    A = Augmenter(32, device=DEV, border=border, fill=(0.2, 0.4, 0.6), fill_label=255 if border == "constant" else None, **FULL)
    params = A.sample(n, key=(0, 7))
    assert A.calls == 0
    x, y = A.apply(torch.from_numpy(images), torch.from_numpy(masks), params=params, mask_size=(24, 36), mask_dtype=torch.uint8)
    want_x, want_y = _restate(A, params, images, masks, (24, 36), np.uint8)
    assert x.dtype == torch.float32 and y.dtype == torch.uint8 and tuple(y.shape) == (n, 24, 36)
    _same_bits(x, want_x, "x")
    _same_bits(y, want_y, "y")
    # a default draw is the (rank, calls) draw; int64 labels out, the default mask size
    x2, y2 = A.apply(torch.from_numpy(images), torch.from_numpy(masks), mask_dtype=torch.long)
    assert A.calls == 1
    want_x, want_y = _restate(A, A.sample(n, key=(0, 0)), images, masks, (32, 32), np.int64)
    assert y2.dtype == torch.long and np.array_equal(y2.cpu().numpy(), want_y)
    _same_bits(x2, want_x, "x2")


def test_paed_binary_recomputes_the_sdfs_of_the_warped_mask():
    n, S = 2, 48
    rng = np.random.default_rng(4)
    images = rng.random((n, 3, 40, 56), dtype=np.float32)
    masks = _binary_masks(60, 60)
    A = Augmenter(S, device=DEV, **FULL)
    params = A.sample(n, key=(0, 3))
    x, m, e, i = A.paed_binary(torch.from_numpy(images), torch.from_numpy(masks)[:, None].float(), params=params)
    want_x, want_m = _restate(A, params, images, (masks != 0).astype(np.uint8), (S, S), np.uint8)
    want_e, want_i = sdf_ref.sdf_ref(want_m)
    assert tuple(m.shape) == (n, 1, S, S) and m.dtype == torch.float32 and 0 < want_m.mean() < 1
    _same_bits(x, want_x, "x")
    assert np.array_equal(m[:, 0].cpu().numpy(), want_m.astype(np.float32))
    _same_bits(e, want_e, "e")
    _same_bits(i, want_i, "i")
    with pytest.raises(ValueError, match="fill_label"):
        Augmenter(S, device=DEV, border="constant", fill_label=255).paed_binary(torch.from_numpy(images), torch.from_numpy(masks))


# ---------------------------------------------------------------------------------------------------------- the trainers
def _bits(t):
    return t.detach().reshape(1).view(torch.int32).cpu()


def test_lightning_training_step_is_the_plain_step_on_the_warped_batch():
    """LightningViTModel(augment=A).training_step == an un-augmented model's step on the restatement's warped (x, y), bit
    for bit; the validation step does not augment."""
    from visiontransformer_amd.config import vit_tiny16
    from visiontransformer_amd.lightning import LightningViTModel
    cfg = vit_tiny16()
    x = synth.make_images(cfg, 2, seed=1)
    y = synth.make_targets(cfg, 2, seed=1)
    assert x.shape == (2, 3, 224, 224) and y.shape == (2, 256, 256)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=2).items()}
    A = Augmenter(224, device=DEV, border="constant", fill_label=255, **FULL)
    want_x, want_y = _restate(A, A.sample(2, key=(0, 0)), x, y, (224, 224), np.uint8)
    assert 0.02 < (want_y == 255).mean() < 0.9
    losses = []
    for aug in (A, None):
        lm = LightningViTModel(cfg.num_classes, cfg.patch_size, cfg.hidden_size, cfg.num_hidden_layers,
                               cfg.num_attention_heads, image_size=224, device=DEV, ignore_index=255, augment=aug)
        lm.model.load_state_dict(sd)
        lm.train()
        batch = (torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)) if aug is not None else \
            (torch.from_numpy(want_x).to(DEV), torch.from_numpy(want_y).to(DEV))
        loss = lm.training_step(batch, 0)
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and torch.isfinite(lm.model.arena.grad).all()
        losses.append((_bits(loss), lm.model.arena.grad.clone()))
        if aug is not None:
            calls = A.calls
            lv = lm.validation_step((torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)), 0)
            assert A.calls == calls == 1 and torch.isfinite(lv)
    assert torch.equal(losses[0][0], losses[1][0])
    assert torch.equal(losses[0][1].view(torch.int32), losses[1][1].view(torch.int32))


def test_paed_trainer_step_is_the_plain_step_on_the_warped_batch():
    from visiontransformer_amd.config import vit_tiny16
    from visiontransformer_amd.paed import PAEDTrainer
    cfg = vit_tiny16(num_classes=1)
    x = synth.make_images(cfg, 2, seed=3)
    masks = _binary_masks(224, 224)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=2).items()}
    A = Augmenter(224, device=DEV, **FULL)
    want_x, want_m = _restate(A, A.sample(2, key=(0, 0)), x, (masks != 0).astype(np.uint8), (224, 224), np.uint8)
    want_e, want_i = sdf_ref.sdf_ref(want_m)
    dummy = torch.zeros((2, 224, 224), device=DEV)   # the batch's own SDFs: replaced by the warped mask's
    losses = []
    for aug in (A, None):
        tr = PAEDTrainer(1, cfg.patch_size, cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, image_size=224,
                         device=DEV, augment=aug)
        tr.model.load_state_dict(sd)
        tr.train()
        if aug is not None:
            batch = (torch.from_numpy(x).to(DEV), torch.from_numpy(masks)[:, None].float().to(DEV), dummy, dummy)
        else:
            batch = (torch.from_numpy(want_x).to(DEV), torch.from_numpy(want_m)[:, None].float().to(DEV),
                     torch.from_numpy(want_e).to(DEV), torch.from_numpy(want_i).to(DEV))
        loss = tr.training_step(batch, 0)
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and torch.isfinite(tr.model.arena.grad).all()
        losses.append((_bits(loss), tr.model.arena.grad.clone()))
    assert A.calls == 1
    assert torch.equal(losses[0][0], losses[1][0])
    assert torch.equal(losses[0][1].view(torch.int32), losses[1][1].view(torch.int32))
