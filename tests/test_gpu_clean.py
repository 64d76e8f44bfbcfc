"""GPU (-m gpu): mask clean-up on the device (vitseg_clean_mask, clean.clean_mask, ViTSegmentationModel.predict_regions and
predict(...) with min_area / fill_holes / max_hole_area) against the committed scipy goldens and the numpy restatement
tests/clean_ref.py."""
import os

import numpy as np
import pytest
import torch

import clean_ref as K
import regions_ref as R
from guard import check, guarded, snapshot, unchanged
from visiontransformer_amd import _lib, clean, regions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "clean", "clean.npz"))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _buffers(n, H, W, fill, scratch_bytes=None):
    nbytes = _lib.clean_symbol("vitseg_clean_scratch_bytes")(n, H, W) if scratch_bytes is None else scratch_bytes
    scratch = guarded((nbytes,), torch.uint8, name="scratch")
    scratch.fill_(fill)
    return guarded((n, H, W), torch.uint8, name="out"), guarded((n, 8), torch.int32, name="stats"), scratch


def _call(mask, bg, variant, fill):
    """One vitseg_clean_mask call through the C ABI with guarded outputs and a scratch pre-filled with `fill`."""
    n, H, W = mask.shape
    a, f, h, c = variant
    out, stats, scratch = _buffers(n, H, W, fill)
    snap = snapshot(mask)
    _lib.check(_lib.clean_symbol("vitseg_clean_mask")(mask.data_ptr(), out.data_ptr(), n, H, W, c, bg, a, f, h, stats.data_ptr(),
                                                      scratch.data_ptr(), scratch.numel(), _stream()))
    torch.cuda.synchronize()
    check(out, stats, scratch)
    unchanged(snap)
    st = stats.cpu().numpy()
    assert (st[:, 6:] == 0).all()
    return out.cpu().numpy(), st[:, :6]


@pytest.mark.parametrize("name", sorted(K.clean_cases()))
def test_golden_cases_through_the_c_abi(name):
    m, bg = Z[f"{name}.mask"], int(Z[f"{name}.background"])
    mask = guarded(m[None].shape, torch.uint8, torch.from_numpy(m[None]).to(DEV), name="mask")
    for v in K.variants(name):
        exp, exp_st = Z[K.key(name, v) + ".mask"], Z[K.key(name, v) + ".stats"]
        runs = [_call(mask, bg, v, fill) for fill in (0x00, 0xFF)]
        for out, st in runs:
            assert dict(zip(K.STATS, st[0].tolist())) == dict(zip(K.STATS, exp_st.tolist())), v
            assert np.array_equal(out[0], exp), (v, int((out[0] != exp).sum()))
        for a, b in zip(runs[0], runs[1]):
            assert np.array_equal(a, b)   # a scratch word read before it is written would tell the two fills apart


def test_stats_may_be_null_and_both_steps_off_copy():
    m, bg = K.clean_cases()["speckle5_97x131"]
    mask = torch.from_numpy(m[None]).to(DEV)
    n, H, W = mask.shape
    for v in ((8, 1, 20, 4), (0, 0, 0, 4), (1, 0, 5, 8)):
        a, f, h, c = v
        out, _, scratch = _buffers(n, H, W, 0xFF)
        _lib.check(_lib.clean_symbol("vitseg_clean_mask")(mask.data_ptr(), out.data_ptr(), n, H, W, c, bg, a, f, h, None,
                                                          scratch.data_ptr(), scratch.numel(), _stream()))
        torch.cuda.synchronize()
        check(out, scratch)
        exp = Z[K.key("speckle5_97x131", v) + ".mask"] if f else m   # 0 and 1 remove nothing
        assert np.array_equal(out[0].cpu().numpy(), exp), v


@pytest.mark.parametrize("conn", [4, 8])
def test_batch_equals_restatement_and_images_alone(conn):
    m = K.speckle(31, 160, 200, 17, n=5)
    v = (8, 1, 30, conn)
    mask = torch.from_numpy(m).to(DEV)
    out, st = _call(mask, 0, v, 0xFF)
    for i in range(5):
        exp, exp_st = K.clean_one(m[i], 8, True, 30, conn, 0)
        assert np.array_equal(st[i], exp_st), i
        assert np.array_equal(out[i], exp), i
    assert (st > 0).all()                                  # every branch on every image
    for i in (0, 2, 4):
        o1, s1 = _call(mask[i:i + 1].contiguous(), 0, v, 0x00)
        assert np.array_equal(o1[0], out[i]) and np.array_equal(s1[0], st[i]), i


def test_laws_on_a_batch_at_512():
    m = torch.from_numpy(K.speckle(32, 512, 512, 5, n=4)).to(DEV)
    k = 12
    for conn in (4, 8):
        s1, st1 = clean.clean_mask(m, min_area=k, connectivity=conn, return_stats=True)
        assert s1.dtype == torch.uint8 and s1.shape == m.shape and s1.is_cuda
        # no region below k is left, and every region of k or more is still there with its area
        before = regions.region_boxes(m, connectivity=conn)
        after = regions.region_boxes(s1, connectivity=conn)
        for i in range(4):
            assert after[i][:, 5].min() >= k
            assert np.array_equal(after[i], before[i][before[i][:, 5] >= k])
            assert st1[i]["regions_removed"] == int((before[i][:, 5] < k).sum()) > 0
        # what step 1 changes becomes background, and that is the count it reports
        ch = s1 != m
        assert bool((s1[ch] == 0).all())
        assert ch.sum(dim=(1, 2)).tolist() == [s["pixels_removed"] for s in st1]
        assert all(s["holes_filled"] == s["pixels_filled"] == s["holes_mixed"] == s["holes_over_area"] == 0 for s in st1)
    # what step 2 changes was background, and that is the count it reports
    s2, st2 = clean.clean_mask(m, fill_holes=True, return_stats=True)
    ch = s2 != m
    assert bool((m[ch] == 0).all()) and bool((s2[ch] != 0).all())
    assert ch.sum(dim=(1, 2)).tolist() == [s["pixels_filled"] for s in st2]
    assert all(s["holes_filled"] > 0 and s["holes_mixed"] > 0 and s["regions_removed"] == 0 for s in st2)
    # a second pass with the same arguments changes nothing
    s3, st3 = clean.clean_mask(s2, fill_holes=True, return_stats=True)
    assert torch.equal(s3, s2) and all(s["holes_filled"] == 0 and s["pixels_filled"] == 0 for s in st3)
    assert [s["holes_mixed"] for s in st3] == [s["holes_mixed"] for s in st2]
    # both steps and an area limit: image 1 against the restatement
    s4, st4 = clean.clean_mask(m, min_area=k, fill_holes=True, max_hole_area=40, connectivity=8, return_stats=True)
    exp, exp_st = K.clean_ref(m[1].cpu().numpy(), min_area=k, fill_holes=True, max_hole_area=40, connectivity=8)
    assert np.array_equal(s4[1].cpu().numpy(), exp) and st4[1] == exp_st


def test_clean_mask_dtypes_ranks_and_background():
    m, _ = K.clean_cases()["speckle5_97x131"]
    kw = dict(min_area=8, fill_holes=True, max_hole_area=20)
    exp, exp_st = K.clean_ref(m, background=3, **kw)
    out, st = clean.clean_mask(m, background=3, return_stats=True, **kw)                  # numpy [H, W]
    assert out.dtype == torch.uint8 and out.shape == (97, 131) and out.is_cuda and st == exp_st
    assert np.array_equal(out.cpu().numpy(), exp)
    lm = torch.from_numpy(m).long().to(DEV)[None]
    out = clean.clean_mask(lm, background=3, **kw)                                        # long [1, H, W] on the device
    assert out.dtype == torch.int64 and out.shape == (1, 97, 131) and np.array_equal(out[0].cpu().numpy(), exp)
    assert clean.clean_mask(lm, min_area=1) is lm


def test_status_codes_and_nothing_written():
    m = torch.from_numpy(K.nested()[None]).to(DEV)
    n, H, W = m.shape
    f = _lib.clean_symbol("vitseg_clean_mask")
    need = _lib.clean_symbol("vitseg_clean_scratch_bytes")(n, H, W)

    def refused(code, *, out_is_mask=False, shape=(n, H, W), conn=4, bg=0, min_area=8, max_hole=0, scratch_bytes=need):
        out, stats, scratch = _buffers(n, H, W, 0xA5, scratch_bytes)
        snap = snapshot(m, out, stats, scratch)
        rc = f(m.data_ptr(), m.data_ptr() if out_is_mask else out.data_ptr(), *shape, conn, bg, min_area, 1, max_hole,
               stats.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream())
        torch.cuda.synchronize()
        assert rc == code and _lib.lib().vitseg_last_error()
        check(out, stats, scratch)
        unchanged(snap)

    refused(_lib.EINVAL, out_is_mask=True)
    refused(_lib.EINVAL, bg=-1)
    refused(_lib.EINVAL, bg=256)
    refused(_lib.EINVAL, conn=6)
    refused(_lib.EINVAL, min_area=-1)
    refused(_lib.EINVAL, max_hole=-1)
    refused(_lib.EWORKSPACE, scratch_bytes=need - 1)
    refused(_lib.ESHAPE, shape=(0, H, W))
    refused(_lib.ESHAPE, shape=(n, 0, W))
    refused(_lib.ESHAPE, shape=(n, 1 << 16, 1 << 15))
    assert f(None, m.data_ptr(), n, H, W, 4, 0, 8, 1, 0, None, m.data_ptr(), need, _stream()) == _lib.EINVAL
    unchanged(snapshot(m))


def test_predict_regions_and_predict_clean():
    from visiontransformer_amd import synth
    from visiontransformer_amd.config import vit_tiny16
    from visiontransformer_amd.model import ViTSegmentationModel
    from visiontransformer_amd.predict import predict
    cfg = vit_tiny16(num_classes=5)
    model = ViTSegmentationModel(cfg.num_classes, cfg.patch_size, cfg.hidden_size, cfg.num_hidden_layers,
                                 cfg.num_attention_heads, image_size=cfg.image_size, device=DEV).eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=4, head_gain=4.0).items()})
    x = torch.from_numpy(synth.make_images(cfg, 3, seed=2)).to(DEV)
    raw = model.predict_mask(x)
    kw = dict(min_area=40, fill_holes=True, max_hole_area=500)
    for conn, bg in [(4, 0), (8, 2)]:
        recs, mask = model.predict_regions(x, connectivity=conn, background=bg, return_mask=True, **kw)
        exp_mask = clean.clean_mask(raw, connectivity=conn, background=bg, **kw)
        assert torch.equal(mask, exp_mask)
        assert np.array_equal(mask.cpu().numpy(), K.clean_ref(raw.cpu().numpy(), connectivity=conn, background=bg, **kw)[0])
        exp = regions.region_boxes(exp_mask, connectivity=conn, background=bg)
        assert len(recs) == 3 and all(np.array_equal(a, b) for a, b in zip(recs, exp))
        assert all(r[:, 5].min() >= 40 for r in recs if len(r))
        # the defaults: today's predict_regions
        recs0, mask0 = model.predict_regions(x, connectivity=conn, background=bg, return_mask=True)
        assert torch.equal(mask0, raw)
        assert all(np.array_equal(a, b) for a, b in zip(recs0, regions.region_boxes(raw, connectivity=conn, background=bg)))
    img = (np.random.RandomState(3).rand(224, 224, 3) * 255).astype(np.uint8)
    pal = np.arange(15, dtype=np.uint8).reshape(5, 3)
    plain = predict(img, model)
    mask, rgb, boxes = predict(img, model, index_to_color=pal, return_boxes=True, **kw)
    assert np.array_equal(mask, K.clean_ref(plain, **kw)[0])
    assert np.array_equal(rgb, pal[mask])
    assert boxes == R.boxes_by_class(R.regions_one(mask, 0, 4)[0])
    m2, logits = predict(img, model, return_logits=True, min_area=40)
    assert np.array_equal(m2, K.clean_ref(plain, min_area=40)[0])
    assert np.array_equal(logits, predict(img, model, return_logits=True)[1])   # the logits are not touched
