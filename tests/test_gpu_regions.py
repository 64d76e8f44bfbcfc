"""GPU (-m gpu): connected regions and their boxes on the device (vitseg_regions, regions.region_boxes,
ViTSegmentationModel.predict_regions, predict(..., return_boxes=True)) against the committed scipy goldens and the numpy
restatement tests/regions_ref.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import regions_ref as R
from guard import check, guarded, snapshot, unchanged
from visiontransformer_amd import _lib, regions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "regions", "regions.npz"))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(mask, conn, bg, max_regions, fill):
    """One vitseg_regions call through the C ABI with guarded outputs and a scratch pre-filled with `fill`."""
    n, H, W = mask.shape
    nbytes = _lib.region_symbol("vitseg_regions_scratch_bytes")(n, H, W)
    scratch = guarded((nbytes,), torch.uint8, name="scratch")
    scratch.fill_(fill)
    counts = guarded((n,), torch.int32, name="counts")
    recs = guarded((n, max_regions, 8), torch.int32, name="regions")
    labels = guarded((n, H, W), torch.int32, name="labels")
    snap = snapshot(mask)
    _lib.check(_lib.region_symbol("vitseg_regions")(mask.data_ptr(), n, H, W, conn, bg, counts.data_ptr(), recs.data_ptr(),
                                                    max_regions, labels.data_ptr(), scratch.data_ptr(), nbytes, _stream()))
    torch.cuda.synchronize()
    check(scratch, counts, recs, labels)
    unchanged(snap)
    return counts.cpu().numpy(), recs.cpu().numpy(), labels.cpu().numpy()


@pytest.mark.parametrize("name", sorted(R.golden_cases()))
@pytest.mark.parametrize("conn,bg", R.GOLDEN_VARIANTS)
def test_golden_cases_through_the_c_abi(name, conn, bg):
    m = Z[f"{name}.mask"]
    exp = Z[f"{name}.c{conn}.b{bg}"]
    _, exp_lab = R.regions_one(m, bg, conn)
    mask = guarded(m[None].shape, torch.uint8, torch.from_numpy(m[None]).to(DEV), name="mask")
    k = len(exp)
    runs = [_call(mask, conn, bg, k + 2, fill) for fill in (0x00, 0xFF)]
    for counts, recs, labels in runs:
        assert counts.tolist() == [k]
        assert np.array_equal(recs[0, :k, :7], exp)
        assert (recs[0, :k, 7] == 0).all() and (recs[0, k:] == 0).all()   # padding and rows past the count are zero
        assert np.array_equal(labels[0], exp_lab)
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)   # a scratch word read before it is written would tell the two fills apart


def _properties(m, recs, labels, bg, conn):
    """Conservation and adjacency laws for a whole batch, on the device."""
    m = m.to(DEV).long()
    lab = labels.to(DEV).long()
    n, H, W = m.shape
    valid = m != bg
    assert torch.equal(lab >= 0, valid)
    for i in range(n):
        r = torch.from_numpy(recs[i]).to(DEV).long()
        assert int(r[:, 5].sum()) == int(valid[i].sum())
        k = r.shape[0]
        li = lab[i][valid[i]]
        assert (int(li.max()) == k - 1) if k else (li.numel() == 0)
        ys, xs = torch.nonzero(valid[i], as_tuple=True)
        area = torch.bincount(li, minlength=k)
        ymin = torch.full((k,), H, device=DEV).scatter_reduce(0, li, ys, "amin")
        ymax = torch.full((k,), -1, device=DEV).scatter_reduce(0, li, ys, "amax")
        xmin = torch.full((k,), W, device=DEV).scatter_reduce(0, li, xs, "amin")
        xmax = torch.full((k,), -1, device=DEV).scatter_reduce(0, li, xs, "amax")
        first = torch.full((k,), H * W, device=DEV).scatter_reduce(0, li, ys * W + xs, "amin")
        assert torch.equal(torch.stack([m[i].reshape(-1)[first], ymin, xmin, ymax, xmax, area, first], 1), r)

    def same_label(a, b, la, lb):
        eq = (a == b) & (a != bg)
        assert torch.equal(la[eq], lb[eq])
    same_label(m[:, :, 1:], m[:, :, :-1], lab[:, :, 1:], lab[:, :, :-1])
    same_label(m[:, 1:], m[:, :-1], lab[:, 1:], lab[:, :-1])
    if conn == 8:
        same_label(m[:, 1:, 1:], m[:, :-1, :-1], lab[:, 1:, 1:], lab[:, :-1, :-1])
        same_label(m[:, 1:, :-1], m[:, :-1, 1:], lab[:, 1:, :-1], lab[:, :-1, 1:])


@pytest.mark.parametrize("C", [2, 17])
@pytest.mark.parametrize("conn", [4, 8])
def test_batch_of_32_at_512(C, conn):
    m = R.blobs(20 + C, 512, 512, C, n=32)
    recs, labels = regions.region_boxes(torch.from_numpy(m), connectivity=conn, return_labels=True)
    assert len(recs) == 32 and labels.shape == (32, 512, 512)
    for i in (0, 13, 31):
        exp, exp_lab = R.regions_one(m[i], 0, conn)
        assert np.array_equal(recs[i], exp), i
        assert np.array_equal(labels[i].cpu().numpy(), exp_lab), i
    _properties(torch.from_numpy(m), recs, labels, 0, conn)


def test_worst_cases_at_full_size():
    cb = torch.from_numpy(np.stack([R.checkerboard(512, 512)]))
    assert len(regions.region_boxes(cb, connectivity=4, background=-1)[0]) == 512 * 512
    assert len(regions.region_boxes(cb, connectivity=8, background=-1)[0]) == 2
    recs, labels = regions.region_boxes(cb, connectivity=4, background=-1, return_labels=True)
    assert np.array_equal(labels[0].cpu().numpy().reshape(-1)[recs[0][:, 6]], np.arange(512 * 512))
    s = R.serpentine(512, 512)
    for conn in (4, 8):
        for bg in (0, -1):
            got = regions.region_boxes(torch.from_numpy(s), connectivity=conn, background=bg)
            assert (got[:, 0] == 1).sum() == 1
            assert np.array_equal(got, R.regions_one(s, bg, conn)[0])


def test_reproducible_independent_and_truncated():
    m = torch.from_numpy(R.blobs(5, 512, 512, 17, n=32)).to(DEV)
    cap = 1 << 15
    a = _call(m, 4, 0, cap, 0x00)
    b = _call(m, 4, 0, cap, 0xFF)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    counts, recs, labels = a
    assert counts.max() <= cap
    for i in (0, 7, 31):
        c1, r1, l1 = _call(m[i:i + 1].contiguous(), 4, 0, cap, 0x00)
        assert c1[0] == counts[i] and np.array_equal(r1[0], recs[i]) and np.array_equal(l1[0], labels[i])
    t = max(1, int(counts.min()) // 2)
    ct, rt, lt = _call(m, 4, 0, t, 0xFF)
    assert np.array_equal(ct, counts)                       # the true count, not the capacity
    assert np.array_equal(rt, recs[:, :t])                  # the leading records
    assert np.array_equal(lt, labels)                       # full indices, also past the capacity
    # region_boxes' second call for an image with more than DEFAULT_MAX_REGIONS regions gives the same bits
    cb = torch.from_numpy(R.checkerboard(64, 64)).to(DEV)
    got = regions.region_boxes(cb, background=-1)
    assert len(got) == 4096 > regions.DEFAULT_MAX_REGIONS
    assert np.array_equal(got, Z["checker_64.c4.b-1"])


def test_predict_regions_and_predict_boxes():
    from visiontransformer_amd import synth
    from visiontransformer_amd.config import vit_tiny16
    from visiontransformer_amd.model import ViTSegmentationModel
    from visiontransformer_amd.predict import predict
    cfg = vit_tiny16(num_classes=5)
    model = ViTSegmentationModel(cfg.num_classes, cfg.patch_size, cfg.hidden_size, cfg.num_hidden_layers,
                                 cfg.num_attention_heads, image_size=cfg.image_size, device=DEV).eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=4, head_gain=4.0).items()})
    x = torch.from_numpy(synth.make_images(cfg, 3, seed=2)).to(DEV)
    for conn, bg in [(4, 0), (8, -1)]:
        recs, mask = model.predict_regions(x, connectivity=conn, background=bg, return_mask=True)
        assert torch.equal(mask, model.predict_mask(x))
        exp = regions.region_boxes(model.predict_mask(x), connectivity=conn, background=bg)
        assert len(recs) == 3 and all(np.array_equal(a, b) for a, b in zip(recs, exp))
        assert all(np.array_equal(a, b) for a, b in zip(recs, R.region_boxes_ref(mask.cpu().numpy(), bg, conn)))
    img = (np.random.RandomState(3).rand(224, 224, 3) * 255).astype(np.uint8)
    mask, boxes = predict(img, model, return_boxes=True)
    assert np.array_equal(predict(img, model), mask)
    assert boxes == R.boxes_by_class(R.regions_one(mask, 0, 4)[0])
    assert 0 not in boxes and list(boxes) == sorted(boxes)
