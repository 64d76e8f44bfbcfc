"""GPU (-m gpu): per-region measurements on the device (vitseg_region_props, regions.region_props, predict_regions(props=True),
Evaluator.region_props, evaluate_to_csv(props_classes=...)) against the numpy restatement tests/props_ref.py.  Everything the
device returns is an integer: every comparison is bit for bit.  Outputs and scratch live in guard-banded, poisoned buffers."""
import csv
import ctypes
import os

import numpy as np
import pytest
import torch

import props_ref as PR
import regions_ref as RR
import skeleton_ref as SK
from guard import check, guarded, snapshot, unchanged
from visiontransformer_amd import _lib, clean, metrics, regions, scripts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AUTO, RESIDENT, GLOBAL = 0, 1, 2
_REF = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(mask, classes=(), connectivity=4, background=0, route=AUTO, max_regions=512, want_labels=True, fill=0xFF):
    """One vitseg_region_props call through the C ABI on a device tensor, with guarded outputs and a scratch pre-filled with
    `fill`: (counts, props [n, max_regions, 20], labels or None) as numpy arrays."""
    n, H, W = mask.shape
    K = len(classes)
    nbytes = _lib.props_symbol("vitseg_region_props_scratch_bytes")(n, H, W, K, route)
    assert nbytes > 0
    scratch = guarded((nbytes,), torch.uint8, name="scratch")
    scratch.fill_(fill)
    counts = guarded((n,), torch.int32, name="counts")
    props = guarded((n, max_regions, 20), torch.int64, name="props")
    labels = guarded((n, H, W), torch.int32, name="labels") if want_labels else None
    snap = snapshot(mask)
    cls = (ctypes.c_int32 * K)(*classes) if K else None
    _lib.check(_lib.props_symbol("vitseg_region_props")(
        mask.data_ptr(), n, H, W, connectivity, background, cls, K, route, counts.data_ptr(), props.data_ptr(), max_regions,
        None if labels is None else labels.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream()))
    torch.cuda.synchronize()
    check(counts, props, labels, scratch)
    unchanged(snap)
    return tuple(None if t is None else t.cpu().numpy() for t in (counts, props, labels))


def _dev(m):
    m = np.asarray(m, np.uint8)
    if m.ndim == 2:
        m = m[None]
    return guarded(m.shape, torch.uint8, torch.from_numpy(m).to(DEV), name="mask")


def _ref(key, m, classes, connectivity, background=0):
    """The restatement's (rows per image, labels [n, H, W]) with every class of `classes` measured, computed once per key."""
    if key not in _REF:
        _REF[key] = PR.props_ref(np.asarray(m), classes, background, connectivity, return_labels=True)
    return _REF[key]


def _subset(rows, classes):
    """The rows when only `classes` are measured: a class plane's skeleton and distances do not depend on the others."""
    out = rows.copy()
    out[~np.isin(out[:, 0], list(classes)), 14:19] = -1
    return out


def _assert_rows(got, counts, exp, what=""):
    """got [n, max_regions, 20] against the expected rows per image: the first max_regions exact, the rest zero."""
    for i, e in enumerate(exp):
        assert counts[i] == len(e), (what, i, counts[i], len(e))
        k = min(len(e), got.shape[1])
        bad = np.argwhere(got[i, :k] != e[:k])
        assert bad.size == 0, (what, i, bad[:8].tolist(), got[i, bad[0][0]].tolist(), e[bad[0][0]].tolist())
        assert not got[i, k:].any(), (what, i)


MIXED = PR.mixed_batch(70, 97)   # n = 3; 70 x 97: no multiple of the 32-pixel tile, the 64-lane wave or the 4096-pixel chunk


@pytest.mark.parametrize("connectivity", [4, 8])
def test_mixed_batch_equals_the_restatement(connectivity):
    exp, exp_labels = _ref(("mixed", connectivity), MIXED, (1, 2, 3, 4), connectivity)
    assert all(len(e) > 8 for e in exp) and {int(c) for e in exp for c in e[:, 0]} == {1, 2, 3, 4}
    mask = _dev(MIXED)
    for classes in ((), (3, 1), (1, 2, 3, 4)):
        runs = [_call(mask, classes, connectivity, fill=fill) for fill in (0x00, 0xFF)]
        for counts, props, labels in runs:
            _assert_rows(props, counts, [_subset(e, classes) for e in exp], (connectivity, classes))
            assert np.array_equal(labels, exp_labels)
        for a, b in zip(*runs):
            assert np.array_equal(a, b)   # two calls, the same bits; a scratch word read before it is written would differ
    check(mask)


def test_no_background_measures_every_class():
    exp, exp_labels = _ref(("mixed_nobg", 4), MIXED[:1], (0, 1, 2, 3, 4), 4, background=-1)
    counts, props, labels = _call(_dev(MIXED[:1]), (0, 1, 2, 3, 4), 4, background=-1)
    _assert_rows(props, counts, exp)
    assert np.array_equal(labels, exp_labels) and (labels >= 0).all()


def test_runs_that_end_one_pixel_into_the_next_tile():
    m = SK.crack_map(33, 65, 5)
    exp, exp_labels = _ref(("crack", 8), m[None], (1, 2), 8)
    assert exp[0][:, 15].sum() > 50 and exp[0][:, 16].sum() > 2
    counts, props, labels = _call(_dev(m), (1, 2), 8)
    _assert_rows(props, counts, exp)
    assert np.array_equal(labels, exp_labels)
    counts, props, _ = _call(_dev(m), (2,), 4, want_labels=False)
    _assert_rows(props, counts, _ref(("crack4", 4), m[None], (2,), 4)[0])


def test_one_class_filling_a_wide_image():
    m = np.ones((8, 4096), np.uint8)   # a run spans whole waves; the whole plane is the class: d2 from the virtual point
    exp, _ = _ref(("wide", 4), m[None], (1,), 4)
    assert len(exp[0]) == 1 and exp[0][0, 10] > 1 << 32 and exp[0][0, 14] == 64 + 4095 * 4095
    for classes in ((), (1,)):
        counts, props, labels = _call(_dev(m), classes, 4)
        _assert_rows(props, counts, [_subset(exp[0], classes)])
        assert not labels.any()


def test_diagonal_staircase_under_both_connectivities():
    m = PR.staircase(40, 40)
    e4, e8 = _ref(("stairs", 4), m[None], (1,), 4)[0][0], _ref(("stairs", 8), m[None], (1,), 8)[0][0]
    assert len(e4) == 40 and len(e8) == 1   # the documented difference: 40 regions share the one plane's skeleton
    c4, p4, _ = _call(_dev(m), (1,), 4)
    c8, p8, _ = _call(_dev(m), (1,), 8)
    _assert_rows(p4, c4, [e4])
    _assert_rows(p8, c8, [e8])
    assert p4[0, :40, 15].tolist() == [1] * 40 and p8[0, 0, 15] == 40 and p4[0, :40, 16].sum() == p8[0, 0, 16] == 2
    assert p4[0, :40, 18].sum() == p8[0, 0, 18]


def test_isolated_square_has_no_skeleton():
    counts, props, _ = _call(_dev(PR.square2(16, 16)), (1,), 4)
    assert counts.tolist() == [1] and props[0, 0, 14:19].tolist() == [1, 0, 0, -1, 0] and props[0, 0, 2] == 4
    _assert_rows(props, counts, _ref(("square2", 4), PR.square2(16, 16)[None], (1,), 4)[0])


def test_more_regions_than_rows():
    m = RR.checkerboard(130, 130)
    exp, exp_labels = _ref(("checker", 4), m[None], (1,), 4)
    total = len(exp[0])
    assert total == 130 * 130 // 2
    mask = _dev(m)
    counts, props, labels = _call(mask, (1,), 4, max_regions=100)
    assert counts.tolist() == [total]                       # the true total, and the guard bands held (checked in _call)
    assert np.array_equal(props[0], exp[0][:100]) and np.array_equal(labels, exp_labels)
    counts, props, _ = _call(mask, (1,), 4, max_regions=total, want_labels=False)
    _assert_rows(props, counts, exp)
    # max_regions == 0: the counts and the labels alone, props may be NULL
    n, H, W = mask.shape
    nbytes = _lib.props_symbol("vitseg_region_props_scratch_bytes")(n, H, W, 0, 0)
    scratch, cnt = guarded((nbytes,), torch.uint8, name="scratch"), guarded((1,), torch.int32, name="counts")
    _lib.check(_lib.props_symbol("vitseg_region_props")(mask.data_ptr(), n, H, W, 4, 0, None, 0, 0, cnt.data_ptr(), None, 0, None,
                                                        scratch.data_ptr(), nbytes, _stream()))
    torch.cuda.synchronize()
    check(scratch, cnt)
    assert cnt.cpu().tolist() == [total]


def test_routes_give_identical_bits():
    exp, _ = _ref(("mixed", 8), MIXED, (1, 2, 3, 4), 8)
    mask = _dev(MIXED)
    res, glo = _call(mask, (2, 4), 8, route=RESIDENT), _call(mask, (2, 4), 8, route=GLOBAL, fill=0x00)
    for a, b in zip(res, glo):
        assert np.array_equal(a, b)
    _assert_rows(res[1], res[0], [_subset(e, (2, 4)) for e in exp])


def test_each_image_alone_gives_the_bits_it_has_in_the_batch():
    mask = _dev(MIXED)
    counts, props, labels = _call(mask, (1, 2, 3, 4), 4)
    for i in range(3):
        c1, p1, l1 = _call(mask[i:i + 1].contiguous(), (1, 2, 3, 4), 4, fill=0x00)
        assert c1[0] == counts[i] and np.array_equal(p1[0], props[i]) and np.array_equal(l1[0], labels[i])


@pytest.mark.parametrize("connectivity,background", [(4, 0), (8, -1)])
def test_labels_and_record_fields_are_those_of_vitseg_regions(connectivity, background):
    mask = _dev(MIXED)
    counts, props, labels = _call(mask, (2,), connectivity, background)
    n, H, W = mask.shape
    nbytes = _lib.region_symbol("vitseg_regions_scratch_bytes")(n, H, W)
    scratch = guarded((nbytes,), torch.uint8, name="scratch")
    rc, rec, rl = guarded((n,), torch.int32), guarded((n, 512, 8), torch.int32), guarded((n, H, W), torch.int32)
    _lib.check(_lib.region_symbol("vitseg_regions")(mask.data_ptr(), n, H, W, connectivity, background, rc.data_ptr(),
                                                    rec.data_ptr(), 512, rl.data_ptr(), scratch.data_ptr(), nbytes, _stream()))
    torch.cuda.synchronize()
    check(scratch, rc, rec, rl)
    rec = rec.cpu().numpy().astype(np.int64)
    assert np.array_equal(rc.cpu().numpy(), counts) and np.array_equal(rl.cpu().numpy(), labels) and counts.max() <= 512
    # (class, y_min, x_min, y_max, x_max, area, first) -> (class, first, area, y_min, x_min, y_max, x_max)
    assert np.array_equal(props[:, :, :7], rec[:, :, [0, 6, 5, 1, 2, 3, 4]])


# ---- the Python surface ----

def test_region_props_python():
    exp, exp_labels = _ref(("mixed", 4), MIXED, (1, 2, 3, 4), 4)
    got, labels = regions.region_props(MIXED, skeleton_classes="all", return_labels=True)
    assert len(got) == 3 and labels.is_cuda and np.array_equal(labels.cpu().numpy(), exp_labels)
    for g, e in zip(got, exp):
        assert g.dtype == np.int64 and np.array_equal(g, e)
    one = regions.region_props(torch.from_numpy(MIXED[1]).long(), skeleton_classes=[3])
    assert np.array_equal(one, _subset(exp[1], (3,)))
    plain = regions.region_props(torch.from_numpy(MIXED).to(DEV))
    boxes = regions.region_boxes(MIXED)
    for p, e, b in zip(plain, exp, boxes):
        assert np.array_equal(p, _subset(e, ())) and np.array_equal(p[:, [0, 3, 4, 5, 6, 2, 1]], b)
    # more regions than the first call holds: one more call sized to the count
    m = RR.checkerboard(130, 130)
    big = regions.region_props(m, skeleton_classes=[1])
    assert len(big) == 8450 > regions.DEFAULT_MAX_REGIONS and np.array_equal(big, _ref(("checker", 4), m[None], (1,), 4)[0][0])
    with pytest.raises(ValueError):
        regions.region_props(np.zeros((1, 2000, 2000), np.uint8), skeleton_classes=[1], route="resident")


def test_predict_regions_props_and_evaluator():
    from visiontransformer_amd import synth
    from visiontransformer_amd.model import ViTSegmentationModel
    model = ViTSegmentationModel(3, 16, 192, 1, 3, image_size=224, device=DEV).eval()
    x = torch.from_numpy(synth.make_images(model.cfg, 2, seed=1)).to(DEV)
    recs, mask = model.predict_regions(x, props=True, skeleton_classes=[1, 2], min_area=4, connectivity=8, return_mask=True)
    cleaned = clean.clean_mask(model.predict_mask(x), min_area=4, connectivity=8)
    assert torch.equal(mask, cleaned)
    want = regions.region_props(cleaned, skeleton_classes=[1, 2], connectivity=8)
    assert len(recs) == 2 and all(np.array_equal(a, b) and a.shape[1] == 20 for a, b in zip(recs, want))
    assert all((r[:, 2] >= 4).all() for r in recs)
    boxes = model.predict_regions(x, min_area=4, connectivity=8)   # the default path: the box records of before
    assert all(b.dtype == np.int32 and b.shape[1] == 7 and np.array_equal(b[:, [0, 6, 5]], r[:, :3]) for b, r in zip(boxes, recs))
    with pytest.raises(ValueError):
        model.predict_regions(x, skeleton_classes=[1])
    # Evaluator.region_props: both maps, a ground truth of another size
    from visiontransformer_amd.preprocess import NEAREST_PIL, nearest_table
    pred = np.stack([SK.crack_map(96, 96, 40 + i) for i in range(2)])
    big = np.stack([SK.crack_map(130, 171, 50 + i) for i in range(2)])
    small = big[:, nearest_table(130, 96, NEAREST_PIL)][:, :, nearest_table(171, 96, NEAREST_PIL)]
    ev = metrics.Evaluator(3, DEV)
    got = ev.region_props(torch.from_numpy(pred), torch.from_numpy(big), skeleton_classes=[1, 2], connectivity=8,
                          pixel_size=0.5)
    assert len(got) == 2
    for i, d in enumerate(got):
        for name, m in (("pred", pred[i]), ("gt", small[i])):
            exp = regions.props_from_records(PR.props_one(m, (1, 2), 0, 8)[0], 0.5)
            assert len(d[name]) == len(exp) > 0
            for a, b in zip(d[name], exp):
                assert a.keys() == b.keys() == set(regions.PROPS_KEYS)
                for key in a:
                    assert a[key] == pytest.approx(b[key], rel=1e-12, nan_ok=True), key
    assert list(ev.region_props(torch.from_numpy(pred))[0]) == ["pred"]


def test_evaluate_to_csv_writes_the_props_file_and_leaves_the_first(tmp_path):
    from visiontransformer_amd.model import ViTSegmentationModel
    model = ViTSegmentationModel(3, 16, 192, 1, 3, image_size=224, device=DEV).eval()
    batches = scripts.ce_batches(model.cfg, 4, 2, seed=3)
    info = (7, "ID7P16H192A3", 16, 192, 1, 3)
    plain, both = str(tmp_path / "a" / "m_metrics.csv"), str(tmp_path / "b" / "m_metrics.csv")
    scripts.evaluate_to_csv(model, batches, info, plain, 3, 2, DEV)
    scripts.evaluate_to_csv(model, batches, info, both, 3, 2, DEV, props_classes=[1, 2], props_pixel_size=0.5, min_area=4,
                            region_connectivity=8)
    assert os.listdir(tmp_path / "a") == ["m_metrics.csv"]       # without the argument: the file of before
    assert sorted(os.listdir(tmp_path / "b")) == ["m_metrics.csv", "m_region_props.csv"]
    rows = list(csv.reader(open(tmp_path / "b" / "m_region_props.csv", newline="")))
    assert rows[0] == regions.PROPS_CSV_COLUMNS
    col = {k: i for i, k in enumerate(rows[0])}
    ev = metrics.Evaluator(3, DEV)
    want = []
    for bn in range(2):
        with torch.no_grad():
            mask = clean.clean_mask(model.predict_mask(batches[bn][0].to(DEV)), min_area=4)
        gt = batches[bn][1].reshape(2, batches[bn][1].shape[-2], batches[bn][1].shape[-1])
        for idx, m in enumerate(ev.region_props(mask, gt, skeleton_classes=[1, 2], connectivity=8, pixel_size=0.5)):
            for source in ("pred", "gt"):
                want += [regions.props_csv_row(source, info, bn, idx, r, d) for r, d in enumerate(m[source])]
    assert len(rows) == 1 + len(want) and {r[0] for r in rows[1:]} == {"pred", "gt"}
    for r, w in zip(rows[1:], want):
        assert r[:11] == [str(v) for v in w[:11]]
        for key in ("Area", "Major_Axis", "Orientation", "Perimeter", "Length", "Width_Mean"):
            assert float(r[col[key]]) == pytest.approx(float(w[col[key]]), rel=1e-12, nan_ok=True), key
