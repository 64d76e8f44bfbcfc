"""CPU (-m "not gpu"): the numpy restatement of vitseg_regions (tests/regions_ref.py) against scipy.ndimage.label + the
reference's box rule and against the committed goldens; argument checks of regions.region_boxes before any library call."""
import os

import numpy as np
import pytest
import torch

import regions_ref as R
from visiontransformer_amd import _lib, regions

Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "regions", "regions.npz"))


@pytest.mark.parametrize("connectivity", [4, 8])
def test_restatement_equals_scipy_label(connectivity):
    pytest.importorskip("scipy")
    rs = np.random.RandomState(11 + connectivity)
    for t in range(40):
        H, W = rs.randint(1, 40, size=2)
        C = [2, 3, 17, 256][t % 4]
        m = rs.randint(0, C, size=(H, W)).astype(np.uint8)
        if t % 3 == 0:
            m = R.blobs(t, H, W, min(C, 5), radius=2)
        for bg in (0, -1, int(m.flat[0])):
            rec, lab = R.regions_one(m, bg, connectivity)
            exp, exp_lab = R.scipy_records(m, bg, connectivity)
            assert np.array_equal(rec, exp), (t, H, W, bg)
            assert np.array_equal(lab, exp_lab), (t, H, W, bg)


@pytest.mark.parametrize("name", sorted(R.golden_cases()))
def test_restatement_equals_goldens(name):
    m = Z[f"{name}.mask"]
    assert np.array_equal(m, R.golden_cases()[name])   # the generator still makes the committed masks
    for conn, bg in R.GOLDEN_VARIANTS:
        rec, lab = R.regions_one(m, bg, conn)
        assert np.array_equal(rec, Z[f"{name}.c{conn}.b{bg}"]), (conn, bg)
        # the labels map is consistent with the records: area and box of every index
        for i, r in enumerate(rec[:64]):
            ys, xs = np.nonzero(lab == i)
            assert (len(ys), ys.min(), xs.min(), ys.max(), xs.max()) == (r[5], r[1], r[2], r[3], r[4])
        assert ((lab >= 0) == (m != bg)).all() if bg >= 0 else (lab >= 0).all()


def test_golden_worst_cases_have_the_expected_counts():
    assert len(Z["checker_64.c4.b-1"]) == 64 * 64 and len(Z["checker_64.c8.b-1"]) == 2
    assert len(Z["serpentine_96.c4.b0"]) == 1 and len(Z["serpentine_96.c8.b0"]) == 1
    assert len(Z["u_70x45.c4.b0"]) == 1
    assert set(np.unique(Z["all256_48.mask"])) == set(range(256))


def test_boxes_by_class_matches_the_reference_loop():
    m = R.golden_cases()["rings_96"]
    rec, _ = R.regions_one(m, 0, 4)
    got = regions.boxes_by_class(rec)
    assert list(got) == sorted(got) and 0 not in got
    assert got == R.boxes_by_class(rec)
    pytest.importorskip("scipy")
    from scipy.ndimage import label
    for c in np.unique(m):   # the reference's loop: get_bounding_boxes(pred_labels == class_idx), class 0 skipped
        if c == 0:
            continue
        lab, nf = label(m == c)
        boxes = []
        for k in range(1, nf + 1):
            coords = np.argwhere(lab == k)
            boxes.append((*coords.min(axis=0).tolist(), *coords.max(axis=0).tolist()))
        assert got[int(c)] == boxes


def test_region_boxes_rejects_bad_arguments_before_the_library(monkeypatch):
    def no_call(name):
        raise AssertionError(f"{name} reached")
    monkeypatch.setattr(_lib, "region_symbol", no_call)
    ok = torch.zeros(2, 4, 4, dtype=torch.uint8)
    bad = [
        (torch.zeros(2, 4, 4, dtype=torch.float32), {}),          # dtype
        (torch.zeros(2, 4, 4, dtype=torch.int32), {}),
        (torch.zeros(4, dtype=torch.uint8), {}),                  # shape
        (torch.zeros(1, 2, 4, 4, dtype=torch.uint8), {}),
        (torch.zeros(2, 0, 4, dtype=torch.uint8), {}),
        (ok, {"connectivity": 6}),                                # connectivity
        (ok, {"background": 256}),                                # background
        (ok, {"background": -2}),
        (torch.full((3, 3), 256, dtype=torch.long), {}),          # value range
        (torch.full((3, 3), -1, dtype=torch.long), {}),
        ([[0, 1]], {}),
    ]
    for mask, kw in bad:
        with pytest.raises(ValueError):
            regions.region_boxes(mask, **kw)


def test_region_symbols_are_declared_and_exported():
    assert "vitseg_regions" in _lib.EXPORTS and "vitseg_regions_scratch_bytes" in _lib.EXPORTS
    f = _lib.region_symbol("vitseg_regions_scratch_bytes")
    assert f(0, 4, 4) == 0 and f(1, 0, 4) == 0 and f(1, 1 << 16, 1 << 15) == 0   # bad shapes: no size
    assert f(2, 64, 64) >= 2 * 64 * 64 * 24
    assert f(32, 512, 512) >= f(1, 512, 512) * 32 - 32 * 255
