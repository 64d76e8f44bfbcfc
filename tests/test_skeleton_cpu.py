"""CPU (-m "not gpu"): the numpy restatement of Zhang-Suen thinning (tests/skeleton_ref.py) against hand-derived cases and
its own invariants, the host arithmetic of the crack metrics (metrics.crack_from_stats), the exports, the shim and the
scratch-size functions' answer to bad shapes.  Where skimage is installed the restatement is compared with
skimage.morphology.skeletonize, the function the reference calls."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import skeleton_ref as R
from visiontransformer_amd import _lib, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(33, 65), (64, 100)]


# ---- hand-derived cases ----

def test_a_3_by_36_bar_thins_to_its_33_pixel_centre_line():
    m = np.zeros((9, 40), np.uint8)
    m[3:6, 2:38] = 1
    s, passes = R.skeleton_one(m)
    want = np.zeros((9, 40), np.uint8)
    want[4, 3:36] = 1
    assert np.array_equal(s, want) and passes == 2 and R.end_points(s) == 2


def test_an_isolated_2_by_2_square_vanishes():
    m = np.zeros((6, 7), np.uint8)
    m[2:4, 3:5] = 1
    s, passes = R.skeleton_one(m)
    assert not s.any() and passes == 2


def test_one_pixel_wide_shapes_are_unchanged():
    L = np.zeros((12, 11), np.uint8)
    L[1:10, 2] = 1
    L[9, 2:9] = 1
    for m in (L, R.diagonal(9, 13), R.diagonal(13, 9)[:, ::-1], R.single(5, 5), R.empty(4, 4)):
        s, passes = R.skeleton_one(m)
        assert np.array_equal(s, m) and passes == 1


def test_a_full_square_thins_to_one_pixel_in_41_passes():
    s, passes = R.skeleton_one(R.full(80, 80))
    assert int(s.sum()) == 1 and passes == 41


def test_a_disc_of_radius_40_thins_to_one_pixel_in_29_passes():
    y, x = np.mgrid[-45:46, -45:46]
    s, passes = R.skeleton_one(y * y + x * x <= 1600)
    assert int(s.sum()) == 1 and passes == 29


def test_values_other_than_one_are_mask_pixels():
    m = R.crack(33, 65, 5, 2)
    assert np.array_equal(R.skeleton_one(m * 255)[0], R.skeleton_one(m)[0])


# ---- properties on every generator ----

@pytest.mark.parametrize("H,W", SIZES + [(96, 96), (100, 70), (1, 9), (7, 1), (2, 2)])
def test_subset_idempotence_and_components(H, W):
    for name, m in R.all_masks(H, W, seed=H + W).items():
        b = (m != 0).astype(np.uint8)
        s, passes = R.skeleton_one(m)
        assert s.dtype == np.uint8 and set(np.unique(s)) <= {0, 1}, name
        assert not (s & (1 - b)).any(), name                                    # a subset of the mask
        s2, p2 = R.skeleton_one(s)
        assert np.array_equal(s2, s) and p2 == 1, name                          # idempotent
        if min(H, W) < 33:
            continue
        if name in ("crack1", "crack2"):
            assert R.components(s) == R.components(b) == 1, name                # a band across the image stays one piece
        if name == "blobs":
            # No piece is ever split.  A compact piece may vanish whole: a roundish blob thins to a 2 x 2 square, and that
            # vanishes (at 33 x 65 a 20-pixel blob of this mask does), so the count itself is no invariant even here.
            lab, n = R.labelled(b)
            per = [R.components(s * (lab == i)) for i in range(1, n + 1)]
            assert n > 3 and max(per) == 1 and sum(per) == R.components(s), (name, per)


def test_noise_may_lose_components():
    """2 x 2-like specks vanish, so the component count is no invariant of the algorithm: the 64 x 64 noise mask of density
    0.5 goes from 34 pieces to 33."""
    m = (np.random.RandomState(0).rand(64, 64) < 0.5).astype(np.uint8)
    s = R.skeleton_one(m)[0]
    assert R.components(s) <= R.components(m)


def test_stats_ref_on_a_hand_made_pair():
    """gt: a 3-wide horizontal bar; pred: the same bar two rows lower.  The centre lines are 33 pixels long, do not meet the
    other bar's centre row but lie inside / outside its 3 rows as counted by hand."""
    gt, pred = np.zeros((1, 12, 40), np.uint8), np.zeros((1, 12, 40), np.uint8)
    gt[0, 3:6, 2:38] = 1      # centre line: row 4, columns 3..35
    pred[0, 5:8, 2:38] = 1    # centre line: row 6
    si, sf = R.stats_ref(gt, pred, [1, 7])
    assert si[0, 0].tolist() == [108, 108, 33, 33, 0, 0, 4, 4, 2, 2]     # d2 = 2^2 on the centre row of a 3-wide bar
    assert sf[0, 0].tolist() == [66.0, 66.0]
    assert si[0, 1].tolist() == [0, 0, 0, 0, 0, 0, -1, -1, 0, 0] and sf[0, 1].tolist() == [0.0, 0.0]
    pred[0] = 0
    pred[0, 4:7, 2:38] = 1    # one row lower: its centre line (row 5) lies in gt's last row, gt's (row 4) in its first
    si, _ = R.stats_ref(gt, pred, [1])
    assert si[0, 0, 4:6].tolist() == [33, 33]


# ---- the host arithmetic ----

def test_crack_from_stats_on_hand_made_integers():
    si = np.zeros((1, 5, 10), np.int64)
    sf = np.zeros((1, 5, 2), np.float64)
    si[0, 0] = [108, 90, 33, 30, 22, 24, 4, 9, 2, 3]
    sf[0, 0] = [66.0, 75.0]
    si[0, 1] = [0, 0, 0, 0, 0, 0, -1, -1, 0, 0]          # the class is absent from both maps
    si[0, 2] = [50, 0, 10, 0, 0, 0, 1, -1, 2, 0]         # nothing predicted
    sf[0, 2] = [10.0, 0.0]
    si[0, 3] = [0, 40, 0, 8, 0, 0, -1, 1, 0, 2]          # nothing in the ground truth
    sf[0, 3] = [0.0, 8.0]
    si[0, 4] = [30, 30, 6, 6, 0, 0, 1, 1, 2, 2]          # both present, the centre lines miss each other entirely
    sf[0, 4] = [6.0, 6.0]
    rows = metrics.crack_from_stats(si, sf)
    assert len(rows) == 1 and len(rows[0]) == 5
    a, b, c, d, e = rows[0]
    assert a["cl_precision"] == 24 / 30 and a["cl_sensitivity"] == 22 / 33
    assert a["cldice"] == pytest.approx(2 * 0.8 * (2 / 3) / (0.8 + 2 / 3), rel=1e-15)
    assert (a["length_gt"], a["length_pred"], a["endpoints_gt"], a["endpoints_pred"], a["n"], a["m"]) == (33, 30, 2, 3, 108, 90)
    assert a["mean_width_gt"] == 3.0 and a["mean_width_pred"] == 4.0
    assert a["max_width_gt"] == 3.0 and a["max_width_pred"] == 5.0
    for key in ("cldice", "cl_precision", "cl_sensitivity", "mean_width_gt", "mean_width_pred", "max_width_gt", "max_width_pred"):
        assert math.isnan(b[key]), key
    assert (b["length_gt"], b["length_pred"], b["endpoints_gt"], b["endpoints_pred"]) == (0, 0, 0, 0)
    assert c["cl_sensitivity"] == 0.0 and math.isnan(c["cl_precision"]) and math.isnan(c["cldice"])
    assert c["mean_width_gt"] == 1.0 and c["max_width_gt"] == 1.0 and math.isnan(c["mean_width_pred"]) and math.isnan(c["max_width_pred"])
    assert d["cl_precision"] == 0.0 and math.isnan(d["cl_sensitivity"]) and math.isnan(d["cldice"])
    assert d["mean_width_pred"] == 1.0 and math.isnan(d["mean_width_gt"])
    assert e["cl_precision"] == 0.0 and e["cl_sensitivity"] == 0.0 and e["cldice"] == 0.0
    with pytest.raises(ValueError):
        metrics.crack_from_stats(np.zeros((1, 2, 6), np.int64), np.zeros((1, 2, 2)))
    with pytest.raises(ValueError):
        metrics.crack_from_stats(si, np.zeros((1, 4, 2)))


def test_crack_from_stats_follows_the_restatement():
    gt = np.stack([R.crack_map(48, 80, s) for s in (1, 2)])
    pred = np.stack([R.crack_map(48, 80, s) for s in (1, 3)])
    pred[0] = np.roll(pred[0], 1, axis=0)
    si, sf = R.stats_ref(gt, pred, [1, 2])
    rows = metrics.crack_from_stats(si, sf)
    for i in range(2):
        for k, c in enumerate([1, 2]):
            G, P = gt[i] == c, pred[i] == c
            SG, SP = R.skeleton_one(G)[0] == 1, R.skeleton_one(P)[0] == 1
            r = rows[i][k]
            assert r["cl_precision"] == (SP & G).sum() / SP.sum() and r["cl_sensitivity"] == (SG & P).sum() / SG.sum()
            assert r["length_gt"] == SG.sum() and r["length_pred"] == SP.sum()
            assert 1.0 <= r["mean_width_gt"] <= r["max_width_gt"] and 1.0 <= r["mean_width_pred"] <= r["max_width_pred"]


# ---- the binding ----

def test_exports_and_header():
    assert _lib.SKELETON_EXPORTS == ["vitseg_skeleton_scratch_bytes", "vitseg_skeleton", "vitseg_skeleton_stats_scratch_bytes",
                                     "vitseg_skeleton_stats"]
    assert set(_lib.SKELETON_EXPORTS) <= set(_lib._LATE_EXPORTS) <= set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "vitseg.h")).read()
    assert re.search(r"#define\s+VITSEG_VERSION\s+110\b", hdr) and _lib.VERSION == 110
    for name in _lib.SKELETON_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert _lib.skeleton_symbol(name) is not None


def test_scratch_size_functions_return_0_for_bad_shapes():
    for name in ("vitseg_skeleton_scratch_bytes", "vitseg_skeleton_stats_scratch_bytes"):
        f = _lib.skeleton_symbol(name)
        for route in (0, 1, 2):
            assert f(0, 8, 8, route) == 0 and f(32768, 8, 8, route) == 0
            assert f(2, 0, 8, route) == 0 and f(2, 8, 0, route) == 0
            assert f(2, 16385, 8, route) == 0 and f(2, 8, 16385, route) == 0
        assert f(2, 8, 8, -1) == 0 and f(2, 8, 8, 3) == 0
        assert f(2, 8, 8, 2) > 0 and f(1, 16384, 16384, 2) > 2 * 16384 * 16384 // 8


def test_error_statuses_without_a_device():
    """Argument checks come before anything touches a device."""
    fn = _lib.skeleton_symbol("vitseg_skeleton")
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    assert fn(None, 1, 8, 8, 0, p, None, p, 64, None) == _lib.EINVAL
    assert fn(p, 1, 8, 8, 0, None, None, p, 64, None) == _lib.EINVAL
    assert fn(p, 1, 8, 8, 3, p, None, p, 64, None) == _lib.EINVAL
    assert fn(p, 0, 8, 8, 0, p, None, p, 64, None) == _lib.ESHAPE
    assert fn(p, 1, 8, 16385, 0, p, None, p, 64, None) == _lib.ESHAPE
    assert fn(p, 1, 8, 8, 2, p, None, p, 0, None) == _lib.EWORKSPACE
    fs = _lib.skeleton_symbol("vitseg_skeleton_stats")
    ok, bad = (ctypes.c_int32 * 1)(1), (ctypes.c_int32 * 1)(256)
    assert fs(p, p, 1, 8, 8, bad, 1, 2, p, p, p, 1 << 20, None) == _lib.EINVAL
    assert fs(p, p, 1, 8, 8, None, 1, 2, p, p, p, 1 << 20, None) == _lib.EINVAL
    assert fs(p, p, 1, 8, 8, ok, 0, 2, p, p, p, 1 << 20, None) == _lib.ESHAPE
    assert fs(p, p, 1, 8, 8, ok, 257, 2, p, p, p, 1 << 20, None) == _lib.ESHAPE
    assert fs(p, p, 1, 8, 8, ok, 1, 2, p, p, p, 0, None) == _lib.EWORKSPACE


def test_the_segmentation_shim_resolves_the_reference_names():
    code = "from segmentation import CrackSeg, compute_sdf; print(CrackSeg.skeletonize.__name__, compute_sdf.__name__)"
    path = os.pathsep.join(p for p in (os.path.join(ROOT, "model", "PAED"), os.environ.get("PYTHONPATH")) if p)
    env = dict(os.environ, PYTHONPATH=path)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["skeletonize", "compute_sdf"]


def test_python_surface_rejects_bad_input_before_the_device():
    import torch
    from visiontransformer_amd import skeleton
    with pytest.raises(ValueError):
        skeleton.skeletonize(np.zeros((2, 2, 2, 2), np.uint8))
    with pytest.raises(ValueError):
        skeleton.skeletonize(np.zeros((0, 4), np.uint8))
    with pytest.raises(ValueError):
        skeleton.skeletonize(np.zeros((4, 4), np.uint8), route="fast")
    with pytest.raises(ValueError):
        skeleton.CrackSeg.skeletonize(torch.zeros(1, 4, 4))


def test_the_resident_kernel_keeps_its_words_in_registers(tmp_path):
    """skeleton.hip's resident kernel holds up to 40 new words per thread in registers across a barrier, in a block of 1024
    threads: 4 waves per SIMD, so 128 registers per lane.  Past that, or with the word addresses of all 40 kept live, the
    compiler spills to private memory (seen while writing it: 68 registers), and nothing at run time reports that."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "skeleton.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    os.path.join(ROOT, "visiontransformer_amd", "csrc", "skeleton.hip"), "-o", str(out)], check=True,
                   capture_output=True)
    body = re.search(r"\.amdhsa_kernel (\S*skel_resident_kernel\S*)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S).group(2)
    nv = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
    private = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
    assert nv <= 128 and private == 0, (nv, private)


# ---- skimage, where it is installed ----

def test_the_restatement_against_skimage():
    """skimage's 2-D skeletonize cites the same paper; its implementation is a table-driven variant, so this comparison shows
    where (if anywhere) the library departs from the paper's rules on these masks."""
    morphology = pytest.importorskip("skimage.morphology")
    for H, W in SIZES:
        for name, m in R.all_masks(H, W, seed=H + W).items():
            want = morphology.skeletonize(m != 0, method="zhang").astype(np.uint8)
            assert np.array_equal(R.skeleton_one(m)[0], want), (H, W, name)
