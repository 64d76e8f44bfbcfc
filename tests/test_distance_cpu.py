"""CPU (-m "not gpu"): the numpy restatement of vitseg_distance_stats (tests/distance_ref.py) -- its routes against each other
and against the committed goldens -- and the host arithmetic of the boundary-distance metrics (metrics.distances_from_stats):
the percentile against np.percentile, PAED against the reference's formula run in float32 torch, the empty-set rules; the
exports."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import distance_ref as R
from visiontransformer_amd import _lib, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "distance", "distance.npz"))


def _random_cases(count, seed, max_h=31, max_w=47):
    """(gt, pred) pairs of labels 0 / 1 from 1 x 9 up to max_h x max_w, both sets non-empty."""
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < count:
        H, W = (1, 9) if not out else (int(rs.randint(1, max_h + 1)), int(rs.randint(1, max_w + 1)))
        dens = rs.choice([0.05, 0.3, 0.7])
        gt = (rs.rand(H, W) < dens).astype(np.uint8)
        pred = R.shifted(gt, int(rs.randint(0, 3)) % H, int(rs.randint(0, 3)) % W) if rs.rand() < 0.3 else \
            (rs.rand(H, W) < dens).astype(np.uint8)
        if gt.any() and pred.any():
            out.append((gt, pred))
    return out


CASES = _random_cases(200, 11)


def _assert_same_stats(a, b, what):
    (ai, af), (bi, bf) = a, b
    assert np.array_equal(ai, bi), (what, ai, bi)
    N = ai[..., 0] + ai[..., 1]
    tol = R.sum_bound(N)[..., None] * np.abs(bf)
    assert (np.abs(af - bf) <= tol).all(), (what, af, bf)


def _small_inputs():
    rs = np.random.RandomState(5)
    for H, W in [(1, 1), (1, 9), (7, 1), (5, 5), (13, 21), (32, 32), (17, 32)]:
        for name, (g, p) in R.mask_cases(H, W, seed=H + W).items():
            yield f"{name}_{H}x{W}", g, p, [0, 1, 7]
    for H, W in [(9, 14), (32, 27)]:
        yield f"classes_{H}x{W}", R.class_map(int(rs.randint(99)), H, W, 3), R.class_map(int(rs.randint(99)), H, W, 3), [0, 1, 2]


def test_brute_force_and_edt_routes_agree():
    for what, g, p, classes in _small_inputs():
        for mode in (0, 1):
            a = R.stats_ref_multi(g[None], p[None], classes, mode, R.GOLDEN_PERCENTILES, "brute")
            b = R.stats_ref_multi(g[None], p[None], classes, mode, R.GOLDEN_PERCENTILES, "edt")
            for pct in a:
                _assert_same_stats(a[pct], b[pct], (what, mode, pct))


def test_brute_force_and_scipy_routes_agree():
    pytest.importorskip("scipy")
    for what, g, p, classes in _small_inputs():
        assert np.array_equal(R.border_numpy(g == 1), R.border_scipy(g == 1)), what
        for mode in (0, 1):
            a = R.stats_ref_multi(g[None], p[None], classes, mode, R.GOLDEN_PERCENTILES, "brute")
            b = R.stats_ref_multi(g[None], p[None], classes, mode, R.GOLDEN_PERCENTILES, "scipy")
            for pct in a:
                _assert_same_stats(a[pct], b[pct], (what, mode, pct))


def test_goldens_equal_the_restatement():
    cases = R.golden_cases()
    assert {k.split(".")[0] for k in Z.files} == set(cases)
    for name, (g, p, classes) in cases.items():
        assert np.array_equal(Z[f"{name}.gt"], g) and np.array_equal(Z[f"{name}.pred"], p)
        assert list(Z[f"{name}.classes"]) == classes
        route = "brute" if g.size <= 1200 else "edt"
        for mode in (0, 1):
            res = R.stats_ref_multi(g[None], p[None], classes, mode, R.GOLDEN_PERCENTILES, route)
            for (num, den), (si, sf) in res.items():
                _assert_same_stats((Z[f"{name}.m{mode}.p{num}_{den}.i"], Z[f"{name}.m{mode}.p{num}_{den}.f"]),
                                   (si[0], sf[0]), (name, mode, num, den))


def test_straddle_and_plateau_cases_are_what_they_claim():
    for a, b, bit in [(31, 33, 10), (1023, 1025, 20)]:
        g, p = R.bucket_straddle_case(a, b)
        si, _ = R.stats_one(g, p, 1, 0, 1, 2)
        assert list(si) == [1, 2, a * a, b * b, a * a, b * b] and a * a < (1 << bit) < b * b
    g, p = R.plateau_case()
    n, m, ap, pa, _ = R.fields_one(g, p, 1, 0)
    pooled = np.sort(np.concatenate([ap, pa]))
    assert n + m == 141 and int((pooled == 25).sum()) > 120 and pooled[0] < 25
    for num, den in R.GOLDEN_PERCENTILES[1:3]:
        si, _ = R.stats_of_fields((n, m, ap, pa, np.zeros(2)), num, den)
        assert si[4] == si[5] == 25


def test_percentile_equals_numpy():
    """The rational position lo + frac against np.percentile's float position q / 100 * (N - 1): they can round apart only
    where frac is within an ulp of 0 or 1, which rtol = 1e-12 covers."""
    worst = 0.0
    for k, (g, p) in enumerate(CASES):
        mode = k % 2
        if mode == 1 and not (R.border_numpy(g == 1).any() and R.border_numpy(p == 1).any()):
            mode = 0
        d = R.pooled_distances(g, p, 1, mode)
        for q in (0, 50, 95, 100, 99.5, 12.5):
            num, den = metrics.percentile_fraction(q)
            si, sf = R.stats_ref(g[None], p[None], [1], mode, num, den)
            got = metrics.distances_from_stats(si, sf, num, den)[0][0]["hd_percentile"]
            exp = float(np.percentile(d, q))
            assert got == pytest.approx(exp, rel=1e-12, abs=0.0), (k, q, got, exp)
            if exp:
                worst = max(worst, abs(got - exp) / exp)
    print(f"worst relative difference to np.percentile: {worst:.3g}")


def _paed_float32_torch(gt, pred):
    """The reference's formula (model/PAED/classes.py:209-258) on the pixel sets of two 0 / 1 maps, in float32 torch."""
    a = torch.from_numpy(np.argwhere(gt)).float()
    b = torch.from_numpy(np.argwhere(pred)).float()
    n, m = len(a), len(b)
    if n == 0 and m == 0:
        return 0.0
    if n == 0:
        return float(torch.sum(torch.sqrt(b[:, 0] ** 2 + b[:, 1] ** 2)) / m)
    if m == 0:
        return float(torch.sum(torch.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2)) / n)
    d = torch.sqrt(torch.sum((a[:, None, :] - b[None, :, :]) ** 2, dim=2))
    s1, s2 = torch.sum(d.min(dim=1).values), torch.sum(d.min(dim=0).values)
    return float((s1 + s2 + 0.001) / (n + m + 0.001))


def test_paed_equals_the_formula_in_float32_torch():
    """N float32 roundings of non-negative terms (the roots, the running sums) and the two of the quotient: (N + 2) 2^-23."""
    worst = 0.0
    for g, p in CASES:
        si, sf = R.stats_ref(g[None], p[None], [1], 0, 19, 20)
        got = metrics.distances_from_stats(si, sf, 19, 20)[0][0]["paed"]
        exp = _paed_float32_torch(g, p)
        N = int(si[0, 0, 0] + si[0, 0, 1])
        bound = (N + 2) * 2.0 ** -23
        assert abs(got - exp) <= bound * abs(got), (g.shape, got, exp)
        worst = max(worst, abs(got - exp) / (bound * abs(got)))
    print(f"worst |fp64 - float32| / bound: {worst:.3g}")
    for g, p in [(np.zeros((5, 7), np.uint8), CASES[3][1]), (CASES[4][0], np.zeros_like(CASES[4][0])),
                 (np.zeros((3, 3), np.uint8), np.zeros((3, 3), np.uint8))]:   # the empty-set branches
        si, sf = R.stats_ref(g[None], p[None], [1], 0, 19, 20)
        got = metrics.distances_from_stats(si, sf, 19, 20)[0][0]["paed"]
        N = int(si[0, 0, 0] + si[0, 0, 1])
        assert abs(got - _paed_float32_torch(g, p)) <= (N + 2) * 2.0 ** -23 * abs(got)


def test_empty_set_rules_through_distances_from_stats():
    g = np.zeros((4, 6), np.uint8)
    g[1, 2] = g[3, 5] = 1
    z = np.zeros_like(g)
    origin_sum = np.sqrt(1.0 + 4.0) + np.sqrt(9.0 + 25.0)
    for mode in (0, 1):
        both = metrics.distances_from_stats(*R.stats_ref(z[None], z[None], [1], mode, 19, 20), 19, 20)[0][0]
        assert both["n"] == both["m"] == 0 and both["paed"] == 0.0
        for gt, pred, key in [(g, z, "n"), (z, g, "m")]:
            si, sf = R.stats_ref(gt[None], pred[None], [1], mode, 19, 20)
            assert list(si[0, 0, 2:]) == [-1, -1, -1, -1]
            d = metrics.distances_from_stats(si, sf, 19, 20)[0][0]
            assert d[key] == 2 and d["n"] + d["m"] == 2
            assert d["paed"] == (origin_sum / 2 if mode == 0 else 0.0)
            for k in ("hausdorff", "hd_percentile", "assd", "mean_AP", "mean_PA"):
                assert np.isnan(d[k]), k
        for k in ("hausdorff", "hd_percentile", "assd", "mean_AP", "mean_PA"):
            assert np.isnan(both[k]), k
    # hand-made statistics: a full record, and the sums of an empty side never reach the other numbers
    si = np.array([[[2, 3, 16, 9, 4, 9]]], np.int64)
    sf = np.array([[[6.0, 5.0]]])
    d = metrics.distances_from_stats(si, sf, 1, 2)[0][0]
    assert d["hausdorff"] == 4.0 and d["hd_percentile"] == 2.0 and d["assd"] == 11.0 / 5
    assert d["mean_AP"] == 3.0 and d["mean_PA"] == 5.0 / 3 and d["paed"] == (11.0 + 0.001) / (5 + 0.001)
    assert metrics.distances_from_stats(si, sf, 5, 8)[0][0]["hd_percentile"] == 2.0 + 0.5   # 5 * 4 / 8 = 2.5: lo = 2, frac 0.5
    with pytest.raises(ValueError):
        metrics.distances_from_stats(si[0], sf, 1, 2)
    with pytest.raises(ValueError):
        metrics.distances_from_stats(si, sf, 3, 2)
    assert metrics.percentile_fraction(95) == (19, 20) and metrics.percentile_fraction(99.5) == (199, 200)
    assert metrics.percentile_fraction(0) == (0, 1) and metrics.percentile_fraction(100) == (1, 1)
    for bad in (-1, 100.5, 33.333):
        with pytest.raises(ValueError):
            metrics.percentile_fraction(bad)


def test_exports_are_declared_and_sized_on_the_host():
    assert _lib.DISTANCE_EXPORTS == ["vitseg_distance_scratch_bytes", "vitseg_distance_stats"]
    assert set(_lib.DISTANCE_EXPORTS) <= set(_lib._LATE_EXPORTS) <= set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "vitseg.h")).read()
    declared = set(re.findall(r"\b(vitseg_[a-z0-9_]+)\s*\(", hdr))
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in _lib.DISTANCE_EXPORTS:
        assert name in declared and hasattr(l, name), name
        assert _lib.distance_symbol(name) is not None
    f = _lib.distance_symbol("vitseg_distance_scratch_bytes")   # host arithmetic
    assert f(0, 4, 4) == 0 and f(1, 0, 4) == 0 and f(1, 4, 16385) == 0 and f(32768, 1, 1) == 0
    assert f(32767, 1, 1) > 0 and f(1, 16384, 16384) > 0
    px = 32 * 512 * 512
    assert 10 * px <= f(32, 512, 512) <= 10.2 * px   # about ten bytes per pixel of the batch
    assert metrics.CSV_COLUMNS[8:11] == ["Accuracy", "Mean_IoU", "Mean_Dice"] and len(metrics.CSV_COLUMNS) == 16
