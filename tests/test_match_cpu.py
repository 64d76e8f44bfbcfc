"""CPU: the numpy restatement of vitseg_region_match (tests/match_ref.py) against its naive second form and the committed
scipy goldens, the laws the statistics obey, and the host arithmetic and argument checks of metrics.py."""
import math
import os

import numpy as np
import pytest
import torch

import match_ref as M
import regions_ref as R
from visiontransformer_amd import metrics
from visiontransformer_amd._lib import MATCH_EXPORTS, MATCH_STATS

Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "match", "match.npz"))
CASES = M.match_cases()
_RESULTS = {}


def _ref(name):
    """The restatement's (stats, pred_info, gt_info) of a case, computed once."""
    if name not in _RESULTS:
        c = CASES[name]
        _RESULTS[name] = M.match_ref(c["pred"], c["gt"], c["classes"], **M.case_kwargs(c))
    return _RESULTS[name]


def test_golden_holds_the_cases():
    assert MATCH_STATS == M.STATS and MATCH_EXPORTS == ["vitseg_region_match_scratch_bytes", "vitseg_region_match"]
    for name, c in CASES.items():
        assert np.array_equal(Z[f"{name}.pred"], c["pred"]) and np.array_equal(Z[f"{name}.gt"], c["gt"]), name
        assert Z[f"{name}.classes"].tolist() == c["classes"]
        assert Z[f"{name}.params"].tolist() == [c["connectivity"], c["background"], c["ignore_label"], *c["thr"], *c["cov"]]


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_golden(name):
    stats, pinfo, ginfo = _ref(name)
    assert stats.dtype == np.int64 and np.array_equal(stats, Z[f"{name}.stats"])
    for i in range(len(stats)):
        assert np.array_equal(M.table(pinfo[i]), Z[f"{name}.pred_table.{i}"]), i
        assert np.array_equal(M.table(ginfo[i]), Z[f"{name}.gt_table.{i}"]), i


# the naive form takes kp * kg masks per class: the single images of up to 97 x 131 pixels (the goldens pin the others with it)
@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["pred"].size <= 97 * 131 and len(c["classes"]) < 16))
def test_restatement_equals_the_naive_form(name):
    c = CASES[name]
    for a, b in zip(_ref(name), M.match_ref(c["pred"], c["gt"], c["classes"], form=M.match_naive, **M.case_kwargs(c))):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", sorted(CASES))
def test_partners_are_unique_and_mutual_and_the_laws_hold(name):
    c = CASES[name]
    stats, pinfo, ginfo = _ref(name)
    for i in range(len(stats)):
        pt, gt = M.table(pinfo[i]), M.table(ginfo[i])
        pm, gm = pt[pt[:, 1] >= 0], gt[gt[:, 1] >= 0]
        assert len(set(pm[:, 1])) == len(pm) and len(set(gm[:, 1])) == len(gm)               # no partner twice
        assert sorted(zip(pm[:, 0], pm[:, 1])) == sorted(zip(gm[:, 1], gm[:, 0]))            # and each is its partner's
        assert len(pm) == stats[i, :, 2].sum()
        assert len(gt) == stats[i, :, 0].sum() and len(pt) == stats[i, :, 1].sum()
    n_gt, n_pred, tp, found, confirmed, sq, si, su = np.moveaxis(stats, 2, 0)
    assert (tp <= np.minimum(n_gt, n_pred)).all() and (si <= su).all() and (sq <= tp * M.ONE).all()
    assert (found <= n_gt).all() and (confirmed <= n_pred).all()
    if c["cov"][0] * c["thr"][1] <= c["thr"][0] * c["cov"][1]:   # coverage <= threshold: a matched region is covered enough
        assert (found >= tp).all() and (confirmed >= tp).all()
    # the threshold sits strictly below every matched pair's IoU: sum_q / 2^32 > tp * thr
    assert (sq * c["thr"][1] >= tp * M.ONE * c["thr"][0]).all()


def test_the_cases_the_thresholds_turn_on():
    half, tq = _ref("iou_steps_half")[0][0], _ref("iou_steps_three_quarters")[0][0]
    assert half[:, 2].tolist() == [3, 1] and tq[:, 2].tolist() == [2, 1]     # 2/4 and 6/12 never; 3/4 only at one half
    assert half[0, 5] == (3 * M.ONE) // 4 + (4 * M.ONE) // 5 + M.ONE
    st = _ref("straddle_40x70")[0][0]
    assert st[0].tolist()[:5] == [2, 1, 0, 2, 1] and st[1].tolist()[:5] == [2, 1, 1, 2, 1]
    vb = _ref("void_band_36x48")
    assert vb[0][0, :, 1].tolist() == [1, 2]                                  # the region inside the band does not exist
    assert M.table(vb[1][0])[:, 2].tolist() == [32, 40, 48]                   # half of 8 x 8 counted, all of it covered
    assert _ref("empty_pred")[0][0, 0].tolist() == [2, 0, 0, 0, 0, 0, 0, 0]
    assert _ref("empty_gt")[0][0, 0].tolist() == [0, 1, 0, 0, 0, 0, 0, 0]
    one = _ref("class_in_one_map")[0][0]
    assert one[1, :3].tolist() == [2, 0, 0] and one[2, :3].tolist() == [0, 1, 0]
    ch = _ref("checker_40x51")[0][0]
    assert ch[:, 2].sum() == 40 * 49 and ch[:, 1].sum() == 40 * 51           # every pixel a region; the two columns differ


@pytest.mark.parametrize("name", ["speckle5_97x131", "checker_40x51", "batch5_160x200_c8", "k16_64x80"])
def test_a_map_against_itself_matches_everything(name):
    c = CASES[name]
    kw = dict(M.case_kwargs(c), ignore_label=-1)
    stats, pinfo, ginfo = M.match_ref(c["pred"], c["pred"], c["classes"], **kw)
    n_gt, n_pred, tp, found, confirmed, sq, si, su = np.moveaxis(stats, 2, 0)
    assert (tp == n_gt).all() and (tp == n_pred).all() and (found == tp).all() and (confirmed == tp).all()
    assert (sq == tp * M.ONE).all() and (si == su).all() and tp.sum() > 0
    assert np.array_equal(pinfo, ginfo)


@pytest.mark.parametrize("name", ["speckle5_97x131_novoid", "straddle_40x70", "strip_1x70", "k16_64x80"])
def test_swapping_the_maps_swaps_the_roles(name):
    c = CASES[name]
    assert c["ignore_label"] < 0
    a = _ref(name)
    b = M.match_ref(c["gt"], c["pred"], c["classes"], **M.case_kwargs(c))
    assert np.array_equal(a[0][:, :, [1, 0, 2, 4, 3, 5, 6, 7]], b[0])
    assert np.array_equal(a[1], b[2]) and np.array_equal(a[2], b[1])


def test_every_branch_on_every_image_of_the_batch():
    """What tests/test_gpu_match.py relies on: the seed of batch5_160x200 gives every image matched, missed and false regions,
    found regions that are not matched, and predicted regions that the void band reduces."""
    c = CASES["batch5_160x200"]
    stats, pinfo, _ = _ref("batch5_160x200")
    tot = stats.sum(axis=1)
    n_gt, n_pred, tp, found = tot[:, 0], tot[:, 1], tot[:, 2], tot[:, 3]
    assert (tp > 0).all() and (n_pred - tp > 0).all() and (n_gt - tp > 0).all() and (found > tp).all()
    for i in range(5):
        rec, lab = R.regions_one(c["pred"][i], 0, 4)
        void = c["gt"][i] == 255
        in_void = np.bincount(lab[void & (lab >= 0)], minlength=len(rec))
        asked = np.isin(rec[:, 0], c["classes"])
        assert ((in_void > 0) & (in_void < rec[:, 5]) & asked).any(), i     # a region the band reduces
        assert ((in_void == rec[:, 5]) & asked).any(), i                    # and one it removes
        assert asked.sum() - ((in_void == rec[:, 5]) & asked).sum() == stats[i, :, 1].sum()


def test_matches_from_stats_and_pooling():
    st = np.zeros((2, 3, 8), np.int64)
    st[0, 0] = (4, 3, 2, 3, 2, M.ONE + M.ONE // 2, 30, 40)     # tp 2, fp 1, fn 2, IoU sum 1.5
    st[0, 1] = (0, 0, 0, 0, 0, 0, 0, 0)                        # nothing anywhere
    st[0, 2] = (2, 0, 0, 1, 0, 0, 0, 0)                        # only missed
    st[1, 0] = (1, 1, 1, 1, 1, M.ONE, 7, 7)
    rows = metrics.matches_from_stats(st)
    assert len(rows) == 2 and len(rows[0]) == 3
    r = rows[0][0]
    assert (r["n_gt"], r["n_pred"], r["tp"], r["fp"], r["fn"]) == (4, 3, 2, 1, 2)
    assert r["rq"] == 2 / 3.5 and r["sq"] == 0.75 and r["pq"] == 1.5 / 3.5 and math.isclose(r["pq"], r["sq"] * r["rq"])
    assert r["precision"] == 2 / 3 and r["recall"] == 0.5 and r["f1"] == 4 / 7
    assert r["found_rate"] == 0.75 and r["confirmed_rate"] == 2 / 3 and r["mean_matched_iou"] == 0.75
    assert all(math.isnan(rows[0][1][k]) for k in metrics.REGION_KEYS)
    m = rows[0][2]
    assert m["pq"] == 0.0 and m["rq"] == 0.0 and m["recall"] == 0.0 and m["found_rate"] == 0.5 and m["f1"] == 0.0
    assert all(math.isnan(m[k]) for k in ("sq", "precision", "confirmed_rate", "mean_matched_iou"))
    assert rows[1][0]["pq"] == 1.0
    pooled = metrics.pool_region_stats([st[:1], st[1:], st[1]])
    assert pooled.shape == (3, 8) and np.array_equal(pooled, st[0] + 2 * st[1])
    p = metrics.matches_from_stats(pooled)
    assert len(p) == 3 and p[0]["tp"] == 4 and p[0]["pq"] == 3.5 / 5.5
    assert np.array_equal(metrics.pool_region_stats([torch.from_numpy(st)]), st.sum(axis=0))
    for bad in ([], [st, st[:, :2]], [np.zeros((2, 7))]):
        with pytest.raises(ValueError):
            metrics.pool_region_stats(bad)
    with pytest.raises(ValueError):
        metrics.matches_from_stats(np.zeros((2, 3, 6)))
    row = metrics.region_csv_row((7, "m"), "pooled", "", 2, 0.5, 0.5, p[0])
    assert len(row) == len(metrics.REGION_CSV_COLUMNS) and row[:10] == [7, "m", "pooled", "", 2, 0.5, 0.5, 6, 5, 4]


def test_fractions():
    assert metrics.iou_threshold_fraction(0.5) == (1, 2) and metrics.iou_threshold_fraction(0.75) == (3, 4)
    assert metrics.iou_threshold_fraction("0.999") == (999, 1000) and metrics.coverage_fraction(1) == (1, 1)
    assert metrics.coverage_fraction(0.001) == (1, 1000)
    for bad in (0.49, 1, 1.5, 0.5001, -0.5):
        with pytest.raises(ValueError):
            metrics.iou_threshold_fraction(bad)
    for bad in (0, 1.01, 0.3333, -1):
        with pytest.raises(ValueError):
            metrics.coverage_fraction(bad)


def test_region_metrics_checks_its_arguments_before_the_library(monkeypatch):
    from visiontransformer_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "match_symbol", boom)
    ev = metrics.Evaluator(5, device="cpu")
    pred = torch.zeros((1, 4, 4), dtype=torch.uint8)
    for kw in (dict(iou_threshold=0.4), dict(iou_threshold=1.0), dict(iou_threshold=0.12345), dict(coverage=0), dict(coverage=1.5),
               dict(connectivity=6), dict(background=-1), dict(background=256), dict(background=True), dict(ignore_label=0),
               dict(ignore_label=300), dict(ignore_label=2, classes=[1, 2]), dict(classes=[]), dict(classes=[1, 1]),
               dict(classes=[0, 1]), dict(classes=[256]), dict(classes=list(range(1, 255)) + [1, 2, 3])):
        with pytest.raises(ValueError):
            ev.region_metrics(pred, pred, **kw)
    for bad in (pred.long(), pred[0], pred.numpy()):
        with pytest.raises(ValueError):
            ev.region_metrics(bad, pred)
    with pytest.raises(ValueError, match="must be equal"):
        ev.region_metrics(pred, torch.zeros((2, 4, 4), dtype=torch.uint8))
    # classes=None: every class but the background and the ignore label
    assert ev._region_arguments(None, 0.5, 0.5, 4, 2, 4)[0] == [0, 1, 3]
