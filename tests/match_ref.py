"""numpy restatement of vitseg_region_match (include/vitseg.h): the regions of a prediction matched against the regions of
the ground truth per class, on top of regions_ref's labelling.  Two forms: `match_one` counts the pairs from the roots of
both maps by sorting pair keys; `match_naive` enumerates all region pairs of a class through boolean masks and takes a
labelling function, so that tools/make_golden_match.py can pin the goldens with scipy.ndimage.label.  Also the cases of
tests/golden/match/match.npz.  A plain helper module, imported like regions_ref.py."""
import numpy as np

import clean_ref as K
import regions_ref as R

BATCH_SEED = 31   # tests/test_match_cpu.py: every branch on every image of batch5_160x200
STATS = ("n_gt", "n_pred", "tp", "gt_found", "pred_confirmed", "sum_q", "sum_i", "sum_u")
ONE = 1 << 32   # q of a pair with IoU 1


def _void_masked(gt, background, ignore_label):
    void = gt == ignore_label if ignore_label >= 0 else np.zeros(gt.shape, bool)
    return void, np.where(void, np.uint8(background), gt)


def _empty_info(H, W):
    info = np.zeros((H, W, 2), np.int32)
    info[..., 0] = -2
    return info


def match_one(pred, gt, classes, connectivity=4, background=0, ignore_label=-1, thr=(1, 2), cov=(1, 2)):
    """(stats int64 [K, 8] in the order of STATS, pred_info int32 [H, W, 2], gt_info int32 [H, W, 2]) of one image."""
    pred, gt = np.asarray(pred, np.uint8), np.asarray(gt, np.uint8)
    assert pred.ndim == 2 and pred.shape == gt.shape
    H, W = pred.shape
    P = H * W
    void, gm = _void_masked(gt, background, ignore_label)
    rp = R._roots(pred, background, connectivity)
    rg = R._roots(gm, background, connectivity)
    pf, gf, vf = pred.reshape(-1), gm.reshape(-1), void.reshape(-1)
    a = np.bincount(rp[(rp >= 0) & ~vf], minlength=P)      # indexed by root
    b = np.bincount(rg[rg >= 0], minlength=P)
    idx = np.arange(P)
    stats = np.zeros((len(classes), 8), np.int64)
    pinfo, ginfo = _empty_info(H, W), _empty_info(H, W)
    pi, gi = pinfo.reshape(P, 2), ginfo.reshape(P, 2)
    for k, c in enumerate(classes):
        hit = (pf == c) & (gf == c)
        keys, inter = np.unique(rp[hit] * P + rg[hit], return_counts=True)
        i, j = keys // P, keys % P
        union = a[i] + b[j] - inter
        m = inter * thr[1] > thr[0] * union
        proots = idx[(rp == idx) & (pf == c) & (a > 0)]
        groots = idx[(rg == idx) & (gf == c)]
        covp = np.bincount(rp[hit], minlength=P)
        covg = np.bincount(rg[hit], minlength=P)
        pi[proots, 0], pi[proots, 1] = -1, covp[proots]
        gi[groots, 0], gi[groots, 1] = -1, covg[groots]
        pi[i[m], 0], gi[j[m], 0] = j[m], i[m]
        stats[k] = (len(groots), len(proots), int(m.sum()), int((covg[groots] * cov[1] >= cov[0] * b[groots]).sum()),
                    int((covp[proots] * cov[1] >= cov[0] * a[proots]).sum()),
                    sum((int(x) << 32) // int(u) for x, u in zip(inter[m], union[m])), int(inter[m].sum()), int(union[m].sum()))
    return stats, pinfo, ginfo


def match_naive(pred, gt, classes, connectivity=4, background=0, ignore_label=-1, thr=(1, 2), cov=(1, 2),
                records=R.regions_one):
    """The same result from the definitions alone: every predicted region of a class against every true one through boolean
    masks.  records(mask, background, connectivity) -> (records [k, 7], labels [H, W]) as regions_ref.regions_one or
    regions_ref.scipy_records."""
    pred, gt = np.asarray(pred, np.uint8), np.asarray(gt, np.uint8)
    H, W = pred.shape
    void, gm = _void_masked(gt, background, ignore_label)
    rec_p, lab_p = records(pred, background, connectivity)
    rec_g, lab_g = records(gm, background, connectivity)
    stats = np.zeros((len(classes), 8), np.int64)
    pinfo, ginfo = _empty_info(H, W), _empty_info(H, W)
    pi, gi = pinfo.reshape(-1, 2), ginfo.reshape(-1, 2)
    for k, c in enumerate(classes):
        ps = [r for r in range(len(rec_p)) if rec_p[r, 0] == c and ((lab_p == r) & ~void).any()]
        gs = [r for r in range(len(rec_g)) if rec_g[r, 0] == c]
        n_tp = found = confirmed = sq = si = su = 0
        for r in gs:
            G = lab_g == r
            covered = int((G & (pred == c)).sum())
            found += covered * cov[1] >= cov[0] * int(G.sum())
            gi[rec_g[r, 6]] = (-1, covered)
        for r in ps:
            Pm = (lab_p == r) & ~void
            covered = int((Pm & (gm == c)).sum())
            confirmed += covered * cov[1] >= cov[0] * int(Pm.sum())
            pi[rec_p[r, 6]] = (-1, covered)
        if ps and gs:   # the intersections of all pairs at once: counts below 2^24 are exact in float32
            PM = np.stack([((lab_p == r) & ~void).reshape(-1) for r in ps]).astype(np.float32)
            GM = np.stack([(lab_g == r).reshape(-1) for r in gs]).astype(np.float32)
            assert H * W < 1 << 24
            inter = (PM @ GM.T).astype(np.int64)
            a, b = PM.sum(axis=1).astype(np.int64), GM.sum(axis=1).astype(np.int64)
            for x, y in zip(*np.nonzero(inter)):   # a pair without a shared pixel cannot match
                r, s = ps[x], gs[y]
                I = int(inter[x, y])
                U = int(a[x]) + int(b[y]) - I
                if I * thr[1] > thr[0] * U:
                    n_tp, sq, si, su = n_tp + 1, sq + (I << 32) // U, si + I, su + U
                    assert pi[rec_p[r, 6], 0] == -1 and gi[rec_g[s, 6], 0] == -1   # at most one partner each
                    pi[rec_p[r, 6], 0], gi[rec_g[s, 6], 0] = rec_g[s, 6], rec_p[r, 6]
        stats[k] = (len(gs), len(ps), n_tp, found, confirmed, sq, si, su)
    return stats, pinfo, ginfo


def match_ref(pred, gt, classes, form=match_one, **kw):
    """A batch [n, H, W] through `form`: (stats [n, K, 8], pred_info [n, H, W, 2], gt_info [n, H, W, 2])."""
    outs = [form(p, g, classes, **kw) for p, g in zip(np.asarray(pred), np.asarray(gt))]
    return tuple(np.stack([o[i] for o in outs]) for i in range(3))


def table(info):
    """int32 [k, 3] rows (first, partner's first or -1, covered) of one image's info plane, by first pixel."""
    flat = np.asarray(info).reshape(-1, 2)
    first = np.nonzero(flat[:, 0] != -2)[0]
    return np.concatenate([first[:, None], flat[first]], axis=1).astype(np.int32).reshape(-1, 3)


def joined_tables(pred, gt, pred_info, gt_info, classes, connectivity=4, background=0, ignore_label=-1):
    """What Evaluator.region_metrics(return_matches=True) returns for one image: {"gt": [kg, 9], "pred": [kp, 9]}, rows
    regions_ref's seven fields in (class, first) order + (partner's row in the other list or -1, covered)."""
    _, gm = _void_masked(np.asarray(gt, np.uint8), background, ignore_label)
    out, rows = {}, {}
    for name, m, info in (("pred", pred, pred_info), ("gt", gm, gt_info)):
        rec = R.regions_one(m, background, connectivity)[0]
        flat = np.asarray(info).reshape(-1, 2)
        rec = rec[np.isin(rec[:, 0], classes) & (flat[rec[:, 6], 0] != -2)]
        rows[name] = {int(f): r for r, f in enumerate(rec[:, 6])}
        out[name] = np.concatenate([rec, flat[rec[:, 6]]], axis=1).astype(np.int32).reshape(-1, 9)
    for name, other in (("pred", "gt"), ("gt", "pred")):
        for row in out[name]:
            row[7] = rows[other][int(row[7])] if row[7] >= 0 else -1
    return out


# ---- test maps ----

def pair_maps(seed, H, W, C, n=None, void=255):
    """(pred, gt) uint8 [n, H, W] (or [H, W]): one blob field with different speckle in the two maps and the prediction moved
    by a pixel, so that the large regions match and the small ones do not.  Every image also gets, in its upper left corner,
    one predicted rectangle of class 1 over two true ones (both found, neither matched), and across its middle a band of
    `void` in the ground truth that some regions cross (void < 0: no band)."""
    shape = (1, H, W) if n is None else (n, H, W)
    gt = K.speckle(seed, H, W, C, n=shape[0])
    pred = np.roll(K.speckle(seed, H, W, C, n=shape[0], fraction=0.0), 1, axis=2)
    rs = np.random.RandomState(2000 + seed)
    hit = rs.rand(*shape) < 0.02
    pred[hit] = rs.randint(0, C, size=int(hit.sum())).astype(np.uint8)
    if H >= 16 and W >= 24:
        for m in (pred, gt):
            m[:, 1:10, 1:22] = 0
        pred[:, 3:8, 3:20] = 1
        gt[:, 3:8, 3:11] = 1
        gt[:, 3:8, 12:20] = 1
    if void >= 0:
        gt[:, H // 2 - 2:H // 2 + 3, :] = void
    return (pred[0], gt[0]) if n is None else (pred, gt)


def _iou_steps():
    """Pairs of class 1 with IoU 2/4, 3/4, 4/5 and 1, apart from one another, and one of class 2 with IoU 5/9."""
    pred, gt = np.zeros((12, 40), np.uint8), np.zeros((12, 40), np.uint8)
    gt[2, 2:6], pred[2, 2:4] = 1, 1          # 2 of 4 shared: exactly one half
    gt[2, 10:14], pred[2, 10:13] = 1, 1      # 3 of 4: exactly three quarters
    gt[2, 20:25], pred[2, 20:24] = 1, 1      # 4 of 5
    gt[2, 30:36], pred[2, 30:36] = 1, 1      # the same region
    gt[6:9, 2:5], pred[6:9, 3:6] = 2, 2      # 6 shared of 12: one half again
    gt[6:9, 10:13], pred[6:9, 10:13] = 2, 2
    pred[8, 12] = 0                          # 8 of 9
    return pred, gt


def _straddle():
    """One predicted region over two true ones with a gap between them, and one over a large and a small true region."""
    pred, gt = np.zeros((40, 70), np.uint8), np.zeros((40, 70), np.uint8)
    pred[4:10, 4:30] = 1
    gt[4:10, 4:16], gt[4:10, 18:30] = 1, 1
    pred[20:30, 4:60] = 3
    gt[20:30, 4:50], gt[20:30, 52:60] = 3, 3
    return pred, gt


def _void_band():
    """A void band that holds one predicted region entirely and half of another; a true region continues under it."""
    pred, gt = np.zeros((36, 48), np.uint8), np.zeros((36, 48), np.uint8)
    gt[10:20] = 255
    pred[12:16, 4:10] = 1                    # inside the band: it does not exist
    pred[6:14, 20:28] = 1                    # half inside
    gt[4:10, 20:28] = 1                      # the true region ends where the band begins
    pred[24:30, 4:12], gt[24:30, 4:12] = 2, 2
    gt[18:24, 30:40] = 2                     # rows 18, 19 are void
    gt[10:20] = 255
    pred[20:24, 30:40] = 2
    return pred, gt


def match_cases():
    """name -> dict(pred, gt uint8 [n, H, W], classes, connectivity, background, ignore_label, thr, cov): the cases of
    tests/golden/match/match.npz."""
    rs = np.random.RandomState(5)

    def case(pred, gt, classes, connectivity=4, background=0, ignore_label=-1, thr=(1, 2), cov=(1, 2)):
        pred, gt = np.asarray(pred, np.uint8), np.asarray(gt, np.uint8)
        if pred.ndim == 2:
            pred, gt = pred[None], gt[None]
        return dict(pred=pred, gt=gt, classes=list(classes), connectivity=connectivity, background=background,
                    ignore_label=ignore_label, thr=thr, cov=cov)

    cases = {
        "one_1x1_same": case([[1]], [[1]], [1]),
        "one_1x1_missed": case([[0]], [[1]], [1, 2]),
        "strip_1x70": case(rs.randint(0, 3, size=(1, 70)), rs.randint(0, 3, size=(1, 70)), [1, 2]),
        "seam_33x31": case(*pair_maps(21, 33, 31, 3), [1, 2], ignore_label=255),
        "seam_33x31_c8": case(*pair_maps(21, 33, 31, 3), [1, 2], connectivity=8, ignore_label=255),
    }
    sp, sg = pair_maps(22, 97, 131, 5)
    cases["speckle5_97x131"] = case(sp, sg, [1, 2, 3, 4], ignore_label=255)
    cases["speckle5_97x131_c8"] = case(sp, sg, [1, 2, 3, 4], connectivity=8, ignore_label=255, thr=(2, 3), cov=(3, 4))
    cases["speckle5_97x131_bg3"] = case(sp, sg, [4, 0, 1], background=3, ignore_label=255)
    cases["speckle5_97x131_novoid"] = case(*pair_maps(23, 97, 131, 5, void=-1), [1, 2, 3, 4], cov=(1, 1))
    cases["batch5_160x200"] = case(*pair_maps(BATCH_SEED, 160, 200, 6, n=5), [1, 2, 3, 4, 5], ignore_label=255)
    cases["batch5_160x200_c8"] = case(*pair_maps(BATCH_SEED, 160, 200, 6, n=5), [1, 2, 3, 4, 5], connectivity=8,
                                      ignore_label=255)
    board = (R.checkerboard(40, 51) + 1).astype(np.uint8)
    shifted = np.roll(3 - board, 1, axis=1).astype(np.uint8)   # the complement moved by a pixel: the board but for a column
    cases["checker_40x51"] = case(board, shifted, [1, 2])
    cases["checker_40x51_c8"] = case(board, shifted, [1, 2], connectivity=8)
    cases["iou_steps_half"] = case(*_iou_steps(), [1, 2])
    cases["iou_steps_three_quarters"] = case(*_iou_steps(), [1, 2], thr=(3, 4))
    cases["straddle_40x70"] = case(*_straddle(), [1, 3])
    cases["void_band_36x48"] = case(*_void_band(), [1, 2], ignore_label=255)
    cases["empty_pred"] = case(np.zeros((20, 30), np.uint8), _straddle()[1][:20, :30], [1])
    cases["empty_gt"] = case(_straddle()[0][:20, :30], np.zeros((20, 30), np.uint8), [1])
    one_map = _straddle()
    cases["class_in_one_map"] = case(np.where(one_map[0] == 3, 5, one_map[0]), one_map[1], [1, 3, 5])
    kp, kg = pair_maps(24, 64, 80, 17, void=-1)
    cases["k1_64x80"] = case(kp, kg, [3])
    cases["k16_64x80"] = case(kp, kg, range(1, 17))
    return cases


def case_kwargs(c):
    return dict(connectivity=c["connectivity"], background=c["background"], ignore_label=c["ignore_label"], thr=c["thr"],
                cov=c["cov"])
