"""GPU (-m gpu): the line simplification on the device (vitseg_simplify_lines, simplify.simplify_device / simplify,
region_polygons(simplify=), trace(simplify=), predict(simplify=), evaluate_to_csv(simplify_tolerance=)) against the Python
restatement tests/simplify_ref.py.  Everything the device returns is an integer: every comparison is bit for bit.  Outputs and
scratch live in guard-banded, poisoned buffers."""
import json
import os

import numpy as np
import pytest
import torch

import centerlines_ref as CR
import simplify_ref as SR
from guard import check, guarded, snapshot, unchanged
from visiontransformer_amd import _ext, _lib, centerlines, polygons, regions, simplify

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHORT, RESIDENT = simplify.SHORT, simplify.RESIDENT
TOLERANCES = (0, 0.5, 0.75, 1, 2.5, 10)


def _sym(name):
    return _ext.ext_symbol("simplify", name)


def _pack(images, stride=2, pad_points=0, pad_lines=0):
    """images: per image a list of (points [v, stride], closed).  (points int32 [n, P, stride], rows int64 [n, K, 3] of
    (offset, count, closed), counts int32 [n]) as numpy arrays, the lines of an image one after the other."""
    P = max(sum(len(p) for p, _ in im) for im in images) + pad_points
    K = max(len(im) for im in images) + pad_lines
    pts = np.zeros((len(images), P, stride), np.int32)
    rows = np.zeros((len(images), K, 3), np.int64)
    for i, im in enumerate(images):
        o = 0
        for j, (p, closed) in enumerate(im):
            p = np.asarray(p, np.int32).reshape(-1, stride)
            pts[i, o:o + len(p)] = p
            rows[i, j] = (o, len(p), int(closed))
            o += len(p)
    return pts, rows, np.array([len(im) for im in images], np.int32)


def _call(pts, rows, counts, tol2, cols=(0, 1, 2), max_out=None, fill=0xFF):
    """One vitseg_simplify_lines call through the C ABI with guarded outputs and a scratch pre-filled with `fill`:
    (out_counts, out_lines, out_points or None) as numpy arrays."""
    n, P, stride = pts.shape
    K, rs = rows.shape[1:]
    max_out = P if max_out is None else max_out
    d_pts = guarded(pts.shape, torch.int32, torch.from_numpy(pts).to(DEV), name="points")
    d_rows = guarded(rows.shape, torch.int64, torch.from_numpy(rows).to(DEV), name="lines")
    d_cnt = guarded((n,), torch.int32, torch.from_numpy(counts).to(DEV), name="line_counts")
    nbytes = _sym("vitseg_simplify_scratch_bytes")(n, K, P)
    assert nbytes > 0
    scratch = guarded((nbytes,), torch.uint8, name="scratch")
    scratch.fill_(fill)
    oc = guarded((n,), torch.int64, name="out_counts")
    ol = guarded((n, K, 8), torch.int64, name="out_lines")
    op = guarded((n, max_out, stride), torch.int32, name="out_points") if max_out else None
    snap = snapshot(d_pts, d_rows, d_cnt)
    _lib.check(_sym("vitseg_simplify_lines")(
        d_pts.data_ptr(), P, stride, d_rows.data_ptr(), K, rs, cols[0], cols[1], cols[2], d_cnt.data_ptr(), n, int(tol2),
        oc.data_ptr(), ol.data_ptr(), None if op is None else op.data_ptr(), max_out, scratch.data_ptr(), scratch.numel(),
        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    check(d_pts, d_rows, d_cnt, oc, ol, op, scratch)
    unchanged(snap)
    return tuple(None if t is None else t.cpu().numpy() for t in (oc, ol, op))


def _expected(pts, rows, counts, tol2, cols=(0, 1, 2)):
    return [SR.simplify_image(pts[i], rows[i, :counts[i]], cols, int(tol2)) for i in range(len(pts))]


def _assert_equal(got, exp, what=""):
    """One call's arrays against the restatement: true counts, rows exact, points exact up to the capacity, zero past the
    counts."""
    oc, ol, op = got
    for i, (e_rows, e_pts) in enumerate(exp):
        assert oc[i] == len(e_pts), (what, i, oc[i], len(e_pts))
        bad = np.nonzero((ol[i, :len(e_rows)] != e_rows).any(axis=1))[0]
        assert not len(bad), (what, i, bad[:4], ol[i, bad[:4]], e_rows[bad[:4]])
        assert not ol[i, len(e_rows):].any(), (what, i)
        if op is not None:
            k = min(len(e_pts), op.shape[1])
            assert np.array_equal(op[i, :k], e_pts[:k]), (what, i)
            assert not op[i, k:].any(), (what, i)


def _both_fills(pts, rows, counts, tol2, **kw):
    """The call with the scratch pre-filled with 0x00 and with 0xFF: the same bits; returns the second."""
    runs = [_call(pts, rows, counts, tol2, fill=fill, **kw) for fill in (0x00, 0xFF)]
    for a, b in zip(*runs):
        assert (a is None and b is None) or np.array_equal(a, b)
    return runs[1]


# ---- the kernel against the restatement ----

@pytest.mark.parametrize("tolerance", [0, 0.5, 0.75, 1.5, 5])
def test_hand_made_lines(tolerance):
    images = [[(np.asarray(p) + 3, closed) for p, closed in SR.HAND.values()],
              [(np.asarray(p)[::-1] + 1, closed) for p, closed in list(SR.HAND.values())[::-1]]]
    pts, rows, counts = _pack(images)
    t2 = SR.tol2_q8(tolerance)
    _assert_equal(_both_fills(pts, rows, counts, t2), _expected(pts, rows, counts, t2), tolerance)


def _boundary_images():
    rs = np.random.RandomState(11)
    sizes = [1, 2, 3, 4, 5, SHORT - 1, SHORT, SHORT + 1, RESIDENT - 1, RESIDENT, RESIDENT + 1]
    images = [[(SR.walk(rs, c), closed) for c in sizes for closed in (False, True)],
              [(SR.walk(rs, c, step=1), bool(k % 2)) for k, c in enumerate(sizes[::-1] + [7, 33, 200])]]
    return _pack(images, pad_points=5, pad_lines=2)


@pytest.mark.parametrize("tolerance", [0.75, 4, 40])
def test_class_boundaries_mixed_in_one_call(tolerance):
    """Lines either side of SHORT and of RESIDENT, open and closed, in one call: the wave, the resident and the long class."""
    pts, rows, counts = _boundary_images()
    t2 = SR.tol2_q8(tolerance)
    _assert_equal(_both_fills(pts, rows, counts, t2), _expected(pts, rows, counts, t2), tolerance)


def test_extra_columns_travel_with_the_kept_points():
    rs = np.random.RandomState(5)
    for stride in (3, 4):
        images = [[(np.concatenate([SR.walk(rs, c), rs.randint(-9, 1 << 30, size=(c, stride - 2))], axis=1), closed)
                   for c, closed in ((40, False), (90, True), (5, False))]]
        pts, rows, counts = _pack(images, stride=stride)
        t2 = SR.tol2_q8(2)
        _assert_equal(_call(pts, rows, counts, t2), _expected(pts, rows, counts, t2), stride)


@pytest.mark.parametrize("count", [2 * SHORT + 3, 2000, RESIDENT + 13])
def test_decreasing_sawtooth_runs_a_round_per_tooth(count):
    """The recursion is half as deep as the line is long: about count / 2 rounds, in the resident and in the long class."""
    saw = SR.sawtooth(count)
    keep = SR.keep_indices(saw, SR.tol2_q8(1.0))
    assert len(keep) == count   # every tooth survives: nothing is collinear
    images = [[(saw, False), (saw[:, ::-1].copy(), True)]]
    pts, rows, counts = _pack(images)
    for tolerance in (1.0, 30.0):
        t2 = SR.tol2_q8(tolerance)
        _assert_equal(_call(pts, rows, counts, t2), _expected(pts, rows, counts, t2), (count, tolerance))


def _turning_rings():
    rs = np.random.RandomState(5)   # a seed at which every size has rings that turn over at 40 px and rings that do not
    return [[(SR.walk(rs, c), True) for _ in range(12)] for c in (40, SHORT, SHORT + 1, RESIDENT, RESIDENT + 1, 3000)]


def test_rings_that_turn_over_are_returned_as_they_are():
    """The sign guard in the wave, the resident and the long class: closed random walks whose kept points would have no area or
    the opposite one keep every point, next to walks that are thinned as usual."""
    images = _turning_rings()
    pts, rows, counts = _pack(images)
    for tolerance in (4, 40):
        t2 = SR.tol2_q8(tolerance)
        exp = _expected(pts, rows, counts, t2)
        got = _call(pts, rows, counts, t2)
        _assert_equal(got, exp, tolerance)
        for i, im in enumerate(images):
            whole = exp[i][0][:, 1] == exp[i][0][:, 2]
            assert tolerance == 4 or (whole.any() and not whole.all()), i   # every class returns a ring whole and thins another
            for k, (p, _) in enumerate(im):   # the kept area never loses the sign of the full ring's
                full = SR.area2(p)
                assert full == 0 or (got[1][i, k, 3] > 0) == (full > 0), (i, k)


def test_capacities_cut_the_points_and_keep_the_counts():
    pts, rows, counts = _boundary_images()
    t2 = SR.tol2_q8(1.5)
    exp = _expected(pts, rows, counts, t2)
    full = _call(pts, rows, counts, t2)
    _assert_equal(full, exp)
    for cap in (0, 1, int(full[0].min()) - 1, int(full[0].max()) - 1):
        got = _call(pts, rows, counts, t2, max_out=cap)
        _assert_equal(got, exp, cap)
        assert np.array_equal(got[0], full[0]) and np.array_equal(got[1], full[1])
    # line_counts above max_lines are clamped; a count of 0 leaves the image empty
    over = counts.copy()
    over[0] = 1 << 20   # the rows past the image's lines are zero: empty lines
    got = _call(pts, rows, over, t2)
    assert all(np.array_equal(a, b) for a, b in zip(got, full))
    none = _call(pts, rows, np.zeros_like(counts), t2)
    assert not none[0].any() and not none[1].any() and not none[2].any()


def test_rows_with_bad_data_are_skipped_and_their_neighbours_are_right():
    rs = np.random.RandomState(3)
    images = [[(SR.walk(rs, c), closed) for c, closed in ((30, False), (300, True), (SHORT, False), (2100, False), (9, True))]]
    pts, rows, counts = _pack(images, pad_points=4)
    P = pts.shape[1]
    t2 = SR.tol2_q8(1.0)
    for line, change in ((1, ("offset", P - 10)), (1, ("offset", -1)), (2, ("count", 0)), (2, ("count", -5)), (0, ("count", 1 << 40)),
                         (3, ("offset", 1 << 40)), (0, ("coord", -1)), (1, ("coord", 16385)), (3, ("coord", 1 << 20)),
                         (4, ("coord", -(1 << 31)))):
        p, r = pts.copy(), rows.copy()
        if change[0] == "coord":
            p[0, r[0, line, 0] + r[0, line, 1] // 2, line % 2] = change[1]
        else:
            r[0, line, 0 if change[0] == "offset" else 1] = change[1]
        exp = _expected(p, r, counts, t2)
        assert exp[0][0][line, 1] == 0 and (exp[0][0][np.arange(5) != line, 1] > 0).all()
        _assert_equal(_call(p, r, counts, t2), exp, (line, change))


def test_an_image_alone_as_in_a_batch_and_twice_the_same():
    pts, rows, counts = _boundary_images()
    rs = np.random.RandomState(2)
    others = _pack([[(SR.walk(rs, c), c % 2 == 0) for c in (5, 70, 2500, 64)] for _ in range(4)])
    P, K = max(pts.shape[1], others[0].shape[1]), max(rows.shape[1], others[1].shape[1])
    bp, br = np.zeros((5, P, 2), np.int32), np.zeros((5, K, 3), np.int64)
    bp[:4, :others[0].shape[1]], br[:4, :others[1].shape[1]] = others[0], others[1]
    bp[4, :pts.shape[1]], br[4, :rows.shape[1]] = pts[1], rows[1]
    bc = np.concatenate([others[2], counts[1:2]])
    t2 = SR.tol2_q8(2.0)
    batch = _call(bp, br, bc, t2)
    again = _call(bp, br, bc, t2, fill=0x5A)
    alone = _call(bp[4:], br[4:], bc[4:], t2)
    for a, b, c in zip(batch, again, alone):
        assert np.array_equal(a, b) and np.array_equal(a[4:], c)
    _assert_equal(batch, _expected(bp, br, bc, t2))


def test_every_error_status_leaves_the_outputs_untouched():
    pts, rows, counts = _pack([[(SR.walk(np.random.RandomState(1), 20), False)]])
    n, P, stride = pts.shape
    K = rows.shape[1]
    d_pts, d_rows, d_cnt = (torch.from_numpy(a).to(DEV) for a in (pts, rows, counts))
    need = _sym("vitseg_simplify_scratch_bytes")(n, K, P)
    scratch = guarded((need,), torch.uint8, name="scratch")
    oc = guarded((n,), torch.int64, name="out_counts")
    ol = guarded((n, K, 8), torch.int64, name="out_lines")
    op = guarded((n, P, stride), torch.int32, name="out_points")
    snap = snapshot(oc, ol, op, scratch)

    def call(points=d_pts.data_ptr(), max_points=P, stride=2, lines=d_rows.data_ptr(), max_lines=K, row_stride=3, cols=(0, 1, 2),
             line_counts=d_cnt.data_ptr(), n=1, tol2=64, out_counts=oc.data_ptr(), out_lines=ol.data_ptr(), out_points=op.data_ptr(),
             max_out=P, scr=scratch.data_ptr(), nbytes=need):
        return _sym("vitseg_simplify_lines")(points, max_points, stride, lines, max_lines, row_stride, cols[0], cols[1], cols[2],
                                             line_counts, n, tol2, out_counts, out_lines, out_points, max_out, scr, nbytes, None)
    for kw in (dict(points=None), dict(lines=None), dict(line_counts=None), dict(out_counts=None), dict(out_lines=None),
               dict(scr=None), dict(out_points=None), dict(stride=1), dict(stride=5), dict(row_stride=0), dict(cols=(3, 1, 2)),
               dict(cols=(0, 0, 2)), dict(cols=(0, -1, 2)), dict(cols=(0, 1, 3)), dict(cols=(0, 1, -2)), dict(tol2=-1),
               dict(tol2=(1 << 38) + 1), dict(max_out=-1)):
        assert call(**kw) == _lib.EINVAL, kw
        assert b"simplify_lines" in _lib.lib().vitseg_last_error()
    for kw in (dict(n=0), dict(n=65536), dict(max_lines=-1), dict(max_lines=(1 << 24) + 1), dict(max_points=-1),
               dict(max_points=(1 << 30) + 1)):
        assert call(**kw) == _lib.ESHAPE, kw
    assert call(nbytes=need - 1) == _lib.EWORKSPACE
    torch.cuda.synchronize()
    unchanged(snap)
    check(oc, ol, op, scratch)
    assert call() == 0
    torch.cuda.synchronize()
    check(oc, ol, op, scratch)
    assert int(oc[0]) == len(SR.keep_indices(pts[0], 64))


def test_simplify_of_a_callers_own_lines():
    rs = np.random.RandomState(9)
    lines = [SR.walk(rs, c) for c in (1, 2, 17, 64, 65, 900, 2300)]
    for closed in (False, True):
        for tolerance in (0, 1.25, 6):
            got = simplify.simplify(lines, tolerance, closed=closed)
            assert len(got) == len(lines)
            for g, p in zip(got, lines):
                assert g.dtype == np.int32 and np.array_equal(g, p[SR.keep_indices(p, SR.tol2_q8(tolerance), closed)])
    with_extra = [np.concatenate([p, np.arange(len(p))[:, None]], axis=1) for p in lines]
    got = simplify.simplify(with_extra, 3.0)
    for g, p in zip(got, lines):
        assert g[:, 2].tolist() == SR.keep_indices(p, SR.tol2_q8(3.0))
    assert simplify.simplify([], 1.0) == []


# ---- the outlines and the centre-lines of real masks ----

def _maps():
    """Random class maps 64 x 64 and 96 x 80 at densities 0.2 .. 0.9, concentric rings, a serpentine and a pixel checkerboard."""
    rs = np.random.RandomState(21)
    out = [(rs.rand(H, W) < d).astype(np.uint8) * rs.randint(1, 3, size=(H, W)).astype(np.uint8)
           for (H, W) in ((64, 64), (96, 80)) for d in (0.2, 0.5, 0.7, 0.9)]
    board = (np.add.outer(np.arange(24), np.arange(24)) % 2).astype(np.uint8)
    return out + [CR.nested_rings(16), CR.serpentine(16), board]


def _assert_polygons(m, connectivity, tolerance):
    full = polygons.region_polygons(m, connectivity=connectivity)
    thin = polygons.region_polygons(m, connectivity=connectivity, simplify=tolerance)
    t2 = SR.tol2_q8(tolerance)
    boxes = regions.region_boxes(m, connectivity=connectivity)
    rings = 0
    for (rec, polys), (trec, tpolys), box in zip(full, thin, boxes):
        assert np.array_equal(trec, rec) and np.array_equal(trec, box) and trec.dtype == np.int32
        assert isinstance(tpolys, simplify.Simplified) and tpolys.tolerance == float(tolerance) and len(tpolys) == len(polys)
        assert tpolys.full == [sum(len(r) for r in region) for region in polys]
        for region, tregion, row in zip(polys, tpolys, rec):
            assert len(region) == len(tregion)
            for k, (ring, tring) in enumerate(zip(region, tregion)):
                assert tring.dtype == np.int32 and np.array_equal(tring, ring[SR.keep_indices(ring, t2, True)])
                assert len(tring) >= 3
                rings += 1
            assert int(tregion[0][0, 0]) * m.shape[-1] + int(tregion[0][0, 1]) == row[6]   # the outer ring starts at `first`
    return rings


@pytest.mark.parametrize("connectivity", [4, 8])
def test_region_polygons_simplified_are_the_restatement_of_the_full_rings(connectivity):
    rings = 0
    for m in _maps():
        for tolerance in TOLERANCES:
            rings += _assert_polygons(m[None], connectivity, tolerance)
    assert rings > 1000


@pytest.mark.parametrize("tolerance", TOLERANCES)
@pytest.mark.parametrize("connectivity", [4, 8])
def test_simplified_rings_keep_the_sign_of_their_area(connectivity, tolerance):
    """Outer rings keep a positive and holes a negative area, at every tolerance.  Douglas-Peucker alone does not give this:
    the few kept vertices of a thin sprawling 8-connected ring can come out in the other order (on these maps 1 ring of 5679
    at 2.5 px, 28 vertices of area 13 kept as 5 of area -1, and 1 of 5679 at 10 px, 96 vertices of area 71 kept as 5 of area
    -15).  The rule's sign guard returns such a ring as it is."""
    wrong = total = 0
    for m in _maps():
        for rec, polys in polygons.region_polygons(m[None], connectivity=connectivity, simplify=tolerance):
            for region in polys:
                for k, ring in enumerate(region):
                    area = polygons.ring_area(ring)
                    wrong += not (area > 0 if k == 0 else area < 0)
                    total += 1
    print(f"connectivity {connectivity}, tolerance {tolerance}: {wrong} of {total} rings changed the sign of their area")
    assert wrong == 0 and total > 1000


def test_region_polygons_simplified_in_a_batch_and_single():
    ms = np.stack(_maps()[:4])
    assert _assert_polygons(ms, 4, 0.75) > 300
    rec, polys = polygons.region_polygons(ms[1], simplify=2.5)
    (rec_b, polys_b) = polygons.region_polygons(ms, simplify=2.5)[1]
    assert np.array_equal(rec, rec_b) and all(np.array_equal(a, b) for x, y in zip(polys, polys_b) for a, b in zip(x, y))
    (res, labels) = polygons.region_polygons(ms[:2], simplify=1, return_labels=True)
    assert torch.equal(labels, polygons.region_polygons(ms[:2], return_labels=True)[1])
    empty = polygons.region_polygons(np.zeros((5, 5), np.uint8), simplify=1.0)
    assert empty[0].shape == (0, 7) and list(empty[1]) == []


def _assert_trace(m, tolerance, **kw):
    full = centerlines.trace(m, **kw)
    thin = centerlines.trace(m, simplify=tolerance, **kw)
    t2 = SR.tol2_q8(tolerance)
    count = 0
    for (nodes, branches, points), (tn, tb, tp) in zip(full, thin):
        assert np.array_equal(tn, nodes) and isinstance(tp, simplify.Simplified) and tp.tolerance == float(tolerance)
        assert np.array_equal(np.delete(tb, [2, 3], axis=1), np.delete(branches, [2, 3], axis=1))
        assert tp.full == branches[:, 3].tolist() and tb[:, 3].tolist() == [len(p) for p in tp]
        assert np.array_equal(tb[:, 2], np.cumsum(tb[:, 3]) - tb[:, 3])
        node_at = {(int(y), int(x)) for y, x in nodes[:, :2]}
        for row, p, q in zip(branches, points, tp):
            assert q.dtype == np.int32 and np.array_equal(q, p[SR.keep_indices(p, t2, bool(row[4]))])
            if row[4] == 0:   # both ends of an open branch are node pixels still
                assert tuple(q[0, :2]) in node_at and tuple(q[-1, :2]) in node_at
                assert np.array_equal(q[0], p[0]) and np.array_equal(q[-1], p[-1])
            count += 1
        assert centerlines.summary(tn, tb) == centerlines.summary(nodes, branches)
        table, ttable = centerlines.branch_table(branches, 1.0, points), centerlines.branch_table(tb, 1.0, tp)
        assert [{k: v for k, v in d.items() if k != "points"} for d in table] == [
            {k: v for k, v in d.items() if k != "points"} for d in ttable]
    return count


def test_trace_simplified_is_the_restatement_of_the_full_branches():
    count = 0
    for m in _maps():
        for tolerance in TOLERANCES:
            count += _assert_trace((m != 0).astype(np.uint8)[None], tolerance, thin=tolerance in (0.75, 10))
    assert count > 500
    per_class = centerlines.trace(np.stack(_maps()[:2]), classes=[1, 2], simplify=1.0)
    full = centerlines.trace(np.stack(_maps()[:2]), classes=[1, 2])
    for a, b in zip(per_class, full):
        for c in (1, 2):
            assert [q.tolist() for q in a[c][2]] == [p[SR.keep_indices(p, 256, bool(r[4]))].tolist() for p, r in zip(b[c][2], b[c][1])]
    empty = centerlines.trace(np.zeros((5, 6), np.uint8), simplify=1.0)
    assert empty[0].shape == (0, 4) and empty[1].shape == (0, 9) and list(empty[2]) == []


def test_simplify_none_launches_and_returns_what_it_did(monkeypatch):
    """Without the keyword nothing of the family is asked for and every output is what the call without it returns."""
    ms = np.stack(_maps()[:2])
    want_p = polygons.region_polygons(ms, return_labels=True)
    want_t = centerlines.trace(ms, classes=[1])

    def no_call(*a, **k):
        raise AssertionError("the simplification was requested")
    monkeypatch.setattr(simplify, "simplify_device", no_call)
    got_p = polygons.region_polygons(ms, return_labels=True, simplify=None)
    assert torch.equal(got_p[1], want_p[1])
    for (rec, polys), (wrec, wpolys) in zip(got_p[0], want_p[0]):
        assert np.array_equal(rec, wrec) and type(polys) is list
        assert all(np.array_equal(a, b) for x, y in zip(polys, wpolys) for a, b in zip(x, y))
    for g, w in zip(centerlines.trace(ms, classes=[1], simplify=None), want_t):
        assert np.array_equal(g[1][0], w[1][0]) and np.array_equal(g[1][1], w[1][1]) and type(g[1][2]) is list
        assert all(np.array_equal(a, b) for a, b in zip(g[1][2], w[1][2]))


# ---- the model, predict() and the evaluation loop ----

def test_predict_and_the_model_pass_the_tolerance_on():
    from visiontransformer_amd import synth
    from visiontransformer_amd.metrics import Evaluator
    from visiontransformer_amd.model import ViTSegmentationModel
    from visiontransformer_amd.predict import predict
    model = ViTSegmentationModel(3, 16, 192, 1, 3, image_size=224, device=DEV).eval()
    img = (synth.make_images(model.cfg, 1, seed=4)[0].transpose(1, 2, 0) * 255).astype(np.uint8)
    mask, (rec, polys), graph = predict(img, model, return_polygons=True, return_centerlines=True, centerline_classes=[1, 2],
                                        simplify=0.75)
    assert np.array_equal(mask, predict(img, model))
    frec, fpolys = polygons.region_polygons(mask)
    assert np.array_equal(rec, frec) and len(rec) > 0
    for region, tregion in zip(fpolys, polys):
        for ring, tring in zip(region, tregion):
            assert np.array_equal(tring, ring[SR.keep_indices(ring, 144, True)])
    fgraph = centerlines.trace(mask, classes=[1, 2])
    for c in (1, 2):
        for p, q, row in zip(fgraph[c][2], graph[c][2], fgraph[c][1]):
            assert np.array_equal(q, p[SR.keep_indices(p, 144, bool(row[4]))])
    with pytest.raises(ValueError):
        predict(img, model, simplify=0.75)
    x = torch.from_numpy(synth.make_images(model.cfg, 2, seed=1)).to(DEV)
    raw = model.predict_mask(x)
    for (a, pa), (b, pb) in zip(model.predict_polygons(x, simplify=2.0), polygons.region_polygons(raw, simplify=2.0)):
        assert np.array_equal(a, b) and all(np.array_equal(r, s) for x1, y1 in zip(pa, pb) for r, s in zip(x1, y1))
    want = centerlines.trace(raw, classes=[1], simplify=2.0)
    for g, w, e in zip(model.predict_centerlines(x, [1], simplify=2.0), want, Evaluator(3, DEV).crack_graph(raw, [1], simplify=2.0)):
        assert np.array_equal(g[1][1], w[1][1]) and all(np.array_equal(p, q) for p, q in zip(g[1][2], w[1][2]))
        assert np.array_equal(e[1]["branches"], w[1][1]) and e[1]["table"] == centerlines.branch_table(w[1][1], 1.0, w[1][2])


def test_evaluate_to_csv_with_the_tolerance_writes_the_same_files(tmp_path):
    from visiontransformer_amd import scripts
    from visiontransformer_amd.model import ViTSegmentationModel
    model = ViTSegmentationModel(3, 16, 192, 1, 3, image_size=224, device=DEV).eval()
    batches = scripts.ce_batches(model.cfg, 2, 1, seed=3)
    info = (7, "ID7P16H192A3", 16, 192, 1, 3)
    docs = {}
    for name, kw in (("full", {}), ("thin", dict(simplify_tolerance=0.75))):
        path = str(tmp_path / name / "m_metrics.csv")
        scripts.evaluate_to_csv(model, batches, info, path, 3, 1, DEV, polygons_path=str(tmp_path / name / "m_region_polygons.geojson"),
                                crack_graph_classes=[1, 2], **kw)
        docs[name] = {f: open(tmp_path / name / f).read() for f in sorted(os.listdir(tmp_path / name))}
    assert list(docs["full"]) == list(docs["thin"]) == ["m_crack_branches.csv", "m_crack_graph.geojson", "m_metrics.csv",
                                                        "m_region_polygons.geojson"]
    for name in ("m_region_polygons.geojson", "m_crack_graph.geojson"):
        full, thin = json.loads(docs["full"][name])["features"], json.loads(docs["thin"][name])["features"]
        assert len(full) == len(thin) > 0
        for f, t in zip(full, thin):
            extra = {k: t["properties"].pop(k) for k in ("simplify_tolerance", "vertices_full")}
            assert extra["simplify_tolerance"] == 0.75 and extra["vertices_full"] >= 2
            if name == "m_crack_graph.geojson":
                assert extra["vertices_full"] == f["properties"]["points"] >= t["properties"].pop("points")
                f["properties"].pop("points")
            assert t["properties"] == f["properties"]
            flat = lambda g: g if isinstance(g[0][0], float) else [p for ring in g for p in ring]
            assert len(flat(t["geometry"]["coordinates"])) <= len(flat(f["geometry"]["coordinates"]))
    assert sum(len(f["geometry"]["coordinates"][0]) for f in json.loads(docs["thin"]["m_region_polygons.geojson"])["features"]) < sum(
        len(f["geometry"]["coordinates"][0]) for f in json.loads(docs["full"]["m_region_polygons.geojson"])["features"])
