"""GPU (-m gpu): crack centre-lines as a graph on the device (vitseg_centerlines, centerlines.trace, Evaluator.crack_graph,
predict_centerlines, predict(return_centerlines=True), evaluate_to_csv(crack_graph_classes=...)) against the per-pixel
restatement tests/centerlines_ref.py.  Everything the device returns is an integer: every comparison is bit for bit.  Outputs
and scratch live in guard-banded, poisoned buffers."""
import csv
import json
import os
import types

import numpy as np
import pytest
import torch

import centerlines_ref as CR
import skeleton_ref as SR
from guard import check, guarded, snapshot, unchanged
from visiontransformer_amd import _ext, _lib, centerlines, clean, scripts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_REF = {}


def _sym(name):
    return _ext.ext_symbol("centerlines", name)


def _dev(m):
    m = np.asarray(m, np.uint8)
    if m.ndim == 2:
        m = m[None]
    return guarded(m.shape, torch.uint8, torch.from_numpy(m).to(DEV), name="mask")


def _call(mask, value=-1, thin=0, route=0, max_nodes=64, max_branches=64, max_points=512, fill=0xFF):
    """One vitseg_centerlines call through the C ABI on a device tensor, with guarded outputs and a scratch pre-filled with
    `fill`: (node counts, branch counts, point counts, nodes, branches, points) as numpy arrays (None for a capacity of 0)."""
    n, H, W = mask.shape
    nbytes = _sym("vitseg_centerlines_scratch_bytes")(n, H, W, route)
    assert nbytes > 0
    scratch = guarded((nbytes,), torch.uint8, name="scratch")
    scratch.fill_(fill)
    nc = guarded((n,), torch.int32, name="node_counts")
    bc = guarded((n,), torch.int32, name="branch_counts")
    pc = guarded((n,), torch.int64, name="point_counts")
    nodes = guarded((n, max_nodes, 4), torch.int32, name="nodes") if max_nodes else None
    branches = guarded((n, max_branches, 9), torch.int64, name="branches") if max_branches else None
    points = guarded((n, max_points, 3), torch.int32, name="points") if max_points else None
    snap = snapshot(mask)
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(_sym("vitseg_centerlines")(
        mask.data_ptr(), n, H, W, value, thin, route, nc.data_ptr(), bc.data_ptr(), pc.data_ptr(), ptr(nodes), max_nodes,
        ptr(branches), max_branches, ptr(points), max_points, scratch.data_ptr(), scratch.numel(),
        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    check(nc, bc, pc, nodes, branches, points, scratch)
    unchanged(snap)
    return tuple(None if t is None else t.cpu().numpy() for t in (nc, bc, pc, nodes, branches, points))


def _ref(key, m, value=-1, thin=False):
    """The restatement of every image of m [n, H, W], computed once per key: [(nodes, branches, points)]."""
    if key not in _REF:
        _REF[key] = [CR.trace_ref(mi, value, thin) for mi in np.asarray(m)]
    return _REF[key]


def _caps(exp, extra=3):
    return dict(max_nodes=max(len(e[0]) for e in exp) + extra, max_branches=max(len(e[1]) for e in exp) + extra,
                max_points=max(len(e[2]) for e in exp) + extra)


def _assert_equal(got, exp, what=""):
    """One call's arrays against the restatement: true counts, rows exact up to the capacities, zero past the counts."""
    nc, bc, pc, nodes, branches, points = got
    for i, (e_nodes, e_branches, e_points) in enumerate(exp):
        assert (nc[i], bc[i], pc[i]) == (len(e_nodes), len(e_branches), len(e_points)), (what, i, nc[i], bc[i], pc[i])
        for out, e, name in ((nodes, e_nodes, "nodes"), (branches, e_branches, "branches"), (points, e_points, "points")):
            if out is None:
                continue
            k = min(len(e), out.shape[1])
            assert np.array_equal(out[i, :k], e[:k]), (what, i, name, out[i, :k][:6], e[:k][:6])
            assert not out[i, k:].any(), (what, i, name)


def _both_fills(mask, **kw):
    """The call with the scratch pre-filled with 0x00 and with 0xFF: the same bits (a scratch word read before it is written
    would differ), which is also two calls in a row; returns the second."""
    runs = [_call(mask, fill=fill, **kw) for fill in (0x00, 0xFF)]
    for a, b in zip(*runs):
        assert (a is None and b is None) or np.array_equal(a, b)
    return runs[1]


# ---- thin = 0: the plane as it is ----

@pytest.mark.parametrize("name", list(CR.HAND))
def test_hand_planes(name):
    m = CR.HAND[name][None]
    exp = _ref(name, m)
    _assert_equal(_both_fills(_dev(m), **_caps(exp)), exp, name)


def _random(H, W, density, seed):
    return (np.random.RandomState(seed).rand(H, W) < density).astype(np.uint8)


@pytest.mark.parametrize("density", [0.15, 0.35, 0.7])
@pytest.mark.parametrize("H, W", [(1, 1), (1, 7), (5, 1), (33, 65), (97, 130)])
def test_random_planes(H, W, density):
    m = _random(H, W, density, 100 * H + W + int(100 * density))[None]
    if H * W == 1:
        m[:] = density > 0.3
    exp = _ref(("random", H, W, density), m)
    _assert_equal(_both_fills(_dev(m), **_caps(exp)), exp, (H, W, density))


def test_full_plane_is_all_nodes():
    """Every pixel but the four corners (degree 2) a node of degree 3 or 4, every branch of one link but the four round the
    corners: the most nodes, branches and points a plane can have."""
    m = np.ones((1, 17, 19), np.uint8)
    exp = _ref("full", m)
    nodes, branches, points = exp[0]
    links = 17 * 18 + 16 * 19
    assert len(nodes) == 17 * 19 - 4 and len(branches) == links - 4 and len(points) == 2 * (links - 8) + 3 * 4
    assert nodes[:, 2].min() == 3 and nodes[:, 2].max() == 4 and sorted(set(branches[:, 3].tolist())) == [2, 3]
    _assert_equal(_both_fills(_dev(m), **_caps(exp)), exp, "full")


def test_serpentine_is_one_long_branch():
    m = CR.serpentine(128)[None]
    exp = _ref("serpentine", m)
    nodes, branches, points = exp[0]
    assert len(nodes) == 2 and len(branches) == 1 and branches[0, 3] == len(points) == int(m.sum()) > 8000
    _assert_equal(_both_fills(_dev(m), **_caps(exp)), exp, "serpentine")


def test_nested_rings_are_closed_branches():
    m = CR.nested_rings(64)[None]
    exp = _ref("rings", m)
    nodes, branches, points = exp[0]
    assert len(nodes) == 0 and len(branches) == 16 and np.all(branches[:, 4] == 1) and len(points) == int(m.sum())
    _assert_equal(_both_fills(_dev(m), **_caps(exp)), exp, "rings")


def test_more_than_256_pixel_chunks():
    """262 x 1030: 264 pixel chunks and 1055 half-link chunks, so both chunk scans carry over more than one block of 256
    chunk totals and every chunk base past the first block is used.  Row 254 is one open branch across pixel 262144, the
    first pixel of chunk 256; the ring is a closed branch in chunk 259."""
    H, W = 262, 1030
    m = np.zeros((1, H, W), np.uint8)
    lollipop, ring = CR.HAND["lollipop"], CR.HAND["ring_4x4"]
    m[0, :lollipop.shape[0], :lollipop.shape[1]] = lollipop
    m[0, 254, :] = 1
    m[0, 257:257 + ring.shape[0], 1020:1020 + ring.shape[1]] = ring
    exp = _ref("chunks", m)
    nodes, branches, points = exp[0]
    assert (len(nodes), len(branches), len(points)) == (4, 4, 1055)
    assert branches[:, [0, 1, 3, 4]].tolist() == [[2063, 2063, 9, 0], [2063, 2066, 4, 0], [261620, 262649, 1030, 0],
                                                  [265730, 265730, 12, 1]]
    _assert_equal(_both_fills(_dev(m), **_caps(exp)), exp, "chunks")


# ---- thin = 1: the skeleton of the plane ----

def _thin_mask(kind, H, W):
    if kind == "blobs":
        return SR.blobs(H, W, 5)
    return SR.crack_map(H, W, 7)   # classes 1 and 2: thin strokes


@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("value", [-1, 1])
@pytest.mark.parametrize("kind", ["blobs", "strokes"])
@pytest.mark.parametrize("H, W", [(64, 64), (97, 130)])
def test_thinned_planes(H, W, kind, value, route):
    m = _thin_mask(kind, H, W)[None]
    exp = _ref(("thin", H, W, kind, value), m, value, True)
    assert len(exp[0][2]) > 20
    _assert_equal(_both_fills(_dev(m), value=value, thin=1, route=route, **_caps(exp)), exp, (H, W, kind, value, route))


# ---- batches and capacities ----

def _batch():
    """n = 3 at 33 x 65: a sparse random plane, an empty image, rings and strokes."""
    m = np.zeros((3, 33, 65), np.uint8)
    m[0] = _random(33, 65, 0.3, 11)
    m[2, :32, :32] = CR.nested_rings(32)
    m[2, 5:28, 40:60] = _random(23, 20, 0.25, 12)
    return m


def test_an_image_gets_the_same_bits_alone_as_in_a_batch():
    m = _batch()
    exp = _ref("batch", m)
    caps = _caps(exp)
    got = _both_fills(_dev(m), **caps)
    _assert_equal(got, exp, "batch")
    assert (got[0][1], got[1][1], got[2][1]) == (0, 0, 0)   # the empty image
    for i in range(3):
        alone = _call(_dev(m[i]), **caps)
        for a, b in zip(alone, got):
            assert np.array_equal(a[0], b[i]), (i,)


def test_capacities_cut_the_outputs_and_keep_the_counts():
    m = _batch()
    exp = _ref("batch", m)
    true = (min(len(e[0]) for e in (exp[0], exp[2])), min(len(e[1]) for e in (exp[0], exp[2])), min(len(e[2]) for e in (exp[0], exp[2])))
    assert min(true) > 8
    mask = _dev(m)
    query = _call(mask, max_nodes=0, max_branches=0, max_points=0)
    assert query[3] is None and query[4] is None and query[5] is None
    _assert_equal(query, exp, "query")
    for caps in ((true[0] - 1, true[1] - 1, true[2] - 1), (1, 1, 1), (5, 0, 7), (0, 9, 0)):
        got = _both_fills(mask, max_nodes=caps[0], max_branches=caps[1], max_points=caps[2])
        _assert_equal(got, exp, caps)


def test_every_error_returns_its_status_with_nothing_written():
    mask = _dev(_random(9, 9, 0.4, 3))
    n, H, W = mask.shape
    need = _sym("vitseg_centerlines_scratch_bytes")(n, H, W, 0)
    outs = dict(nc=guarded((n,), torch.int32), bc=guarded((n,), torch.int32), pc=guarded((n,), torch.int64),
                nodes=guarded((n, 8, 4), torch.int32), branches=guarded((n, 8, 9), torch.int64),
                points=guarded((n, 64, 3), torch.int32), scratch=guarded((need,), torch.uint8))
    fn = _sym("vitseg_centerlines")

    def call(**kw):
        a = dict(mask=mask.data_ptr(), n=n, H=H, W=W, value=-1, thin=1, route=0, max_nodes=8, max_branches=8, max_points=64,
                 nbytes=need, **{k: t.data_ptr() for k, t in outs.items()})
        a.update(kw)
        return fn(a["mask"], a["n"], a["H"], a["W"], a["value"], a["thin"], a["route"], a["nc"], a["bc"], a["pc"], a["nodes"],
                  a["max_nodes"], a["branches"], a["max_branches"], a["points"], a["max_points"], a["scratch"], a["nbytes"],
                  torch.cuda.current_stream().cuda_stream)
    cases = [(_lib.EINVAL, kw) for kw in (dict(mask=None), dict(nc=None), dict(bc=None), dict(pc=None), dict(scratch=None),
                                          dict(nodes=None), dict(branches=None), dict(points=None), dict(max_nodes=-1),
                                          dict(max_branches=-1), dict(max_points=-1), dict(value=-2), dict(value=256),
                                          dict(thin=2), dict(route=3), dict(route=-1))]
    cases += [(_lib.ESHAPE, kw) for kw in (dict(n=0), dict(H=0), dict(W=-1), dict(n=32768), dict(H=16385), dict(W=16385),
                                           dict(H=16384, W=32768), dict(H=2048, W=2048, route=1))]
    cases += [(_lib.EWORKSPACE, dict(nbytes=need - 1)), (_lib.EWORKSPACE, dict(nbytes=0))]
    for status, kw in cases:
        assert call(**kw) == status, kw
        assert b"centerlines" in _lib.lib().vitseg_last_error()
    torch.cuda.synchronize()
    for t in outs.values():
        check(t)
        assert bool((t.view(-1).view(torch.uint8) == 0xFF).all())   # nothing was written
    assert _sym("vitseg_centerlines_scratch_bytes")(1, 2048, 2048, 1) == 0
    assert call() == _lib.OK   # the same arguments, unchanged, are a good call
    torch.cuda.synchronize()


# ---- the Python surface, the model, predict() and the evaluation loop ----

def _same_graph(a, b):
    (nodes_a, branches_a, points_a), (nodes_b, branches_b, points_b) = a, b
    assert np.array_equal(nodes_a, nodes_b) and np.array_equal(branches_a, branches_b) and len(points_a) == len(points_b)
    assert all(p.dtype == np.int32 and np.array_equal(p, q) for p, q in zip(points_a, points_b))


def _as_trace(ref):
    nodes, branches, points = ref
    return nodes, branches, [points[int(o):int(o + c)] for o, c in zip(branches[:, 2], branches[:, 3])]


def test_trace_returns_the_restatement():
    m = np.stack([SR.crack_map(64, 64, 7), SR.crack_map(64, 64, 9)])
    got = centerlines.trace(m, classes=[1, 2])
    assert len(got) == 2 and all(list(g) == [1, 2] for g in got)
    for i in range(2):
        for c in (1, 2):
            nodes, branches, points = got[i][c]
            assert nodes.dtype == np.int32 and branches.dtype == np.int64
            _same_graph(got[i][c], _as_trace(CR.trace_ref(m[i], c, True)))
    # a [H, W] mask read as binary, thinned or as it is, from the host or the device
    _same_graph(centerlines.trace(m[0]), _as_trace(CR.trace_ref(m[0], -1, True)))
    ring = CR.HAND["lollipop"]
    _same_graph(centerlines.trace(torch.from_numpy(ring).to(DEV), thin=False, route="resident"), _as_trace(CR.trace_ref(ring)))
    _same_graph(centerlines.trace(ring.astype(bool), thin=False), _as_trace(CR.trace_ref(ring)))
    empty = centerlines.trace(np.zeros((5, 6), np.uint8))
    assert empty[0].shape == (0, 4) and empty[1].shape == (0, 9) and empty[2] == []


def test_crack_graph_predict_centerlines_and_predict():
    from visiontransformer_amd import synth
    from visiontransformer_amd.metrics import Evaluator
    from visiontransformer_amd.model import ViTSegmentationModel
    from visiontransformer_amd.predict import predict
    model = ViTSegmentationModel(3, 16, 192, 1, 3, image_size=224, device=DEV).eval()
    x = torch.from_numpy(synth.make_images(model.cfg, 2, seed=1)).to(DEV)
    raw = model.predict_mask(x)
    got, mask = model.predict_centerlines(x, [1, 2], return_mask=True)
    assert torch.equal(mask, raw)
    want = centerlines.trace(raw, classes=[1, 2])
    for g, w in zip(got, want):
        for c in (1, 2):
            _same_graph(g[c], w[c])
    assert sum(len(g[c][1]) for g in got for c in (1, 2)) > 0
    got, mask = model.predict_centerlines(x, [1], min_area=8, fill_holes=True, return_mask=True)
    cleaned = clean.clean_mask(raw, min_area=8, fill_holes=True)
    assert torch.equal(mask, cleaned)
    for g, w in zip(got, centerlines.trace(cleaned, classes=[1])):
        _same_graph(g[1], w[1])
    graph = Evaluator(3, DEV).crack_graph(raw, [1, 2], pixel_size=0.5)
    for g, w in zip(graph, want):
        for c in (1, 2):
            _same_graph((g[c]["nodes"], g[c]["branches"], g[c]["points"]), w[c])
            assert g[c]["table"] == centerlines.branch_table(w[c][1], 0.5, w[c][2])
            assert g[c]["summary"] == centerlines.summary(w[c][0], w[c][1], 0.5)
    img = (synth.make_images(model.cfg, 1, seed=4)[0].transpose(1, 2, 0) * 255).astype(np.uint8)
    plain = predict(img, model)
    m1, boxes, graph = predict(img, model, return_boxes=True, return_centerlines=True, centerline_classes=[1, 2])
    assert np.array_equal(m1, plain) and list(graph) == [1, 2]
    for c in (1, 2):
        _same_graph(graph[c], centerlines.trace(plain, classes=[c])[c])
    m2, graph2 = predict(img, model, return_centerlines=True, centerline_classes=[1], min_area=8, fill_holes=True, tta="hflip")
    _same_graph(graph2[1], centerlines.trace(m2, classes=[1])[1])


def test_evaluate_to_csv_writes_the_graph_and_leaves_the_first(tmp_path):
    from visiontransformer_amd.model import ViTSegmentationModel
    model = ViTSegmentationModel(3, 16, 192, 1, 3, image_size=224, device=DEV).eval()
    batches = scripts.ce_batches(model.cfg, 4, 2, seed=3)
    info = (7, "ID7P16H192A3", 16, 192, 1, 3)
    plain, both = str(tmp_path / "a" / "m_metrics.csv"), str(tmp_path / "b" / "m_metrics.csv")
    scripts.evaluate_to_csv(model, batches, info, plain, 3, 2, DEV)
    args = types.SimpleNamespace(crack_graph="1,2")
    rows = scripts.evaluate_to_csv(model, batches, info, both, 3, 2, DEV, min_area=4, props_pixel_size=0.5,
                                   **scripts.crack_graph_options(args, both))
    assert os.listdir(tmp_path / "a") == ["m_metrics.csv"] and len(rows) == 4   # without the argument: the file of before
    assert sorted(os.listdir(tmp_path / "b")) == ["m_crack_branches.csv", "m_crack_graph.geojson", "m_metrics.csv"]
    assert open(plain).read().split("\n")[0] == open(both).read().split("\n")[0]
    doc = json.load(open(tmp_path / "b" / "m_crack_graph.geojson"))
    assert doc["type"] == "FeatureCollection"
    want, want_rows = [], []
    for bn in range(2):
        with torch.no_grad():
            mask = clean.clean_mask(model.predict_mask(batches[bn][0].to(DEV)), min_area=4)
        for idx, per_class in enumerate(centerlines.trace(mask, classes=[1, 2])):
            for c, (nodes, branches, points) in per_class.items():
                for f in centerlines.centerlines_to_geojson(branches, points, pixel_size=0.5, image_id=f"{bn}/{idx}",
                                                            class_id=c)["features"]:
                    f["properties"].update(model_id=7, model_name="ID7P16H192A3", batch_num=bn, image_idx=idx)
                    want.append(f)
                want_rows += centerlines.csv_rows(info, bn, idx, c, centerlines.branch_table(branches, 0.5, points),
                                                  centerlines.summary(nodes, branches, 0.5))
    assert len(want) > 0 and doc["features"] == json.loads(json.dumps(want))
    assert all(f["geometry"]["type"] == "LineString" for f in doc["features"]) and doc["features"][0]["properties"]["image_id"] == "0/0"
    table = list(csv.reader(open(tmp_path / "b" / "m_crack_branches.csv")))
    assert table[0] == centerlines.CSV_COLUMNS and table[1:] == [[str(v) for v in r] for r in want_rows]
    assert sum(r[5] == "summary" for r in table[1:]) == 2 * 2 * 2   # per image and class
