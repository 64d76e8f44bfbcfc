"""CPU (-m "not gpu"): the restatement of the line simplification against literal results and its own properties, the family
header against `_ext.EXT_LATER`, the argument checks, the flag of the evaluation scripts and the GeoJSON properties.  No
compute entry point runs."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest

import simplify_ref as SR
from test_binding_cpu import parse_header, signature_errors
from visiontransformer_amd import _ext, _lib, centerlines, polygons, scripts, simplify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vitseg_simplify.h")
NAMES = ["vitseg_simplify_version", "vitseg_simplify_scratch_bytes", "vitseg_simplify_lines"]


# ---- the restatement ----

def _keep(name, tolerance):
    p, closed = SR.HAND[name]
    return SR.keep_indices(np.array(p), SR.tol2_q8(tolerance), closed)


def test_restatement_on_hand_made_lines():
    assert (SR.tol2_q8(0), SR.tol2_q8(0.5), SR.tol2_q8(0.75), SR.tol2_q8(2)) == (0, 64, 144, 1024)
    for t in (0, 0.5, 100):
        assert _keep("straight", t) == [0, 8]
    assert _keep("ell", 0) == _keep("ell", 2) == [0, 3, 6] and _keep("ell", 2.2) == [0, 6]   # the corner is 3 / sqrt 2 away
    # a 1-px staircase: its corners are sqrt(1/2) = 0.707 px from the diagonal
    assert _keep("staircase", 0) == list(range(13))
    assert _keep("staircase", 0.5) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12]
    assert _keep("staircase", 0.75) == [0, 12]
    # the hook: every point is within 1 px of the LINE through the ends, but (1, 14) is sqrt(17) from the SEGMENT's end
    assert _keep("hook", 1.5) == _keep("hook", 2) == [0, 2, 4] and _keep("hook", 4.2) == [0, 4]
    # a loop at a node, p0 == pk: the distance is to the point; the far corner is sqrt(32) = 5.66 away
    assert _keep("node_loop", 3) == _keep("node_loop", 5.6) == [0, 2, 4] and _keep("node_loop", 5.7) == [0, 4]
    # a 1 x 200 hairline stays a polygon whatever the tolerance: the first split of each half is unconditional
    assert _keep("hairline", 5) == _keep("hairline", 100) == [0, 1, 2, 3]
    # all five peaks of the zigzag are 4 px from the base: the smallest index wins, not the last or the middle one
    assert _keep("zigzag", 3.5) == [0, 1, 10] and _keep("zigzag", 4.0) == [0, 10] and _keep("zigzag", 0) == list(range(11))
    # tolerance 0 drops exactly the points on the segment between kept neighbours
    assert _keep("collinear_ring", 0) == [0, 2, 4, 6] == _keep("collinear_ring", 3)
    # short lines are returned as they are
    for c in (1, 2):
        assert SR.keep_indices(np.zeros((c, 2), int), 0) == list(range(c))
    for c in (1, 2, 3):
        assert SR.keep_indices(np.zeros((c, 2), int), 0, True) == list(range(c))
    assert SR.keep_indices(np.full((6, 2), 7), 0, True) == [0]   # a ring of one repeated point keeps p0 alone


def test_vector_scores_are_the_scalar_rule():
    rs = np.random.RandomState(4)
    for _ in range(300):
        P = rs.randint(0, 12, size=(7, 2)).astype(np.int64)
        for l, r in ((0, 6), (2, 7), (1, 4)):
            N, L = SR.scores(P, l, r)
            exp = [SR.score(tuple(P[i]), tuple(P[l]), tuple(P[r % 7])) for i in range(l + 1, r)]
            assert N.tolist() == [e[0] for e in exp] and all(e[1] == L for e in exp)
    big = np.array([[0, 0], [16384, 0], [0, 16384], [16384, 16384]], np.int64)
    N, L = SR.scores(big, 0, 3)
    assert L == 2 * 16384 ** 2 and N.tolist() == [16384 ** 4] * 2 and 16384 ** 4 * 2 < 2 ** 59
    assert SR.far(1, 256, 1) is False and SR.far(1, 255, 1) is True and SR.far(0, 0, 0) is False and SR.far(1, 0, 255) is True


def _within(P, keep, tol2, closed):
    """Every dropped point is within the tolerance of the segment between its kept neighbours (exact)."""
    c = len(P)
    ends = keep + [c] if closed else keep
    for a, b in zip(ends[:-1], ends[1:]):
        for i in range(a + 1, b):
            N, L = SR.score(tuple(P[i]), tuple(P[a]), tuple(P[b % c]))
            if SR.far(N, L, tol2):
                return False
    return True


def test_properties_on_random_lattice_walks():
    rs = np.random.RandomState(8)
    checked = 0
    for it in range(150):
        c = int(rs.randint(1, 120))
        P = SR.walk(rs, c, step=int(rs.randint(1, 4))).astype(np.int64)
        for closed in (False, True):
            for tolerance in (0, 0.5, 0.75, 1, 2.5, 10):
                t2 = SR.tol2_q8(tolerance)
                keep = SR.keep_indices(P, t2, closed)
                assert keep == sorted(set(keep)) and keep[0] == 0 and all(0 <= k < c for k in keep)
                if not closed:
                    assert keep[-1] == c - 1
                    assert _within(P, keep, t2, closed)
                elif c >= 4 and len(set(map(tuple, P))) > 1:
                    assert len(keep) >= 2
                    # the unconditional first splits may keep a point inside the tolerance; no dropped point is outside it
                    assert _within(P, keep, t2, closed)
                assert SR.keep_indices(P + np.array([37, 1000]), t2, closed) == keep   # translation
                checked += 1
    assert checked == 1800


def test_a_ring_never_degenerates():
    rs = np.random.RandomState(1)
    for it in range(100):
        h, w = int(rs.randint(1, 9)), int(rs.randint(1, 60))
        ring = np.array([[0, x] for x in range(w)] + [[y, w] for y in range(h)] + [[h, w - x] for x in range(w)]
                        + [[h - y, 0] for y in range(h)])
        keep = SR.keep_indices(ring, SR.tol2_q8(1000), True)
        assert len(keep) >= 3 and abs(SR.area2(ring[keep])) > 0


def test_a_ring_that_turns_over_is_returned_as_it_is():
    """The sign guard on closed random walks of 48 points at 40 px: where the points Douglas-Peucker alone keeps have no area or
    the opposite one, the rule returns the ring whole; elsewhere it returns just those points.  Open lines and rings of area 0
    have no guard."""
    bow = np.array([[0, 0], [0, 10], [10, 0], [10, 10]])   # a bow tie: the two lobes cancel, area 0
    assert SR.area2(bow) == 0 and SR.keep_indices(bow, SR.tol2_q8(1), True) == [0, 1, 2, 3]
    rs = np.random.RandomState(5)
    turned = thinned = 0
    for _ in range(60):
        P = SR.walk(rs, 48).astype(np.int64)
        t2 = SR.tol2_q8(40)
        keep = SR.keep_indices(P, t2, True)
        f = int(np.argmax(((P - P[0]) ** 2).sum(axis=1)))
        plain = sorted({0, f} | set(SR._halves(P, [(0, f, True), (f, len(P), True)], t2)))   # Douglas-Peucker alone
        A, K = SR.area2(P), SR.area2(P[plain])
        if A != 0 and (K == 0 or (K > 0) != (A > 0)):
            assert keep == list(range(len(P)))
            turned += 1
        else:
            assert keep == plain
            thinned += len(plain) < len(P)
        assert A == 0 or (SR.area2(P[keep]) > 0) == (A > 0)
        assert SR.keep_indices(P, t2, False) == sorted({0, len(P) - 1} | set(SR._halves(P, [(0, len(P) - 1, False)], t2)))
    assert turned >= 5 and thinned >= 20


def test_simplify_image_numbers_the_kept_points_in_point_order():
    pts = np.array(SR.HAND["ell"][0] + SR.HAND["hairline"][0] + [[0, 0]], np.int32)
    rows = np.array([[7, 4, 1], [0, 7, 0], [11, 1, 0], [5, 9, 0], [0, 0, 0]], np.int64)   # the fourth runs past the points
    lines, kept = SR.simplify_image(pts, rows, (0, 1, 2), SR.tol2_q8(1))
    assert lines.tolist() == [[3, 4, 4, 400, 0, 0, 1, 200], [0, 3, 7, 0, 0, 0, 3, 3], [7, 1, 1, 0, 0, 0, 0, 0],
                              [0, 0, 9, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0]]
    assert kept.tolist() == [[0, 0], [3, 0], [3, 3], [0, 0], [0, 200], [1, 200], [1, 0], [0, 0]]


# ---- the family header and its table ----

def _table():
    return {name: (restype, list(argtypes)) for name, restype, argtypes in _ext.EXT_LATER["simplify"][2]}


def test_family_header_is_the_table_both_ways():
    decls, structs, enums, defines = parse_header(open(HEADER).read())
    assert _ext.EXT_LATER["simplify"][:2] == ("vitseg_simplify.h", "the line simplification")
    assert sorted(decls) == sorted(NAMES) == sorted(_table()) and not structs and not enums
    assert signature_errors(decls, _table()) == []
    assert len(decls["vitseg_simplify_lines"][1]) == 19 and decls["vitseg_simplify_lines"][1][11] == ("int64_t", 0)
    assert defines == {"VITSEG_SIMPLIFY_VERSION": 100, "VITSEG_SIMPLIFY_SHORT": simplify.SHORT,
                       "VITSEG_SIMPLIFY_RESIDENT": simplify.RESIDENT}
    assert _ext.SIMPLIFY_VERSION == 100 and 1 <= simplify.SHORT < simplify.RESIDENT
    # the comparison can fail
    tab = _table()
    tab["vitseg_simplify_lines"] = (C.c_int, tab["vitseg_simplify_lines"][1][:11] + [C.c_int] + tab["vitseg_simplify_lines"][1][12:])
    assert signature_errors(decls, tab) == ["vitseg_simplify_lines: argument 11: c_int for int64_t"]
    tab = _table()
    del tab["vitseg_simplify_version"]
    assert signature_errors(decls, tab) == ["vitseg_simplify_version: declared in the header, no row in the table"]


def test_family_stays_beside_the_pinned_tables():
    assert list(_ext.EXT_SIGNATURES) == ["polygons"] and list(_ext.EXT_FAMILIES) == ["centerlines"]
    assert "simplify" in _ext.EXT_LATER and not set(_ext.EXT_LATER) & (set(_ext.EXT_SIGNATURES) | set(_ext.EXT_FAMILIES))
    assert all("simplify" not in name for name in _lib.EXPORTS)
    assert "simplify" not in open(os.path.join(ROOT, "include", "vitseg.h")).read().lower()
    assert '#include "vitseg.h"' in open(HEADER).read()
    assert _ext.EXT_VERSIONS["simplify"] == ("vitseg_simplify_version", 100)
    assert set(_ext.EXT_VERSIONS) == set(_ext.EXT_SIGNATURES) | set(_ext.EXT_FAMILIES) | set(_ext.EXT_LATER)
    text = open(HEADER).read()
    assert "independently" in text and "touch or cross itself" in text   # the two stated limits


def test_library_exports_the_family_at_its_version():
    l = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(l, name), name
    assert _ext.ext_symbol("simplify", "vitseg_simplify_version")() == 100
    fn = _ext.ext_symbol("simplify", "vitseg_simplify_lines")
    assert fn.restype is C.c_int and list(fn.argtypes) == _table()["vitseg_simplify_lines"][1]
    assert _ext.ext_symbol("simplify", "vitseg_simplify_lines") is fn
    assert _ext.ext_symbol("simplify", "vitseg_simplify_scratch_bytes").restype is C.c_size_t
    assert _ext.ext_symbol("polygons", "vitseg_polygons_version")() == 100        # the first two tables are still consulted
    assert _ext.ext_symbol("centerlines", "vitseg_centerlines_version")() == 100


def test_ext_symbol_names_the_rebuild_for_a_missing_name(monkeypatch):
    msg = r"has no vitseg_simplify_rings \(built before the line simplification\): rebuild it \(python -m visiontransformer_amd\.build\)"
    with pytest.raises(RuntimeError, match=msg):
        _ext.ext_symbol("simplify", "vitseg_simplify_rings")

    class Old:   # a library built before the line simplification
        def __getattr__(self, name):
            if "simplify" in name:
                raise AttributeError(name)
            return getattr(_lib._lib, name)
    _lib.lib()
    monkeypatch.setattr(_lib, "lib", Old)
    with pytest.raises(RuntimeError, match=r"has no vitseg_simplify_lines \(built before the line simplification\): rebuild it"):
        _ext.ext_symbol("simplify", "vitseg_simplify_lines")


def test_every_status_code_without_a_device():
    """The argument checks come before any launch: every address is a live host buffer that no call reaches."""
    fn = _ext.ext_symbol("simplify", "vitseg_simplify_lines")
    size = _ext.ext_symbol("simplify", "vitseg_simplify_scratch_bytes")
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    need = size(1, 4, 64)
    assert need > 0 and size(2, 4, 64) > need and size(1, 4, 128) > need and size(1, 0, 0) > 0
    for bad in ((0, 4, 64), (65536, 4, 64), (1, -1, 64), (1, (1 << 24) + 1, 64), (1, 4, -1), (1, 4, (1 << 30) + 1)):
        assert size(*bad) == 0, bad

    def call(points=p, max_points=64, stride=2, lines=p, max_lines=4, row_stride=4, cols=(1, 2, -1), counts=p, n=1, tol2=144,
             out_counts=p, out_lines=p, out_points=p, max_out=64, scratch=p, nbytes=need):
        return fn(points, max_points, stride, lines, max_lines, row_stride, cols[0], cols[1], cols[2], counts, n, tol2, out_counts,
                  out_lines, out_points, max_out, scratch, nbytes, None)
    for kw in (dict(points=None), dict(lines=None), dict(counts=None), dict(out_counts=None), dict(out_lines=None),
               dict(scratch=None), dict(out_points=None), dict(stride=1), dict(stride=5), dict(row_stride=0), dict(row_stride=65),
               dict(cols=(4, 2, -1)), dict(cols=(1, 4, -1)), dict(cols=(1, 1, -1)), dict(cols=(-1, 2, -1)), dict(cols=(1, 2, 4)),
               dict(cols=(1, 2, -2)), dict(tol2=-1), dict(tol2=(1 << 38) + 1), dict(max_out=-1)):
        assert call(**kw) == _lib.EINVAL, kw
        assert b"simplify_lines" in _lib.lib().vitseg_last_error()
    for kw in (dict(n=0), dict(n=65536), dict(max_lines=-1), dict(max_lines=(1 << 24) + 1), dict(max_points=-1),
               dict(max_points=(1 << 30) + 1)):
        assert call(**kw) == _lib.ESHAPE, kw
        with pytest.raises(ValueError, match="simplify_lines: bad shape"):
            _lib.check(_lib.ESHAPE)
    assert call(nbytes=need - 1) == _lib.EWORKSPACE
    assert bytes(buf) == bytes(4096)   # nothing was written


# ---- the Python surface ----

def test_tolerances_taken_and_refused():
    assert simplify.tol2_q8(0) == 0 and simplify.tol2_q8(0.75) == 144 and simplify.tol2_q8(np.float32(2)) == 1024
    assert simplify.tol2_q8(np.int64(3)) == 2304 and simplify.tol2_q8(32768) == 1 << 38
    for t in (0, 0.3, 0.75, 1, 2.5, 10, 1234.5):
        assert simplify.tol2_q8(t) == SR.tol2_q8(t)
    for bad in (-0.1, float("nan"), float("inf"), 32768.5, "1", None, True, [1.0]):
        with pytest.raises(ValueError):
            simplify.tol2_q8(bad)


def test_bad_arguments_are_refused_before_the_library(monkeypatch):
    def no_call(*a, **k):
        raise AssertionError(f"{a} requested")
    monkeypatch.setattr(_ext, "ext_symbol", no_call)
    monkeypatch.setattr(_lib, "symbol", no_call)
    import torch
    ok = [np.array([[0, 0], [1, 1], [2, 0]])]
    for lines, kw in ((ok, dict(tolerance=-1)), (ok, dict(tolerance=float("nan"))), (ok, dict(tolerance=1e9)),
                      (ok, dict(tolerance=1.0, closed=1)), ([np.zeros((3, 1), int)], dict(tolerance=1.0)),
                      ([np.zeros((3, 5), int)], dict(tolerance=1.0)), ([np.zeros((0, 2), int)], dict(tolerance=1.0)),
                      ([np.zeros((3, 2))], dict(tolerance=1.0)), ([np.zeros(3, int)], dict(tolerance=1.0)),
                      (ok + [np.zeros((2, 3), int)], dict(tolerance=1.0)), ([np.array([[0, -1], [1, 1]])], dict(tolerance=1.0)),
                      ([np.array([[0, 16385], [1, 1]])], dict(tolerance=1.0)),
                      ([np.array([[0, 1, 1 << 40], [1, 1, 0]])], dict(tolerance=1.0))):
        with pytest.raises(ValueError):
            simplify.simplify(lines, **kw)
    pts, rows, cnt = torch.zeros((1, 8, 2), dtype=torch.int32), torch.zeros((1, 2, 4), dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    for args in ((pts, rows, cnt, (1, 2, -1), -1.0), (pts.long(), rows, cnt, (1, 2, -1), 1.0), (pts, rows.int(), cnt, (1, 2, -1), 1.0),
                 (pts, rows, cnt.long(), (1, 2, -1), 1.0), (pts[0], rows, cnt, (1, 2, -1), 1.0), (pts, rows, cnt, (1, 2, -1), 1.0),
                 (np.zeros((1, 8, 2), np.int32), rows, cnt, (1, 2, -1), 1.0)):
        with pytest.raises(ValueError):   # the sixth: host tensors
            simplify.simplify_device(*args)
    m = np.zeros((4, 4), np.uint8)
    for bad in (-1, float("inf"), "1", True):
        with pytest.raises(ValueError):
            polygons.region_polygons(m, simplify=bad)
        with pytest.raises(ValueError):
            centerlines.trace(m, simplify=bad)


def _options(argv):
    ap = argparse.ArgumentParser()
    scripts.add_evaluation_arguments(ap)
    return scripts.evaluation_options(ap, ap.parse_args(argv), "out/ID1/ID1_metrics.csv")


def test_the_flag_needs_a_geometry_file_and_adds_one_key():
    plain = _options(["--region-polygons"])
    assert "simplify_tolerance" not in plain and "simplify_tolerance" not in _options([])
    assert _options(["--region-polygons", "--simplify", "0.75"]) == dict(plain, simplify_tolerance=0.75)
    graph = _options(["--crack-graph", "1"])
    assert _options(["--crack-graph", "1", "--simplify", "2"]) == dict(graph, simplify_tolerance=2.0)
    for argv in (["--simplify", "1"], ["--region-metrics", "--simplify", "1"], ["--region-polygons", "--simplify", "-1"],
                 ["--region-polygons", "--simplify", "nan"], ["--region-polygons", "--simplify", "x"],
                 ["--crack-graph", "--simplify", "1e9"]):
        with pytest.raises(SystemExit):
            _options(argv)
    with pytest.raises(ValueError, match="simplify_tolerance needs"):
        scripts.evaluate_to_csv(None, [], (1, "m"), "x_metrics.csv", 2, 1, "cpu", simplify_tolerance=1.0)
    with pytest.raises(ValueError):
        scripts.evaluate_to_csv(None, [], (1, "m"), "x_metrics.csv", 2, 1, "cpu", polygons_path="p.geojson", simplify_tolerance=-1.0)


def test_geojson_features_gain_two_properties():
    rec = np.array([[1, 0, 0, 3, 3, 16, 0]], np.int32)
    ring = np.array([[0, 0], [0, 4], [4, 4], [4, 0]], np.int32)
    plain = polygons.polygons_to_geojson(rec, [[ring]])
    thin = polygons.polygons_to_geojson(rec, simplify.Simplified([[ring]], 0.75, [12]))
    assert set(thin["features"][0]["properties"]) - set(plain["features"][0]["properties"]) == {"simplify_tolerance", "vertices_full"}
    assert thin["features"][0]["properties"]["simplify_tolerance"] == 0.75 and thin["features"][0]["properties"]["vertices_full"] == 12
    for f in thin["features"]:
        f["properties"].pop("simplify_tolerance"), f["properties"].pop("vertices_full")
    assert thin == plain
    # a branch of 5 points thinned to its corner points: the widths are the full branch's, the count is the kept one
    branches = np.array([[9, 28, 0, 3, 0, 3, 1, 65536 * 7, 4]], np.int64)
    full_pts = np.array([[1, 1, 1], [1, 2, 4], [1, 3, 4], [2, 3, 1], [3, 4, 1]], np.int32)
    pts = simplify.Simplified([full_pts[[0, 2, 4]]], 1.0, [5])
    t = centerlines.branch_table(branches, 0.5, pts)[0]
    full = centerlines.branch_table(np.array([[9, 28, 0, 5, 0, 3, 1, 65536 * 7, 4]], np.int64), 0.5, [full_pts])[0]
    assert t["points"] == 3 and {k: v for k, v in t.items() if k != "points"} == {k: v for k, v in full.items() if k != "points"}
    g = centerlines.centerlines_to_geojson(branches, pts, class_id=1)
    props = g["features"][0]["properties"]
    assert props["simplify_tolerance"] == 1.0 and props["vertices_full"] == 5 and props["points"] == 3
    assert g["features"][0]["geometry"]["coordinates"] == [[1.5, 1.5], [3.5, 1.5], [4.5, 3.5]]
    assert "simplify_tolerance" not in centerlines.centerlines_to_geojson(branches, [full_pts[[0, 2, 4]]])["features"][0]["properties"]
