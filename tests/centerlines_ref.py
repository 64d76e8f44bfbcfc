"""Plain per-pixel restatement of vitseg_centerlines (include/vitseg_centerlines.h), written from the header's words: a dict of
links, explicit walks from every node, then the curves without a node.  No half-link ids, no scans, no pointer jumping, so
it shares no trick with the kernel.  thin = 1 uses skeleton_ref.skeleton_one, d2 is skeleton_ref.inner_d2.  A plain helper
module, imported like polygons_ref.py."""
import numpy as np

import skeleton_ref as SR

ORTHOGONAL = [(-1, 0), (0, -1), (0, 1), (1, 0)]
DIAGONAL = [(-1, -1), (-1, 1), (1, -1), (1, 1)]


def links_of(S):
    """pixel (y, x) of S -> the sorted list of the pixels it is linked to."""
    S = np.asarray(S) != 0
    H, W = S.shape
    inside = lambda y, x: 0 <= y < H and 0 <= x < W and bool(S[y, x])
    links = {}
    for y in range(H):
        for x in range(W):
            if not S[y, x]:
                continue
            near = [(y + dy, x + dx) for dy, dx in ORTHOGONAL if inside(y + dy, x + dx)]
            for dy, dx in DIAGONAL:   # a diagonal neighbour, unless one of the two pixels next to both is in S
                if inside(y + dy, x + dx) and not inside(y + dy, x) and not inside(y, x + dx):
                    near.append((y + dy, x + dx))
            links[(y, x)] = sorted(near)
    return links


def q16(d2):
    """llrint(sqrt((double) d2) * 65536.0)"""
    return int(np.rint(np.sqrt(np.float64(d2)) * 65536.0))


def planes(mask, value=-1, thin=False):
    """(S bool, d2 int64) of one image."""
    mask = np.asarray(mask)
    X = mask != 0 if value < 0 else mask == value
    S = SR.skeleton_one(X)[0] == 1 if thin else X
    return S, SR.inner_d2(X)


def trace_ref(mask, value=-1, thin=False):
    """(nodes int32 [k, 4], branches int64 [b, 9], points int32 [v, 3]) of one image [H, W], as the header lists them."""
    S, d2 = planes(mask, value, thin)
    return graph_ref(S, d2)


def graph_ref(S, d2):
    H, W = S.shape
    links = links_of(S)
    idx = lambda p: p[0] * W + p[1]
    nodes = [(y, x, len(links[(y, x)]), int(d2[y, x])) for (y, x) in sorted(links) if len(links[(y, x)]) != 2]
    walks, on_open = [], set()
    for p0 in sorted(links):
        if len(links[p0]) == 2:
            continue
        for p1 in links[p0]:
            walk = [p0, p1]
            while len(links[walk[-1]]) == 2:
                a, b = links[walk[-1]]
                walk.append(b if a == walk[-2] else a)
            on_open.update(walk)
            if (idx(walk[0]), idx(walk[1])) < (idx(walk[-1]), idx(walk[-2])):   # found from both ends: the smaller pair reports
                walks.append((walk, 0))
            else:
                assert (idx(walk[0]), idx(walk[1])) != (idx(walk[-1]), idx(walk[-2]))
    seen = set()
    for p0 in sorted(links):   # the first pixel met of a curve without a node is its smallest
        if len(links[p0]) != 2 or p0 in on_open or p0 in seen:
            continue
        walk = [p0, links[p0][0]]
        while True:
            a, b = links[walk[-1]]
            nxt = b if a == walk[-2] else a
            if nxt == p0:
                break
            walk.append(nxt)
        seen.update(walk)
        walks.append((walk, 1))
    walks.sort(key=lambda wk: (idx(wk[0][0]), idx(wk[0][1])))
    branches, points = [], []
    for walk, kind in walks:
        steps = list(zip(walk, walk[1:] + [walk[0]])) if kind else list(zip(walk, walk[1:]))
        diag = sum(1 for a, b in steps if a[0] != b[0] and a[1] != b[1])
        ds = [int(d2[p]) for p in walk]
        branches.append((idx(walk[0]), idx(walk[0] if kind else walk[-1]), len(points), len(walk), kind, len(steps) - diag, diag,
                         sum(q16(d) for d in ds), max(ds)))
        points += [(p[0], p[1], d) for p, d in zip(walk, ds)]
    return (np.asarray(nodes, np.int32).reshape(-1, 4), np.asarray(branches, np.int64).reshape(-1, 9),
            np.asarray(points, np.int32).reshape(-1, 3))


def rasterize(points, H, W):
    """The set of pixels the points cover, as a bool plane."""
    out = np.zeros((H, W), bool)
    pts = np.asarray(points).reshape(-1, 3)
    out[pts[:, 0], pts[:, 1]] = True
    return out


# ---- hand planes ----

def plane(rows):
    """A uint8 plane from strings: '#' is set."""
    return np.array([[c == "#" for c in r] for r in rows], np.uint8)


def serpentine(S, gap=2):
    """One chain: full rows every `gap` rows, joined at alternating ends."""
    m = np.zeros((S, S), np.uint8)
    rows = list(range(0, S, gap))
    for k, y in enumerate(rows):
        m[y, :] = 1
        if k + 1 < len(rows):
            m[y:rows[k + 1] + 1, S - 1 if k % 2 == 0 else 0] = 1
    return m


def nested_rings(S):
    """Concentric square outlines, one background pixel between them."""
    m = np.zeros((S, S), np.uint8)
    for k in range(0, S // 2 - 1, 2):
        m[k, k:S - k] = m[S - 1 - k, k:S - k] = 1
        m[k:S - k, k] = m[k:S - k, S - 1 - k] = 1
    return m


HAND = {
    "single": plane(["...", ".#.", "..."]),
    "line_1x7": plane(["#######"]),
    "corner": plane(["#.", "##"]),
    "diagonal": plane(["#...", ".#..", "..#.", "...#"]),
    "tee": plane(["#####", "..#..", "..#.."]),
    "plus": plane(["..#..", "..#..", "#####", "..#..", "..#.."]),
    "ring_4x4": plane(["####", "#..#", "#..#", "####"]),
    "lollipop": plane([".###...", ".#.#...", ".######", "......."]),
    "parallel": plane(["..###..", "..#.#..", "###.###", "..#.#..", "..###.."]),
}
