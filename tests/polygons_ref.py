"""Plain Python / numpy restatement of vitseg_region_polygons (include/vitseg_polygons.h) on regions_ref's labels: the set of
directed unit edges with the region on their right, the successor rule with its saddle case, the rings as cycles of
successors, their vertices, signed areas and numbering.  Also `rasterize`, the inverse: the pixels a list of rings encloses.
A plain helper module, imported like regions_ref.py."""
import numpy as np

import regions_ref

E, S, W_, N = 0, 1, 2, 3
STEP = ((0, 1), (1, 0), (0, -1), (-1, 0))       # (dy, dx) of a direction
OUTSIDE = ((-1, 0), (0, 1), (1, 0), (0, -1))    # the neighbour across side E (top), S (right), W (bottom), N (left)
TAIL = ((0, 0), (0, 1), (1, 1), (1, 0))         # the tail corner of a pixel's side, relative to the pixel


def edges_of(labels):
    """{(tail_y, tail_x, direction): region} of a label plane int [H, W] (-1 = no region)."""
    H, W = labels.shape
    out = {}
    for r in range(H):
        for c in range(W):
            R = int(labels[r, c])
            if R < 0:
                continue
            for side in range(4):
                y, x = r + OUTSIDE[side][0], c + OUTSIDE[side][1]
                if 0 <= y < H and 0 <= x < W and labels[y, x] == R:
                    continue
                out[(r + TAIL[side][0], c + TAIL[side][1], side)] = R
    return out


def successor(edges, e, connectivity):
    """The edge after e = (tail_y, tail_x, direction) on its ring."""
    y, x, d = e
    h = (y + STEP[d][0], x + STEP[d][1])
    R = edges[e]
    turns = [t for t in ((d + 1) % 4, d, (d + 3) % 4) if edges.get((h[0], h[1], t)) == R]   # right, straight, left
    if len(turns) == 1:
        return (h[0], h[1], turns[0])
    # a saddle: both turns, never the straight edge
    assert turns == [(d + 1) % 4, (d + 3) % 4], (e, turns)
    return (h[0], h[1], turns[0] if connectivity == 4 else turns[1])


def ring_area(ring):
    """The shoelace sum 1/2 sum (x_i y_{i+1} - x_{i+1} y_i) of a ring of (y, x) vertices: an integer."""
    v = np.asarray(ring, dtype=np.int64).reshape(-1, 2)
    y, x = v[:, 0], v[:, 1]
    twice = int(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))
    assert twice % 2 == 0
    return twice // 2


def ring_length(ring):
    """The length of a ring of (y, x) vertices in unit edges."""
    v = np.asarray(ring, dtype=np.int64).reshape(-1, 2)
    return int(np.abs(v - np.roll(v, -1, axis=0)).sum())


def polygons_one(labels, connectivity=4):
    """(rings int64 [r, 4]: region, vertex offset, vertex count, signed area; vertices int32 [v, 2]: (y, x)) of one label
    plane, rings in the order of their start edges."""
    edges = edges_of(np.asarray(labels))
    pred = {}
    for e in edges:
        s = successor(edges, e, connectivity)
        assert edges[s] == edges[e] and s not in pred
        pred[s] = e
    assert set(pred) == set(edges)   # the successor is a permutation: the edges fall into cycles
    seen = set()
    rings, vertices = [], []
    for e in sorted(edges):
        if e in seen:
            continue
        # e is its ring's smallest edge: the ring starts at its tail
        ring, cur = [], e
        while cur not in seen:
            seen.add(cur)
            if pred[cur][2] != cur[2]:
                ring.append((cur[0], cur[1]))
            cur = successor(edges, cur, connectivity)
        assert cur == e and ring[0] == (e[0], e[1])
        rings.append((edges[e], len(vertices), len(ring), ring_area(ring)))
        vertices += ring
    return (np.asarray(rings, dtype=np.int64).reshape(-1, 4), np.asarray(vertices, dtype=np.int32).reshape(-1, 2))


def region_polygons_ref(mask, background=0, connectivity=4):
    """One image's (records, polygons, rings, vertices, labels): regions_ref's records and labels, polygons[i] = the list of
    region i's rings (int32 [v, 2] arrays, in ring order), and the flat rows `polygons_one` gives."""
    rec, lab = regions_ref.regions_one(np.asarray(mask), background, connectivity)
    rings, vertices = polygons_one(lab, connectivity)
    return rec, group_rings(rings, vertices, len(rec)), rings, vertices, lab


def group_rings(rings, vertices, k):
    """polygons[i] = [int32 [v, 2]] of region i, from the flat rows."""
    out = [[] for _ in range(k)]
    for region, off, cnt, _ in np.asarray(rings).reshape(-1, 4):
        out[int(region)].append(np.ascontiguousarray(vertices[int(off):int(off) + int(cnt)]))
    return out


def rasterize(rings, H, W):
    """bool [H, W]: the pixels inside a list of rings ((y, x) vertex arrays; holes run the other way and cancel): the
    cumulative sum along x of +1 per N-going and -1 per S-going vertical unit edge."""
    acc = np.zeros((H, W + 1), np.int64)
    for ring in rings:
        v = np.asarray(ring, dtype=np.int64).reshape(-1, 2)
        for (y0, x0), (y1, x1) in zip(v, np.roll(v, -1, axis=0)):
            if x0 != x1:
                continue
            if y1 < y0:
                acc[y1:y0, x0] += 1   # going N: the region lies to the right, x >= x0
            else:
                acc[y0:y1, x0] -= 1
    inside = np.cumsum(acc, axis=1)[:, :W]
    assert inside.min() >= 0 and inside.max() <= 1, (inside.min(), inside.max())
    return inside == 1
