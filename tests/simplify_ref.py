"""The line simplification of include/vitseg_simplify.h restated in plain Python integers: Douglas-Peucker with the segment
distance, the winner's tie-break, the anchors, the unconditional first split and the sign guard of a closed line.  An explicit stack of bases,
no rounds: it does not mirror the kernel.  (A helper module, imported like util.py.)"""
import numpy as np

MAX_COORD = 16384


def score(p, a, b):
    """(N, L) of the point p against the base (a, b); points are (y, x) pairs of Python ints."""
    dy, dx = b[0] - a[0], b[1] - a[1]
    qy, qx = p[0] - a[0], p[1] - a[1]
    L = dy * dy + dx * dx
    if L == 0:
        return qy * qy + qx * qx, 0
    t = qy * dy + qx * dx
    if t < 0:
        return L * (qy * qy + qx * qx), L
    if t > L:
        return L * ((p[0] - b[0]) ** 2 + (p[1] - b[1]) ** 2), L
    return (dy * qx - dx * qy) ** 2, L


def far(N, L, tol2_q8):
    return 256 * N > tol2_q8 * (L if L else 1)


def tol2_q8(tolerance):
    return int(round(float(tolerance) * float(tolerance) * 256.0))


def scores(P, l, r):
    """`score` of the points l+1 .. r-1 of P (int64 [c, 2]) against the base (P[l], P[r mod c]) in one numpy expression: every
    N is below 2^59, so int64 holds it exactly (test_simplify_cpu compares it with `score`).  (N int64 [r - l - 1], L)."""
    a, b = P[l], P[r % len(P)]
    d, q = b - a, P[l + 1:r] - a
    L = int(d[0] * d[0] + d[1] * d[1])
    q2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]
    if L == 0:
        return q2, 0
    t = q[:, 0] * d[0] + q[:, 1] * d[1]
    e = P[l + 1:r] - b
    cross = d[0] * q[:, 1] - d[1] * q[:, 0]
    return np.where(t < 0, L * q2, np.where(t > L, L * (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]), cross * cross)), L


def _halves(P, bases, tol2):
    """The kept interior indices of the bases [(l, r, first)]: indices into P, r may be len(P) (the way back to P[0])."""
    kept, stack = [], list(bases)
    while stack:
        l, r, first = stack.pop()
        if r - l < 2:
            continue
        N, L = scores(P, l, r)
        k = int(np.argmax(N))   # the first of the largest: the smallest index among equals
        if far(int(N[k]), L, tol2) or (first and int(N[k]) > 0):
            kept.append(l + 1 + k)
            stack += [(l, l + 1 + k, False), (l + 1 + k, r, False)]
    return kept


def keep_indices(points, tol2, closed=False):
    """The sorted indices of the points a line keeps; `points` [c, >= 2] of ints, tol2 the tolerance squared in 1/256 px^2."""
    P = np.asarray(points)[:, :2].astype(np.int64)
    c = len(P)
    if closed:
        if c <= 3:
            return list(range(c))
        f = int(np.argmax(((P - P[0]) ** 2).sum(axis=1)))
        keep = sorted({0, f} | set(_halves(P, [(0, f, True), (f, c, True)], tol2)))
        A, K = area2(P), area2(P[keep])
        if A != 0 and (K == 0 or (K > 0) != (A > 0)):   # the sign guard: the ring turned over and is returned as it is
            return list(range(c))
        return keep
    if c <= 2:
        return list(range(c))
    return sorted({0, c - 1} | set(_halves(P, [(0, c - 1, False)], tol2)))


def area2(points):
    """Twice the signed shoelace area sum (x_i y_(i+1) - x_(i+1) y_i) of a closed run of (y, x) points."""
    P = [(int(p[0]), int(p[1])) for p in points]
    return sum(P[i][1] * P[(i + 1) % len(P)][0] - P[(i + 1) % len(P)][1] * P[i][0] for i in range(len(P)))


def simplify_image(points, lines, cols, tol2):
    """One image as vitseg_simplify_lines returns it: (out_lines int64 [k, 8], out_points int32 [kept, stride]).  points
    [max_points, stride], lines [k, row_stride], cols = (offset_col, count_col, closed_col)."""
    points = np.asarray(points)
    lines = np.asarray(lines)
    oc, cc, kc = cols
    rows = np.zeros((len(lines), 8), np.int64)
    marks = []   # (offset, line, kept indices)
    for j, row in enumerate(lines):
        off, cnt = int(row[oc]), int(row[cc])
        closed = True if kc < 0 else bool(row[kc])
        rows[j, 2] = cnt
        if cnt < 1 or off < 0 or off + cnt > len(points):
            continue
        P = points[off:off + cnt]
        if P[:, :2].min() < 0 or P[:, :2].max() > MAX_COORD:
            continue
        keep = keep_indices(P, tol2, closed)
        rows[j, 1] = len(keep)
        rows[j, 3] = area2(P[keep]) if closed else 0
        rows[j, 4:6] = P[:, :2].min(axis=0)
        rows[j, 6:8] = P[:, :2].max(axis=0)
        marks.append((off, j, keep))
    out, pos = [], 0
    for off, j, keep in sorted(marks):   # point order
        rows[j, 0] = pos
        out.append(points[off + np.asarray(keep, np.int64)])
        pos += len(keep)
    out = np.concatenate(out) if out else np.zeros((0, points.shape[1]), points.dtype)
    return rows, out.astype(np.int32)


# ---- lines for the tests ----

def walk(rs, count, side=4096, step=3):
    """A random lattice walk of `count` points inside 0..side."""
    d = rs.randint(-step, step + 1, size=(count, 2))
    p = np.cumsum(d, axis=0)
    p -= p.min(axis=0)
    return np.minimum(p, side).astype(np.int32)


def sawtooth(count):
    """A decreasing sawtooth: teeth whose height shrinks from left to right, so that the winner of every base is its
    leftmost tooth and the recursion is about half as deep as the line is long."""
    k = np.arange(count)
    y = np.where(k % 2 == 1, 2 * (count - k) + 4, 0)
    return np.stack([y, 3 * k], axis=1).astype(np.int32)


HAND = {
    # name: (points, closed)
    "straight": ([[5, x] for x in range(9)], False),
    "ell": ([[0, 0], [1, 0], [2, 0], [3, 0], [3, 1], [3, 2], [3, 3]], False),
    "staircase": ([[i // 2, (i + 1) // 2] for i in range(13)], False),
    # runs past b = (0, 10) to x = 14 at a height of 1 px and returns: every point is within 1 px of the LINE through a and b
    "hook": ([[0, 0], [1, 5], [1, 14], [0, 14], [0, 10]], False),
    "node_loop": ([[4, 4], [4, 8], [8, 8], [8, 4], [4, 4]], False),
    "hairline": ([[0, 0], [0, 200], [1, 200], [1, 0]], True),
    "zigzag": ([[0 if i % 2 == 0 else 4, 2 * i] for i in range(11)], False),
    "collinear_ring": ([[0, 0], [0, 2], [0, 4], [2, 4], [4, 4], [4, 2], [4, 0], [2, 0]], True),
}
