/*
 * vitseg_simplify.h -- the line simplification (Douglas-Peucker on the device): a family header of libvitseg.so's C ABI.
 *
 * A family header declares the entry points of one feature beside vitseg.h, which stays as it is: it includes vitseg.h,
 * keeps its conventions (extern "C", 0 or a negative VITSEG_E* code, the message through vitseg_last_error(), the caller
 * owns all device memory, work is enqueued on `stream`, a hipStream_t passed as void*), carries a version of its own and
 * uses only int, size_t, int32_t, int64_t, uint8_t, pointers to them and void*.  The Python side states the family once in
 * visiontransformer_amd/_ext.py (EXT_LATER, the table of this and every later family), and tests compare that table with
 * this file.
 *
 * ---- the rings of vitseg_region_polygons and the polylines of vitseg_centerlines thinned where they lie, between the
 *      tracing call and the copy to the host (the usual host answer is cv2.approxPolyDP per contour, or shapely's simplify
 *      with preserve_topology = False) ----
 * The rule.  Exact integer geometry.  A line is a run of points (y, x[, extra ...]), open or closed, 0 <= y, x <= 16384.
 * Simplification keeps a subset of its points, in order, with their extra columns.
 * Distance of a point p from a base (a, b), L = |b - a|^2:
 *   L = 0: to the point: N = |p - a|^2, and p is far iff 256 N > tol2_q8;
 *   else:  to the SEGMENT, not the infinite line (a thin hook that runs past b and returns is not lost): t = (p - a).(b - a);
 *          N = L |p - a|^2 if t < 0, N = L |p - b|^2 if t > L, else N = cross(b - a, p - a)^2; p is far iff 256 N > tol2_q8 L.
 * N < 2^59; the comparison is exact in 128 bits; there is no floating point anywhere.  tol2_q8 is the tolerance squared in
 * 1/256 px^2, at most 2^38 (a tolerance of 32768 px).
 * Open line p0 .. pk.  p0 and pk are kept.  A base (a, b) with interior points has a winner: the interior point of largest N,
 *   on equal N the smallest index.  If the winner is far it is kept and both halves are treated the same way; otherwise every
 *   interior point goes.  A line of one or two points is returned as it is.  tol2_q8 = 0 drops only points that lie on the
 *   segment between kept neighbours.
 * Closed line p0 .. p(c-1), joined back to p0.  The anchors are p0 and f, the point of largest |p - p0|^2 (smallest index on
 *   ties).  The two halves [0 .. f] and [f .. c-1, back to 0] are open lines, and the first split of each half is
 *   unconditional whenever its winner has N > 0: a ring never degenerates to two points, and a hairline crack's outline stays
 *   a sliver polygon of 3-4 vertices whatever the tolerance.  Closed lines of <= 3 points are returned as they are.  (A ring
 *   whose points all coincide has f = 0 and keeps p0 alone.)
 *   The sign guard.  Let A be the shoelace sum of the whole closed line and K that of its kept points.  If A != 0 and K = 0 or
 *   K has the other sign -- the kept points of a thin sprawling ring can cross and come out in the other order -- the line is
 *   returned as it is, every point kept: an outer ring keeps a positive area and a hole a negative one.
 * Result.  p0 stays first; the ends of open lines are always kept, so simplified branches still meet at their node pixels.
 * The two limits: (1) lines are simplified independently of each other, so neighbouring regions may gap or overlap by up to
 * the tolerance along a shared border; (2) a simplified ring may come to touch or cross itself (the sign guard catches only
 * the ring that turned over as a whole).
 *
 * points int32 [n, max_points, stride], stride 2..4: (y, x, extra ...);
 * lines  int64 [n, max_lines, row_stride]: one row per line, its offset into the image's points in column offset_col, its
 *   point count in column count_col, and in column closed_col a non-zero word for a closed line (closed_col = -1: every line
 *   is closed).  Ring rows of vitseg_region_polygons [., 4] go in with (1, 2, -1), branch rows of vitseg_centerlines [., 9]
 *   with (2, 3, 4).  The lines of an image must not overlap in `points` (overlapping lines stay in bounds and terminate; their
 *   result is unspecified);
 * line_counts int32 [n]: the number of rows of each image, clamped to max_lines;
 * out_counts int64 [n]: the kept points of each image, the true totals also above max_out_points;
 * out_lines int64 [n, max_lines, 8]: per line (offset of its first kept point in the image's output list, kept count, input
 *   count, twice the signed shoelace area sum (x_i y_(i+1) - x_(i+1) y_i) of the kept points -- 0 for an open line --, then
 *   ymin, xmin, ymax, xmax of the INPUT points);
 * out_points int32 [n, max_out_points, stride]: the kept points, line after line in the order of `points`.
 * A point is written iff its index is below max_out_points: writes beyond the capacity are suppressed.  Rows past the counts
 * are zero.  out_points may be NULL when max_out_points = 0: a count query (out_lines is filled all the same).
 * Bad data in a row.  A line with count <= 0, a negative offset, offset + count > max_points or a coordinate outside 0..16384
 * is skipped: its row is (0, 0, the count as given, 0, 0, 0, 0, 0) and none of its points is read out of bounds or kept.
 * scratch: vitseg_simplify_scratch_bytes(n, max_lines, max_points) device bytes, about 24 per point (a mark word, and the
 *   base indices and the per-base best word of the lines longer than VITSEG_SIMPLIFY_RESIDENT); every word read is written
 *   within the call.  No allocation, no host synchronisation; the number of launches depends on the capacities alone.  One
 *   launch per length class does all the rounds of its lines: <= VITSEG_SIMPLIFY_SHORT points one wave per line, <=
 *   VITSEG_SIMPLIFY_RESIDENT one workgroup per line inside LDS, longer one workgroup per line over `scratch`.  A line's round
 *   loop stops after `count` rounds at the latest.  Everything is an integer and every arg-max is resolved by value, then
 *   index: the same bits on every call, and an image gets the same bits alone as in a batch.
 * Each with nothing launched -- VITSEG_EINVAL: a null points, lines, line_counts, out_counts, out_lines or scratch, a null
 * out_points with a positive capacity, stride outside 2..4, row_stride outside 1..64, offset_col or count_col outside
 * 0..row_stride-1 or equal, closed_col outside -1..row_stride-1, tol2_q8 negative or above 2^38, a negative max_out_points;
 * VITSEG_ESHAPE: n outside 1..65535, max_lines outside 0..2^24, max_points outside 0..2^30; VITSEG_EWORKSPACE: scratch smaller
 * than vitseg_simplify_scratch_bytes (0 for a bad shape).
 */
#ifndef VITSEG_SIMPLIFY_H
#define VITSEG_SIMPLIFY_H

#include "vitseg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITSEG_SIMPLIFY_VERSION 100
#define VITSEG_SIMPLIFY_SHORT 64      /* longest line handled by one wave: a point per lane */
#define VITSEG_SIMPLIFY_RESIDENT 2048 /* longest line handled inside LDS: 24 bytes per point, 48 KiB per workgroup */

int vitseg_simplify_version(void);
size_t vitseg_simplify_scratch_bytes(int n, int max_lines, int64_t max_points);
int vitseg_simplify_lines(const int32_t* points /* [n, max_points, stride] */, int64_t max_points, int stride /* 2..4 */,
                          const int64_t* lines /* [n, max_lines, row_stride] */, int max_lines, int row_stride,
                          int offset_col, int count_col, int closed_col /* -1: every line is closed */,
                          const int32_t* line_counts /* [n], clamped to max_lines */, int n, int64_t tol2_q8,
                          int64_t* out_counts /* [n] kept points, true totals also above the capacity */,
                          int64_t* out_lines /* [n, max_lines, 8] */,
                          int32_t* out_points /* [n, max_out_points, stride] or NULL */, int64_t max_out_points,
                          void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VITSEG_SIMPLIFY_H */
