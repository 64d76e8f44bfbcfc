/*
 * vitseg_polygons.h -- the region outlines: a family header of libvitseg.so's C ABI.
 *
 * A family header declares the entry points of one feature beside vitseg.h, which stays as it is: it includes vitseg.h,
 * keeps its conventions (extern "C", 0 or a negative VITSEG_E* code, the message through vitseg_last_error(), the caller
 * owns all device memory, work is enqueued on `stream`, a hipStream_t passed as void*), carries a version of its own and
 * uses only int, size_t, int32_t, int64_t, uint8_t, pointers to them and void*.  The Python side states the family once in
 * visiontransformer_amd/_ext.py (EXT_SIGNATURES), and tests compare that table with this file.
 *
 * ---- outlines of connected regions as polygon rings with holes (the usual host answer is cv2.findContours or
 *      skimage.measure.find_contours per class and image; the reference draws boxes only) ----
 * Regions are exactly vitseg_regions': the same connectivity (4 or 8), the same background (-1 or 0..255), the same
 * (class, first) order and counts.
 *
 * Corner lattice.  A corner is (y, x) with 0 <= y <= H and 0 <= x <= W; pixel (r, c) is the square with the corners (r, c),
 * (r, c+1), (r+1, c+1), (r+1, c).
 * Directed edges.  Directions are E = 0, S = 1, W = 2, N = 3.  A pixel of region R has a boundary side wherever its
 * 4-neighbour on that side is not in R (another region, the background or outside the image).  Each boundary side is one
 * directed unit edge with R on its right: the top side is tail (r, c) going E, the right side tail (r, c+1) going S, the bottom
 * side tail (r+1, c+1) going W, the left side tail (r+1, c) going N.  (tail, direction) <-> (pixel, side) is a bijection.
 * Successor of an edge with head h and direction d: the one edge of R leaving h with direction d+1 (right turn), d
 * (straight) or d+3 (left turn), mod 4.  Only at a saddle corner -- two diagonal pixels of R meet, the other two pixels of the
 * 2 x 2 block are not in R -- both turns exist: connectivity 4 takes the right turn (the ring stays round its own pixel),
 * connectivity 8 the left turn (the two pixels are one body).  A ring may therefore visit a corner twice.
 * Rings.  A ring is a cycle of successors.  Its vertices are the tails of its edges whose predecessor has another direction
 * (collinear corners are dropped).  It starts at the tail of its smallest edge by (tail y, tail x, direction), which is
 * always a vertex, and its vertices follow in walking order.  Its area is the shoelace sum
 * 1/2 sum (x_i y_{i+1} - x_{i+1} y_i), an integer: positive for the one outer ring of a region, negative for each hole
 * (holes are the components of the complement off the region's outside under the dual connectivity).  The rings of an image
 * are numbered by the (tail y, tail x, direction) order of their start edges; a region's outer ring starts at its `first`
 * pixel's corner going E and precedes every hole of that region.
 *
 * mask uint8 [n, H, W];
 * region_counts int32 [n]: vitseg_regions' counts;  ring_counts int32 [n], vertex_counts int64 [n]: the true totals of each
 *   image, also above the capacities;
 * rings int64 [n, max_rings, 4]: (region index in vitseg_regions' order, offset of the ring's first vertex in the image's
 *   vertex list, vertex count, signed area); row i is written iff i < max_rings; rows past the count are zero; may be NULL
 *   when max_rings == 0;
 * vertices int32 [n, max_vertices, 2]: (y, x), ring after ring; vertex j of an image is written iff j < max_vertices; rows
 *   past the count are zero; may be NULL when max_vertices == 0 (both capacities 0: a pure count query);
 * labels (optional) int32 [n, H, W]: vitseg_regions' labels.
 * scratch: vitseg_region_polygons_scratch_bytes(n, H, W) device bytes (vitseg_regions' plus about 140 bytes per pixel: 28 bytes
 *   for each of the 4 H W vertices an image can have; every word read is written within the call).  No allocation, no host
 * synchronisation; the number of launches depends on (H, W) alone.  Everything is an integer; sums and counts come from
 * order-independent atomics, ring numbers and vertex offsets from scans in lattice order: the same bits on every call, and an
 * image gets the same bits alone as in a batch.
 * Each with nothing launched -- VITSEG_EINVAL: a null mask, counts or scratch, a null output with a positive capacity, a
 * negative capacity, connectivity not 4 / 8, background outside -1..255; VITSEG_ESHAPE: non-positive sizes, H or W above
 * 16384, H * W >= 2^29 (edge ids are 32-bit within an image) or n > 65535; VITSEG_EWORKSPACE: scratch smaller than
 * vitseg_region_polygons_scratch_bytes (0 for a bad shape).
 */
#ifndef VITSEG_POLYGONS_H
#define VITSEG_POLYGONS_H

#include "vitseg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITSEG_POLYGONS_VERSION 100

int vitseg_polygons_version(void);
size_t vitseg_region_polygons_scratch_bytes(int n, int H, int W);
int vitseg_region_polygons(const uint8_t* mask, int n, int H, int W, int connectivity, int background,
                           int32_t* region_counts /* [n] */, int32_t* ring_counts /* [n] */, int64_t* vertex_counts /* [n] */,
                           int64_t* rings /* [n, max_rings, 4] or NULL */, int max_rings,
                           int32_t* vertices /* [n, max_vertices, 2] or NULL */, int64_t max_vertices,
                           int32_t* labels /* [n, H, W] or NULL */, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VITSEG_POLYGONS_H */
