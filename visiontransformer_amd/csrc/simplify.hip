// Line simplification (vitseg_simplify_lines, include/vitseg_simplify.h): Douglas-Peucker over the rings of polygons.hip and
// the polylines of centerlines.hip, exact integer geometry.  The rule -- the segment distance N, the winner of a base with its
// tie-break, the anchors and the unconditional first split of a closed line -- is stated in the header.
//
// The recursion is run as rounds.  A live interior point knows its base (l, r), the kept points on either side of it; the
// points of one base are the contiguous run l+1 .. r-1 and the base is named by l.  A round: every live point scores itself
// against its base; the base takes the largest N and, among the points that have it, the smallest index (by value, then by
// index: nothing depends on arrival order); if that winner splits the base it is kept and the others re-attach to (l, w) or
// (w, r), otherwise all of them retire.  Every round keeps a point or retires a base, so a line of c points is done after
// fewer than c rounds; the loop stops at c whatever the data.  After the rounds a closed line whose kept points do not have
// the sign of the full ring's area (a ring that crossed itself and turned over) keeps all its points.
//   (zero)     out_lines, out_points and the mark words
//   wave       lines of <= SHORT points, one wave per line, a point per lane: the state in registers, the arg-max of all bases
//              of the wave by one segmented prefix scan over the lanes
//   resident   lines of <= RESIDENT points, one workgroup per line: packed coordinates, l, r and the per-base best (N, index)
//              in LDS, LDS atomics, a barrier between the phases of a round
//   long       longer lines, one workgroup of 1024 threads per line: the same code over arrays in scratch, indexed by the
//              point's place in `points` (lines do not overlap), coordinates read from `points`; a wave whose live lanes
//              share a base reduces first and issues one atomic
//              each of the three walks the lines grid-stride (the line counts live on the device), writes its lines' rows
//              (kept count, input count, area, box) and every point's mark: bit 0 kept, the other bits line + 1 at a line's
//              first point
//   count      per chunk of 1024 points: the kept marks
//   (scan)     chunk scan of chains.hip: the chunk bases in point order; the image's total
//   emit       per chunk: every kept point to its place; a line's first point writes the line's new offset
// The only global atomics are those of one workgroup on its own line's words in the long class.
#include "chains.hpp"
#include "kernels.hpp"
#include "../../include/vitseg_simplify.h"

namespace vitseg {
namespace {

constexpr int SHORT = VITSEG_SIMPLIFY_SHORT;
constexpr int RESIDENT = VITSEG_SIMPLIFY_RESIDENT;
constexpr int MAX_COORD = 16384;
constexpr long long MAX_TOL2 = 1ll << 38;
constexpr int LINE_BLOCKS = 256;   // workgroups per image, at most, of the three line-strided launches
constexpr int LONG_THREADS = 1024;   // per workgroup of the long class: a round walks the whole line four times
static_assert(SHORT == WAVE, "the wave class holds a point per lane");
static_assert(RESIDENT * 24 <= 60 * 1024, "the resident class keeps 24 bytes per point in static LDS");

struct Args {
    const int* points;
    long long max_points;
    int stride;
    const long long* lines;
    int max_lines, row_stride, offset_col, count_col, closed_col;
    const int* line_counts;
    long long tol2;
    long long* out_lines;
    int* mark;
};

struct Line {   // one row, checked: ok = the points lie inside `points`
    long long off;
    long long count;   // as given
    bool closed, ok;
};

__device__ __forceinline__ Line read_line(const Args& a, int image, int j) {
    const long long* row = a.lines + ((size_t)image * a.max_lines + j) * a.row_stride;
    Line l;
    l.off = row[a.offset_col];
    l.count = row[a.count_col];
    l.closed = a.closed_col < 0 || row[a.closed_col] != 0;
    l.ok = l.count >= 1 && l.off >= 0 && l.off <= a.max_points && l.count <= a.max_points - l.off;
    return l;
}

__device__ __forceinline__ int unpack_y(int yx) { return yx >> 16; }
__device__ __forceinline__ int unpack_x(int yx) { return yx & 0xffff; }

// N of p against the base (a, b); Lsq = |b - a|^2
__device__ __forceinline__ u64 score(int p, int a, int b, u64& Lsq) {
    const long long ay = unpack_y(a), ax = unpack_x(a);
    const long long dy = unpack_y(b) - ay, dx = unpack_x(b) - ax, qy = unpack_y(p) - ay, qx = unpack_x(p) - ax;
    const long long L = dy * dy + dx * dx;
    Lsq = (u64)L;
    if (L == 0) return (u64)(qy * qy + qx * qx);
    const long long t = qy * dy + qx * dx;
    if (t < 0) return (u64)(L * (qy * qy + qx * qx));
    if (t > L) {
        const long long ry = qy - dy, rx = qx - dx;
        return (u64)(L * (ry * ry + rx * rx));
    }
    const long long c = dy * qx - dx * qy;
    return (u64)(c * c);
}

// 256 N > tol2 * max(L, 1), exactly: both sides as 128-bit words
__device__ __forceinline__ bool far(u64 N, u64 Lsq, u64 tol2) {
    const u64 m = Lsq ? Lsq : 1;
    const u64 lhi = N >> 56, llo = N << 8;
    const u64 rhi = __umul64hi(tol2, m), rlo = tol2 * m;
    return lhi > rhi || (lhi == rhi && llo > rlo);
}

__device__ __forceinline__ long long shoelace(int p, int q) {   // x_p y_q - x_q y_p
    return (long long)unpack_x(p) * unpack_y(q) - (long long)unpack_x(q) * unpack_y(p);
}

// the sign guard of a closed line: the full ring has an area and the kept points have none or the opposite one
__device__ __forceinline__ bool lost_sign(long long full2, long long kept2) {
    return full2 != 0 && (kept2 == 0 || (kept2 > 0) != (full2 > 0));
}

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        const u64 o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
    for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ int wave_min_int(int v) {
    for (int d = WAVE / 2; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ int wave_max_int(int v) {
    for (int d = WAVE / 2; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

__device__ __forceinline__ void write_row(const Args& a, int image, int j, long long kept, long long count, long long area2,
                                          int ymin, int xmin, int ymax, int xmax) {
    long long* row = a.out_lines + ((size_t)image * a.max_lines + j) * 8;
    row[1] = kept;   // row[0], the new offset, comes from the emit launch
    row[2] = count;
    row[3] = area2;
    row[4] = ymin;
    row[5] = xmin;
    row[6] = ymax;
    row[7] = xmax;
}

// ---- the wave class: grid (LINE_BLOCKS or fewer, n), 4 waves per workgroup, a line per wave ----
__global__ __launch_bounds__(256) void simplify_wave_kernel(Args a) {
    const int image = blockIdx.y, lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int nlines = min(max(a.line_counts[image], 0), a.max_lines);
    const int* pts = a.points + (size_t)image * a.max_points * a.stride;
    int* mark = a.mark + (size_t)image * a.max_points;
    for (int j = blockIdx.x * 4 + wave; j < nlines; j += gridDim.x * 4) {
        const Line ln = read_line(a, image, j);
        if (ln.count > SHORT) continue;   // another class's line
        if (!ln.ok) {
            if (lane == 0) write_row(a, image, j, 0, ln.count, 0, 0, 0, 0, 0);
            continue;
        }
        const int c = (int)ln.count;
        const bool mine = lane < c;
        int y = 0, x = 0;
        if (mine) {
            y = pts[(ln.off + lane) * a.stride];
            x = pts[(ln.off + lane) * a.stride + 1];
        }
        if (__ballot(mine && (y < 0 || y > MAX_COORD || x < 0 || x > MAX_COORD))) {
            if (lane == 0) write_row(a, image, j, 0, ln.count, 0, 0, 0, 0, 0);
            continue;
        }
        const int yx = y << 16 | x;
        const int ymin = wave_min_int(mine ? y : MAX_COORD), xmin = wave_min_int(mine ? x : MAX_COORD);
        const int ymax = wave_max_int(y), xmax = wave_max_int(x);
        // L >= 0: live with the base (L, R); otherwise R < 0 kept, R = 0 gone
        int L = -1, R = mine ? -1 : 0, f = 0;
        if (ln.closed) {
            if (c >= 4) {
                const int p0 = __shfl(yx, 0);
                const long long ey = y - unpack_y(p0), ex = x - unpack_x(p0);
                const u64 key = mine ? ((u64)(ey * ey + ex * ex) << 6 | (u64)(WAVE - 1 - lane)) : 0;
                f = WAVE - 1 - (int)(wave_max_u64(key) & (WAVE - 1));
                if (mine && lane != 0 && lane != f) {
                    L = lane < f ? 0 : f;
                    R = lane < f ? f : c;
                }
            }
        } else if (mine && lane > 0 && lane < c - 1) {
            L = 0;
            R = c - 1;
        }
        for (int round = 0; round < c && __ballot(L >= 0); ++round) {
            const bool live = L >= 0;
            const int l = live ? L : 0, r = live ? R : 1;
            const int pa = __shfl(yx, l), pb = __shfl(yx, r == c ? 0 : r);
            u64 Lsq = 1, N = 0;
            int I = lane;
            if (live) N = score(yx, pa, pb, Lsq);
            for (int d = 1; d < WAVE; d <<= 1) {   // prefix arg-max within the base: lanes l+1 .. lane
                const u64 oN = __shfl_up(N, d);
                const int oI = __shfl_up(I, d);
                if (live && lane - d > l && oN >= N) {
                    N = oN;
                    I = oI;
                }
            }
            const int last = live ? r - 1 : lane;   // the base's last lane holds the base's winner
            const u64 bN = __shfl(N, last);
            const int bI = __shfl(I, last);
            if (live) {
                const bool first = ln.closed && ((l == 0 && r == f) || (l == f && r == c));
                if (!(far(bN, Lsq, (u64)a.tol2) || (first && bN > 0))) {
                    L = -1;
                    R = 0;
                } else if (lane == bI) {
                    L = -1;
                    R = -1;
                } else if (lane < bI) {
                    R = bI;
                } else {
                    L = bI;
                }
            }
        }
        bool kept = mine && L < 0 && R < 0;
        u64 km = __ballot(kept);
        long long area2 = 0;
        if (ln.closed) {
            const u64 after = lane == WAVE - 1 ? 0 : km >> (lane + 1);
            const int nx = after ? lane + 1 + __builtin_ctzll(after) : (km ? __builtin_ctzll(km) : 0);
            const int q = __shfl(yx, nx);
            area2 = wave_sum_i64(kept ? shoelace(yx, q) : 0);
            const int succ = __shfl(yx, lane + 1 < c ? lane + 1 : 0);
            const long long full2 = wave_sum_i64(mine ? shoelace(yx, succ) : 0);
            if (lost_sign(full2, area2)) {   // the ring is returned as it is
                kept = mine;
                km = __ballot(kept);
                area2 = full2;
            }
        }
        if (mine) mark[ln.off + lane] = (int)kept | (lane == 0 ? (j + 1) << 1 : 0);
        if (lane == 0) write_row(a, image, j, __popcll(km), ln.count, area2, ymin, xmin, ymax, xmax);
    }
}

// ---- the resident and the long class: grid (LINE_BLOCKS or fewer, n), a line per workgroup ----
struct Red {   // the words a workgroup reduces into, in LDS
    u64 far_key;
    long long area2, full2;
    int ymin, xmin, ymax, xmax, kept, bad;
};

// at least two lanes are live (l >= 0) and all live lanes name the same base
__device__ __forceinline__ bool one_base(int l) {
    const u64 live = __ballot(l >= 0);
    if (__popcll(live) < 2) return false;
    const int first = __shfl(l, __builtin_ctzll(live));
    return __ballot(l >= 0 && l != first) == 0;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One line of c points by a whole workgroup.  yx, L, R, bN, bI: c words each, in LDS (IN_LDS: yx is filled here) or in
// scratch (yx unused: the coordinates are read from pts).  Every index read back from the arrays is clamped to the line, so
// that lines that overlap in `points` against the contract still stay inside it.
template <bool IN_LDS, int NT>
__device__ __forceinline__ void block_line(const Args& a, int image, int j, const Line& ln, const int* __restrict__ pts, int* mark,
                                           int* yx, int* L, int* R, u64* bN, int* bI, Red* red) {
    const int c = (int)ln.count, tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int* p0 = pts + ln.off * a.stride;
    auto at = [&](int i) -> int { return IN_LDS ? yx[i] : (p0[(size_t)i * a.stride] << 16 | p0[(size_t)i * a.stride + 1]); };
    __syncthreads();   // the line before is done with red and the arrays
    if (tid == 0) {
        red->far_key = 0;
        red->area2 = red->full2 = 0;
        red->ymin = red->xmin = MAX_COORD;
        red->ymax = red->xmax = 0;
        red->kept = 0;
        red->bad = 0;
    }
    __syncthreads();
    {   // the coordinates: range check and box
        int ymin = MAX_COORD, xmin = MAX_COORD, ymax = 0, xmax = 0;
        bool bad = false;
        for (int i = tid; i < c; i += NT) {
            const int y = p0[(size_t)i * a.stride], x = p0[(size_t)i * a.stride + 1];
            if (y < 0 || y > MAX_COORD || x < 0 || x > MAX_COORD) {
                bad = true;
            } else {
                if (IN_LDS) yx[i] = y << 16 | x;
                ymin = min(ymin, y), xmin = min(xmin, x), ymax = max(ymax, y), xmax = max(xmax, x);
            }
        }
        ymin = wave_min_int(ymin), xmin = wave_min_int(xmin), ymax = wave_max_int(ymax), xmax = wave_max_int(xmax);
        if (lane == 0) {
            atomicMin(&red->ymin, ymin), atomicMin(&red->xmin, xmin), atomicMax(&red->ymax, ymax), atomicMax(&red->xmax, xmax);
        }
        if (__syncthreads_or(bad)) {   // skipped: no mark is written (they are zero), the row says kept 0
            if (tid == 0) write_row(a, image, j, 0, ln.count, 0, 0, 0, 0, 0);
            return;
        }
    }
    int f = 0;
    const bool halves = ln.closed && c >= 4;
    if (halves) {   // the far anchor: largest |p - p0|^2, smallest index
        const int q0 = at(0);
        u64 key = 0;
        for (int i = tid; i < c; i += NT) {
            const int q = at(i);
            const long long ey = unpack_y(q) - unpack_y(q0), ex = unpack_x(q) - unpack_x(q0);
            const u64 k = (u64)(ey * ey + ex * ex) << 32 | (u64)(0xffffffffu - (u32)i);
            key = k > key ? k : key;
        }
        key = wave_max_u64(key);
        if (lane == 0) atomicMax(&red->far_key, key);
        __syncthreads();
        f = clampi((int)(0xffffffffu - (u32)(red->far_key & 0xffffffffull)), 0, c - 1);
    }
    // L >= 0: live with the base (L, R).  L = -1: settled, R < 0 kept and the next kept point is -1 - R (c: the line's end, or
    // the way back to p0), R = 0 gone.  L <= -2: kept in this round out of the base (-2 - L, .)
    for (int i = tid; i < c; i += NT) {
        int l = -1, r;
        if (ln.closed && !halves) {
            r = -1 - (i + 1);
        } else if (halves) {
            if (i == 0) r = -1 - (f ? f : c);
            else if (i == f) r = -1 - c;
            else l = i < f ? 0 : f, r = i < f ? f : c;
        } else {
            if (i == c - 1) r = -1 - c;
            else if (i == 0) r = -1 - (c - 1);
            else l = 0, r = c - 1;
        }
        L[i] = l;
        R[i] = r;
        bN[i] = 0;
        bI[i] = 0x7fffffff;
    }
    __syncthreads();
    for (int round = 0; round < c; ++round) {
        // The lanes of a wave hold consecutive points, which mostly share a base.  Over scratch the wave then reduces first and
        // one lane updates the base's word in global memory; in LDS every live lane does (an LDS atomic on one word costs less
        // than the reduction: measured).  Whole waves run both loops (the reductions need every lane).
        for (int b0 = 0; b0 < c; b0 += NT) {   // the largest N of every base
            const int i = b0 + tid;
            const int l = i < c ? min(L[i], c - 1) : -1;
            u64 N = 0;
            if (l >= 0) {
                const int r = clampi(R[i], 1, c);
                u64 Lsq;
                N = score(at(i), at(l), at(r == c ? 0 : r), Lsq);
            }
            if (!IN_LDS && one_base(l)) {
                const u64 best = wave_max_u64(N);
                const int base = wave_max_int(l);
                if (lane == 0) atomicMax(&bN[base], best);
            } else if (l >= 0) {
                atomicMax(&bN[l], N);
            }
        }
        __syncthreads();
        for (int b0 = 0; b0 < c; b0 += NT) {   // the smallest index that has it
            const int i = b0 + tid;
            const int l = i < c ? min(L[i], c - 1) : -1;
            int cand = 0x7fffffff;
            if (l >= 0) {
                const int r = clampi(R[i], 1, c);
                u64 Lsq;
                if (score(at(i), at(l), at(r == c ? 0 : r), Lsq) == bN[l]) cand = i;
            }
            if (!IN_LDS && one_base(l)) {
                const int first_i = wave_min_int(cand);
                const int base = wave_max_int(l);
                if (lane == 0 && first_i != 0x7fffffff) atomicMin(&bI[base], first_i);
            } else if (cand != 0x7fffffff) {
                atomicMin(&bI[l], cand);
            }
        }
        __syncthreads();
        bool live = false;
        for (int i = tid; i < c; i += NT) {   // split or retire
            const int l = min(L[i], c - 1);
            if (l < 0) continue;
            const int r = clampi(R[i], 1, c);
            const int pa = at(l), pb = at(r == c ? 0 : r);
            const long long dy = unpack_y(pb) - unpack_y(pa), dx = unpack_x(pb) - unpack_x(pa);
            const u64 best = bN[l];
            const int w = clampi(bI[l], 0, c - 1);
            const bool first = halves && ((l == 0 && r == f) || (l == f && r == c));
            if (!(far(best, (u64)(dy * dy + dx * dx), (u64)a.tol2) || (first && best > 0))) {
                L[i] = -1;
                R[i] = 0;
            } else if (i == w) {
                L[i] = -2 - l;
                R[i] = -1 - r;
            } else {
                if (i < w) R[i] = w;
                else L[i] = w;
                live = true;
            }
        }
        const int more = __syncthreads_or(live);
        for (int i = tid; i < c; i += NT) {   // the winners: fresh best words for the two new bases, the link l -> w
            const int s = L[i];
            if (s > -2) continue;
            const int l = clampi(-2 - s, 0, c - 1);
            bN[l] = 0, bI[l] = 0x7fffffff, bN[i] = 0, bI[i] = 0x7fffffff;
            R[l] = -1 - i;
            L[i] = -1;
        }
        __syncthreads();
        if (!more) break;
    }
    // a loop stopped by its cap leaves live points: they count as gone
    int kept = 0;
    long long area2 = 0, full2 = 0;
    for (int i = tid; i < c; i += NT) {
        const bool k = L[i] < 0 && R[i] < 0;
        kept += k;
        if (ln.closed) {
            const int p = at(i);
            full2 += shoelace(p, at(i + 1 < c ? i + 1 : 0));
            if (k) {
                const int nx = clampi(-1 - R[i], 0, c);
                area2 += shoelace(p, at(nx == c ? 0 : nx));
            }
        }
        mark[ln.off + i] = (int)k | (i == 0 ? (j + 1) << 1 : 0);
    }
    kept = wave_sum(kept);
    area2 = wave_sum_i64(area2);
    full2 = wave_sum_i64(full2);
    if (lane == 0) {
        atomicAdd(&red->kept, kept);
        atomicAdd((u64*)&red->area2, (u64)area2);
        atomicAdd((u64*)&red->full2, (u64)full2);
    }
    __syncthreads();
    if (lost_sign(red->full2, red->area2)) {   // the same words on every thread: the ring is returned as it is
        for (int i = tid; i < c; i += NT) mark[ln.off + i] = 1 | (i == 0 ? (j + 1) << 1 : 0);
        if (tid == 0) write_row(a, image, j, c, ln.count, red->full2, red->ymin, red->xmin, red->ymax, red->xmax);
        return;
    }
    if (tid == 0) write_row(a, image, j, red->kept, ln.count, red->area2, red->ymin, red->xmin, red->ymax, red->xmax);
}

// The workgroup's lines -- blockIdx.x, blockIdx.x + gridDim.x, ... -- whose count lies in (lo, hi], handed to `body` one by
// one on every thread.  Each thread reads the count of one line, NT lines at a time, and the hits queue up in LDS: most rows
// belong to another class and cost one load, not one per wave.  The order within the queue is arbitrary; lines do not depend
// on each other.  queue [NT], qn: shared.
template <int NT, class Body>
__device__ __forceinline__ void for_lines(const Args& a, int image, int nlines, long long lo, long long hi, int* queue, int* qn,
                                          Body&& body) {
    for (long long b0 = blockIdx.x; b0 < nlines; b0 += (long long)gridDim.x * NT) {
        __syncthreads();   // the queue of the batch before is used up
        if (threadIdx.x == 0) *qn = 0;
        __syncthreads();
        const long long j = b0 + (long long)threadIdx.x * gridDim.x;
        if (j < nlines) {
            const long long cnt = a.lines[((size_t)image * a.max_lines + j) * a.row_stride + a.count_col];
            if (cnt > lo && cnt <= hi) queue[atomicAdd(qn, 1)] = (int)j;
        }
        __syncthreads();
        const int hits = *qn;
        for (int q = 0; q < hits; ++q) body(queue[q]);
    }
}

__global__ __launch_bounds__(256) void simplify_resident_kernel(Args a) {
    __shared__ int yx[RESIDENT], L[RESIDENT], R[RESIDENT], bI[RESIDENT];
    __shared__ u64 bN[RESIDENT];
    __shared__ Red red;
    __shared__ int queue[256], qn;
    const int image = blockIdx.y;
    const int nlines = min(max(a.line_counts[image], 0), a.max_lines);
    const int* pts = a.points + (size_t)image * a.max_points * a.stride;
    int* mark = a.mark + (size_t)image * a.max_points;
    for_lines<256>(a, image, nlines, SHORT, RESIDENT, queue, &qn, [&](int j) {
        const Line ln = read_line(a, image, j);   // the same words on every thread: the branch is uniform
        if (!ln.ok) {
            if (threadIdx.x == 0) write_row(a, image, j, 0, ln.count, 0, 0, 0, 0, 0);
            return;
        }
        block_line<true, 256>(a, image, j, ln, pts, mark, yx, L, R, bN, bI, &red);
    });
}

__global__ __launch_bounds__(LONG_THREADS) void simplify_long_kernel(Args a, int* gL, int* gR, u64* gN, int* gI) {
    __shared__ Red red;
    __shared__ int queue[LONG_THREADS], qn;
    const int image = blockIdx.y;
    const int nlines = min(max(a.line_counts[image], 0), a.max_lines);
    const int* pts = a.points + (size_t)image * a.max_points * a.stride;
    const size_t at = (size_t)image * a.max_points;
    for_lines<LONG_THREADS>(a, image, nlines, RESIDENT, 0x7fffffffffffffffll, queue, &qn, [&](int j) {
        const Line ln = read_line(a, image, j);
        if (!ln.ok) {
            if (threadIdx.x == 0) write_row(a, image, j, 0, ln.count, 0, 0, 0, 0, 0);
            return;
        }
        const size_t o = at + ln.off;
        block_line<false, LONG_THREADS>(a, image, j, ln, pts, a.mark + at, nullptr, gL + o, gR + o, gN + o, gI + o, &red);
    });
}

// grid (ceil(max_points / 1024), n): the kept marks of every chunk
__global__ __launch_bounds__(256) void simplify_count_kernel(const int* __restrict__ mark, int* __restrict__ ctot,
                                                             long long max_points, int nchunks) {
    __shared__ int wsum[4];
    const int* m = mark + (size_t)blockIdx.y * max_points;
    int cnt = 0;
    for (int k = 0; k < 4; ++k) {
        const long long p = (long long)blockIdx.x * CHUNK + threadIdx.x * 4 + k;
        if (p < max_points) cnt += m[p] & 1;
    }
    int total;
    block_scan(cnt, wsum, total);
    if (threadIdx.x == 0) ctot[(size_t)blockIdx.y * nchunks + blockIdx.x] = total;
}

// grid as count: every kept point to its place in point order; a line's first point carries the line's new offset
__global__ __launch_bounds__(256) void simplify_emit_kernel(const int* __restrict__ points, const int* __restrict__ mark,
                                                            const int* __restrict__ ctot, long long* __restrict__ out_lines,
                                                            int* __restrict__ out_points, long long max_points, int stride,
                                                            int max_lines, long long max_out, int nchunks) {
    __shared__ int wsum[4];
    const int* m = mark + (size_t)blockIdx.y * max_points;
    const int* src = points + (size_t)blockIdx.y * max_points * stride;
    int w[4], cnt = 0;
    for (int k = 0; k < 4; ++k) {
        const long long p = (long long)blockIdx.x * CHUNK + threadIdx.x * 4 + k;
        w[k] = p < max_points ? m[p] : 0;
        cnt += w[k] & 1;
    }
    int total;
    long long pos = ctot[(size_t)blockIdx.y * nchunks + blockIdx.x] + block_scan(cnt, wsum, total);
    for (int k = 0; k < 4; ++k) {
        if (w[k] == 0) continue;
        const long long p = (long long)blockIdx.x * CHUNK + threadIdx.x * 4 + k;
        const int line = (w[k] >> 1) - 1;
        if (line >= 0 && line < max_lines) out_lines[((size_t)blockIdx.y * max_lines + line) * 8] = pos;
        if (w[k] & 1) {
            if (pos < max_out) {
                int* dst = out_points + ((size_t)blockIdx.y * max_out + pos) * stride;
                for (int e = 0; e < stride; ++e) dst[e] = src[p * stride + e];
            }
            ++pos;
        }
    }
}

bool shape_ok(int n, int max_lines, long long max_points) {
    return n >= 1 && n <= 65535 && max_lines >= 0 && max_lines <= (1 << 24) && max_points >= 0 && max_points <= (1ll << 30);
}

struct Layout {   // [n][max_points] each but ctot [n][nchunks]
    size_t mark, gL, gR, gI, gN, ctot, total;
    int nchunks;
};

Layout layout(int n, int max_lines, long long max_points) {
    Layout l{};
    const size_t P = (size_t)n * (size_t)max_points;
    l.nchunks = (int)((max_points + CHUNK - 1) / CHUNK);
    if (l.nchunks < 1) l.nchunks = 1;
    size_t o = 0;
    l.mark = o;  o += up256(P * sizeof(int));
    l.gL = o;    o += up256(P * sizeof(int));
    l.gR = o;    o += up256(P * sizeof(int));
    l.gI = o;    o += up256(P * sizeof(int));
    l.gN = o;    o += up256(P * sizeof(u64));
    l.ctot = o;  o += up256((size_t)n * l.nchunks * sizeof(int));
    l.total = o;
    return l;
}

}  // namespace

size_t simplify_scratch_bytes(int n, int max_lines, long long max_points) {
    return shape_ok(n, max_lines, max_points) ? layout(n, max_lines, max_points).total : 0;
}

int launch_simplify_lines(const int* points, long long max_points, int stride, const long long* lines, int max_lines,
                          int row_stride, int offset_col, int count_col, int closed_col, const int* line_counts, int n,
                          long long tol2_q8, long long* out_counts, long long* out_lines, int* out_points, long long max_out_points,
                          void* scratch, size_t scratch_bytes, hipStream_t s) {
    VITSEG_CHECK_ARG(points && lines && line_counts && out_counts && out_lines && scratch, VITSEG_EINVAL,
                     "simplify_lines: null points, lines, counts, out_lines or scratch");
    VITSEG_CHECK_ARG(max_out_points >= 0, VITSEG_EINVAL, "simplify_lines: negative max_out_points");
    VITSEG_CHECK_ARG(out_points || max_out_points == 0, VITSEG_EINVAL, "simplify_lines: null out_points with a positive capacity");
    VITSEG_CHECK_ARG(stride >= 2 && stride <= 4, VITSEG_EINVAL, "simplify_lines: stride must be 2..4, got %d", stride);
    VITSEG_CHECK_ARG(row_stride >= 1 && row_stride <= 64 && offset_col >= 0 && offset_col < row_stride && count_col >= 0 &&
                         count_col < row_stride && offset_col != count_col && closed_col >= -1 && closed_col < row_stride,
                     VITSEG_EINVAL, "simplify_lines: bad columns (%d, %d, %d) for rows of %d words", offset_col, count_col,
                     closed_col, row_stride);
    VITSEG_CHECK_ARG(tol2_q8 >= 0 && tol2_q8 <= MAX_TOL2, VITSEG_EINVAL, "simplify_lines: tol2_q8 must be 0..2^38, got %lld",
                     tol2_q8);
    VITSEG_CHECK_ARG(shape_ok(n, max_lines, max_points), VITSEG_ESHAPE,
                     "simplify_lines: bad shape n=%d max_lines=%d max_points=%lld (1 <= n <= 65535, 0 <= max_lines <= 2^24, "
                     "0 <= max_points <= 2^30)", n, max_lines, max_points);
    const Layout l = layout(n, max_lines, max_points);
    VITSEG_CHECK_ARG(scratch_bytes >= l.total, VITSEG_EWORKSPACE, "simplify_lines: scratch of %zu bytes, %zu needed", scratch_bytes,
                     l.total);
    char* base = (char*)scratch;
    int* mark = (int*)(base + l.mark);
    int* ctot = (int*)(base + l.ctot);
    hipError_t e = hipMemsetAsync(out_counts, 0, (size_t)n * sizeof(long long), s);
    if (e == hipSuccess && max_lines > 0) e = hipMemsetAsync(out_lines, 0, (size_t)n * max_lines * 8 * sizeof(long long), s);
    if (e == hipSuccess && max_out_points > 0)
        e = hipMemsetAsync(out_points, 0, (size_t)n * (size_t)max_out_points * stride * sizeof(int), s);
    if (e == hipSuccess && max_points > 0) e = hipMemsetAsync(mark, 0, (size_t)n * (size_t)max_points * sizeof(int), s);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(simplify_lines)");
    if (max_lines == 0 || max_points == 0) return VITSEG_OK;   // no line can hold a point: every count is zero
    const Args a{points, max_points, stride, lines, max_lines, row_stride, offset_col, count_col, closed_col, line_counts, tol2_q8,
                 out_lines, mark};
    const int wave_blocks = (max_lines + 3) / 4;
    const dim3 wgrid(wave_blocks < LINE_BLOCKS ? wave_blocks : LINE_BLOCKS, n);
    const dim3 lgrid(max_lines < LINE_BLOCKS ? max_lines : LINE_BLOCKS, n), cgrid(l.nchunks, n);
    hipLaunchKernelGGL(simplify_wave_kernel, wgrid, dim3(256), 0, s, a);
    VITSEG_LAUNCH_CHECK("simplify_lines wave");
    hipLaunchKernelGGL(simplify_resident_kernel, lgrid, dim3(256), 0, s, a);
    VITSEG_LAUNCH_CHECK("simplify_lines resident");
    hipLaunchKernelGGL(simplify_long_kernel, lgrid, dim3(LONG_THREADS), 0, s, a, (int*)(base + l.gL), (int*)(base + l.gR),
                       (u64*)(base + l.gN), (int*)(base + l.gI));
    VITSEG_LAUNCH_CHECK("simplify_lines long");
    hipLaunchKernelGGL(simplify_count_kernel, cgrid, dim3(256), 0, s, mark, ctot, max_points, l.nchunks);
    VITSEG_LAUNCH_CHECK("simplify_lines count");
    if (const int rc = launch_chunk_scan(ctot, n, l.nchunks, 1, ScanOut{{nullptr, nullptr}, {out_counts, nullptr}}, s)) return rc;
    hipLaunchKernelGGL(simplify_emit_kernel, cgrid, dim3(256), 0, s, points, mark, ctot, out_lines, out_points, max_points, stride,
                       max_lines, max_out_points, l.nchunks);
    VITSEG_LAUNCH_CHECK("simplify_lines emit");
    return VITSEG_OK;
}

}  // namespace vitseg

extern "C" {

int vitseg_simplify_version(void) { return VITSEG_SIMPLIFY_VERSION; }

size_t vitseg_simplify_scratch_bytes(int n, int max_lines, int64_t max_points) {
    return vitseg::simplify_scratch_bytes(n, max_lines, (long long)max_points);
}

int vitseg_simplify_lines(const int32_t* points, int64_t max_points, int stride, const int64_t* lines, int max_lines, int row_stride,
                          int offset_col, int count_col, int closed_col, const int32_t* line_counts, int n, int64_t tol2_q8,
                          int64_t* out_counts, int64_t* out_lines, int32_t* out_points, int64_t max_out_points, void* scratch,
                          size_t scratch_bytes, void* stream) {
    return vitseg::launch_simplify_lines(points, (long long)max_points, stride, (const long long*)lines, max_lines, row_stride,
                                         offset_col, count_col, closed_col, line_counts, n, (long long)tol2_q8,
                                         (long long*)out_counts, (long long*)out_lines, out_points, (long long)max_out_points,
                                         scratch, scratch_bytes, (hipStream_t)stream);
}

}  // extern "C"
