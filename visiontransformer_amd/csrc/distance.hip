// Boundary-distance statistics of class maps: the integers and fp64 sums behind PAED (the reference's pixel average Euclidean
// distance, model/PAED/classes.py:209-258), the Hausdorff distance, its percentiles (HD95) and the average symmetric distance.
//
// Per image and class c: A = {gt == c}, P = {pred == c} (mode 0), or their borders S ^ binary_erosion(S) with the cross
// structure and border_value 0 (mode 1).  The distance of a pixel of A to the nearest pixel of P is the exact squared distance
// field of P (sdf.hip, "ext" field, int32) read at the pixel, so the O(|A| |P|) loop of the reference becomes, per class:
//  1. planes    the 2 n binary images (image i: plane 2 i = A, plane 2 i + 1 = P) and their pixel counts (integer atomicAdd);
//  2. fields    launch_sdf_d2 over the 2 n planes: d2 int32, field j = squared distance to the nearest pixel of plane j;
//  3. reduce    block (chunk, plane j): over the pixels of plane j in the chunk, the fp64 sum of sqrt((double) d2) and the
//               integer maximum of d2 read from field j ^ 1 -> one partial per block.  A thread adds its pixels in index
//               order, the block adds its threads by a butterfly: the order is a function of H * W alone;
//  4. finish    block i: the partials of planes 2 i, 2 i + 1 added in a fixed order; writes n, m, the maxima and the sums,
//               and the two pooled ranks lo, hi of the percentile (from the device counts) as the select's start state;
//  5. select    three rounds of {histogram of the next 10 key bits over the pooled keys whose higher bits equal the prefix;
//               scan: the bucket holding the rank extends the prefix} for both ranks at once.  Keys are < 2^30, the
//               histograms are integer atomics: exact and order-independent.  The scan leaves the histogram zeroed.
// Empty sets are decided on the device from the counts: with n == 0 or m == 0 the maxima and order statistics are -1 and the
// select is skipped; the sums are 0 in mode 1; in mode 0 a pixel whose other set is empty adds sqrt(y^2 + x^2) of its
// (row, column) index, the reference's rule (classes.py:230-235).  The field of an empty plane (sdf.hip's virtual feature) is
// never read.
#include "kernels.hpp"
#include "plane_reduce.hpp"

namespace vitseg {
namespace {

constexpr int DIST_MAX_SIDE = 16384, DIST_MAX_BATCH = 32767;   // the planes are a batch of 2 n <= 65534 for sdf.hip
constexpr int CHUNK = PLANE_CHUNK;   // pixels per block of the reduce and histogram passes (plane_reduce.hpp)
constexpr int BINS = 1024;     // 10 key bits per select round

struct Layout {
    size_t d2, planes, psum, pmax, counts, state, hist, total;
    int NB;
};

Layout layout(int n, int H, int W) {
    Layout l;
    const size_t P = (size_t)H * W, M = 2 * (size_t)n;
    l.NB = (int)((P + CHUNK - 1) / CHUNK);
    size_t o = 0;
    l.d2 = o;      o += up256(M * P * sizeof(int));
    l.planes = o;  o += up256(M * P);
    l.psum = o;    o += up256(M * l.NB * sizeof(double));
    l.pmax = o;    o += up256(M * l.NB * sizeof(int));
    l.counts = o;  o += up256(3 * M * sizeof(int));   // counts [2 n], then sdf.hip's maxima [4 n]: zeroed together per class
    l.state = o;   o += up256((size_t)n * 4 * sizeof(int));
    l.hist = o;    o += up256((size_t)n * 2 * BINS * sizeof(unsigned));
    l.total = o;
    return l;
}

bool shape_ok(int n, int H, int W) {
    return n >= 1 && n <= DIST_MAX_BATCH && H >= 1 && H <= DIST_MAX_SIDE && W >= 1 && W <= DIST_MAX_SIDE;
}

__device__ __forceinline__ bool is_border(const unsigned char* m, int c, int y, int x, int H, int W) {
    const unsigned char* p = m + (size_t)y * W + x;
    return !(y > 0 && p[-W] == c && y < H - 1 && p[W] == c && x > 0 && p[-1] == c && x < W - 1 && p[1] == c);
}

// grid (ceil(P / 1024), n): planes 2 i (gt == c) and 2 i + 1 (pred == c) of image i, in mode 1 their 4-neighbour borders
__global__ __launch_bounds__(256) void dist_planes_kernel(const unsigned char* __restrict__ pred,
                                                          const unsigned char* __restrict__ gt,
                                                          unsigned char* __restrict__ planes, int* __restrict__ counts, int H,
                                                          int W, int c, int mode) {
    const int P = H * W, i = blockIdx.y;
    const unsigned char* g = gt + (size_t)i * P;
    const unsigned char* p = pred + (size_t)i * P;
    unsigned char* pa = planes + (size_t)(2 * i) * P;
    unsigned char* pp = pa + P;
    int ca = 0, cp = 0;
    for (int k = 0; k < 4; ++k) {
        const int idx = blockIdx.x * 1024 + k * 256 + threadIdx.x;
        if (idx >= P) break;
        bool a = g[idx] == c, b = p[idx] == c;
        if (mode == 1 && (a || b)) {
            const int y = idx / W, x = idx - y * W;
            a = a && is_border(g, c, y, x, H, W);
            b = b && is_border(p, c, y, x, H, W);
        }
        pa[idx] = a;
        pp[idx] = b;
        ca += a;
        cp += b;
    }
    ca = wave_sum(ca);
    cp = wave_sum(cp);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        if (ca) atomicAdd(&counts[2 * i], ca);
        if (cp) atomicAdd(&counts[2 * i + 1], cp);
    }
}

// grid (NB, 2 n): partial sum and maximum of block (chunk b, source plane j)
__global__ __launch_bounds__(256) void dist_reduce_kernel(const unsigned char* __restrict__ planes, const int* __restrict__ d2,
                                                          const int* __restrict__ counts, double* __restrict__ psum,
                                                          int* __restrict__ pmax, int P, int W, int mode) {
    __shared__ double shd[4];
    __shared__ int shi[4];
    const int j = blockIdx.y;
    const unsigned char* src = planes + (size_t)j * P;
    const int* fld = d2 + (size_t)(j ^ 1) * P;
    const bool other = counts[j ^ 1] != 0;
    double s = 0.0;
    int mx = 0;
    for_source_pixels(src, P, (P & 3) == 0, [&](int idx) {
        int v = 0;
        if (other) {
            v = fld[idx];
        } else if (mode == 0) {   // the reference's rule for an empty other set: the pixel's distance to the index origin
            const int y = idx / W, x = idx - y * W;
            v = y * y + x * x;
        }
        s += sqrt((double)v);
        mx = max(mx, v);
    });
    s = block_sum(s, shd);
    mx = block_max(mx, shi);
    if (threadIdx.x == 0) {
        psum[(size_t)j * gridDim.x + blockIdx.x] = s;
        pmax[(size_t)j * gridDim.x + blockIdx.x] = mx;
    }
}

// grid (n): the fixed-order sum of the partials, the integer fields of image i and class slot k, the select's start state
__global__ __launch_bounds__(256) void dist_finish_kernel(const double* __restrict__ psum, const int* __restrict__ pmax,
                                                          const int* __restrict__ counts, int* __restrict__ state,
                                                          long long* __restrict__ stats_i, double* __restrict__ stats_f, int NB,
                                                          int K, int k, int pct_num, int pct_den) {
    __shared__ double shd[4];
    __shared__ int shi[4];
    const int i = blockIdx.x;
    double sum[2];
    int mx[2];
    for (int side = 0; side < 2; ++side) {
        const size_t base = (size_t)(2 * i + side) * NB;
        double s = 0.0;
        int m = 0;
        for (int b = threadIdx.x; b < NB; b += 256) {
            s += psum[base + b];
            m = max(m, pmax[base + b]);
        }
        sum[side] = block_sum(s, shd);
        mx[side] = block_max(m, shi);
    }
    if (threadIdx.x != 0) return;
    const long long na = counts[2 * i], np = counts[2 * i + 1];
    const bool both = na > 0 && np > 0;
    const size_t o = (size_t)i * K + k;
    stats_i[o * 6 + 0] = na;
    stats_i[o * 6 + 1] = np;
    stats_i[o * 6 + 2] = both ? mx[0] : -1;
    stats_i[o * 6 + 3] = both ? mx[1] : -1;
    stats_f[o * 2 + 0] = sum[0];
    stats_f[o * 2 + 1] = sum[1];
    int lo = -1, hi = -1;
    if (both) {
        const long long N = na + np;
        lo = (int)((long long)pct_num * (N - 1) / pct_den);
        hi = (int)min((long long)lo + 1, N - 1);
    } else {
        stats_i[o * 6 + 4] = -1;
        stats_i[o * 6 + 5] = -1;
    }
    state[4 * i + 0] = 0;    // prefix of rank lo: the key bits decided so far
    state[4 * i + 1] = 0;    // prefix of rank hi
    state[4 * i + 2] = lo;   // rank among the keys that carry the prefix; -1: nothing to select
    state[4 * i + 3] = hi;
}

// grid (NB, 2 n): round r of the select.  Among the keys of source plane j whose bits above 30 - 10 r equal a rank's prefix,
// count the next 10 bits into that rank's histogram of image j / 2 (one histogram while both ranks share a prefix).
__global__ __launch_bounds__(256) void dist_hist_kernel(const unsigned char* __restrict__ planes, const int* __restrict__ d2,
                                                        const int* __restrict__ state, unsigned* __restrict__ hist, int P,
                                                        int round) {
    __shared__ unsigned h[2 * BINS];
    const int j = blockIdx.y, i = j >> 1;
    if (state[4 * i + 2] < 0) return;
    const int pre0 = state[4 * i + 0], pre1 = state[4 * i + 1];
    const bool same = pre0 == pre1;
    const int nb = same ? BINS : 2 * BINS;
    for (int b = threadIdx.x; b < nb; b += 256) h[b] = 0;
    __syncthreads();
    const unsigned char* src = planes + (size_t)j * P;
    const int* fld = d2 + (size_t)(j ^ 1) * P;
    const int hs = 30 - 10 * round, ds = 20 - 10 * round;
    for_source_pixels(src, P, (P & 3) == 0, [&](int idx) {
        const int key = fld[idx], top = key >> hs, dig = (key >> ds) & (BINS - 1);
        if (top == pre0) atomicAdd(&h[dig], 1u);
        if (!same && top == pre1) atomicAdd(&h[BINS + dig], 1u);
    });
    __syncthreads();
    unsigned* g = hist + (size_t)i * 2 * BINS;
    for (int b = threadIdx.x; b < nb; b += 256)
        if (h[b]) atomicAdd(&g[b], h[b]);
}

// grid (n), 1024 threads: the bucket that holds each rank extends its prefix; after the last round the prefixes are the keys
__global__ __launch_bounds__(1024) void dist_scan_kernel(unsigned* __restrict__ hist, int* __restrict__ state,
                                                         long long* __restrict__ stats_i, int K, int k, int round) {
    __shared__ unsigned sc[BINS];
    __shared__ int res[4];
    const int i = blockIdx.x, t = threadIdx.x;
    if (state[4 * i + 2] < 0) return;
    const int pre[2] = {state[4 * i + 0], state[4 * i + 1]};
    const int rank[2] = {state[4 * i + 2], state[4 * i + 3]};
    const bool same = pre[0] == pre[1];
    unsigned* g = hist + (size_t)i * 2 * BINS;
    const unsigned v0 = g[t], v1 = same ? v0 : g[BINS + t];
    g[t] = 0;
    g[BINS + t] = 0;
    for (int r = 0; r < 2; ++r) {
        const unsigned v = r ? v1 : v0;
        sc[t] = v;
        __syncthreads();
        for (int d = 1; d < BINS; d <<= 1) {
            const unsigned add = t >= d ? sc[t - d] : 0u;
            __syncthreads();
            sc[t] += add;
            __syncthreads();
        }
        const unsigned incl = sc[t], excl = incl - v, rk = (unsigned)rank[r];
        if (excl <= rk && rk < incl) {
            res[r] = (pre[r] << 10) | t;
            res[2 + r] = (int)(rk - excl);
        }
        __syncthreads();
    }
    if (t == 0) {
        state[4 * i + 0] = res[0];
        state[4 * i + 1] = res[1];
        state[4 * i + 2] = res[2];
        state[4 * i + 3] = res[3];
        if (round == 2) {
            const size_t o = (size_t)i * K + k;
            stats_i[o * 6 + 4] = res[0];
            stats_i[o * 6 + 5] = res[1];
        }
    }
}

}  // namespace

size_t distance_scratch_bytes(int n, int H, int W) { return shape_ok(n, H, W) ? layout(n, H, W).total : 0; }

int launch_distance_stats(const unsigned char* pred, const unsigned char* gt, int n, int H, int W, const int* classes, int K,
                          int mode, int pct_num, int pct_den, long long* stats_i, double* stats_f, void* scratch,
                          size_t scratch_bytes, hipStream_t s) {
    VITSEG_CHECK_ARG(pred && gt && classes && stats_i && stats_f && scratch, VITSEG_EINVAL, "distance: null pointer");
    VITSEG_CHECK_ARG(mode == 0 || mode == 1, VITSEG_EINVAL, "distance: mode must be 0 (sets) or 1 (borders), got %d", mode);
    VITSEG_CHECK_ARG(pct_num >= 0 && pct_num <= pct_den && pct_den >= 1 && pct_den <= 1000, VITSEG_EINVAL,
                     "distance: percentile %d / %d outside 0 <= num <= den <= 1000", pct_num, pct_den);
    VITSEG_CHECK_ARG(shape_ok(n, H, W) && K >= 1 && K <= 256, VITSEG_ESHAPE,
                     "distance: bad shape n=%d H=%d W=%d K=%d (1 <= H, W <= %d, 1 <= n <= %d, 1 <= K <= 256)", n, H, W, K,
                     DIST_MAX_SIDE, DIST_MAX_BATCH);
    for (int k = 0; k < K; ++k)
        VITSEG_CHECK_ARG(classes[k] >= 0 && classes[k] <= 255, VITSEG_EINVAL, "distance: class value %d outside 0..255",
                         classes[k]);
    const Layout l = layout(n, H, W);
    VITSEG_CHECK_ARG(scratch_bytes >= l.total, VITSEG_EWORKSPACE, "distance: scratch of %zu bytes, %zu needed", scratch_bytes,
                     l.total);
    char* base = (char*)scratch;
    int* d2 = (int*)(base + l.d2);
    unsigned char* planes = (unsigned char*)(base + l.planes);
    double* psum = (double*)(base + l.psum);
    int* pmax = (int*)(base + l.pmax);
    int* counts = (int*)(base + l.counts);
    int* maxw = counts + 2 * n;
    int* state = (int*)(base + l.state);
    unsigned* hist = (unsigned*)(base + l.hist);
    const int P = H * W, M = 2 * n;
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)n * 2 * BINS * sizeof(unsigned), s);   // every scan leaves it zeroed again
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(distance histograms)");
    for (int k = 0; k < K; ++k) {
        e = hipMemsetAsync(counts, 0, (size_t)3 * M * sizeof(int), s);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(distance counts)");
        hipLaunchKernelGGL(dist_planes_kernel, dim3((P + 1023) / 1024, n), dim3(256), 0, s, pred, gt, planes, counts, H, W,
                           classes[k], mode);
        VITSEG_LAUNCH_CHECK("distance planes");
        const int rc = launch_sdf_d2(planes, M, H, W, d2, maxw, s);
        if (rc != VITSEG_OK) return rc;
        hipLaunchKernelGGL(dist_reduce_kernel, dim3(l.NB, M), dim3(256), 0, s, planes, d2, counts, psum, pmax, P, W, mode);
        VITSEG_LAUNCH_CHECK("distance reduce");
        hipLaunchKernelGGL(dist_finish_kernel, dim3(n), dim3(256), 0, s, psum, pmax, counts, state, stats_i, stats_f, l.NB, K, k,
                           pct_num, pct_den);
        VITSEG_LAUNCH_CHECK("distance finish");
        for (int round = 0; round < 3; ++round) {
            hipLaunchKernelGGL(dist_hist_kernel, dim3(l.NB, M), dim3(256), 0, s, planes, d2, state, hist, P, round);
            VITSEG_LAUNCH_CHECK("distance histogram");
            hipLaunchKernelGGL(dist_scan_kernel, dim3(n), dim3(BINS), 0, s, hist, state, stats_i, K, k, round);
            VITSEG_LAUNCH_CHECK("distance scan");
        }
    }
    return VITSEG_OK;
}

}  // namespace vitseg

extern "C" {

size_t vitseg_distance_scratch_bytes(int n, int H, int W) { return vitseg::distance_scratch_bytes(n, H, W); }

int vitseg_distance_stats(const uint8_t* pred, const uint8_t* gt, int n, int H, int W, const int32_t* classes, int K, int mode,
                          int pct_num, int pct_den, int64_t* stats_i, double* stats_f, void* scratch, size_t scratch_bytes,
                          void* stream) {
    return vitseg::launch_distance_stats(pred, gt, n, H, W, classes, K, mode, pct_num, pct_den, (long long*)stats_i, stats_f,
                                         scratch, scratch_bytes, (hipStream_t)stream);
}

}  // extern "C"
