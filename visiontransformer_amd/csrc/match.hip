// Region-level detection statistics: the regions of a prediction matched against the regions of the ground truth
// (vitseg_region_match; the panoptic-quality construction of Kirillov et al. 2019 per class, and coverage hit rates beside
// it).  The reference draws the predicted regions (model/CE/testViTModel.py:34-42, 171-185) and compares nothing with the
// ground truth's; the usual host answer is scipy.ndimage.label twice per class and image and a loop over region pairs.
//
// Planes: 2n of them in one staged copy, pred 0..n-1 and gt n..2n-1 with gt == ignore_label turned into background, so that
// one run of the labelling launches of regions.hip leaves every pixel's root and every root's area for both maps (a void
// pixel has no true region; the predicted regions are those of the whole prediction).
//   stage      the copy.
//   (labels)   tile_label, seam_merge, resolve of regions.hip on the 2n planes.
//   pair       a wave on 64 consecutive pixels.  Where pred == gt == c, c in `classes`, the pixel belongs to the pair
//              (rootP, rootG); a run of lanes with one pair adds its length once to the pair's count, to cov[rootP] and to
//              cov[rootG].  With an ignore label, a run of non-void lanes with one rootP adds its length to a[rootP]
//              (without one, a is the labelling's area).  The pair counts live in a per-image open-addressing table of
//              2 * H * W slots keyed by rootP << 32 | rootG: a slot is claimed by a 64-bit atomicCAS on its key (empty = all
//              ones, which no key is: roots are below 2^31) and counted by an integer atomicAdd; linear probing.  An image
//              has at most H * W distinct pairs (each needs a pixel of its own where pred == gt), so at least half of the
//              slots stay empty and every probe sequence ends at an empty slot or at its own key.
//   decide     one thread per slot: an occupied slot's pair matches iff I * thr_den > thr_num * (a + b - I).  A match adds
//              (1, floor(I * 2^32 / U), I, U) to its class in the block's LDS and writes each root's partner; at or above
//              one half a region has at most one partner, so no two threads write one partner word.  One 64-bit integer
//              atomicAdd per block, class and non-zero sum.
//   roots      one thread per pixel: at a root of a class in `classes` (a predicted one only with a > 0) it counts the
//              region, tests its coverage and writes (partner, covered) to the optional planes; (-2, 0) elsewhere.
// The words at roots that pair / decide / roots use are arrays of the labelling that nothing reads after resolve: link (the
// coverage), xmin of the predicted planes (a) and xmax (the partner), set by hipMemsetAsync after the labelling.  Data passes
// between workgroups only at kernel boundaries.  Which slot a pair takes depends on timing; nothing read from the table
// does.  Everything is an integer from order-independent operations: bitwise reproducible, and an image's result does
// not depend on the batch it is in.
#include "kernels.hpp"

namespace vitseg {
namespace {

constexpr int CHUNK = 4096;   // pixels (slots) per block of the three passes
constexpr unsigned long long EMPTY = ~0ull;
enum { N_GT, N_PRED, TP, GT_FOUND, PRED_CONFIRMED, SUM_Q, SUM_I, SUM_U, NSTATS = 8 };

struct ClassMap {   // label value -> index in `classes`, -1 = not asked for
    short k[256];
};

struct Fractions {
    int thr_num, thr_den, cov_num, cov_den;
};

typedef unsigned long long u64;

__global__ __launch_bounds__(256) void stage_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ gt,
                                                    unsigned char* __restrict__ planes, size_t N, int background, int ignore) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const unsigned char g = gt[i];
    planes[i] = pred[i];
    planes[N + i] = (int)g == ignore ? (unsigned char)background : g;
}

// the lanes of a wave hold 64 consecutive pixels; `valid` lanes carry a key and same_as_prev says that lane - 1 carries the
// same one.  At the first lane of every run of equal keys: the run's length; 0 at every other lane.  Whole waves call it.
__device__ __forceinline__ int run_length(bool valid, bool same_as_prev, int lane) {
    const u64 upto = (2ull << lane) - 1ull;   // this lane and the ones below it
    const bool head = valid && (lane == 0 || !same_as_prev);
    const u64 stops = __ballot(head || !valid) & ~upto;
    if (!head) return 0;
    return (stops ? __ffsll((long long)stops) - 1 : WAVE) - lane;
}

// adds cnt to the count of `key` in one image's table.  At most H * W of the cap = 2 * H * W slots are ever claimed (file
// header), so the walk meets an empty slot or its own key within cap steps; the bound on i only keeps the loop finite.
__device__ __forceinline__ void table_add(u64* __restrict__ keys, int* __restrict__ counts, u64 cap, u64 key, int cnt) {
    u64 slot = (((key * 0x9E3779B97F4A7C15ull) >> 32) * cap) >> 32;   // cap < 2^32: below cap
    for (u64 i = 0; i < cap; ++i) {
        const u64 old = atomicCAS(&keys[slot], EMPTY, key);
        if (old == EMPTY || old == key) {
            atomicAdd(&counts[slot], cnt);
            return;
        }
        if (++slot == cap) slot = 0;
    }
}

__global__ __launch_bounds__(256) void pair_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ gt,
                                                   const int* __restrict__ root, int* __restrict__ a, int* __restrict__ cov,
                                                   u64* __restrict__ keys, int* __restrict__ counts, ClassMap km, int n, int P,
                                                   int ignore) {
    const int lane = threadIdx.x & (WAVE - 1);
    const size_t img = (size_t)blockIdx.y * P, baseP = img, baseG = ((size_t)n + blockIdx.y) * P;
    const u64 cap = 2ull * (u64)P;
    keys += (size_t)blockIdx.y * cap;
    counts += (size_t)blockIdx.y * cap;
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long long pl = (long long)blockIdx.x * CHUNK + k * 256 + threadIdx.x;   // a wave: 64 consecutive pixels
        const bool in = pl < P;
        const int p = in ? (int)pl : 0;
        const int cp = pred[img + p], cg = gt[img + p];
        const int rP = in ? root[baseP + p] : -1, rG = in ? root[baseG + p] : -1;
        const int rP_prev = __shfl_up(rP, 1), rG_prev = __shfl_up(rG, 1);
        if (ignore >= 0) {   // the same for every thread of the launch
            const int ka = cg == ignore ? -1 : rP;
            const int ka_prev = __shfl_up(ka, 1);
            const int len = run_length(ka >= 0, ka_prev == ka, lane);
            if (len) atomicAdd(&a[baseP + rP], len);
        }
        // cp == cg in `classes`: neither background nor void, so both roots are there
        const bool hit = in && cp == cg && km.k[cp] >= 0;
        const bool hit_prev = __shfl_up((int)hit, 1);
        const int len = run_length(hit, hit_prev && rP_prev == rP && rG_prev == rG, lane);
        if (len) {
            table_add(keys, counts, cap, ((u64)(unsigned)rP << 32) | (unsigned)rG, len);
            atomicAdd(&cov[baseP + rP], len);
            atomicAdd(&cov[baseG + rG], len);
        }
    }
}

// the block's sums per class, four 64-bit words each, go to `stats` by one atomicAdd per non-zero word
__device__ __forceinline__ void flush_sums(const u64* acc, long long* stats, int K, int f0, int f1, int f2, int f3) {
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * K; i += 256) {
        const int f = i & 3, which = f == 0 ? f0 : f == 1 ? f1 : f == 2 ? f2 : f3;
        if (acc[i]) atomicAdd((u64*)&stats[((size_t)blockIdx.y * K + (i >> 2)) * NSTATS + which], acc[i]);
    }
}

__global__ __launch_bounds__(256) void decide_kernel(const unsigned char* __restrict__ pred, const u64* __restrict__ keys,
                                                     const int* __restrict__ counts, const int* __restrict__ a,
                                                     const int* __restrict__ area, int* __restrict__ partner,
                                                     long long* __restrict__ stats, ClassMap km, int K, int n, int P,
                                                     Fractions fr) {
    __shared__ u64 acc[4 * 256];
    for (int i = threadIdx.x; i < 4 * K; i += 256) acc[i] = 0;
    __syncthreads();
    const size_t baseP = (size_t)blockIdx.y * P, baseG = ((size_t)n + blockIdx.y) * P;
    const u64 cap = 2ull * (u64)P;
    keys += (size_t)blockIdx.y * cap;
    counts += (size_t)blockIdx.y * cap;
    for (int k = 0; k < CHUNK / 256; ++k) {
        const u64 s = (u64)blockIdx.x * CHUNK + k * 256 + threadIdx.x;
        if (s >= cap) break;
        const u64 key = keys[s];
        if (key == EMPTY) continue;
        const int rP = (int)(key >> 32), rG = (int)(key & 0xFFFFFFFFull);
        const long long I = counts[s], U = (long long)a[baseP + rP] + area[baseG + rG] - I;
        if (I * fr.thr_den > fr.thr_num * U) {
            const int kk = km.k[pred[baseP + rP]];
            atomicAdd(&acc[4 * kk + 0], 1ull);
            atomicAdd(&acc[4 * kk + 1], ((u64)I << 32) / (u64)U);   // I < 2^31: the product fits
            atomicAdd(&acc[4 * kk + 2], (u64)I);
            atomicAdd(&acc[4 * kk + 3], (u64)U);
            partner[baseP + rP] = rG;   // at or above one half no other pair holds rP or rG
            partner[baseG + rG] = rP;
        }
    }
    flush_sums(acc, stats, K, TP, SUM_Q, SUM_I, SUM_U);
}

__global__ __launch_bounds__(256) void roots_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ gt,
                                                    const int* __restrict__ root, const int* __restrict__ a,
                                                    const int* __restrict__ area, const int* __restrict__ cov,
                                                    const int* __restrict__ partner, long long* __restrict__ stats,
                                                    int* __restrict__ pred_info, int* __restrict__ gt_info, ClassMap km, int K,
                                                    int n, int P, Fractions fr) {
    __shared__ u64 acc[4 * 256];
    for (int i = threadIdx.x; i < 4 * K; i += 256) acc[i] = 0;
    __syncthreads();
    const size_t img = (size_t)blockIdx.y * P, baseP = img, baseG = ((size_t)n + blockIdx.y) * P;
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long long pl = (long long)blockIdx.x * CHUNK + k * 256 + threadIdx.x;
        if (pl >= P) break;
        const int p = (int)pl;
        // a root of the void-masked ground truth is neither void nor background: gt itself has its class
        auto at_root = [&](size_t base, const unsigned char* m, const int* size, int count_at, int hit_at, int* info) {
            int mate = -2, covered = 0;
            const int kk = root[base + p] == p ? km.k[m[img + p]] : -1;
            const long long sz = kk >= 0 ? size[base + p] : 0;
            if (sz > 0) {
                mate = partner[base + p];
                covered = cov[base + p];
                atomicAdd(&acc[4 * kk + count_at], 1ull);
                if ((long long)covered * fr.cov_den >= fr.cov_num * sz) atomicAdd(&acc[4 * kk + hit_at], 1ull);
            }
            if (info) {
                info[2 * (img + p)] = mate;
                info[2 * (img + p) + 1] = covered;
            }
        };
        at_root(baseG, gt, area, 0, 2, gt_info);
        at_root(baseP, pred, a, 1, 3, pred_info);
    }
    flush_sums(acc, stats, K, N_GT, N_PRED, GT_FOUND, PRED_CONFIRMED);
}

bool shape_ok(int n, int H, int W) { return n > 0 && n <= 32767 && regions_shape_ok(2 * n, H, W); }

struct Layout {   // the labelling's scratch for 2n planes, the staged planes, the pair table
    size_t planes, keys, counts, total;
};

Layout layout(int n, int H, int W) {
    Layout l{};
    const size_t N = (size_t)n * H * W;
    l.planes = up256(regions_scratch_bytes(2 * n, H, W));
    l.keys = l.planes + up256(2 * N);
    l.counts = l.keys + up256(2 * N * sizeof(u64));
    l.total = l.counts + up256(2 * N * sizeof(int));
    return l;
}

}  // namespace

size_t region_match_scratch_bytes(int n, int H, int W) { return shape_ok(n, H, W) ? layout(n, H, W).total : 0; }

int launch_region_match(const unsigned char* pred, const unsigned char* gt, int n, int H, int W, const int* classes, int K,
                        int connectivity, int background, int ignore_label, int thr_num, int thr_den, int cov_num, int cov_den,
                        long long* stats, int* pred_info, int* gt_info, void* scratch, size_t scratch_bytes, hipStream_t s) {
    VITSEG_CHECK_ARG(pred && gt && classes && stats && scratch, VITSEG_EINVAL, "region_match: null pointer");
    VITSEG_CHECK_ARG(connectivity == 4 || connectivity == 8, VITSEG_EINVAL, "region_match: connectivity must be 4 or 8, got %d",
                     connectivity);
    VITSEG_CHECK_ARG(background >= 0 && background <= 255, VITSEG_EINVAL,
                     "region_match: background must be 0..255 (regions need a background), got %d", background);
    VITSEG_CHECK_ARG(ignore_label >= -1 && ignore_label <= 255 && ignore_label != background, VITSEG_EINVAL,
                     "region_match: ignore_label must be -1 or 0..255 and differ from the background %d, got %d", background,
                     ignore_label);
    VITSEG_CHECK_ARG(thr_den >= 1 && thr_den <= 1000 && thr_num < thr_den && 2 * thr_num >= thr_den, VITSEG_EINVAL,
                     "region_match: the IoU threshold %d / %d is outside den / 2 <= num < den <= 1000", thr_num, thr_den);
    VITSEG_CHECK_ARG(cov_num > 0 && cov_num <= cov_den && cov_den <= 1000, VITSEG_EINVAL,
                     "region_match: the coverage %d / %d is outside 0 < num <= den <= 1000", cov_num, cov_den);
    VITSEG_CHECK_ARG(shape_ok(n, H, W) && K >= 1 && K <= 256, VITSEG_ESHAPE,
                     "region_match: bad shape n=%d H=%d W=%d K=%d (positive sizes, H*W < 2^31, n <= 32767, K 1..256)", n, H, W, K);
    ClassMap km;
    for (int c = 0; c < 256; ++c) km.k[c] = -1;
    for (int k = 0; k < K; ++k) {
        const int c = classes[k];
        VITSEG_CHECK_ARG(c >= 0 && c <= 255 && c != background && c != ignore_label && km.k[c] < 0, VITSEG_EINVAL,
                         "region_match: classes[%d] = %d is outside 0..255, the background, the ignore label or repeated", k, c);
        km.k[c] = (short)k;
    }
    const Layout l = layout(n, H, W);
    VITSEG_CHECK_ARG(scratch_bytes >= l.total, VITSEG_EWORKSPACE, "region_match: scratch of %zu bytes, %zu needed", scratch_bytes,
                     l.total);
    const RegionWords w = region_words(scratch, 2 * n, H, W);
    unsigned char* planes = (unsigned char*)scratch + l.planes;
    u64* keys = (u64*)((char*)scratch + l.keys);
    int* counts = (int*)((char*)scratch + l.counts);
    const int P = H * W;
    const size_t N = (size_t)n * P;
    const Fractions fr{thr_num, thr_den, cov_num, cov_den};
    hipError_t e = hipMemsetAsync(stats, 0, (size_t)n * K * NSTATS * sizeof(long long), s);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(region_match stats)");
    hipLaunchKernelGGL(stage_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, pred, gt, planes, N, background,
                       ignore_label);
    VITSEG_LAUNCH_CHECK("region_match stage");
    if (const int rc = launch_region_labels(planes, 2 * n, H, W, connectivity, background, w, s)) return rc;
    // resolve was the last reader of the links and nothing here needs the boxes: the words at roots
    int *cov = w.link, *a = ignore_label >= 0 ? w.xmin : w.area, *partner = w.xmax;
    e = hipMemsetAsync(cov, 0, 2 * N * sizeof(int), s);
    if (e == hipSuccess && ignore_label >= 0) e = hipMemsetAsync(a, 0, N * sizeof(int), s);
    if (e == hipSuccess) e = hipMemsetAsync(partner, 0xFF, 2 * N * sizeof(int), s);   // -1
    if (e == hipSuccess) e = hipMemsetAsync(keys, 0xFF, 2 * N * sizeof(u64), s);      // EMPTY
    if (e == hipSuccess) e = hipMemsetAsync(counts, 0, 2 * N * sizeof(int), s);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(region_match words)");
    const dim3 chunks((unsigned)(((long long)P + CHUNK - 1) / CHUNK), n), slots((unsigned)((2ll * P + CHUNK - 1) / CHUNK), n);
    hipLaunchKernelGGL(pair_kernel, chunks, dim3(256), 0, s, pred, gt, w.root, a, cov, keys, counts, km, n, P, ignore_label);
    VITSEG_LAUNCH_CHECK("region_match pair");
    hipLaunchKernelGGL(decide_kernel, slots, dim3(256), 0, s, pred, keys, counts, a, w.area, partner, stats, km, K, n, P, fr);
    VITSEG_LAUNCH_CHECK("region_match decide");
    hipLaunchKernelGGL(roots_kernel, chunks, dim3(256), 0, s, pred, gt, w.root, a, w.area, cov, partner, stats, pred_info,
                       gt_info, km, K, n, P, fr);
    VITSEG_LAUNCH_CHECK("region_match roots");
    return VITSEG_OK;
}

}  // namespace vitseg

extern "C" {

size_t vitseg_region_match_scratch_bytes(int n, int H, int W) { return vitseg::region_match_scratch_bytes(n, H, W); }

int vitseg_region_match(const uint8_t* pred, const uint8_t* gt, int n, int H, int W, const int32_t* classes, int K,
                        int connectivity, int background, int ignore_label, int thr_num, int thr_den, int cov_num,
                        int cov_den, int64_t* stats, int32_t* pred_info, int32_t* gt_info, void* scratch,
                        size_t scratch_bytes, void* stream) {
    return vitseg::launch_region_match(pred, gt, n, H, W, classes, K, connectivity, background, ignore_label, thr_num, thr_den,
                                       cov_num, cov_den, (long long*)stats, pred_info, gt_info, scratch, scratch_bytes,
                                       (hipStream_t)stream);
}

}  // extern "C"
