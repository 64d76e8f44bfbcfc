// Mask clean-up: regions below a minimum area become background, enclosed holes are filled (vitseg_clean_mask).  The
// reference has no counterpart (its get_bounding_boxes labels the raw argmax, model/CE/testViTModel.py:34-42); the usual host
// answer is remove_small_objects + scipy.ndimage.binary_fill_holes per class and image.
//
// Step 1 (min_area > 1): the labelling launches of regions.hip on `mask` leave every pixel's root and every root's area;
//   drop_small     out[p] = area[root[p]] < min_area ? background : mask[p]; regions (at p == root[p]) and pixels removed,
//                  summed over each block and added to the image's counters by one integer atomicAdd per block.
// Without step 1, out is a copy of mask.
// Step 2 (fill_holes): the same labelling on `out` with no background and connectivity 4, so that every pixel has a root, the
// background components included; a component's box is at its root and its first row is root / W, so "touches the frame"
// is four comparisons.  Two words per root, both -1 before:
//   hole_ring      a background pixel of a hole raises the words at its root to 255 - c and to c for the class c of each of
//                  its non-background 4-neighbours (integer atomicMax; a wave first folds its lanes of equal root): after the
//                  launch they hold 255 - (smallest bordering class) and the largest.
//   fill           in place on out: a background pixel whose root is a hole within the area limit with one bordering class
//                  takes it; the hole counts are taken at roots.  It reads its own pixel and words at its root alone.
// The first word lives in the labelling's link array, which nothing reads after resolve.  Data passes between workgroups only
// at kernel boundaries, as in regions.hip: the words at roots are written by atomics in one launch and read in the next.
// Everything is an integer from order-independent operations: bitwise reproducible, and an image's result does not depend on
// the batch it is in.
#include "kernels.hpp"

namespace vitseg {
namespace {

constexpr int CHUNK = 4096;   // pixels per block of the two passes that count

enum { REGIONS_REMOVED, PIXELS_REMOVED, HOLES_FILLED, PIXELS_FILLED, HOLES_MIXED, HOLES_OVER_AREA, NSTATS = 8 };

// the block's sum of v goes to one counter of its image by a single integer atomicAdd (integer sums: any order gives the
// same bits; one atomic per block and counter keeps thousands of waves off the same few words)
__device__ __forceinline__ void add_stat(int* stats, int which, int v, int* part /* LDS, one int per wave */) {
    v = wave_sum(v);
    if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = v;
    __syncthreads();
    if (threadIdx.x == 0 && stats) {
        int t = 0;
        for (int w = 0; w < 256 / WAVE; ++w) t += part[w];
        if (t) atomicAdd(&stats[(size_t)blockIdx.y * NSTATS + which], t);
    }
    __syncthreads();
}

// one block per 4096-pixel chunk, a wave on 64 consecutive pixels at a time
__global__ __launch_bounds__(256) void drop_small_kernel(const unsigned char* __restrict__ mask, unsigned char* __restrict__ out,
                                                         const int* __restrict__ root, const int* __restrict__ area,
                                                         int* __restrict__ stats, int P, int background, int min_area) {
    __shared__ int part[256 / WAVE];
    const size_t base = (size_t)blockIdx.y * P;
    int gone = 0, gone_roots = 0;
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long long pl = (long long)blockIdx.x * CHUNK + k * 256 + threadIdx.x;
        if (pl >= P) break;
        const int p = (int)pl, r = root[base + p];
        const bool g = r >= 0 && area[base + r] < min_area;
        gone += g;
        gone_roots += g && r == p;
        out[base + p] = g ? (unsigned char)background : mask[base + p];
    }
    add_stat(stats, REGIONS_REMOVED, gone_roots, part);
    add_stat(stats, PIXELS_REMOVED, gone, part);
}

struct Holes {   // the labelling of `out` without a background: per-pixel root, words at roots
    const int* root;
    const int* xmin;
    const int* xmax;
    const int* ymax;
    const int* area;
    int* lo;   // 255 - the smallest bordering class, -1 = none yet
    int* hi;   // the largest bordering class, -1 = none yet
};

// a component that does not touch the image frame; r = its root = its first raster pixel, so r / W is its first row
__device__ __forceinline__ bool off_frame(const Holes& h, size_t base, int r, int H, int W) {
    return r >= W && h.xmin[base + r] > 0 && h.xmax[base + r] < W - 1 && h.ymax[base + r] < H - 1;
}

__global__ __launch_bounds__(256) void hole_ring_kernel(const unsigned char* __restrict__ out, Holes h, int H, int W,
                                                        int background) {
    const int P = H * W, lane = threadIdx.x & (WAVE - 1);
    const long long pl = (long long)blockIdx.x * 256 + threadIdx.x;   // a wave: 64 consecutive pixels
    const size_t base = (size_t)blockIdx.y * P;
    int r = -1, lo = -1, hi = -1;   // r = -1: not a background pixel
    if (pl < P) {
        const int p = (int)pl;
        const unsigned char* m = out + base;
        if (m[p] == background) {
            r = h.root[base + p];
            const int y = p / W, x = p - y * W;
            auto look = [&](bool inside, int q) {
                if (!inside) return;
                const int c = m[q];
                if (c == background) return;
                lo = max(lo, 255 - c);
                hi = max(hi, c);
            };
            look(x > 0, p - 1);
            look(x < W - 1, p + 1);
            look(y > 0, p - W);
            look(y < H - 1, p + W);
        }
    }
    // fold the lanes of equal root: lane i takes lane i + d's values when the roots agree.  Over a run of consecutive lanes
    // with one root the run's first lane ends with the whole run (max is idempotent, so what else joins in from another
    // run of the same root changes nothing); it alone goes to memory
    for (int d = 1; d < WAVE; d <<= 1) {
        const int r2 = __shfl_down(r, d), lo2 = __shfl_down(lo, d), hi2 = __shfl_down(hi, d);
        if (lane + d < WAVE && r2 == r) {
            lo = max(lo, lo2);
            hi = max(hi, hi2);
        }
    }
    const int r_prev = __shfl_up(r, 1);
    if (r >= 0 && hi >= 0 && (lane == 0 || r_prev != r) && off_frame(h, base, r, H, W)) {
        atomicMax(&h.lo[base + r], lo);
        atomicMax(&h.hi[base + r], hi);
    }
}

__global__ __launch_bounds__(256) void fill_kernel(unsigned char* out, Holes h, int* __restrict__ stats, int H, int W,
                                                   int background, int max_hole_area) {
    __shared__ int part[256 / WAVE];
    const int P = H * W;
    const size_t base = (size_t)blockIdx.y * P;
    int filled = 0, filled_px = 0, mixed = 0, over = 0;
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long long pl = (long long)blockIdx.x * CHUNK + k * 256 + threadIdx.x;
        if (pl >= P) break;
        const int p = (int)pl;
        if (out[base + p] != background) continue;
        const int r = h.root[base + p];
        if (!off_frame(h, base, r, H, W)) continue;
        const int a = h.area[base + r], cmin = 255 - h.lo[base + r], cmax = h.hi[base + r];
        const bool too_big = max_hole_area > 0 && a > max_hole_area;
        const bool one = !too_big && cmin == cmax;   // a hole has a bordering pixel, so both words were raised
        if (one) out[base + p] = (unsigned char)cmin;
        if (r == p) {   // the hole counts are taken at roots
            over += too_big;
            mixed += !too_big && !one;
            filled += one;
            filled_px += one ? a : 0;
        }
    }
    add_stat(stats, HOLES_FILLED, filled, part);
    add_stat(stats, PIXELS_FILLED, filled_px, part);
    add_stat(stats, HOLES_MIXED, mixed, part);
    add_stat(stats, HOLES_OVER_AREA, over, part);
}

}  // namespace

// the labelling's scratch, then one more int32 per pixel (the `hi` words)
size_t clean_scratch_bytes(int n, int H, int W) {
    if (!regions_shape_ok(n, H, W)) return 0;
    return up256(regions_scratch_bytes(n, H, W)) + up256((size_t)n * H * W * sizeof(int));
}

int launch_clean_mask(const unsigned char* mask, unsigned char* out, int n, int H, int W, int connectivity, int background,
                      int min_area, int fill_holes, int max_hole_area, int* stats, void* scratch, size_t scratch_bytes,
                      hipStream_t s) {
    VITSEG_CHECK_ARG(mask && out && scratch, VITSEG_EINVAL, "clean_mask: null pointer");
    VITSEG_CHECK_ARG(out != mask, VITSEG_EINVAL, "clean_mask: out must not be mask (the mask is read after out is written)");
    VITSEG_CHECK_ARG(connectivity == 4 || connectivity == 8, VITSEG_EINVAL, "clean_mask: connectivity must be 4 or 8, got %d",
                     connectivity);
    VITSEG_CHECK_ARG(background >= 0 && background <= 255, VITSEG_EINVAL,
                     "clean_mask: background must be 0..255 (clean-up needs a background), got %d", background);
    VITSEG_CHECK_ARG(min_area >= 0 && max_hole_area >= 0, VITSEG_EINVAL,
                     "clean_mask: min_area and max_hole_area must not be negative, got %d and %d", min_area, max_hole_area);
    VITSEG_CHECK_ARG(regions_shape_ok(n, H, W), VITSEG_ESHAPE,
                     "clean_mask: bad shape n=%d H=%d W=%d (positive sizes, H*W < 2^31, n <= 65535)", n, H, W);
    const size_t need = clean_scratch_bytes(n, H, W);
    VITSEG_CHECK_ARG(scratch_bytes >= need, VITSEG_EWORKSPACE, "clean_mask: scratch of %zu bytes, %zu needed", scratch_bytes, need);
    const RegionWords w = region_words(scratch, n, H, W);
    int* hi = (int*)((char*)scratch + up256(regions_scratch_bytes(n, H, W)));
    const int P = H * W;
    const size_t N = (size_t)n * P;
    const dim3 grid((unsigned)(((long long)P + 255) / 256), n), chunks((unsigned)(((long long)P + CHUNK - 1) / CHUNK), n);
    hipError_t e;
    if (stats) {
        e = hipMemsetAsync(stats, 0, (size_t)n * NSTATS * sizeof(int), s);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(clean stats)");
    }
    if (min_area > 1) {
        if (const int rc = launch_region_labels(mask, n, H, W, connectivity, background, w, s)) return rc;
        hipLaunchKernelGGL(drop_small_kernel, chunks, dim3(256), 0, s, mask, out, w.root, w.area, stats, P, background, min_area);
        VITSEG_LAUNCH_CHECK("clean drop_small");
    } else {
        e = hipMemcpyAsync(out, mask, N, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(clean out)");
    }
    if (fill_holes) {
        if (const int rc = launch_region_labels(out, n, H, W, 4, -1, w, s)) return rc;
        e = hipMemsetAsync(w.link, 0xFF, N * sizeof(int), s);   // -1; resolve was the last reader of the links
        if (e == hipSuccess) e = hipMemsetAsync(hi, 0xFF, N * sizeof(int), s);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(clean ring words)");
        const Holes h{w.root, w.xmin, w.xmax, w.ymax, w.area, w.link, hi};
        hipLaunchKernelGGL(hole_ring_kernel, grid, dim3(256), 0, s, out, h, H, W, background);
        VITSEG_LAUNCH_CHECK("clean hole_ring");
        hipLaunchKernelGGL(fill_kernel, chunks, dim3(256), 0, s, out, h, stats, H, W, background, max_hole_area);
        VITSEG_LAUNCH_CHECK("clean fill");
    }
    return VITSEG_OK;
}

}  // namespace vitseg

extern "C" {

size_t vitseg_clean_scratch_bytes(int n, int H, int W) { return vitseg::clean_scratch_bytes(n, H, W); }

int vitseg_clean_mask(const uint8_t* mask, uint8_t* out, int n, int H, int W, int connectivity, int background, int min_area,
                      int fill_holes, int max_hole_area, int32_t* stats, void* scratch, size_t scratch_bytes, void* stream) {
    return vitseg::launch_clean_mask(mask, out, n, H, W, connectivity, background, min_area, fill_holes, max_hole_area, stats,
                                     scratch, scratch_bytes, (hipStream_t)stream);
}

}  // extern "C"
