// A class decided by threshold, with hysteresis (vitseg_decide, include/vitseg_decide.h): a pixel is kept when its 16-bit
// score q reaches low_q and it hangs together, through pixels that reach low_q, with one that reaches high_q.  The host answer
// writes the full-size logits, takes the sigmoid and runs skimage.filters.apply_hysteresis_threshold per image; here q is
// re-generated per pixel from the low-res head output (conf_score.hpp: vitseg_confidence's arithmetic under a mask that states
// one class everywhere, the plane vitseg_pr_counts bins) and the components come from the labelling launches of regions.hip.
//
//  1. score      grid (ceil(S S / CHUNK), n), confidence.hip's scheme: a workgroup takes CHUNK consecutive pixels of one image,
//                a thread V consecutive pixels at a time (V = 4 with 4-byte loads and stores when S % 4 == 0 and the planes are
//                aligned, V = 1 otherwise); STAGED copies the low-res rows the chunk interpolates between to LDS first.  The
//                weak and strong pixels are summed over the thread's pixels, the wave and the workgroup, then one 64-bit
//                atomic per workgroup and counter.  With low_q == high_q it writes the final mask (kept == strong) and is
//                the whole call.
//                Otherwise it writes two one-byte planes: level = weak + strong (0 / 1 / 2) and on = level > 0.
//  2. - 4.       launch_region_labels on `on`, background 0, the caller's connectivity: root[p] = the smallest raster index of
//                p's component of weak pixels, -1 where on == 0.  Nothing reads `on` after it.
//  5. (memset)   `on`'s bytes become the flag plane: all 0.
//  6. flag       every strong pixel stores 1 into the flag byte at its root: many equal stores of one value.  The launch reads
//                level and root, which it does not write, and writes flags, which it does not read.
//  7. select     kept = root >= 0 && flag[root]; writes the mask by the `base` rule and adds the kept count like launch 1.
// A root is its component's smallest raster index and a flag is 1 exactly when some strong pixel has that root, so nothing
// depends on the order in which workgroups run; data passes between workgroups only at kernel boundaries, as in regions.hip.
//
// scratch (vitseg_decide_scratch_bytes, hysteresis only), every part rounded up to 256 bytes:
//   [0, R)          R = regions_scratch_bytes(n, S, S): the labelling's words (region_words)
//   [R, R + N)      level, one byte per pixel (N = n S S)
//   [R + N', + N)   on, then flag, one byte per pixel
#include "conf_score.hpp"
#include "kernels.hpp"
#include "run_reduce.hpp"
#include "../../include/vitseg_decide.h"

namespace vitseg {
namespace {

constexpr int CHUNK = 4096;              // pixels per workgroup
constexpr int DECIDE_MAX_SIDE = 16384, DECIDE_MAX_BATCH = 65535;   // vitseg_pr_counts' limits
constexpr int STAGE_LIMIT = 48 * 1024;   // bytes of LDS for the staged low-res rows (the decoder tail's limit)

struct DecideArgs {
    const float* Z;
    const unsigned char* base;
    unsigned char* mask;
    unsigned char* level;
    unsigned char* on;
    i64* counts;
    int C, g, S, cls, kind, high_q, low_q, value, off;
};

template <int V> struct Vec;
template <> struct Vec<1> {
    typedef unsigned char u8;
    typedef int i32;
};
template <> struct Vec<4> {
    typedef uchar4 u8;
    typedef int4 i32;
};

// mask value of a pixel: `value` where kept, else off, or what base states unless that is `value`
__device__ __forceinline__ unsigned char decided(bool kept, bool has_base, int b, int value, int off) {
    return (unsigned char)(kept ? value : (has_base && b != value) ? b : off);
}

// the workgroup's sums of two counts below 2^16 each, packed as lo | hi << 16: over each wave first, then over the waves
// through LDS; returned on thread 0, which alone adds to the image's counters (64-bit integer atomics: any order gives the
// same bits; one atomic per workgroup and counter keeps thousands of waves off one cache line).  Every thread arrives here.
__device__ __forceinline__ int block_sum2(int packed, int* part /* LDS, one int per wave */) {
    packed = wave_sum(packed);
    if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = packed;
    __syncthreads();
    int t = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < 256 / WAVE; ++w) t += part[w];
    return t;
}

__device__ __forceinline__ void add_count(i64* counts, int which, int v) {
    if (v) atomicAdd((u64*)&counts[(size_t)blockIdx.y * 3 + which], (u64)v);
}

template <int V, bool STAGED, bool HYST>
__global__ __launch_bounds__(256) void decide_score_kernel(const DecideArgs a) {
    extern __shared__ __attribute__((aligned(16))) float zs[];   // STAGED: [class][source row - ymin][g]
    __shared__ int part[256 / WAVE];
    const int S = a.S, g = a.g, C = a.C, P = S * S;
    const int tid = threadIdx.x;
    const int pfirst = (int)blockIdx.x * CHUNK, plast = min(pfirst + CHUNK, P) - 1;
    const size_t img = (size_t)blockIdx.y * P;
    const float scale = (float)g / (float)S;
    int ymin = 0, nr = g;
    if (STAGED) {
        int ya, yb, yc, yd;
        float w0, w1;
        taps(pfirst / S, scale, g, ya, yb, w0, w1);
        taps(plast / S, scale, g, yc, yd, w0, w1);
        ymin = ya;
        nr = yd - ya + 1;   // <= the bound launch_decide sized zs for
        const int per = nr * g;
        for (int i = tid; i < C * per; i += 256) {
            const int c = i / per, rem = i - c * per;
            zs[i] = a.Z[(((size_t)blockIdx.y * C + c) * g + ymin) * g + rem];
        }
        __syncthreads();
    }
    const float* zb = STAGED ? zs : a.Z + (size_t)blockIdx.y * C * g * g;
    const size_t plane = (size_t)nr * g;
    int nweak = 0, nstrong = 0;   // over the thread's <= CHUNK / 256 pixels
    for (int k = 0; k < CHUNK / (256 * V); ++k) {
        const int p0 = pfirst + (k * 256 + tid) * V;   // a wave: 64 V consecutive pixels; P % V == 0
        if (p0 >= P) break;
        const int Y = p0 / S, X = p0 - Y * S;
        int y0, y1, x0[V], x1[V], cls[V], q[V];
        float wy0, wy1, wx0[V], wx1[V], p[V];
        taps(Y, scale, g, y0, y1, wy0, wy1);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            cls[e] = a.cls;
            taps(X + e, scale, g, x0[e], x1[e], wx0[e], wx1[e]);
        }
        score_pixels<V>(zb, plane, C, a.kind, (y0 - ymin) * g, (y1 - ymin) * g, wy0, wy1, x0, x1, wx0, wx1, cls, p, q);
        typename Vec<V>::u8 o, o2, b4{};
        unsigned char* ob = (unsigned char*)&o;
        unsigned char* ob2 = (unsigned char*)&o2;
        if (!HYST && a.base) b4 = *(const typename Vec<V>::u8*)(a.base + img + p0);
        const unsigned char* bb = (const unsigned char*)&b4;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const int weak = q[e] >= a.low_q, strong = q[e] >= a.high_q;
            nweak += weak;
            nstrong += strong;
            if (HYST) {
                ob[e] = (unsigned char)(weak + strong);
                ob2[e] = (unsigned char)weak;
            } else {
                ob[e] = decided(strong, a.base != nullptr, bb[e], a.value, a.off);
            }
        }
        if (HYST) {
            *(typename Vec<V>::u8*)(a.level + img + p0) = o;
            *(typename Vec<V>::u8*)(a.on + img + p0) = o2;
        } else {
            *(typename Vec<V>::u8*)(a.mask + img + p0) = o;
        }
    }
    if (a.counts) {   // (uniform over the grid; the loop's break brings every thread here; a workgroup holds 4096 pixels)
        const int t = block_sum2(nweak | nstrong << 16, part);
        if (tid == 0) {
            add_count(a.counts, 0, t & 0xffff);
            add_count(a.counts, 1, t >> 16);
            if (!HYST) add_count(a.counts, 2, t >> 16);
        }
    }
}

// one thread per V consecutive pixels: the flag byte at the root of every strong pixel becomes 1
template <int V>
__global__ __launch_bounds__(256) void decide_flag_kernel(const unsigned char* __restrict__ level, const int* __restrict__ root,
                                                          unsigned char* __restrict__ flag, int P) {
    const long long pl = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (pl >= P) return;
    const size_t at = (size_t)blockIdx.y * P + (size_t)pl;
    const typename Vec<V>::u8 l4 = *(const typename Vec<V>::u8*)(level + at);
    const unsigned char* lb = (const unsigned char*)&l4;
    int last = -1;   // the root the thread marked last: a run of strong pixels shares one
#pragma unroll
    for (int e = 0; e < V; ++e)
        if (lb[e] == 2) {
            const int r = root[at + e];   // >= 0: a strong pixel is weak, so it is in a component
            if (r != last && r >= 0) flag[(size_t)blockIdx.y * P + r] = 1;
            last = r;
        }
}

template <int V>
__global__ __launch_bounds__(256) void decide_select_kernel(const int* __restrict__ root, const unsigned char* __restrict__ flag,
                                                            const unsigned char* __restrict__ base, unsigned char* __restrict__ mask,
                                                            i64* __restrict__ counts, int P, int value, int off) {
    __shared__ int part[256 / WAVE];
    const size_t img = (size_t)blockIdx.y * P;
    int nkept = 0;
    for (int k = 0; k < CHUNK / (256 * V); ++k) {
        const long long pl = (long long)blockIdx.x * CHUNK + (long long)(k * 256 + threadIdx.x) * V;
        if (pl >= P) break;
        const size_t at = img + (size_t)pl;
        const typename Vec<V>::i32 r4 = *(const typename Vec<V>::i32*)(root + at);
        const int* rb = (const int*)&r4;
        typename Vec<V>::u8 o, b4{};
        unsigned char* ob = (unsigned char*)&o;
        if (base) b4 = *(const typename Vec<V>::u8*)(base + at);
        const unsigned char* bb = (const unsigned char*)&b4;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const bool kept = rb[e] >= 0 && flag[img + rb[e]] != 0;
            nkept += kept;
            ob[e] = decided(kept, base != nullptr, bb[e], value, off);
        }
        *(typename Vec<V>::u8*)(mask + at) = o;
    }
    if (counts) {
        const int t = block_sum2(nkept, part);
        if (threadIdx.x == 0) add_count(counts, 2, t);
    }
}

bool aligned(const void* p, size_t to) { return ((uintptr_t)p & (to - 1)) == 0; }

bool shape_ok(int n, int S) { return n >= 1 && n <= DECIDE_MAX_BATCH && S >= 1 && S <= DECIDE_MAX_SIDE; }

size_t decide_scratch_bytes(int n, int S, int hysteresis) {
    if (!hysteresis || !shape_ok(n, S)) return 0;
    return up256(regions_scratch_bytes(n, S, S)) + 2 * up256((size_t)n * S * S);
}

template <int V, bool HYST>
void launch_score(const DecideArgs& a, dim3 grid, bool staged, size_t smem, hipStream_t s) {
    if (staged)
        hipLaunchKernelGGL((decide_score_kernel<V, true, HYST>), grid, dim3(256), smem, s, a);
    else
        hipLaunchKernelGGL((decide_score_kernel<V, false, HYST>), grid, dim3(256), 0, s, a);
}

int launch_decide(const float* lowres, int n, int C, int g, int S, int cls, int kind, int high_q, int low_q, int connectivity,
                  const unsigned char* base, int value, int off, unsigned char* mask, long long* counts, void* scratch,
                  size_t scratch_bytes, hipStream_t s) {
    VITSEG_CHECK_ARG(lowres && mask, VITSEG_EINVAL, "decide: null lowres or mask");
    VITSEG_CHECK_ARG(mask != base, VITSEG_EINVAL, "decide: mask must not be base");
    VITSEG_CHECK_ARG(kind == VITSEG_CONF_PROB || kind == VITSEG_CONF_MARGIN, VITSEG_EINVAL,
                     "decide: kind must be 0 (prob) or 1 (margin), got %d", kind);
    VITSEG_CHECK_ARG(low_q >= 0 && low_q <= high_q && high_q <= 65536, VITSEG_EINVAL,
                     "decide: thresholds must be 0 <= low_q <= high_q <= 65536, got low_q=%d high_q=%d", low_q, high_q);
    VITSEG_CHECK_ARG(connectivity == 4 || connectivity == 8, VITSEG_EINVAL, "decide: connectivity must be 4 or 8, got %d",
                     connectivity);
    VITSEG_CHECK_ARG(value >= 0 && value <= 255 && off >= 0 && off <= 255 && value != off, VITSEG_EINVAL,
                     "decide: value and off must be different label values in 0..255, got %d and %d", value, off);
    VITSEG_CHECK_ARG(C >= 1 && C <= 255 && shape_ok(n, S) && g >= 1 && g <= S, VITSEG_ESHAPE,
                     "decide: bad shape n=%d C=%d g=%d S=%d (1 <= C <= 255, 1 <= n <= %d, 1 <= g <= S <= %d)", n, C, g, S,
                     DECIDE_MAX_BATCH, DECIDE_MAX_SIDE);
    VITSEG_CHECK_ARG(kind != VITSEG_CONF_MARGIN || C >= 2, VITSEG_EINVAL, "decide: margin needs C >= 2, got %d", C);
    VITSEG_CHECK_ARG(cls >= 0 && cls < C, VITSEG_EINVAL, "decide: cls must be 0..%d, got %d", C - 1, cls);
    const bool hyst = low_q != high_q;
    const size_t need = decide_scratch_bytes(n, S, hyst);
    VITSEG_CHECK_ARG(scratch || need == 0, VITSEG_EINVAL, "decide: null scratch");
    VITSEG_CHECK_ARG(scratch_bytes >= need, VITSEG_EWORKSPACE, "decide: scratch of %zu bytes, %zu needed", scratch_bytes, need);
    if (counts) {
        const hipError_t e = hipMemsetAsync(counts, 0, (size_t)n * 3 * sizeof(long long), s);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(decide counts)");
    }
    const int P = S * S;
    const size_t N = (size_t)n * P;
    unsigned char* level = nullptr;
    unsigned char* on = nullptr;
    if (hyst) {
        level = (unsigned char*)scratch + up256(regions_scratch_bytes(n, S, S));
        on = level + up256(N);
    }
    const DecideArgs a{lowres, base, mask, level, on, counts, C, g, S, cls, kind, high_q, low_q, value, off};
    const dim3 chunks((unsigned)(((long long)P + CHUNK - 1) / CHUNK), n);
    // a chunk touches at most (CHUNK - 1) / S + 2 output rows; their taps span at most scale * (rows - 1) source rows, + 1
    // for the floor at either end, + 1 for the lower tap of the last, + 1 for the fp32 rounding of the taps
    const int rows_out = min(S, (CHUNK - 1) / S + 2);
    const int nr_max = min(g, (int)((double)(rows_out - 1) * g / S) + 4);
    const size_t smem = (size_t)C * nr_max * g * sizeof(float);
    const bool staged = smem <= (size_t)STAGE_LIMIT && !opt(OPT_UPSAMPLE_GLOBAL);
    // (the planes in scratch start at multiples of 256 bytes from its start, an image at a multiple of P)
    const bool vec = S % 4 == 0 && aligned(mask, 4) && (!base || aligned(base, 4)) && (!hyst || aligned(scratch, 16));
    if (!hyst) {
        if (vec)
            launch_score<4, false>(a, chunks, staged, smem, s);
        else
            launch_score<1, false>(a, chunks, staged, smem, s);
        VITSEG_LAUNCH_CHECK("decide score");
        return VITSEG_OK;
    }
    if (vec)
        launch_score<4, true>(a, chunks, staged, smem, s);
    else
        launch_score<1, true>(a, chunks, staged, smem, s);
    VITSEG_LAUNCH_CHECK("decide score");
    const RegionWords w = region_words(scratch, n, S, S);
    if (const int rc = launch_region_labels(on, n, S, S, connectivity, 0, w, s)) return rc;
    const hipError_t e = hipMemsetAsync(on, 0, N, s);   // resolve was the last reader of `on`: the flag plane from here
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(decide flags)");
    if (vec) {
        hipLaunchKernelGGL(decide_flag_kernel<4>, dim3((unsigned)((P / 4 + 255) / 256), n), dim3(256), 0, s, level, w.root, on, P);
        VITSEG_LAUNCH_CHECK("decide flag");
        hipLaunchKernelGGL(decide_select_kernel<4>, chunks, dim3(256), 0, s, w.root, on, base, mask, counts, P, value, off);
    } else {
        hipLaunchKernelGGL(decide_flag_kernel<1>, dim3((unsigned)(((long long)P + 255) / 256), n), dim3(256), 0, s, level, w.root,
                           on, P);
        VITSEG_LAUNCH_CHECK("decide flag");
        hipLaunchKernelGGL(decide_select_kernel<1>, chunks, dim3(256), 0, s, w.root, on, base, mask, counts, P, value, off);
    }
    VITSEG_LAUNCH_CHECK("decide select");
    return VITSEG_OK;
}

}  // namespace
}  // namespace vitseg

extern "C" {

int vitseg_decide_version(void) { return VITSEG_DECIDE_VERSION; }

size_t vitseg_decide_scratch_bytes(int n, int S, int hysteresis) { return vitseg::decide_scratch_bytes(n, S, hysteresis); }

int vitseg_decide(const float* lowres, int n, int C, int g, int S, int cls, int kind, int high_q, int low_q, int connectivity,
                  const uint8_t* base, int value, int off, uint8_t* mask, int64_t* counts, void* scratch, size_t scratch_bytes,
                  void* stream) {
    return vitseg::launch_decide(lowres, n, C, g, S, cls, kind, high_q, low_q, connectivity, base, value, off, mask,
                                 (long long*)counts, scratch, scratch_bytes, (hipStream_t)stream);
}

}  // extern "C"
