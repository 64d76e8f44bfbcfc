// Confidence of a stated class mask (vitseg_confidence): the per-pixel score p = sigmoid(v_c) of the class c the mask states
// (or its lead over the best other class), its 16-bit form q, per-region score rows keyed by vitseg_regions' labels and a
// per-image calibration histogram against a ground truth.  The host answer writes the full-size fp32 logits (C S S 4 bytes
// per image), then runs sigmoid, gather, the rounding and index_add_ / bincount over them; here v_k is re-generated per pixel
// from the low-resolution head output [n, C, g, g] with the decoder tail's exact arithmetic (tail_math.hpp: taps,
// sigmoid_aten), as the cross-entropy kernel and the window / TTA blends do, so the mandatory traffic is the mask (1 B), the
// labels (4 B), the ground truth (1 B) and the maps asked for (4 + 2 B) per pixel.
//
// One kernel, grid (ceil(S S / CHUNK), n): a workgroup takes CHUNK consecutive pixels of one image, a thread V consecutive
// pixels at a time (V = 4 with 4-, 8- and 16-byte loads and stores when S % 4 == 0 and the planes are aligned: a quad never
// leaves its row; V = 1 otherwise).
//   STAGED   the few low-res rows the chunk's output rows interpolate between are copied to LDS for all classes first
//            (upsample_kernel<STAGED>'s scheme); when C * rows * g floats do not fit (g == S at a large S, C near 255) the
//            kernel reads them from global memory instead.
//   sigmoid  one exact sigmoid per pixel for prob, two for margin (conf_score.hpp, shared with curves.hip).
//   rows     the pre-reduction of props.hip: a lane whose V pixels share a label joins the run of equal labels around it
//            (run_reduce.hpp), the run's head adds once; the runs of up to NK regions per workgroup -- those found at NK
//            pixels spread over the chunk -- add into LDS and reach their rows as one atomic per field, region and workgroup
//            (a chunk of a real mask holds a few large regions side by side: with one slot the others' runs all go to their
//            rows, a few hot rows).  A lane whose pixels differ (a region boundary) adds pixel by pixel.
//   hist     the same runs keyed by bin add into a 32-bit LDS table (a chunk's sum_q stays below 2^32), flushed with one
//            64-bit atomic per non-empty word.
// All global accumulators are 64-bit integer atomicAdd / atomicMax: order-independent bits.
#include "conf_score.hpp"
#include "kernels.hpp"
#include "run_reduce.hpp"

namespace vitseg {
namespace {

constexpr int CHUNK = 4096;            // pixels per workgroup
constexpr int NK = 8;                  // regions whose runs a workgroup collects in LDS
constexpr int CONF_MAX_SIDE = 16384, CONF_MAX_BATCH = 65535, CONF_MAX_BINS = 256;
constexpr int STAGE_LIMIT = 48 * 1024;   // bytes of LDS for the staged low-res rows (the decoder tail's limit)

struct ConfArgs {
    const float* Z;
    const unsigned char* mask;
    float* conf;
    unsigned short* conf_q;
    const int* labels;
    i64* scores;
    const unsigned char* gt;
    i64* hist;
    int C, g, S, kind, max_regions, low_q, ignore_label, bins;
};

template <int V> struct Vec;
template <> struct Vec<1> {
    typedef unsigned char u8;
    typedef int i32;
    typedef float f32;
    typedef unsigned short u16;
};
template <> struct Vec<4> {
    typedef uchar4 u8;
    typedef int4 i32;
    typedef float4 f32;
    typedef ushort4 u16;
};

template <int V, bool STAGED>
__global__ __launch_bounds__(256) void confidence_kernel(const ConfArgs a) {
    extern __shared__ __attribute__((aligned(16))) float zs[];   // STAGED: [class][source row - ymin][g]
    __shared__ unsigned hist_s[CONF_MAX_BINS * 3];
    __shared__ u64 acc[NK][4];   // pixels, sum_q, max_deficit, n_low of the workgroup's regions
    __shared__ int keys[NK];
    const int S = a.S, g = a.g, C = a.C, P = S * S;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int pfirst = (int)blockIdx.x * CHUNK, plast = min(pfirst + CHUNK, P) - 1;
    const size_t img = (size_t)blockIdx.y * P;
    const float scale = (float)g / (float)S;
    const int* lab = a.labels + img;   // (formed, not read, when there are no labels)
    if (a.hist)
        for (int i = tid; i < a.bins * 3; i += 256) hist_s[i] = 0;
    if (tid < NK * 4) acc[tid >> 2][tid & 3] = 0;
    if (tid < NK) {   // the regions found at NK pixels spread over the chunk's rows and columns (the first one at its first pixel)
        int k = -1;
        if (a.scores) k = lab[min(pfirst + tid * (CHUNK / NK) + (tid * 73) % (CHUNK / NK), plast)];
        keys[tid] = (k >= 0 && k < a.max_regions) ? k : -1;
    }
    int ymin = 0, nr = g;
    if (STAGED) {
        int ya, yb, yc, yd;
        float w0, w1;
        taps(pfirst / S, scale, g, ya, yb, w0, w1);
        taps(plast / S, scale, g, yc, yd, w0, w1);
        ymin = ya;
        nr = yd - ya + 1;   // <= the bound launch_confidence sized zs for
        const int per = nr * g;
        for (int i = tid; i < C * per; i += 256) {
            const int c = i / per, rem = i - c * per;
            zs[i] = a.Z[(((size_t)blockIdx.y * C + c) * g + ymin) * g + rem];
        }
    }
    __syncthreads();
    int key[NK];
#pragma unroll
    for (int s = 0; s < NK; ++s) key[s] = keys[s];
    const float* zb = STAGED ? zs : a.Z + (size_t)blockIdx.y * C * g * g;
    const size_t plane = (size_t)nr * g;
    i64* rows = a.scores + (size_t)blockIdx.y * a.max_regions * 4;
    auto iadd = [](int x, int y) { return x + y; };
    auto imax = [](int x, int y) { return x > y ? x : y; };
    auto row_of = [&](int idx) {   // where a region's sums go: its LDS slot (the first that holds it) or its row
        u64* dst = (u64*)(rows + (size_t)idx * 4);
#pragma unroll
        for (int s = NK - 1; s >= 0; --s)
            if (key[s] == idx) dst = acc[s];
        return dst;
    };

    for (int k = 0; k < CHUNK / (256 * V); ++k) {
        const int p0 = pfirst + (k * 256 + tid) * V;   // a wave: 64 V consecutive pixels; P % V == 0
        const bool in = p0 < P;
        int q[V];
        int cls[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            q[e] = 0;
            cls[e] = 255;
        }
        if (in) {
            const typename Vec<V>::u8 m4 = *(const typename Vec<V>::u8*)(a.mask + img + p0);
            const unsigned char* mb = (const unsigned char*)&m4;
            const int Y = p0 / S, X = p0 - Y * S;
            int y0, y1, x0[V], x1[V];
            float wy0, wy1, wx0[V], wx1[V];
            taps(Y, scale, g, y0, y1, wy0, wy1);
            const int rt = (y0 - ymin) * g, rb = (y1 - ymin) * g;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                cls[e] = mb[e];
                taps(X + e, scale, g, x0[e], x1[e], wx0[e], wx1[e]);
            }
            float p[V];
            score_pixels<V>(zb, plane, C, a.kind, rt, rb, wy0, wy1, x0, x1, wx0, wx1, cls, p, q);
            if (a.conf) {
                typename Vec<V>::f32 o;
                float* ob = (float*)&o;
#pragma unroll
                for (int e = 0; e < V; ++e) ob[e] = p[e];
                *(typename Vec<V>::f32*)(a.conf + img + p0) = o;
            }
            if (a.conf_q) {
                typename Vec<V>::u16 o;
                unsigned short* ob = (unsigned short*)&o;
#pragma unroll
                for (int e = 0; e < V; ++e) ob[e] = (unsigned short)q[e];
                *(typename Vec<V>::u16*)(a.conf_q + img + p0) = o;
            }
        }
        if (a.scores) {   // (uniform over the grid; whole waves reach the shuffles)
            int idx[V];
#pragma unroll
            for (int e = 0; e < V; ++e) idx[e] = -1;
            if (in) {
                const typename Vec<V>::i32 l4 = *(const typename Vec<V>::i32*)(lab + p0);
                const int* lb = (const int*)&l4;
#pragma unroll
                for (int e = 0; e < V; ++e) idx[e] = (lb[e] >= 0 && lb[e] < a.max_regions) ? lb[e] : -1;
            }
            bool same = true;
            int sq = 0, md = 0, nl = 0;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                same = same && idx[e] == idx[0];
                sq += q[e];
                md = max(md, 65535 - q[e]);
                nl += q[e] < a.low_q;
            }
            const int lkey = same ? idx[0] : -1;
            const Run r = find_run(lkey, 0, lane);
            const int cnt = run_reduce(V | (nl << 16), lane, r.end, iadd);   // a wave holds 64 V <= 256 pixels: no carry
            const int rsq = run_reduce(sq, lane, r.end, iadd);                // <= 256 * 65535
            const int rmd = run_reduce(md, lane, r.end, imax);
            if (r.head) {
                u64* dst = row_of(lkey);
                atomicAdd(&dst[0], (u64)(cnt & 0xffff));
                if (rsq) atomicAdd(&dst[1], (u64)rsq);
                if (rmd) atomicMax(&dst[2], (u64)rmd);
                if (cnt >> 16) atomicAdd(&dst[3], (u64)(cnt >> 16));
            }
            if (!same) {   // a region boundary inside the lane's pixels
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (idx[e] >= 0) {
                        u64* dst = row_of(idx[e]);
                        atomicAdd(&dst[0], 1ull);
                        if (q[e]) atomicAdd(&dst[1], (u64)q[e]);
                        if (q[e] != 65535) atomicMax(&dst[2], (u64)(65535 - q[e]));
                        if (q[e] < a.low_q) atomicAdd(&dst[3], 1ull);
                    }
            }
        }
        if (a.hist) {   // (uniform over the grid)
            int bin[V], hit[V];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                bin[e] = -1;
                hit[e] = 0;
            }
            if (in) {
                const typename Vec<V>::u8 g4 = *(const typename Vec<V>::u8*)(a.gt + img + p0);
                const unsigned char* gb = (const unsigned char*)&g4;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    if ((int)gb[e] != a.ignore_label) bin[e] = (q[e] * a.bins) >> 16;
                    hit[e] = cls[e] == (int)gb[e];
                }
            }
            bool same = true;
            int sq = 0, nh = 0;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                same = same && bin[e] == bin[0];
                sq += q[e];
                nh += hit[e];
            }
            const int lkey = same ? bin[0] : -1;
            const Run r = find_run(lkey, 0, lane);
            const int cnt = run_reduce(V | (nh << 16), lane, r.end, iadd);
            const int rsq = run_reduce(sq, lane, r.end, iadd);
            if (r.head) {
                unsigned* dst = hist_s + lkey * 3;
                atomicAdd(&dst[0], (unsigned)(cnt & 0xffff));
                if (cnt >> 16) atomicAdd(&dst[1], (unsigned)(cnt >> 16));
                if (rsq) atomicAdd(&dst[2], (unsigned)rsq);
            }
            if (!same) {
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (bin[e] >= 0) {
                        unsigned* dst = hist_s + bin[e] * 3;
                        atomicAdd(&dst[0], 1u);
                        if (hit[e]) atomicAdd(&dst[1], 1u);
                        if (q[e]) atomicAdd(&dst[2], (unsigned)q[e]);
                    }
            }
        }
    }
    __syncthreads();
    if (tid < NK * 4 && keys[tid >> 2] >= 0 && acc[tid >> 2][tid & 3]) {   // (a slot that repeats an earlier key stayed 0)
        u64* dst = (u64*)(rows + (size_t)keys[tid >> 2] * 4) + (tid & 3);
        if ((tid & 3) == 2)
            atomicMax(dst, acc[tid >> 2][2]);
        else
            atomicAdd(dst, acc[tid >> 2][tid & 3]);
    }
    if (a.hist) {
        u64* dst = (u64*)(a.hist + (size_t)blockIdx.y * a.bins * 3);
        for (int i = tid; i < a.bins * 3; i += 256)
            if (hist_s[i]) atomicAdd(&dst[i], (u64)hist_s[i]);
    }
}

bool aligned(const void* p, size_t to) { return ((uintptr_t)p & (to - 1)) == 0; }

int launch_confidence(const float* lowres, const unsigned char* mask, int n, int C, int g, int S, int kind, float* conf,
                      unsigned short* conf_q, const int* labels, long long* scores, int max_regions, int low_q,
                      const unsigned char* gt, int ignore_label, long long* hist, int bins, hipStream_t s) {
    VITSEG_CHECK_ARG(lowres && mask, VITSEG_EINVAL, "confidence: null lowres or mask");
    VITSEG_CHECK_ARG(conf || conf_q || scores || hist, VITSEG_EINVAL, "confidence: no output requested");
    VITSEG_CHECK_ARG(!scores || labels, VITSEG_EINVAL, "confidence: scores without labels");
    VITSEG_CHECK_ARG(!hist || gt, VITSEG_EINVAL, "confidence: hist without gt");
    VITSEG_CHECK_ARG(kind == VITSEG_CONF_PROB || kind == VITSEG_CONF_MARGIN, VITSEG_EINVAL,
                     "confidence: kind must be 0 (prob) or 1 (margin), got %d", kind);
    VITSEG_CHECK_ARG(kind != VITSEG_CONF_MARGIN || C >= 2, VITSEG_EINVAL, "confidence: margin needs C >= 2, got %d", C);
    VITSEG_CHECK_ARG(!scores || max_regions >= 0, VITSEG_EINVAL, "confidence: negative max_regions %d", max_regions);
    VITSEG_CHECK_ARG(!scores || (low_q >= 0 && low_q <= 65536), VITSEG_EINVAL, "confidence: low_q must be 0..65536, got %d",
                     low_q);
    VITSEG_CHECK_ARG(!hist || (bins >= 1 && bins <= CONF_MAX_BINS), VITSEG_EINVAL, "confidence: bins must be 1..%d, got %d",
                     CONF_MAX_BINS, bins);
    VITSEG_CHECK_ARG(!hist || (ignore_label >= -1 && ignore_label <= 255), VITSEG_EINVAL,
                     "confidence: ignore_label must be 0..255 or -1, got %d", ignore_label);
    VITSEG_CHECK_ARG(C >= 1 && C <= 255 && n >= 1 && n <= CONF_MAX_BATCH && S >= 1 && S <= CONF_MAX_SIDE && g >= 1 && g <= S,
                     VITSEG_ESHAPE, "confidence: bad shape n=%d C=%d g=%d S=%d (1 <= C <= 255, 1 <= n <= %d, 1 <= g <= S <= %d)",
                     n, C, g, S, CONF_MAX_BATCH, CONF_MAX_SIDE);
    if (scores && max_regions > 0) {
        const hipError_t e = hipMemsetAsync(scores, 0, (size_t)n * max_regions * 4 * sizeof(long long), s);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(confidence scores)");
    }
    if (hist) {
        const hipError_t e = hipMemsetAsync(hist, 0, (size_t)n * bins * 3 * sizeof(long long), s);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(confidence hist)");
    }
    ConfArgs a{lowres, mask, conf, conf_q, scores ? labels : nullptr, scores, gt, hist, C, g, S, kind, scores ? max_regions : 0,
               low_q, ignore_label, bins};
    const long long P = (long long)S * S;
    const dim3 grid((unsigned)((P + CHUNK - 1) / CHUNK), n);
    // a chunk touches at most (CHUNK - 1) / S + 2 output rows; their taps span at most scale * (rows - 1) source rows, + 1
    // for the floor at either end, + 1 for the lower tap of the last, + 1 for the fp32 rounding of the taps
    const int rows_out = min(S, (CHUNK - 1) / S + 2);
    const int nr_max = min(g, (int)((double)(rows_out - 1) * g / S) + 4);
    const size_t smem = (size_t)C * nr_max * g * sizeof(float);
    const bool staged = smem <= (size_t)STAGE_LIMIT && !opt(OPT_UPSAMPLE_GLOBAL);
    const bool vec = S % 4 == 0 && aligned(mask, 4) && (!conf || aligned(conf, 16)) && (!conf_q || aligned(conf_q, 8)) &&
                     (!a.labels || aligned(a.labels, 16)) && (!hist || aligned(gt, 4));
    if (vec && staged)
        hipLaunchKernelGGL((confidence_kernel<4, true>), grid, dim3(256), smem, s, a);
    else if (vec)
        hipLaunchKernelGGL((confidence_kernel<4, false>), grid, dim3(256), 0, s, a);
    else if (staged)
        hipLaunchKernelGGL((confidence_kernel<1, true>), grid, dim3(256), smem, s, a);
    else
        hipLaunchKernelGGL((confidence_kernel<1, false>), grid, dim3(256), 0, s, a);
    VITSEG_LAUNCH_CHECK("confidence");
    return VITSEG_OK;
}

}  // namespace
}  // namespace vitseg

extern "C" {

int vitseg_confidence(const float* lowres, const uint8_t* mask, int n, int C, int g, int S, int kind, float* conf,
                      uint16_t* conf_q, const int32_t* labels, int64_t* scores, int max_regions, int low_q, const uint8_t* gt,
                      int ignore_label, int64_t* hist, int bins, void* stream) {
    return vitseg::launch_confidence(lowres, mask, n, C, g, S, kind, conf, conf_q, labels, (long long*)scores, max_regions, low_q,
                                     gt, ignore_label, (long long*)hist, bins, (hipStream_t)stream);
}

}  // extern "C"
