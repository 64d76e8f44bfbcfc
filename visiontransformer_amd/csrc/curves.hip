// Precision-recall counts of one class' probability map over all thresholds, with a pixel tolerance (vitseg_pr_counts,
// include/vitseg_curves.h): per image and score bin the valid pixels (pred), those within the tolerance of a true pixel (hit)
// and the true pixels by the best score within the tolerance (found).  The host answer writes the full-size logits, takes the
// sigmoid, runs a grey dilation by a disc and a distance transform per image and three bincounts; here the 16-bit score q is
// re-generated per pixel from the low-res head output (conf_score.hpp: vitseg_confidence's arithmetic under a mask that
// states one class everywhere) and never leaves the workgroup.
//
// One kernel, grid (tiles, n): a workgroup takes a TILE x TILE square of output pixels, a thread PER of them (a wave: 64
// consecutive pixels of one row).  Without dilation 256 threads score 16 independent pixels each; with it 1024 threads, 4 pixels
// each: the planes of a large disc leave room for one workgroup per CU, and its 16 waves hide the latency of the scoring chain
// and of the LDS reads that 4 waves did not.
//   STAGED   the window of low-res rows and columns the tile and its halo interpolate between is copied to LDS for all classes
//            first; when it does not fit (g == S) the kernel reads the taps from global memory: the same bits.
//   DILATE   (tol2 > 0) the tile and a halo of R = floor(sqrt(tol2)) pixels (the disc's last row) are scored into an LDS plane
//            of 32-bit words q | pos << 16 | valid << 17 (0 for a void or out-of-frame pixel: a true pixel is in its own disc
//            and q >= 0, so an absent score may stand as 0).  The disc is the union over dy of the horizontal window of half-width
//            h(dy) = floor(sqrt(tol2 - dy^2)) in row y + dy; a window of any width w is two reads of the plane of running maxima
//            over p = the largest power of two <= w, and those planes come from each other by doubling (two planes, ping-pong;
//            a level serves every dy whose window it fits before the next is built).  Both halves of a word take their maximum
//            in one packed 16-bit max: the low half is the best score in the disc, the high half reaches 3 exactly when the
//            disc holds a true pixel.  About 2 (2R + 1) LDS reads per pixel, not (2R + 1)^2.
//            Without it (tol2 == 0) there is no halo, no plane and no level: hit and found are the pixel's own pos bit.
//   counts   the runs of equal bin within a wave are reduced first (run_reduce.hpp), their heads add into a 32-bit LDS table
//            (a tile holds 4096 pixels), flushed with one 64-bit atomic per non-empty word: order-independent bits.
#include "conf_score.hpp"
#include "kernels.hpp"
#include "run_reduce.hpp"
#include "../../include/vitseg_curves.h"

namespace vitseg {
namespace {

constexpr int TILE = 64;                      // output pixels per side of a workgroup's square
constexpr int MAX_R = 16;                     // sqrt(VITSEG_CURVES_MAX_TOL2)
constexpr int CURVES_MAX_SIDE = 16384, CURVES_MAX_BATCH = 65535;
constexpr int STAGE_LIMIT = 16 * 1024;        // bytes of LDS for the staged low-res window

struct CurveArgs {
    const float* Z;
    const unsigned char* gt;
    i64* counts;
    int C, g, S, cls, kind, bins, ignore_label;
    int R, levels;                       // halo; the planes of running maxima (widths 1, 2, 4 ... 2^(levels - 1))
    unsigned char half[MAX_R + 1];       // h(dy)
    unsigned char level[MAX_R + 1];      // log2 of the largest power of two <= 2 h(dy) + 1
};

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pkmax(unsigned x, unsigned y) {   // the maxima of both 16-bit halves (v_pk_max_u16)
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(u16x2, x), __builtin_bit_cast(u16x2, y)));
}

template <bool STAGED, bool DILATE>
__global__ __launch_bounds__(DILATE ? 1024 : 256) void pr_counts_kernel(const CurveArgs a) {
    constexpr int NT = DILATE ? 1024 : 256, PER = TILE * TILE / NT;   // threads; pixels per thread
    extern __shared__ __attribute__((aligned(16))) unsigned dyn[];   // DILATE: two planes [W][W]; then STAGED: [class][row][col]
    __shared__ unsigned hist_s[VITSEG_CURVES_MAX_BINS * 3];
    const int S = a.S, g = a.g, C = a.C;
    const int R = DILATE ? a.R : 0, W = TILE + 2 * R;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int nt = (S + TILE - 1) / TILE;
    const int ty = (int)blockIdx.x / nt, tx = (int)blockIdx.x - ty * nt;
    const int Y0 = ty * TILE - R, X0 = tx * TILE - R;   // the region's first row and column (negative: outside the frame)
    const size_t img = (size_t)blockIdx.y * S * S;
    const float scale = (float)g / (float)S;
    for (int i = tid; i < a.bins * 3; i += NT) hist_s[i] = 0;

    int ymin = 0, xmin = 0, pitch = g;
    size_t plane = (size_t)g * g;
    const float* zb = a.Z + (size_t)blockIdx.y * C * g * g;
    if (STAGED) {   // the taps are monotone in the pixel: the window is spanned by those of the region's corners inside the frame
        float* zs = (float*)(dyn + (DILATE ? 2 * W * W : 0));
        int ya, yb, yc, yd, xa, xb, xc, xd;
        float w0, w1;
        taps(max(Y0, 0), scale, g, ya, yb, w0, w1);
        taps(min(Y0 + W, S) - 1, scale, g, yc, yd, w0, w1);
        taps(max(X0, 0), scale, g, xa, xb, w0, w1);
        taps(min(X0 + W, S) - 1, scale, g, xc, xd, w0, w1);
        const int nr = yd - ya + 1, nc = xd - xa + 1;   // each <= the bound launch_pr_counts sized zs for
        const int per = nr * nc;
        for (int i = tid; i < C * per; i += NT) {
            const int c = i / per, rem = i - c * per, r = rem / nc, cc = rem - r * nc;
            zs[i] = zb[((size_t)c * g + ya + r) * g + xa + cc];
        }
        ymin = ya;
        xmin = xa;
        pitch = nc;
        plane = (size_t)per;
        zb = zs;
    }
    // q | pos << 16 | valid << 17 of the frame pixel (Y, X); 0 for a void pixel
    auto word_of = [&](int Y, int X) -> unsigned {
        const int gv = a.gt[img + (size_t)Y * S + X];
        if (gv == a.ignore_label) return 0u;
        int y0, y1, x0[1], x1[1], cls[1] = {a.cls}, q[1];
        float wy0, wy1, wx0[1], wx1[1], p[1];
        taps(Y, scale, g, y0, y1, wy0, wy1);
        taps(X, scale, g, x0[0], x1[0], wx0[0], wx1[0]);
        x0[0] -= xmin;
        x1[0] -= xmin;
        score_pixels<1>(zb, plane, C, a.kind, (y0 - ymin) * pitch, (y1 - ymin) * pitch, wy0, wy1, x0, x1, wx0, wx1, cls, p, q);
        return (unsigned)q[0] | (gv == a.cls ? 1u << 16 : 0u) | 1u << 17;
    };
    if (STAGED) __syncthreads();

    unsigned own[PER], acc[PER];
    if (DILATE) {
        unsigned* cur = dyn;
        unsigned* nxt = dyn + W * W;
        for (int r = tid; r < W * W; r += NT) {
            const int ry = r / W, Y = Y0 + ry, X = X0 + (r - ry * W);
            cur[r] = (Y >= 0 && Y < S && X >= 0 && X < S) ? word_of(Y, X) : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int idx = k * NT + tid;
            own[k] = cur[(R + (idx >> 6)) * W + R + (idx & 63)];
            acc[k] = 0;
        }
        for (int lv = 0; lv < a.levels; ++lv) {
            const int p = 1 << lv;
            for (int dy = 0; dy <= R; ++dy) {
                if (a.level[dy] != lv) continue;   // (uniform)
                // the window [x - h, x + h] of row y +- dy, p <= 2 h + 1 < 2 p: the running maxima at x - h and at x + h - p + 1;
                // both lie in the row, R - h >= 0 and the second one's last column is x + h <= W - 1
                const int h = a.half[dy], lo = dy * W - h, hi = dy * W + h - p + 1;
#pragma unroll
                for (int k = 0; k < PER; ++k) {
                    const int idx = k * NT + tid, at = (R + (idx >> 6)) * W + R + (idx & 63);
                    acc[k] = pkmax(acc[k], pkmax(cur[at + lo], cur[at + hi]));
                    if (dy) acc[k] = pkmax(acc[k], pkmax(cur[at - dy * W - h], cur[at - dy * W + h - p + 1]));
                }
            }
            if (lv + 1 < a.levels) {   // the next plane: maxima over 2 p from two over p (the row's last p columns: never read)
                for (int r = tid; r < W * W; r += NT) nxt[r] = (r % W) + p < W ? pkmax(cur[r], cur[r + p]) : cur[r];
                __syncthreads();
                unsigned* t = cur;
                cur = nxt;
                nxt = t;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int idx = k * NT + tid, Y = Y0 + (idx >> 6), X = X0 + (idx & 63);
            own[k] = (Y < S && X < S) ? word_of(Y, X) : 0u;
            acc[k] = own[k];
        }
        __syncthreads();   // hist_s is zero
    }

    auto iadd = [](int x, int y) { return x + y; };
#pragma unroll
    for (int k = 0; k < PER; ++k) {   // (whole waves reach the shuffles: a pixel outside the frame has own == 0)
        int bin = -1, fbin = -1, hit = 0;
        if (own[k] >> 17) {
            bin = (int)((own[k] & 0xffffu) * (unsigned)a.bins) >> 16;
            const bool pos = (own[k] >> 16) & 1u;
            hit = DILATE ? (acc[k] >> 16) == 3u : pos;
            if (pos) fbin = (int)((acc[k] & 0xffffu) * (unsigned)a.bins) >> 16;
        }
        const Run r = find_run(bin, 0, lane);
        const int cnt = run_reduce(1 | (hit << 16), lane, r.end, iadd);   // a wave holds 64 pixels: no carry
        if (r.head) {
            atomicAdd(&hist_s[bin * 3], (unsigned)(cnt & 0xffff));
            if (cnt >> 16) atomicAdd(&hist_s[bin * 3 + 1], (unsigned)(cnt >> 16));
        }
        const Run f = find_run(fbin, 0, lane);
        const int fc = run_reduce(1, lane, f.end, iadd);
        if (f.head) atomicAdd(&hist_s[fbin * 3 + 2], (unsigned)fc);
    }
    __syncthreads();
    u64* dst = (u64*)(a.counts + (size_t)blockIdx.y * a.bins * 3);
    for (int i = tid; i < a.bins * 3; i += NT)
        if (hist_s[i]) atomicAdd(&dst[i], (u64)hist_s[i]);
}

int isqrt(int v) {
    int r = 0;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

template <bool STAGED, bool DILATE>
int launch_kernel(const CurveArgs& a, dim3 grid, size_t smem, hipStream_t s) {
    if (smem > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)pr_counts_kernel<STAGED, DILATE>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(pr_counts)");
    }
    hipLaunchKernelGGL((pr_counts_kernel<STAGED, DILATE>), grid, dim3(DILATE ? 1024 : 256), smem, s, a);
    VITSEG_LAUNCH_CHECK("pr_counts");
    return VITSEG_OK;
}

bool shape_ok(int n, int S) { return n >= 1 && n <= CURVES_MAX_BATCH && S >= 1 && S <= CURVES_MAX_SIDE; }

size_t pr_counts_scratch_bytes(int, int, int) { return 0; }   // the plane and its dilation stay in LDS

int launch_pr_counts(const float* lowres, const unsigned char* gt, int n, int C, int g, int S, int cls, int kind, int bins,
                     int tol2, int ignore_label, long long* counts, void* scratch, size_t scratch_bytes, hipStream_t s) {
    VITSEG_CHECK_ARG(lowres && gt && counts, VITSEG_EINVAL, "pr_counts: null lowres, gt or counts");
    VITSEG_CHECK_ARG(kind == VITSEG_CONF_PROB || kind == VITSEG_CONF_MARGIN, VITSEG_EINVAL,
                     "pr_counts: kind must be 0 (prob) or 1 (margin), got %d", kind);
    VITSEG_CHECK_ARG(bins >= 1 && bins <= VITSEG_CURVES_MAX_BINS, VITSEG_EINVAL, "pr_counts: bins must be 1..%d, got %d",
                     VITSEG_CURVES_MAX_BINS, bins);
    VITSEG_CHECK_ARG(tol2 >= 0 && tol2 <= VITSEG_CURVES_MAX_TOL2, VITSEG_EINVAL, "pr_counts: tol2 must be 0..%d, got %d",
                     VITSEG_CURVES_MAX_TOL2, tol2);
    VITSEG_CHECK_ARG(ignore_label >= -1 && ignore_label <= 255, VITSEG_EINVAL,
                     "pr_counts: ignore_label must be 0..255 or -1, got %d", ignore_label);
    VITSEG_CHECK_ARG(C >= 1 && C <= 255 && shape_ok(n, S) && g >= 1 && g <= S, VITSEG_ESHAPE,
                     "pr_counts: bad shape n=%d C=%d g=%d S=%d (1 <= C <= 255, 1 <= n <= %d, 1 <= g <= S <= %d)", n, C, g, S,
                     CURVES_MAX_BATCH, CURVES_MAX_SIDE);
    VITSEG_CHECK_ARG(kind != VITSEG_CONF_MARGIN || C >= 2, VITSEG_EINVAL, "pr_counts: margin needs C >= 2, got %d", C);
    VITSEG_CHECK_ARG(cls >= 0 && cls < C, VITSEG_EINVAL, "pr_counts: cls must be 0..%d, got %d", C - 1, cls);
    const size_t need = pr_counts_scratch_bytes(n, S, tol2);
    VITSEG_CHECK_ARG(scratch || need == 0, VITSEG_EINVAL, "pr_counts: null scratch");
    VITSEG_CHECK_ARG(scratch_bytes >= need, VITSEG_EWORKSPACE, "pr_counts: scratch of %zu bytes, %zu needed", scratch_bytes, need);
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)n * bins * 3 * sizeof(long long), s);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(pr_counts counts)");

    CurveArgs a{};
    a.Z = lowres;
    a.gt = gt;
    a.counts = counts;
    a.C = C, a.g = g, a.S = S, a.cls = cls, a.kind = kind, a.bins = bins, a.ignore_label = ignore_label;
    a.R = isqrt(tol2);   // the disc's last row: dy^2 <= tol2
    for (int dy = 0; dy <= a.R; ++dy) {
        a.half[dy] = (unsigned char)isqrt(tol2 - dy * dy);
        int lv = 0;
        while ((2 << lv) <= 2 * a.half[dy] + 1) ++lv;
        a.level[dy] = (unsigned char)lv;
        a.levels = max(a.levels, lv + 1);
    }
    const bool dilate = tol2 > 0;
    const int W = TILE + 2 * a.R;
    // a region touches at most min(S, W) output rows; their taps span at most scale * (rows - 1) source rows, + 1 for the
    // floor at either end, + 1 for the lower tap of the last, + 1 for the fp32 rounding of the taps; the same for columns
    const int span = min(S, W);
    const int nr_max = min(g, (int)((double)(span - 1) * g / S) + 4);
    const size_t stage = (size_t)C * nr_max * nr_max * sizeof(float);
    const bool staged = stage <= (size_t)STAGE_LIMIT && !opt(OPT_UPSAMPLE_GLOBAL);
    const size_t smem = (dilate ? (size_t)2 * W * W * sizeof(unsigned) : 0) + (staged ? stage : 0);
    const int nt = (S + TILE - 1) / TILE;
    const dim3 grid((unsigned)(nt * nt), n);
    if (dilate) return staged ? launch_kernel<true, true>(a, grid, smem, s) : launch_kernel<false, true>(a, grid, smem, s);
    return staged ? launch_kernel<true, false>(a, grid, smem, s) : launch_kernel<false, false>(a, grid, smem, s);
}

}  // namespace
}  // namespace vitseg

extern "C" {

int vitseg_curves_version(void) { return VITSEG_CURVES_VERSION; }

size_t vitseg_pr_counts_scratch_bytes(int n, int S, int tol2) { return vitseg::pr_counts_scratch_bytes(n, S, tol2); }

int vitseg_pr_counts(const float* lowres, const uint8_t* gt, int n, int C, int g, int S, int cls, int kind, int bins, int tol2,
                     int ignore_label, int64_t* counts, void* scratch, size_t scratch_bytes, void* stream) {
    return vitseg::launch_pr_counts(lowres, gt, n, C, g, S, cls, kind, bins, tol2, ignore_label, (long long*)counts, scratch,
                                    scratch_bytes, (hipStream_t)stream);
}

}  // extern "C"
