// Test-time augmentation (include/vitseg.h "test-time augmentation"): the model runs on flipped, quarter-turned and
// rescaled copies of a batch (the views, made by vitseg_augment and forwarded by vitseg_forward_lowres), and the views'
// LOW-RES head outputs ([n, C, g_k, g_k] each, in the view's own frame, on grids that may differ) are merged here:
//   vitseg_tta_affine   host arithmetic: the exact normalised affine of one of the eight flip / quarter-turn views
//   vitseg_tta_blend    low-res maps of K views -> merged fp32 [n, C, S, S] and / or mask uint8 [n, S, S], one launch
// For every output pixel the blend un-transforms the coordinate into each view's frame, takes the bilinear value there with
// the decoder tail's arithmetic (tail_math.hpp), weights, averages and decides sigmoid -> argmax, so no per-view full-size
// tensor (C*S*S*4 bytes per view and image) is ever written or read back.  The reference has no counterpart: its scripts
// look at every image once (model/CE/testViTModel.py:92-126).
#include <math.h>

#include "kernels.hpp"
#include "tail_math.hpp"

namespace vitseg {

constexpr int TTA_MAX_VIEWS = 16, TTA_MAX_S = 4096;
constexpr int TTA_CB = 4;   // classes per walk over the views: their taps are formed once per walk (6 classes: 200 VGPRs, 2 waves / SIMD; 4: 3 waves)

namespace {

// the K view descriptors, by value in the kernel arguments (uniform reads from the argument segment, no table upload)
struct TtaViews {
    const float* z[TTA_MAX_VIEWS];
    int g[TTA_MAX_VIEWS];
    int op[TTA_MAX_VIEWS];
    float w[TTA_MAX_VIEWS];
    float scale[TTA_MAX_VIEWS];   // g / S, rounded once to fp32 on the host (IEEE division, whatever the device's default is)
};

// tail_math.hpp's taps(), for scales that are no power of two.  There the coordinate is __fsub_rn(__fmul_rn(scale, d + 0.5), 0.5):
// header functions compiled with contraction on, and hipcc fuses the inlined pair into ONE fma.  For the decoder tail's and
// the window blend's scales (1 / P, powers of two) the product is exact and both forms agree; a view grid that does not
// divide S (scale g / S) needs the product rounded on its own, as ATen and the restatement round it: plain operators
// under contract(off), as augment.hip writes its sums.
__device__ __forceinline__ void taps_rounded(int d, float scale, int n_in, int& i0, int& i1, float& w0, float& w1) {
#pragma clang fp contract(off)
    const float prod = scale * ((float)d + 0.5f);
    float src = prod - 0.5f;
    src = src < 0.f ? 0.f : src;
    i0 = min((int)floorf(src), n_in - 1);
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    w1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
    w0 = 1.f - w1;
}

// Thread = 4 pixels of one output row; a block = blockDim.y rows x 4 * blockDim.x columns of one image (blockDim.x a
// multiple of 64), as window_blend_kernel.  VEC (S % 4 == 0 and aligned outputs): the 4 pixels are consecutive, one
// 16-byte store per class plane and one 4-byte mask store; otherwise they lie blockDim.x apart and every store is one
// element per lane, consecutive across the wave.
// The view-frame position of output pixel (y, x), i.e. unview(U, op)[y, x] = U[yv, xv] with x' = f ? S - 1 - x : x:
//   r = 0: (y, x')    r = 1: (S - 1 - x', y)    r = 2: (S - 1 - y, S - 1 - x')    r = 3: (x', S - 1 - y)
// so per view one tap set comes from y and four from the thread's x; a quarter-turned view swaps which of them indexes the
// low-res rows (consecutive threads then walk a low-res column: the maps are a few KB and stay in L1 / L2).
// Classes go in chunks of TTA_CB so that a view's taps are formed once per chunk, not once per class; within a class the
// views accumulate in view order.  MODE 1 takes ATen's fp32 sigmoid of every view's value before the mean.
// The mask: MODE 1 the first maximal merged probability; MODE 0 the raw argmax where the top-2 margin settles the sigmoid
// comparison (argmax_settled), else the exact fp32 sigmoids of a second walk.
template <bool VEC, int MODE>
__global__ __launch_bounds__(256) void tta_blend_kernel(const TtaViews V, int K, int C, int S, float wsum,
                                                        float* __restrict__ merged, uint8_t* __restrict__ mask) {
    const int y = (int)(blockIdx.y * blockDim.y + threadIdx.y);
    const int b = (int)blockIdx.z;
    if (y >= S) return;
    const int xbase = (int)blockIdx.x * 4 * (int)blockDim.x;
    int px[4], pc[4];
    bool inside[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        px[e] = xbase + (VEC ? 4 * (int)threadIdx.x + e : e * (int)blockDim.x + (int)threadIdx.x);
        inside[e] = px[e] < S;
        pc[e] = inside[e] ? px[e] : S - 1;   // a pixel past the row reads where the last one reads and stores nothing
    }
    if (!inside[0]) return;   // (VEC: S % 4 == 0, so the four pixels are inside together)

    // the merged values of classes [c0, c0 + nc) at the thread's 4 pixels
    auto blend = [&](int c0, int nc, float (&res)[TTA_CB][4]) {
#pragma unroll
        for (int j = 0; j < TTA_CB; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) res[j][e] = 0.f;
        for (int k = 0; k < K; ++k) {
            const int g = V.g[k], op = V.op[k];
            const float wk = V.w[k];
            const float scale = V.scale[k];
            const int r = op & 3;
            const bool flip = (op >> 2) != 0, turn = (r & 1) != 0;
            int a0, a1;
            float wa0, wa1;
            taps_rounded((r & 2) ? S - 1 - y : y, scale, g, a0, a1, wa0, wa1);
            int i00[4], i01[4], i10[4], i11[4];
            float wc0[4], wc1[4], wr0[4], wr1[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int xq = flip ? S - 1 - pc[e] : pc[e];
                int b0, b1;
                float wb0, wb1;
                taps_rounded((r == 1 || r == 2) ? S - 1 - xq : xq, scale, g, b0, b1, wb0, wb1);
                // rows / columns of the view's own frame: a quarter turn takes its rows from x and its columns from y
                const int r0 = turn ? b0 : a0, r1 = turn ? b1 : a1, q0 = turn ? a0 : b0, q1 = turn ? a1 : b1;
                i00[e] = r0 * g + q0;
                i01[e] = r0 * g + q1;
                i10[e] = r1 * g + q0;
                i11[e] = r1 * g + q1;
                wc0[e] = turn ? wa0 : wb0;
                wc1[e] = turn ? wa1 : wb1;
                wr0[e] = turn ? wb0 : wa0;
                wr1[e] = turn ? wb1 : wa1;
            }
            const size_t gg = (size_t)g * g;
            const float* zk = V.z[k] + ((size_t)b * C + c0) * gg;
#pragma unroll
            for (int j = 0; j < TTA_CB; ++j) {
                if (j >= nc) break;
                const float* z = zk + (size_t)j * gg;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float top = __fmaf_rn(z[i00[e]], wc0[e], __fmul_rn(z[i01[e]], wc1[e]));
                    const float bot = __fmaf_rn(z[i10[e]], wc0[e], __fmul_rn(z[i11[e]], wc1[e]));
                    const float u = __fmaf_rn(top, wr0[e], __fmul_rn(bot, wr1[e]));
                    const float t = MODE ? sigmoid_aten(u) : u;
                    res[j][e] = K == 1 ? t : __fmaf_rn(wk, t, res[j][e]);
                }
            }
        }
        if (K > 1) {
#pragma unroll
            for (int j = 0; j < TTA_CB; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) res[j][e] = __fdiv_rn(res[j][e], wsum);
        }
    };

    float t1[4], t2[4], best[4];
    int arg[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        t1[e] = -INFINITY;
        t2[e] = -INFINITY;
        best[e] = 0.f;
        arg[e] = 0;
    }
    // walk 0 stores the merged values and keeps the running top two; walk 1 (MODE 0, only where a margin leaves the sigmoid
    // comparison open) is the exact path: ATen's fp32 sigmoid of the same merged values, first maximal class wins
    for (int walk = 0; walk < 2; ++walk) {
        for (int c0 = 0; c0 < C; c0 += TTA_CB) {
            const int nc = min(TTA_CB, C - c0);
            float v[TTA_CB][4];
            blend(c0, nc, v);
#pragma unroll
            for (int j = 0; j < TTA_CB; ++j) {
                if (j >= nc) break;
                const int c = c0 + j;
                if (walk == 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float sg = sigmoid_aten(v[j][e]);
                        if (c == 0 || sg > best[e]) {
                            best[e] = sg;
                            arg[e] = c;
                        }
                    }
                    continue;
                }
                if (merged) {
                    float* row = merged + (((size_t)b * C + c) * S + y) * S;
                    if (VEC) {
                        const f32x4 v4 = {v[j][0], v[j][1], v[j][2], v[j][3]};
                        __builtin_nontemporal_store(v4, (f32x4*)(row + px[0]));
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (inside[e]) __builtin_nontemporal_store(v[j][e], row + px[e]);
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (c == 0 || v[j][e] > t1[e]) {   // strict: the first maximal class stays
                        t2[e] = t1[e];
                        t1[e] = v[j][e];
                        arg[e] = c;
                    } else {
                        t2[e] = fmaxf(t2[e], v[j][e]);
                    }
                }
            }
        }
        if (!mask) return;
        if (MODE == 1 || walk == 1) break;   // MODE 1: the merged probabilities decide as they are
        bool amb = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) amb = amb || (inside[e] && !argmax_settled(t1[e], t1[e] - t2[e]));
        if (!amb) break;
    }
    uint8_t* mrow = mask + ((size_t)b * S + y) * S;
    if (VEC) {
        uchar4 m4;
        m4.x = (unsigned char)arg[0];
        m4.y = (unsigned char)arg[1];
        m4.z = (unsigned char)arg[2];
        m4.w = (unsigned char)arg[3];
        *(uchar4*)(mrow + px[0]) = m4;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (inside[e]) mrow[px[e]] = (unsigned char)arg[e];
    }
}

}  // namespace

int launch_tta_blend(const vitseg_tta_view* views, int K, int n, int C, int S, int mode, float* merged, uint8_t* mask,
                     hipStream_t s) {
    VITSEG_CHECK_ARG(views, VITSEG_EINVAL, "tta_blend: null view list");
    VITSEG_CHECK_ARG(merged || mask, VITSEG_EINVAL, "tta_blend: both outputs are null");
    VITSEG_CHECK_ARG(K >= 1 && K <= TTA_MAX_VIEWS, VITSEG_EINVAL, "tta_blend: %d views (1..%d)", K, TTA_MAX_VIEWS);
    VITSEG_CHECK_ARG(mode == 0 || mode == 1, VITSEG_EINVAL, "tta_blend: mode %d (0 = mean of logits, 1 = mean of probabilities)",
                     mode);
    for (int k = 0; k < K; ++k) {
        VITSEG_CHECK_ARG(views[k].lowres, VITSEG_EINVAL, "tta_blend: view %d has a null low-res map", k);
        VITSEG_CHECK_ARG(views[k].op >= 0 && views[k].op <= 7, VITSEG_EINVAL, "tta_blend: view %d has op %d (0..7)", k,
                         views[k].op);
        VITSEG_CHECK_ARG(isfinite(views[k].weight) && views[k].weight > 0.f, VITSEG_EINVAL,
                         "tta_blend: view %d has weight %g (finite and > 0)", k, (double)views[k].weight);
    }
    VITSEG_CHECK_ARG(C >= 1 && C <= 255, VITSEG_ESHAPE, "tta_blend: %d classes (1..255)", C);
    VITSEG_CHECK_ARG(S >= 1 && S <= TTA_MAX_S, VITSEG_ESHAPE, "tta_blend: output size %d outside 1..%d", S, TTA_MAX_S);
    VITSEG_CHECK_ARG(n >= 1 && n <= 65535, VITSEG_ESHAPE, "tta_blend: %d images (1..65535)", n);
    TtaViews V{};
    volatile float wsum = 0.f;   // the fp32 sum in view order, each addition rounded to fp32
    for (int k = 0; k < K; ++k) {
        VITSEG_CHECK_ARG(views[k].g >= 1 && views[k].g <= TTA_MAX_S, VITSEG_ESHAPE, "tta_blend: view %d has grid %d (1..%d)", k,
                         views[k].g, TTA_MAX_S);
        V.z[k] = views[k].lowres;
        V.g[k] = views[k].g;
        V.op[k] = views[k].op;
        V.w[k] = views[k].weight;
        V.scale[k] = (float)((double)views[k].g / (double)S);
        wsum = wsum + views[k].weight;
    }
    for (int k = K; k < TTA_MAX_VIEWS; ++k) {   // never read; a valid descriptor all the same
        V.z[k] = V.z[0];
        V.g[k] = V.g[0];
        V.w[k] = 1.f;
        V.scale[k] = V.scale[0];
    }
    const float ws = wsum;
    VITSEG_CHECK_ARG(isfinite(ws), VITSEG_EINVAL, "tta_blend: the weights sum to %g", (double)ws);
    const bool vec = S % 4 == 0 && (uintptr_t)merged % 16 == 0 && (uintptr_t)mask % 4 == 0;
    // threads along x: a whole number of waves covering the row 4 pixels per thread, at most 256; the rest of the block's
    // 256 threads go to further rows
    int tx = ((S + 3) / 4 + 63) / 64 * 64;
    if (tx > 256) tx = 256;
    const int ty = 256 / tx;
    const dim3 block(tx, ty), grid((S + 4 * tx - 1) / (4 * tx), (S + ty - 1) / ty, n);
    if (vec && mode)
        hipLaunchKernelGGL((tta_blend_kernel<true, 1>), grid, block, 0, s, V, K, C, S, ws, merged, mask);
    else if (vec)
        hipLaunchKernelGGL((tta_blend_kernel<true, 0>), grid, block, 0, s, V, K, C, S, ws, merged, mask);
    else if (mode)
        hipLaunchKernelGGL((tta_blend_kernel<false, 1>), grid, block, 0, s, V, K, C, S, ws, merged, mask);
    else
        hipLaunchKernelGGL((tta_blend_kernel<false, 0>), grid, block, 0, s, V, K, C, S, ws, merged, mask);
    VITSEG_LAUNCH_CHECK("tta_blend");
    return VITSEG_OK;
}

// view(., op) as the normalised affine vitseg_augment_matrix takes (output unit square -> source unit square):
// q = c + R(r quarter turns) (p - c) with c = (0.5, 0.5), then u -> 1 - u for the horizontal flip, which acts on the
// source axis (the flip is applied first).  Every entry is 0, +-1 or 0.5 +- 0.5: exact.
int tta_affine(int op, double* a) {
    VITSEG_CHECK_ARG(a, VITSEG_EINVAL, "tta_affine: null pointer");
    VITSEG_CHECK_ARG(op >= 0 && op <= 7, VITSEG_EINVAL, "tta_affine: op %d (0..7)", op);
    static const double QC[4] = {1.0, 0.0, -1.0, 0.0}, QS[4] = {0.0, 1.0, 0.0, -1.0};
    const double c = QC[op & 3], s = QS[op & 3];
    a[0] = c;
    a[1] = -s;
    a[2] = 0.5 - (c - s) * 0.5;
    a[3] = s;
    a[4] = c;
    a[5] = 0.5 - (s + c) * 0.5;
    if (op >> 2) {
        a[0] = -a[0];
        a[1] = -a[1];
        a[2] = 1.0 - a[2];
    }
    for (int i = 0; i < 6; ++i) a[i] += 0.0;   // no negative zeros in the table
    return VITSEG_OK;
}

}  // namespace vitseg

extern "C" {

int vitseg_tta_affine(int op, double* affine6) { return vitseg::tta_affine(op, affine6); }

int vitseg_tta_blend(const vitseg_tta_view* views, int K, int n, int C, int S, int mode, float* merged, uint8_t* mask,
                     void* stream) {
    return vitseg::launch_tta_blend(views, K, n, C, S, mode, merged, mask, (hipStream_t)stream);
}

}  // extern "C"
