// The per-pixel device arithmetic of the fused losses on the regenerated logits, each piece written once: shared by loss_tail.hip
// (CE, CE with options, CE + soft Dice) and hardloss.hip (focal CE, OHEM).  A change to the bad-label rule, the ignore rule or
// a CE term is made here and reaches every loss kernel.
#pragma once
#include "tail_math.hpp"

namespace vitseg {

// One bilinear sample from the two source rows zt / zb: ATen's fma placement (tail_math.hpp, taps) --
//   row = fma(a, wx0, b * wx1);  out = fma(row_top, wy0, row_bot * wy1)
__device__ __forceinline__ float bilinear_fma(const float* zt, const float* zb, int x0, int x1, float wx0, float wx1, float wy0,
                                              float wy1) {
    const float top = __fmaf_rn(zt[x0], wx0, __fmul_rn(zt[x1], wx1));
    const float bot = __fmaf_rn(zb[x0], wx0, __fmul_rn(zb[x1], wx1));
    return __fmaf_rn(top, wy0, __fmul_rn(bot, wy1));
}

// one step of the online log-sum-exp
__device__ __forceinline__ void lse_step(float v, float& m, float& ssum) {
    const float mn = fmaxf(m, v);
    ssum = ssum * expf(m - mn) + expf(v - mn);
    m = mn;
}

struct NoClassSums {
    __device__ __forceinline__ void operator()(int, float) const {}
};

// Where pixel idx of [B, S, S] is: what an ignored pixel needs to write its zeros, before any tap is formed.  X, Y, b in this
// order: the order of the divisions decides the schedule of the whole kernel after it (b first moved a third of
// ce_loss_opts_kernel's instructions; profiles/loss_refactor_isa.txt).
struct PixelAt {
    int X, Y, b;
    __device__ __forceinline__ PixelAt(size_t idx, int S)
        : X((int)(idx % S)), Y((int)((idx / S) % S)), b((int)(idx / ((size_t)S * S))) {}
    // this pixel's element of class c in a [B, C, S, S] tensor
    __device__ __forceinline__ size_t out_index(int c, int C, int S) const { return (((size_t)b * C + c) * S + Y) * S + X; }
};

// The regenerated logits of a pixel: the taps of both axes, logit(c), the online log-sum-exp.
struct Pixel {
    const float* Z;
    int b, X, Y, C, g, y0, y1, x0, x1;
    float wy0, wy1, wx0, wx1;
    __device__ __forceinline__ Pixel(const float* Z_, size_t idx, int C_, int g_, int S) : Pixel(Z_, PixelAt(idx, S), C_, g_, S) {}
    __device__ __forceinline__ Pixel(const float* Z_, const PixelAt& at, int C_, int g_, int S)
        : Z(Z_), b(at.b), X(at.X), Y(at.Y), C(C_), g(g_) {
        const float scale = (float)g / (float)S;
        taps(Y, scale, g, y0, y1, wy0, wy1);
        taps(X, scale, g, x0, x1, wx0, wx1);
    }
    __device__ __forceinline__ float logit(int c) const {
        const float* zt = Z + (((size_t)b * C + c) * g + y0) * g;
        const float* zb = Z + (((size_t)b * C + c) * g + y1) * g;
        return bilinear_fma(zt, zb, x0, x1, wx0, wx1, wy0, wy1);
    }
    // lse over the classes and the logit of class t (0 when t is no class); each(c, logit) sees every class in order
    __device__ __forceinline__ void lse_picked(int t, float& lse, float& picked) const {
        NoClassSums none;
        lse_picked(t, lse, picked, none);
    }
    template <typename Each>
    __device__ __forceinline__ void lse_picked(int t, float& lse, float& picked, Each& each) const {
        float m = -INFINITY, ssum = 0.f;
        picked = 0.f;
        for (int c = 0; c < C; ++c) {
            const float v = logit(c);
            if (c == t) picked = v;
            lse_step(v, m, ssum);
            each(c, v);
        }
        lse = m + logf(ssum);
    }
};

struct CeOpt {
    const float* weight;   // [C] or null (all ones)
    long long ignore;      // read only when has_ignore
    int has_ignore;
    float eps;
};

// What a label is.  kept: it is not the ignore_index (an ignored pixel contributes nothing and its gradient is +0).  bad:
// outside [0, C) and kept: no class (uint8 255, torch's -100, C itself) -- its loss and gradient are NaN, so that the mean is
// NaN rather than a plausible wrong number, and it counts 1 in the mean's denominator.  t: the class, or -1.
// (kept, not its negation, is what the struct carries: `if (l.kept) { ... } else { zeros }` then runs the kept lanes of a
// divergent wave first and the zero fill of the ignored lanes right behind their stores, so that the two partial writes of a
// line of G meet in the cache; the other order cost the G-writing kernels 5 % at C = 17.  The field order is the one that
// leaves ce_loss_kernel's device code as it was.)
struct Label {
    int t;
    bool bad, kept;
};
__device__ __forceinline__ Label classify_label(long long tl /* uint8 widened before the compares */, int C) {   // no ignore_index
    Label l;
    l.kept = true;
    l.bad = tl < 0 || tl >= C;
    l.t = l.bad ? -1 : (int)tl;
    return l;
}
__device__ __forceinline__ Label classify_label(long long tl, const CeOpt& o, int C) {
    Label l = classify_label(tl, C);
    l.kept = !o.has_ignore || tl != o.ignore;
    return l;
}

// ---- the CE terms of a pixel: a = the weight of the picked-class term, bsm = eps / C that of each class's smoothing term ----

// label smoothing: sum_c w[c] z_c and sum_c w[c] in fp64 (exact products, one rounding per add), so that lse sum w - sum w z
// cancels no fp32 roundings.  The functor of Pixel::lse_picked; off: nothing is read.
struct SmoothSums {
    const float* wsh;
    bool on;
    double swz = 0.0, sw = 0.0;
    __device__ __forceinline__ void operator()(int c, float v) {
        if (on) {
            const double wc = (double)wsh[c];
            swz += wc * (double)v;
            sw += wc;
        }
    }
};
__device__ __forceinline__ double ce_picked_term(float a, float lse, float picked, bool bad) {
    return bad ? (double)NAN : (double)a * (double)(lse - picked);
}
__device__ __forceinline__ double ce_smooth_term(float bsm, float lse, double sw, double swz) {
    return (double)bsm * ((double)lse * sw - swz);
}
// d / d z_c of the picked-class term, pc = softmax_c, inv = gscale / den
__device__ __forceinline__ float ce_grad(float a, float pc, bool hit, float inv) { return (a * (pc - (hit ? 1.f : 0.f))) * inv; }
__device__ __forceinline__ float ce_grad_smooth(float bsm, float pc, float swf, float wc, float inv) {
    return (bsm * (pc * swf - wc)) * inv;
}

// ---- reductions ----

// The sum over a block of 256 threads in a fixed order, in its two halves: every thread puts (wave shuffle, one slot of red per
// wave), a barrier, then whoever needs the sum gets it.  A second sum of the same kernel takes a red of its own.
__device__ __forceinline__ void block_sum4_put(double v, double* red /* shared [4] */) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
}
__device__ __forceinline__ double block_sum4_get(const double* red) { return (red[0] + red[1]) + (red[2] + red[3]); }
__device__ __forceinline__ double block_sum4(double v, double* red) {
    block_sum4_put(v, red);
    __syncthreads();
    return block_sum4_get(red);
}

// the fixed-order sum of n per-block partials by one block of 1024 threads: 4 independent strided chains per thread (loads
// in flight), then a tree; the result is in red[0]
__device__ __forceinline__ void ce_fixed_order_sum(const double* __restrict__ partial, int n, double* red /* shared [1024] */) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int i = threadIdx.x;
    for (; i + 3 * 1024 < n; i += 4 * 1024) {
        s0 += partial[i];
        s1 += partial[i + 1024];
        s2 += partial[i + 2 * 1024];
        s3 += partial[i + 3 * 1024];
    }
    for (; i < n; i += 1024) s0 += partial[i];
    red[threadIdx.x] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
}

// class weights of the block in LDS (C <= 255); every thread of the block calls this
__device__ __forceinline__ void ce_stage_weights(float* wsh, const float* __restrict__ weight, int C) {
    if ((int)threadIdx.x < C) wsh[threadIdx.x] = weight ? weight[threadIdx.x] : 1.f;
    __syncthreads();
}

constexpr int CE_COUNT_PPB = 1024;   // targets per block of the count pass over the targets (4 per thread)

}  // namespace vitseg
