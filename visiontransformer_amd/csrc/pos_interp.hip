// Position-embedding table resampled to another patch grid, and its adjoint: what Hugging Face's
// ViTEmbeddings.interpolate_pos_encoding (modeling_vit.py) computes when a model built for a g0 x g0 grid sees an
// input of g1 x g1 patches.  Row 0 (CLS) is copied; the g0 x g0 patch rows, one channel per hidden unit, go through
// F.interpolate(mode="bicubic", align_corners=False): cubic coefficient A = -0.75, source coordinate
// (g0 / g1) * (o + 0.5) - 0.5, the four taps clamped to [0, g0 - 1].
//
// Both directions are elementwise over (row, channel): a thread owns one output value and sums its contributors in a
// fixed order (no atomics), so every result is reproducible bit for bit.  The adjoint runs as two separable passes, x
// then y, through a [g1, g0, D] scratch; clamped border taps that land on the same source index are summed.
#include "kernels.hpp"

namespace vitseg {
namespace {

inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }

// torch's cubic index/weight computation (fp32) for output index o: returns the first tap, fills the four weights.
// The multiply-adds are explicit fmaf: that is how torch's vectorised CPU build evaluates the same expressions (its weights
// are reproduced exactly for most grid pairs and to 1-2 ulp for the others; unfused evaluation differs by up to ~10 ulp).
__device__ inline float cubic1(float x, float A) { return fmaf(fmaf(A + 2.f, x, -(A + 3.f)) * x, x, 1.f); }
__device__ inline float cubic2(float x, float A) { return fmaf(fmaf(fmaf(A, x, -5.f * A), x, 8.f * A), x, -4.f * A); }
__device__ inline int cubic_taps(int o, int in, int out, float w[4]) {
#pragma clang fp contract(off)   // no other contractions than the explicit ones
    const float scale = (float)in / (float)out;
    const float real = fmaf(scale, (float)o + 0.5f, -0.5f);
    int i0 = (int)floorf(real);
    if (i0 > in - 1) i0 = in - 1;
    const float t = fminf(fmaxf(real - (float)i0, 0.f), 1.f);
    const float A = -0.75f;
    w[0] = cubic2(t + 1.f, A);
    w[1] = cubic1(t, A);
    w[2] = cubic1(1.f - t, A);
    w[3] = cubic2((1.f - t) + 1.f, A);
    return i0 - 1;
}

__device__ inline int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// the summed weight of output index o's taps that land on source index x (clamped taps included); false: none does
__device__ inline bool tap_weight(int o, int x, int in, int out, float* wsum) {
    float w[4];
    const int first = cubic_taps(o, in, out, w);
    float s = 0.f;
    bool hit = false;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (clampi(first + k, in - 1) == x) {
            s += w[k];
            hit = true;
        }
    *wsum = s;
    return hit;
}

// dst[1 + g1^2, D] from src[1 + g0^2, D]: out = sum_j wy[j] * (sum_k wx[k] * src[y_j, x_k]), taps in index order
__global__ __launch_bounds__(256) void pos_interp_kernel(const float* __restrict__ src, float* __restrict__ dst, int g0,
                                                         int g1, int D) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ((size_t)g1 * g1 + 1) * D) return;
    const int d = (int)(i % D), r = (int)(i / D);
    if (r == 0) {
        dst[i] = src[d];
        return;
    }
    const int oy = (r - 1) / g1, ox = (r - 1) - oy * g1;
    float wy[4], wx[4];
    const int y0 = cubic_taps(oy, g0, g1, wy), x0 = cubic_taps(ox, g0, g1, wx);
    const float* base = src + D + d;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float* row = base + (size_t)clampi(y0 + j, g0 - 1) * g0 * D;
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) t = fmaf(wx[k], row[(size_t)clampi(x0 + k, g0 - 1) * D], t);
        acc = fmaf(wy[j], t, acc);
    }
    dst[i] = acc;
}

// pass 1 (x): T[oy, x, d] = sum over ox ascending of (summed weight of ox's taps on x) * dout[1 + oy * g1 + ox, d]
__global__ __launch_bounds__(256) void pos_interp_bwd_x_kernel(const float* __restrict__ dout, float* __restrict__ T, int g0,
                                                               int g1, int D) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)g1 * g0 * D) return;
    const int d = (int)(i % D), x = (int)((i / D) % g0), oy = (int)(i / ((size_t)D * g0));
    const float* row = dout + (1 + (size_t)oy * g1) * D + d;
    float acc = 0.f;
    for (int ox = 0; ox < g1; ++ox) {
        float w;
        if (tap_weight(ox, x, g0, g1, &w)) acc = fmaf(w, row[(size_t)ox * D], acc);
    }
    T[i] = acc;
}

// pass 2 (y): din[1 + y * g0 + x, d] = sum over oy ascending of (summed weight of oy's taps on y) * T[oy, x, d];
// row 0 (CLS) copied
__global__ __launch_bounds__(256) void pos_interp_bwd_y_kernel(const float* __restrict__ dout, const float* __restrict__ T,
                                                               float* __restrict__ din, int g0, int g1, int D) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ((size_t)g0 * g0 + 1) * D) return;
    const int d = (int)(i % D), r = (int)(i / D);
    if (r == 0) {
        din[i] = dout[d];
        return;
    }
    const int y = (r - 1) / g0, x = (r - 1) - y * g0;
    const float* col = T + (size_t)x * D + d;
    float acc = 0.f;
    for (int oy = 0; oy < g1; ++oy) {
        float w;
        if (tap_weight(oy, y, g0, g1, &w)) acc = fmaf(w, col[(size_t)oy * g0 * D], acc);
    }
    din[i] = acc;
}

}  // namespace

int launch_pos_interp(const float* src, float* dst, int g0, int g1, int D, hipStream_t s) {
    VITSEG_CHECK_ARG(src && dst && g0 >= 1 && g1 >= 1 && D >= 1, VITSEG_EINVAL, "pos_interp: null pointer or grid %d -> %d, D %d",
                     g0, g1, D);
    hipLaunchKernelGGL(pos_interp_kernel, dim3(blocks_for(((size_t)g1 * g1 + 1) * D)), dim3(256), 0, s, src, dst, g0, g1, D);
    VITSEG_LAUNCH_CHECK("pos_interp");
    return VITSEG_OK;
}

int launch_pos_interp_bwd(const float* dout, float* din, float* scratch, int g0, int g1, int D, hipStream_t s) {
    VITSEG_CHECK_ARG(dout && din && scratch && g0 >= 1 && g1 >= 1 && D >= 1, VITSEG_EINVAL,
                     "pos_interp_bwd: null pointer or grid %d -> %d, D %d", g0, g1, D);
    hipLaunchKernelGGL(pos_interp_bwd_x_kernel, dim3(blocks_for((size_t)g1 * g0 * D)), dim3(256), 0, s, dout, scratch, g0, g1, D);
    VITSEG_LAUNCH_CHECK("pos_interp_bwd_x");
    hipLaunchKernelGGL(pos_interp_bwd_y_kernel, dim3(blocks_for(((size_t)g0 * g0 + 1) * D)), dim3(256), 0, s, dout, scratch, din,
                       g0, g1, D);
    VITSEG_LAUNCH_CHECK("pos_interp_bwd_y");
    return VITSEG_OK;
}

}  // namespace vitseg
