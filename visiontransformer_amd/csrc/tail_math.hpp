// The decoder tail's exact per-pixel arithmetic, shared by decoder_tail.hip (one tile), window.hip (overlapping tiles) and,
// for the taps, the losses on the regenerated logits (loss_pixel.hpp):
// the bilinear taps of F.interpolate(mode='bilinear', align_corners=False) and ATen's fp32 sigmoid.
#pragma once
#include "common.hpp"

namespace vitseg {

// Bit-exact restatement of ATen's CPU kernel as built for x86+FMA (see
// oracle/vitseg_oracle.py:upsample_bilinear): taps src = max(scale*(d+0.5)-0.5, 0),
//   row = fma(a, wx0, b*wx1);  out = fma(row_top, wy0, row_bot*wy1).
// Explicit __f*_rn intrinsics keep hipcc from re-contracting the expression.
__device__ __forceinline__ void taps(int d, float scale, int n_in, int& i0, int& i1, float& w0, float& w1) {
    float src = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)d, 0.5f)), 0.5f);
    src = src < 0.f ? 0.f : src;
    i0 = min((int)floorf(src), n_in - 1);
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    w1 = fminf(fmaxf(__fsub_rn(src, (float)i0), 0.f), 1.f);
    w0 = __fsub_rn(1.f, w1);
}

// `logits.sigmoid()` exactly as ATen's CPU kernel computes it for fp32 (UnaryOpsKernel.cpp sigmoid_kernel, vector path:
// a = 0 - x; a = Sleef_expf_u10(a); a = 1 + a; a = 1 / a) -- restated operation by operation (oracle/vitseg_oracle.py
// sigmoid_aten, pinned bit-for-bit against torch.sigmoid): the mask decision hinges on fp32 sigmoid TIES between
// classes (first index wins), so a 1-ulp difference in exp would move it.  Explicit *_rn intrinsics and fmaf keep
// hipcc from contracting or re-associating.
__device__ __forceinline__ float sigmoid_aten(float x) {
    const float d = __fsub_rn(0.0f, x);
    const float q = __builtin_rintf(__fmul_rn(d, 1.4426950408889634f));        // ties to even, as cvtps_epi32
    float s = __fmaf_rn(q, -0.693145751953125f, d);
    s = __fmaf_rn(q, -1.428606765330187045e-06f, s);
    float u = 0.000198527617612853646278381f;
    u = __fmaf_rn(u, s, 0.00139304355252534151077271f);
    u = __fmaf_rn(u, s, 0.00833336077630519866943359f);
    u = __fmaf_rn(u, s, 0.0416664853692054748535156f);
    u = __fmaf_rn(u, s, 0.166666671633720397949219f);
    u = __fmaf_rn(u, s, 0.5f);
    u = __fadd_rn(1.0f, __fmaf_rn(__fmul_rn(s, s), u, s));
    const int qi = (int)q, h = qi >> 1;
    u = __fmul_rn(__fmul_rn(u, __int_as_float((h + 127) << 23)), __int_as_float((qi - h + 127) << 23));
    u = d < -104.0f ? 0.0f : u;
    u = d > 100.0f ? INFINITY : u;
    return __fdiv_rn(1.0f, __fadd_rn(1.0f, u));
}

// The margin that settles argmax_c sigmoid(v_c) from the raw values alone (decoder_tail.hip upsample_kernel derives it):
// t1 = the largest value, margin = its lead over the second largest.  False: the exact sigmoids decide.
__device__ __forceinline__ bool argmax_settled(float t1, float margin) {
    const float at = fabsf(t1);
    return (at <= 2.0f && margin >= 1e-4f) || (at <= 8.0f && margin >= 4e-3f);
}

}  // namespace vitseg
