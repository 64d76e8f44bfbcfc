// The score of a stated class at V pixels of one output row, shared by confidence.hip (the class the mask states) and
// curves.hip (one class at every pixel): the values v_k re-generated from the low-res head output with the decoder tail's
// taps and fma placement, p = sigmoid(v_c) ("prob") or its lead over the best other class ("margin"), and its 16-bit form
// q = rint(p * 65535).  One exact sigmoid per pixel for prob, two for margin: the best other class is found on the raw values.
#pragma once
#include "tail_math.hpp"

namespace vitseg {

// zb: class 0 of the source rows, `plane` floats from class to class; rt / rb: the offsets of the upper and lower tap rows
// in a plane, x0 / x1: the tap columns within a row; cls >= C scores 0 (the class is clamped before it indexes).
template <int V>
__device__ __forceinline__ void score_pixels(const float* zb, size_t plane, int C, int kind, int rt, int rb, float wy0, float wy1,
                                             const int (&x0)[V], const int (&x1)[V], const float (&wx0)[V],
                                             const float (&wx1)[V], const int (&cls)[V], float (&p)[V], int (&q)[V]) {
    auto value = [&](int c, int e) {   // the decoder tail's fma placement
        const float* z = zb + (size_t)c * plane;
        const float top = __fmaf_rn(z[rt + x0[e]], wx0[e], __fmul_rn(z[rt + x1[e]], wx1[e]));
        const float bot = __fmaf_rn(z[rb + x0[e]], wx0[e], __fmul_rn(z[rb + x1[e]], wx1[e]));
        return __fmaf_rn(top, wy0, __fmul_rn(bot, wy1));
    };
    if (kind == VITSEG_CONF_PROB) {
#pragma unroll
        for (int e = 0; e < V; ++e) {   // (the class is clamped before it indexes: a value >= C reads class C - 1, unused)
            const float sg = sigmoid_aten(value(min(cls[e], C - 1), e));
            p[e] = cls[e] < C ? sg : 0.f;
        }
    } else {
        float vc[V], other[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            vc[e] = 0.f;
            other[e] = -INFINITY;
        }
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float v = value(c, e);
                if (c == cls[e])
                    vc[e] = v;
                else
                    other[e] = fmaxf(other[e], v);
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e)
            p[e] = cls[e] < C ? fminf(fmaxf(__fsub_rn(sigmoid_aten(vc[e]), sigmoid_aten(other[e])), 0.f), 1.f) : 0.f;
    }
#pragma unroll
    for (int e = 0; e < V; ++e) q[e] = min(max((int)rintf(__fmul_rn(p[e], 65535.0f)), 0), 65535);
}

}  // namespace vitseg
