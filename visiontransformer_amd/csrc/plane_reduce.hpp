// The masked reduction over byte planes that distance.hip and skeleton.hip share: the walk over the source pixels of one
// chunk and the fixed-order block sums.  A thread adds its pixels in index order, the block adds its threads by a butterfly
// and its 4 waves in turn: the order of an fp64 sum is a function of H * W alone.
#pragma once
#include "common.hpp"

namespace vitseg {

constexpr int PLANE_CHUNK = 4096;   // pixels per block of 256 threads: 4 groups of 4 pixels per thread

// The pixels of one chunk in the order every pass walks them: thread t takes the groups of 4 pixels t, t + 256, t + 512,
// t + 768 of the chunk; f(index) is called for each source pixel.  vec: P % 4 == 0, the 4 mask bytes are one word.
template <class F>
__device__ __forceinline__ void for_source_pixels(const unsigned char* __restrict__ src, int P, int vec, F f) {
    for (int k = 0; k < 4; ++k) {
        const int idx0 = blockIdx.x * PLANE_CHUNK + (k * 256 + threadIdx.x) * 4;
        if (idx0 >= P) break;
        if (vec) {
            const unsigned w = *reinterpret_cast<const unsigned*>(src + idx0);
            if (w == 0) continue;
            for (int e = 0; e < 4; ++e)
                if ((w >> (8 * e)) & 0xffu) f(idx0 + e);
        } else {
            const int cnt = min(4, P - idx0);
            for (int e = 0; e < cnt; ++e)
                if (src[idx0 + e]) f(idx0 + e);
        }
    }
}

// the sum over a block of 256 threads in a fixed order: butterflies inside each wave, then the 4 waves in turn
__device__ __forceinline__ double block_sum(double v, double* sh) {
    for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & (WAVE - 1)) == 0) sh[threadIdx.x / WAVE] = v;
    __syncthreads();
    const double r = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
    return r;
}

__device__ __forceinline__ int block_max(int v, int* sh) {
    for (int d = WAVE / 2; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
    if ((threadIdx.x & (WAVE - 1)) == 0) sh[threadIdx.x / WAVE] = v;
    __syncthreads();
    const int r = max(max(sh[0], sh[1]), max(sh[2], sh[3]));
    __syncthreads();
    return r;
}

}  // namespace vitseg
