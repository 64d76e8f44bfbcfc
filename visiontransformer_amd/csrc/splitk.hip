// Split-K for the weight gradients: the output is only a weight matrix (36-144 tiles) while the reduction
// runs over every token row, so the K range is cut into `splits` slabs (one grid.y slice each, plain
// stores into partial[split][M][N]) that splitk_reduce_kernel sums in a fixed order (deterministic).
#include "gemm_tiles.hpp"

namespace vitseg {

__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ partial, float* __restrict__ out,
                                                            size_t n4, int splits) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        f32x4 acc = ((const f32x4*)partial)[i];
        for (int sIdx = 1; sIdx < splits; ++sIdx) {
            const f32x4 v = ((const f32x4*)partial)[(size_t)sIdx * n4 + i];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += v[e];
        }
        ((f32x4*)out)[i] = acc;
    }
}

int launch_splitk_reduce(const float* partial, float* out, size_t n4, int splits, hipStream_t s) {
    const int blocks = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, s, partial, out, n4, splits);
    VITSEG_LAUNCH_CHECK("splitk_reduce");
    return VITSEG_OK;
}

int wgrad_splits(int M, int N, int K, int kstep) {
    const int tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
    int splits = 1024 / tiles;   // at most 2 whole rounds of the 512 resident blocks (rounding UP gave a third, nearly empty one)
    const int ksteps = (K + kstep - 1) / kstep;
    if (splits > ksteps / 4) splits = ksteps / 4;    // keep >= 4 K steps per slab
    return splits < 1 ? 1 : splits;
}

size_t wgrad_scratch_floats(int M, int N, int K) { return (size_t)wgrad_splits(M, N, K, 32) * M * N; }

// THE slice count of the bf16 T-form weight gradient: the 8-phase kernel's (p8) or the 128x128 kernel's.  A remainder of K below
// 64 rows is a K step of its own in both kernels; the size query and launch_wgrad_bf16_tt both ask here.
int wgrad_bf16_splits(int M, int N, int K, bool p8) { return p8 ? wgrad_p8_splits(M, N, K) : wgrad_splits(M, N, K, 64); }

// Covers the 128x128 slicing and, for whole 256x256 tiles, the 8-phase kernel's: the router may pick either (wgrad_p8_applies
// also looks at an option and the leading dimensions)
size_t wgrad_bf16_scratch_floats(int M, int N, int K) {
    int splits = wgrad_bf16_splits(M, N, K, false);
    if (M % 256 == 0 && N % 256 == 0) {
        const int sp8 = wgrad_bf16_splits(M, N, K, true);
        if (sp8 > splits) splits = sp8;
    }
    return (size_t)splits * M * N;
}

}  // namespace vitseg
