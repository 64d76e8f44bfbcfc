// What the GEMM router (gemm_dispatch.hip) and the tile-kernel families share.  A kernel in an anonymous namespace can only be
// launched from its own translation unit: one runtime-valued launcher per kernel file, each launching its own kernel only.
#pragma once
#include "kernels.hpp"

namespace vitseg {

constexpr int BM = 128, BN = 128;   // gemm_tile.hip, gemm_tt.hip
constexpr int BKF = 32;             // row length in 4-byte LDS words
constexpr int LBM = 256;            // gemm_large.hip
inline int env_gn() { return (int)opt(OPT_GN); }  // experiments only: VITSEG_GN=<n> forces the column-group width of the tile order

enum GemmType { GT_F32 = 0, GT_BF16 = 1, GT_F16 = 2 };
// 128x128, N-form operands.  out_f32: always for fp32 operands; x3 (fp32): 1 = split A and W while staging, 2 = W pre-split;
// who: the caller's name in the message when (type, out_f32, amode, epi, x3) has no instantiation (VITSEG_EINVAL)
int launch_gemm_tile(GemmType type, bool out_f32, int amode, int epi, int x3, const GemmArgs& a, hipStream_t s, const char* who);
int launch_gemm_tile_bwd(int amode, int ta, int tb, int epi, const GemmArgs& a, hipStream_t s);  // fp32 with T-form operands
// the last a.thin_rows rows of `a` as `slices` K slices of the 128x128 kernel into a.thin_scratch + the reducing epilogue `epi`
int launch_thin_rows(GemmType type, int x3, const GemmArgs& a, int epi, int slices, hipStream_t s);
int launch_gemm_large(bool f16, int amode, int epi, int lbn, const GemmArgs& a, hipStream_t s, const char* who);  // 256 x lbn (128 / 256)
int launch_gemm_tt(const GemmArgs& a, hipStream_t s);  // bf16 T-form x T-form: a.splitk fp32 partials at a.C + y * a.split_stride
// K slices of a weight gradient on 128x128 tiles, `kstep`-deep K steps (32 fp32, 64 16-bit): size queries and launches call THIS
int wgrad_splits(int M, int N, int K, int kstep);

}  // namespace vitseg
