// GEMM on the matrix cores:  C[M,N] = epi(A[M,K] . W[N,K]^T + bias),  fp32 or bf16 operands.
//
// Replaces aten::addmm / mkldnn_convolution behind nn.Linear / Conv2d in the reference
// (56-65 % of the CPU profile): q/k/v/o projections and MLP
// (transformers/models/vit/modeling_vit.py:207-254), patch embedding (:62-69) and
// seg_head.0 (model/CE/classes.py:241) through the gathering A loaders.
//
// T = float : v_mfma_f32_32x32x2_f32, an exact fp32 fmaf chain (no TF32 on gfx950), 64 cycles per
//             issue per SIMD -> matrix-pipe bound by a wide margin (roofline 157.3 TFLOP/s).
// T = bf16  : v_mfma_f32_32x32x16_bf16, fp32 accumulate, 32 cycles per issue (roofline 2.5 PFLOP/s);
//             8x the FLOPs per staged byte, so this tile shape leans on L2 bandwidth.
//
// Both element types share one structure because a staged operand row is 128 bytes either way:
// block 128x128, BK = 128 B of K per row (32 floats / 64 bf16), 4 waves as 2(M) x 2(N), each wave
// 64x64 = 2x2 MFMA tiles of 32x32 (64 accumulator registers).  Lane half h consumes the 16-byte
// chunks 2j+h (j = 0..3) of a row: for bf16 that chunk IS the 32x32x16 operand (k = 8h..8h+7 of
// k-step j); for fp32 the k index inside a 32x32x2 MFMA is arbitrary as long as A and B agree, so
// the chunk's four floats feed four consecutive MFMAs.  Either way a fragment is ONE ds_read_b128
// from a row-major tile whose chunk index is XOR-swizzled with (row >> 1) & 7 (conflict-free).
// Global->LDS goes through registers (the gathering loaders need per-chunk zero-fill),
// double-buffered in LDS with one barrier per K step; fragments are double-buffered in registers.
#include "gemm_tiles.hpp"

namespace vitseg {
namespace {

template <typename T> struct Elem;
template <> struct Elem<float> { static constexpr int CE = 4, BKE = 32; };           // elements per chunk / per row
template <> struct Elem<bf16_t> { static constexpr int CE = 8, BKE = 64; };          // bf16 bits
template <> struct Elem<f16_t> { static constexpr int CE = 8, BKE = 64; };           // IEEE half

template <typename T>
struct ARow {
    // per-row state of the A loader, computed once (row is fixed for a thread)
    const T* base;  // row base pointer (A_PLAIN / A_PATCH: image base of (b, gy, gx))
    int y, x;           // A_CONV3: pixel coordinates
    bool valid;
};

template <typename T, int AMODE>
__device__ __forceinline__ ARow<T> make_arow(const GemmArgs& p, int m) {
    ARow<T> r;
    r.valid = m < p.M;
    r.y = r.x = 0;
    const T* A = (const T*)p.A;
    if (!r.valid) {
        r.base = A;
        return r;
    }
    if (AMODE == A_PLAIN) {
        r.base = A + (size_t)m * p.lda;
    } else if (AMODE == A_PATCH) {
        const int b = m / p.Np, t = m - b * p.Np;
        const int gy = t / p.g, gx = t - gy * p.g;
        r.base = A + ((size_t)b * p.Cin * p.S + (size_t)gy * p.P) * p.S + (size_t)gx * p.P;
    } else {
        const int b = m / p.Np, t = m - b * p.Np;
        r.y = t / p.g;
        r.x = t - r.y * p.g;
        r.base = A + (size_t)m * p.D;  // centre pixel's token row
    }
    return r;
}

// Branch-free: out-of-range chunks read a safe in-bounds address and are zeroed by a select, so
// the whole K step stays one basic block and the scheduler can spread the loads between MFMAs.
template <typename T, int AMODE>
__device__ __forceinline__ f32x4 load_a(const GemmArgs& p, const ARow<T>& r, int k, bool& ok) {
    ok = r.valid && k < p.K;
    const int kc = min(k, p.K - Elem<T>::CE);
    const T* ptr;
    if (AMODE == A_PLAIN) {
        ptr = r.base + kc;
    } else if (AMODE == A_PATCH) {
        const int pp = p.P * p.P;
        const int c = kc / pp, rem = kc - c * pp;
        const int py = rem / p.P, px = rem - py * p.P;
        ptr = r.base + ((size_t)c * p.S + py) * p.S + px;
    } else {
        const int tap = kc / p.D, d = kc - tap * p.D;
        const int ky = tap / 3, kx = tap - ky * 3;
        const int yy = r.y + ky - 1, xx = r.x + kx - 1;
        const bool in = (unsigned)yy < (unsigned)p.g && (unsigned)xx < (unsigned)p.g;
        ok = ok && in;
        ptr = r.base + (in ? ((ptrdiff_t)(ky - 1) * p.g + (kx - 1)) * p.D : 0) + d;
    }
    return *(const f32x4*)ptr;  // zeroed by the caller when !ok, at LDS-write time (keeps the load in flight)
}

// MI x NI MFMA tiles (32x32) per wave; rows start at a_row0, columns at b_col0 inside the block tile.
//   <2,2>: the regular 2(M) x 2(N) wave grid, 64x64 per wave.
//   <1,1>/<2,1>: "thin" row tiles (<= 32 / <= 64 valid rows: the CLS rows that follow the B*Np patch
//   rows); the 4 waves split the 128 columns so such a tile costs 1/4 (1/2) of a regular one and is
//   scheduled first, instead of adding a whole extra round of blocks to the launch.
// TA / TB: operand storage form.  0 ("N-form"): [row][k], the reduction index is contiguous (activations,
// nn.Linear weights).  1 ("T-form", fp32 only): [k][row], the reduction index is the slow one -- what the
// backward GEMMs meet (dgrad reads W as [n][k] with n the reduction; wgrad reads dY and X with the token
// index as the reduction).  T-form tiles are staged as [32 k][128 rows] and read one float per lane per
// MFMA (conflict-free: consecutive lanes = consecutive rows), so no transposed copies are ever made.
//
// X3 (fp32 operands only): "fp32 on the fp16 matrix pipe".  Every operand value is split while it is staged,
// a = hi + lo * 2^-11 with hi = half(a), lo = half((a - hi) * 2^11) (22 significand bits, the scaled low part stays a
// normal half), and the product is accumulated as  acc0 += hi.hi',  acc1 += lo.hi' + hi.lo'  with
// v_mfma_f32_32x32x16_f16 (fp32 accumulate); C = acc0 + acc1 * 2^-11.  Dropped: lo.lo' (2^-22 relative) and the
// rounding of the low parts (2^-22): products are good to ~2^-21 instead of exact, at 3 half-precision MFMAs per
// 16 k instead of 8 fp32 ones (16x slower each).  The hi / lo planes share the 16 KiB an fp32 operand tile uses
// (64-byte rows, chunk index XOR-swizzled with (row >> 1) & 3), so buffering, loaders and epilogue are unchanged.
template <typename T, typename OutT, int AMODE, int EPI, int MI, int NI, int TA = 0, int TB = 0, int X3 = 0>
__device__ __forceinline__ void gemm_tile(const GemmArgs& p, float (*lds)[2][BM * BKF], int m0, int n0, int a_row0,
                                          int b_col0) {
    constexpr int CE = Elem<T>::CE, BKE = Elem<T>::BKE;
    constexpr int BK = BKF;  // LDS words per row
    const int tid = threadIdx.x, lane = tid & 63;

    f32x16 acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    static_assert(sizeof(T) == 4 || (TA == 0 && TB == 0), "T-form operands are implemented for fp32 only");
    static_assert(!X3 || (sizeof(T) == 4 && TA == 0 && TB == 0), "X3 splits N-form fp32 operands");
    f32x16 acc1[X3 ? MI : 1][X3 ? NI : 1];  // X3: the 2^-11-weighted cross terms
    if constexpr (X3) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc1[mi][ni][r] = 0.f;
    }
    const int li = lane & 31, lh = lane >> 5;
    const int sw = (li >> 1) & 7;
    const int a_off = TA ? a_row0 + li : (a_row0 + li) * BK, b_off = TB ? b_col0 + li : (b_col0 + li) * BK;

    // Fragment registers are double-buffered one MFMA group (16 MFMAs = 1024 matrix-pipe cycles)
    // ahead, so no LDS latency is exposed: group j+1's ds_reads are issued before group j's MFMAs.
    // The loop is rotated around the barrier: group 3 of tile kt runs AFTER the barrier that
    // publishes tile kt+1, with tile kt+1's group-0 fragments already being read.
    f32x4 a[2][MI], b[2][NI];
    auto lfrag = [&](int buf, int j, int slot) {
        const int ch = (((2 * j + lh) ^ sw) << 2);
        const int kq = (8 * j + 4 * lh) * BM;  // T-form: element e of the group is k = 8j + 4h + e
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            if constexpr (TA) {
#pragma unroll
                for (int e = 0; e < 4; ++e) a[slot][mi][e] = lds[buf][0][kq + e * BM + a_off + mi * 32];
            } else {
                a[slot][mi] = *(const f32x4*)&lds[buf][0][a_off + mi * 32 * BK + ch];
            }
        }
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            if constexpr (TB) {
#pragma unroll
                for (int e = 0; e < 4; ++e) b[slot][ni][e] = lds[buf][1][kq + e * BN + b_off + ni * 32];
            } else {
                b[slot][ni] = *(const f32x4*)&lds[buf][1][b_off + ni * 32 * BK + ch];
            }
        }
    };
    // one group = the MFMAs fed by one 16-byte chunk per operand: 4 k-steps of 32x32x2 (fp32, quarter
    // q = one float of the chunk) or 1 k-step of 32x32x16 (bf16, issued with quarter 0)
    auto mfma_group = [&](int slot, int e0, int e1) {
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int e = e0; e < e1; ++e)
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[slot][mi][e], b[slot][ni][e],
                                                                           acc[mi][ni], 0, 0, 0);
        } else {
            if (e0 == 0) {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
                        acc[mi][ni] = H16<T>::mfma(__builtin_bit_cast(bf16x8, a[slot][mi]),
                                                   __builtin_bit_cast(bf16x8, b[slot][ni]), acc[mi][ni]);
            }
        }
    };

    // split-K: blockIdx.y owns K steps [kt0, kt0 + KT) and writes its own partial C (p.C + y * split_stride)
    const int KT_all = (p.K + BKE - 1) / BKE;
    const int nsplit = gridDim.y, split = blockIdx.y;
    const int kt0 = (int)((long long)KT_all * split / nsplit);
    const int KT = (int)((long long)KT_all * (split + 1) / nsplit) - kt0;
    if constexpr (sizeof(T) == 4) {
        // ---- global -> register staging ----
        // N-form: thread owns 16-B chunk lc (of 8) of rows lr + 32 i.  T-form: chunk tc (of 32) of k rows tr + 8 i.
        const int lc = tid & 7, lr = tid >> 3;
        const int tc = tid & 31, tr = tid >> 5;
        ARow<T> arow[4];
        const T* wrow[4];
        bool wvalid[4];
        if constexpr (!TA) {
#pragma unroll
            for (int i = 0; i < 4; ++i) arow[i] = make_arow<T, AMODE>(p, m0 + lr + 32 * i);
        }
        if constexpr (!TB) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n0 + lr + 32 * i;
                wvalid[i] = n < p.N;
                wrow[i] = (const T*)p.W + (size_t)(wvalid[i] ? n : 0) * p.ldw;
            }
        }
        const bool ta_col_ok = m0 + tc * 4 < p.M, tb_col_ok = n0 + tc * 4 < p.N;
        f32x4 ra[4], rb[4];
        bool oka[4], okb[4];
        auto gload = [&](int kt) {
            const int k = (kt + kt0) * BKE + lc * CE;
            const int kc = min(k, p.K - CE);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (TA) {
                    const int kr = (kt + kt0) * BKE + tr + 8 * i;
                    oka[i] = ta_col_ok && kr < p.K;
                    ra[i] = *(const f32x4*)((const T*)p.A + (size_t)(oka[i] ? kr : 0) * p.lda +
                                            (oka[i] ? m0 + tc * 4 : 0));
                } else {
                    ra[i] = load_a<T, AMODE>(p, arow[i], k, oka[i]);
                }
                if constexpr (TB) {
                    const int kr = (kt + kt0) * BKE + tr + 8 * i;
                    okb[i] = tb_col_ok && kr < p.K;
                    rb[i] = *(const f32x4*)((const T*)p.W + (size_t)(okb[i] ? kr : 0) * p.ldw +
                                            (okb[i] ? n0 + tc * 4 : 0));
                } else {
                    rb[i] = *(const f32x4*)(wrow[i] + kc);
                    okb[i] = wvalid[i] && k < p.K;
                }
            }
        };
        const int wpos = lr * BK + ((lc ^ ((lr >> 1) & 7)) << 2);  // N-form; + 32*i rows -> same swizzle term
        const int tpos = tr * BM + tc * 4;                          // T-form: [k][128], + 8*i k-rows
        // X3: row r of an operand tile = 64 B of hi halves (plane 0, first 8 KiB) and 64 B of lo halves (plane 1);
        // this thread's 4 floats are half `lc & 1` of 16-byte chunk `lc >> 1`, stored at chunk ^ ((r >> 1) & 3)
        const int xpos = lr * 16 + ((((lc >> 1) ^ ((lr >> 1) & 3)) << 2) | ((lc & 1) << 1));  // in 4-byte words
        auto split = [&](const f32x4& v, uint2& hi, uint2& lo) {
            const _Float16 h0 = (_Float16)v[0], h1 = (_Float16)v[1], h2 = (_Float16)v[2], h3 = (_Float16)v[3];
            hi.x = __builtin_bit_cast(unsigned, f16x2{h0, h1});
            hi.y = __builtin_bit_cast(unsigned, f16x2{h2, h3});
            lo.x = H16<f16_t>::pack2((v[0] - (float)h0) * 2048.f, (v[1] - (float)h1) * 2048.f);
            lo.y = H16<f16_t>::pack2((v[2] - (float)h2) * 2048.f, (v[3] - (float)h3) * 2048.f);
        };
        auto swrite = [&](int buf) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (X3) {
                    uint2 hi, lo;
                    split(oka[i] ? ra[i] : z, hi, lo);
                    *(uint2*)&lds[buf][0][xpos + 32 * i * 16] = hi;
                    *(uint2*)&lds[buf][0][2048 + xpos + 32 * i * 16] = lo;
                    if constexpr (X3 == 2) {  // weights pre-split (vitseg_cast_params_split): 16 B = 4 hi halves | 4 lo halves
                        const f32x4 w = okb[i] ? rb[i] : z;
                        hi = uint2{__float_as_uint(w[0]), __float_as_uint(w[1])};
                        lo = uint2{__float_as_uint(w[2]), __float_as_uint(w[3])};
                    } else {
                        split(okb[i] ? rb[i] : z, hi, lo);
                    }
                    *(uint2*)&lds[buf][1][xpos + 32 * i * 16] = hi;
                    *(uint2*)&lds[buf][1][2048 + xpos + 32 * i * 16] = lo;
                } else {
                    *(f32x4*)&lds[buf][0][TA ? tpos + 8 * i * BM : wpos + 32 * i * BK] = oka[i] ? ra[i] : z;
                    *(f32x4*)&lds[buf][1][TB ? tpos + 8 * i * BN : wpos + 32 * i * BK] = okb[i] ? rb[i] : z;
                }
            }
        };
        if constexpr (X3) {
            // two 16-k steps per staged tile; per step and operand one hi and one lo fragment (16 B = 8 halves)
            f32x4 ah[2][MI], al[2][MI], bh[2][NI], bl[2][NI];
            const int xsw = (li >> 1) & 3;
            auto lfragx = [&](int buf, int st, int slot) {
                const int ch = ((2 * st + lh) ^ xsw) << 2;
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    const float* r = &lds[buf][0][(a_row0 + li + mi * 32) * 16 + ch];
                    ah[slot][mi] = *(const f32x4*)r;
                    al[slot][mi] = *(const f32x4*)(r + 2048);
                }
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) {
                    const float* r = &lds[buf][1][(b_col0 + li + ni * 32) * 16 + ch];
                    bh[slot][ni] = *(const f32x4*)r;
                    bl[slot][ni] = *(const f32x4*)(r + 2048);
                }
            };
            auto mfmax = [&](int slot) {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni) {
                        const bf16x8 xh = __builtin_bit_cast(bf16x8, ah[slot][mi]), xl = __builtin_bit_cast(bf16x8, al[slot][mi]);
                        const bf16x8 yh = __builtin_bit_cast(bf16x8, bh[slot][ni]), yl = __builtin_bit_cast(bf16x8, bl[slot][ni]);
                        acc[mi][ni] = H16<f16_t>::mfma(xh, yh, acc[mi][ni]);
                        acc1[mi][ni] = H16<f16_t>::mfma(xl, yh, acc1[mi][ni]);
                        acc1[mi][ni] = H16<f16_t>::mfma(xh, yl, acc1[mi][ni]);
                    }
            };
            gload(0);
            swrite(0);
            __syncthreads();
            lfragx(0, 0, 0);
            for (int kt = 0; kt < KT; ++kt) {
                const int buf = kt & 1;
                const int kn = min(kt + 1, KT - 1);
                gload(kn);
                lfragx(buf, 1, 1);
                __builtin_amdgcn_sched_barrier(0);
                mfmax(0);
                __builtin_amdgcn_sched_barrier(0);
                swrite(buf ^ 1);   // split + store of the next tile (VALU) in the shadow of the MFMAs around it
                __syncthreads();
                lfragx(buf ^ 1, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                mfmax(1);
            }
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[mi][ni][r] = fmaf(acc1[mi][ni][r], 1.0f / 2048.0f, acc[mi][ni][r]);
        } else {
        gload(0);
        swrite(0);
        __syncthreads();
        lfrag(0, 0, 0);
        for (int kt = 0; kt < KT; ++kt) {
            const int buf = kt & 1;
            const int kn = min(kt + 1, KT - 1);  // the last step re-stages its own tile: keeps the body branch-free
            // group 0: next tile's global loads are issued here and stay in flight for ~2 groups
            gload(kn);
            lfrag(buf, 1, 1);
            __builtin_amdgcn_sched_barrier(0);  // pin: hipcc otherwise sinks the loads down to their use
            mfma_group(0, 0, 4);
            // group 1
            lfrag(buf, 2, 0);
            __builtin_amdgcn_sched_barrier(0);
            mfma_group(1, 0, 4);
            // group 2: the staged tile is zero-masked and written to the idle LDS buffer mid-group
            lfrag(buf, 3, 1);
            __builtin_amdgcn_sched_barrier(0);
            mfma_group(0, 0, 2);
            __builtin_amdgcn_sched_barrier(0);
            swrite(buf ^ 1);
            __builtin_amdgcn_sched_barrier(0);
            mfma_group(0, 2, 4);
            // group 3: one barrier hands the buffers over, then the next tile's first fragments are read
            __syncthreads();
            lfrag(buf ^ 1, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            mfma_group(1, 0, 4);
        }
        }
    } else {
        // ---- bf16: global -> LDS directly (global_load_lds_dwordx4), no staging registers, no VALU ----
        // One wave instruction fills 1 KiB = 8 staged rows, lane l -> row l>>3, LDS chunk position l&7.
        // The LDS image is lane-linear, so the XOR swizzle is applied to the per-lane SOURCE chunk
        // (position p of row r holds logical chunk p ^ ((r>>1)&7)) and again on the fragment reads.
        // Rows beyond M / N are clamped (their results are never stored); 3x3 taps outside the image
        // read a zero page.  Requires K % 64 == 0 (checked by the launcher).
        const int wave = tid >> 6;
        const T* asrc[4];
        const T* wsrc[4];
        int ay[4], ax[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (wave * 4 + i) * 8 + (lane >> 3);
            const int cpos = (lane & 7) ^ ((row >> 1) & 7);
            const int m = min(m0 + row, p.M - 1), n = min(n0 + row, p.N - 1);
            wsrc[i] = (const T*)p.W + (size_t)n * p.ldw + cpos * CE;
            if (AMODE == A_PLAIN) {
                asrc[i] = (const T*)p.A + (size_t)m * p.lda + cpos * CE;
                ay[i] = ax[i] = 0;
            } else {  // A_CONV3
                const int bimg = m / p.Np, t = m - bimg * p.Np;
                ay[i] = t / p.g;
                ax[i] = t - ay[i] * p.g;
                asrc[i] = (const T*)p.A + (size_t)m * p.D + cpos * CE;
            }
        }
        auto issue = [&](int kt, int buf) {
            const int k0 = (kt + kt0) * BKE;
            int tap = 0, d0 = k0, ky = 1, kx = 1;
            if (AMODE == A_CONV3) {
                tap = k0 / p.D;  // a 64-wide K step lies inside one tap (D % 64 == 0)
                d0 = k0 - tap * p.D;
                ky = tap / 3;
                kx = tap - ky * 3;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const T* ga;
                if (AMODE == A_PLAIN) {
                    ga = asrc[i] + k0;
                } else {
                    const int yy = ay[i] + ky - 1, xx = ax[i] + kx - 1;
                    const bool in = (unsigned)yy < (unsigned)p.g && (unsigned)xx < (unsigned)p.g;
                    ga = in ? asrc[i] + ((ptrdiff_t)(ky - 1) * p.g + (kx - 1)) * p.D + d0
                            : (const T*)p.zeros + ((lane & 7) ^ 0) * CE;
                }
                const int lrow = (wave * 4 + i) * 8;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)ga,
                                                 (__attribute__((address_space(3))) void*)&lds[buf][0][lrow * BK], 16,
                                                 0, 0);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc[i] + k0),
                                                 (__attribute__((address_space(3))) void*)&lds[buf][1][lrow * BK], 16,
                                                 0, 0);
            }
        };
        issue(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (KT > 1) issue(1, 1);
        lfrag(0, 0, 0);
        for (int kt = 0; kt < KT; ++kt) {
            const int buf = kt & 1;
            lfrag(buf, 1, 1);
            mfma_group(0, 0, 4);
            lfrag(buf, 2, 0);
            mfma_group(1, 0, 4);
            lfrag(buf, 3, 1);
            mfma_group(0, 0, 4);
            // tile kt+1 (issued one K step ago) must have landed for every wave, and every wave's
            // reads of this buffer must be complete before it is refilled
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (kt + 2 < KT) issue(kt + 2, buf);
            lfrag(buf ^ 1, 0, 0);
            mfma_group(1, 0, 4);
        }
    }

    // ---- epilogue, staged through LDS so that global traffic is whole rows ----
    // acc reg r of lane (li, lh) = C[row (r&3) + 8 (r>>2) + 4 lh][col li]: one column per lane, which
    // would mean 64 scattered 2/4-byte stores per lane.  Each wave instead parks its sub-tile in its own
    // 16 KiB of the (now idle) operand buffers and re-reads it row-wise: 4 consecutive columns per
    // lane, so bias / residual / output move as 16-byte (fp32) or 8-byte (bf16) vectors along rows.
    __syncthreads();  // every wave is done with the operand tiles
    {
        const int wave = tid >> 6;
        float* wl = &lds[0][0][0] + wave * 4096;  // [64 rows][64 cols] fp32, wave-private
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    wl[(mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * 64 + ni * 32 + li] = acc[mi][ni][r];
        constexpr int LPR = NI * 8;        // lanes per row (4 columns each)
        constexpr int RPP = 64 / LPR;      // rows per pass
        const int rr = lane / LPR, c4 = (lane % LPR) * 4;
        const int gcol = n0 + b_col0 + c4;
        if (gcol < p.N) {
            f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
            if (p.bias) bias4 = *(const f32x4*)(p.bias + gcol);
            OutT* C = (OutT*)p.C + (size_t)blockIdx.y * p.split_stride;
            // all LDS reads (and residual / position loads) first, the stores last: in a kernel that contains
            // LDS-DMA hipcc waits vmcnt(0) before every use of a ds_read result, which would otherwise
            // serialise the 16 row stores one memory round trip at a time
            constexpr int NPS = MI * 32 / RPP;
            f32x4 v[NPS], extra[NPS];
#pragma unroll
            for (int ps = 0; ps < NPS; ++ps) {
                const int row = ps * RPP + rr;
                const int grow = min(m0 + a_row0 + row, p.M - 1);
                v[ps] = *(const f32x4*)&wl[row * 64 + c4];
                if (EPI == EPI_RESADD || (EPI == EPI_DGELU && sizeof(T) == 4))
                    extra[ps] = *(const f32x4*)(p.R + (size_t)grow * p.ldc + gcol);
                if constexpr (EPI == EPI_DGELU && sizeof(T) == 2) {  // 16-bit training: R = the saved gelu'(u), 16-bit
                    const uint2 u = *(const uint2*)((const T*)p.R + (size_t)grow * p.ldc + gcol);
                    extra[ps][0] = H16<T>::lo(u.x);
                    extra[ps][1] = H16<T>::hi(u.x);
                    extra[ps][2] = H16<T>::lo(u.y);
                    extra[ps][3] = H16<T>::hi(u.y);
                }
                if (EPI == EPI_POS) extra[ps] = *(const f32x4*)(p.R + (size_t)(1 + grow % p.Np) * p.N + gcol);
            }
#pragma unroll
            for (int ps = 0; ps < NPS; ++ps) {
                const int grow = m0 + a_row0 + ps * RPP + rr;
                if (grow >= p.M) continue;
                const size_t o = (size_t)grow * p.ldc + gcol;
                f32x4 aux4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float x = v[ps][e] + bias4[e];
                    // saved for the backward: fp32 keeps the pre-activation u, the 16-bit path keeps gelu'(u) itself
                    // (the backward epilogue is then one multiply instead of an erf + exp per element)
                    if (EPI == EPI_GELU) {
                        if (sizeof(T) == 4) {
                            if (p.aux) aux4[e] = x;
                            x = gelu_erf(x);
                        } else if (p.aux) {
                            { const GeluPair gp = gelu_erf_pair_fast(x); x = gp.g; aux4[e] = gp.d; }
                        } else {
                            x = gelu_erf_fast(x);
                        }
                    }
                    if (EPI == EPI_RELU) x = fmaxf(x, 0.f);
                    if (EPI == EPI_RESADD && p.drop.thresh)
                        x = drop_keep(drop_key(p.drop.seed, p.drop.stream, grow + p.row_base), gcol + e, p.drop.thresh)
                                ? x * p.drop.scale : 0.f;
                    if (EPI == EPI_RESADD || EPI == EPI_POS) x = extra[ps][e] + x;
                    if (EPI == EPI_DGELU) x *= sizeof(T) == 4 ? gelu_erf_grad(extra[ps][e]) : extra[ps][e];
                    v[ps][e] = x;
                }
                if (EPI == EPI_GELU && p.aux) {  // pre-activation, saved for the backward pass
                    if constexpr (sizeof(OutT) == 4) {
                        *(f32x4*)((float*)p.aux + o) = aux4;
                    } else {
                        uint2 h;
                        h.x = H16<OutT>::pack2(aux4[0], aux4[1]);
                        h.y = H16<OutT>::pack2(aux4[2], aux4[3]);
                        *(uint2*)((OutT*)p.aux + o) = h;
                    }
                }
                if constexpr (sizeof(OutT) == 4) {
                    *(f32x4*)(C + o) = v[ps];
                } else {
                    uint2 h;
                    h.x = H16<OutT>::pack2(v[ps][0], v[ps][1]);
                    h.y = H16<OutT>::pack2(v[ps][2], v[ps][3]);
                    *(uint2*)(C + o) = h;
                }
            }
        }
    }
}

template <typename T, typename OutT, int AMODE, int EPI, int TA = 0, int TB = 0, int X3 = 0>
__global__ __launch_bounds__(256, 2) void gemm_kernel(const GemmArgs p) {
    __shared__ __attribute__((aligned(16))) float lds[2][2][BM * BKF];  // [buffer][A|W][row*32 + swizzled chunk]

    const int wave = threadIdx.x >> 6;
    const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
    // Logical tile order (each XCD runs a contiguous piece of it, xcd_remap):
    //  1. a thin last row tile (the CLS rows) goes first;
    //  2. the rest is walked in column groups of GN tiles, row panels marching inside a group.  The ~64
    //     blocks resident on an XCD then form an 8x8 patch of tiles (each operand slice shared 8x) and a
    //     group's W panel (GN*128 rows of K) stays in the 4 MiB L2 while the A panels stream past it.
    //     (n-fastest order measured 62 % L2 hit rate / 16x over-fetch on the N = 3072 GEMM.)
    int t = xcd_remap(blockIdx.x, gridDim.x);
    const int GN = p.gn ? p.gn : 8;  // 4/8/16 time within 1.5 % of each other (tools/gn_sweep.sh); 8 fetches least
    const bool thin_last = p.M - (tiles_m - 1) * BM <= 64 && tiles_m > 1;
    int tile_m, tile_n;
    if (thin_last && t < tiles_n) {
        tile_m = tiles_m - 1;
        tile_n = t;
    } else {
        const int rows = thin_last ? tiles_m - 1 : tiles_m;
        if (thin_last) t -= tiles_n;
        const int gsz = rows * GN, ngroups = (tiles_n + GN - 1) / GN;
        const int grp = min(t / gsz, ngroups - 1);
        const int rem = t - grp * gsz;
        const int gcols = min(GN, tiles_n - grp * GN);
        tile_m = rem / gcols;
        tile_n = grp * GN + rem - tile_m * gcols;
    }
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int rows_valid = p.M - m0;
    if (rows_valid <= 32)
        gemm_tile<T, OutT, AMODE, EPI, 1, 1, TA, TB, X3>(p, lds, m0, n0, 0, wave * 32);
    else if (rows_valid <= 64)
        gemm_tile<T, OutT, AMODE, EPI, 2, 1, TA, TB, X3>(p, lds, m0, n0, 0, wave * 32);
    else
        gemm_tile<T, OutT, AMODE, EPI, 2, 2, TA, TB, X3>(p, lds, m0, n0, (wave >> 1) * 64, (wave & 1) * 64);
}

template <typename T, typename OutT, int AMODE, int EPI, int TA = 0, int TB = 0, int X3 = 0>
int launch_one(GemmArgs a, hipStream_t s) {
    if (a.ldw == 0) a.ldw = TB ? a.N : a.K;
    if (!a.gn) a.gn = env_gn();
    const int tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
    const int splits = a.splitk > 1 ? a.splitk : 1;
    hipLaunchKernelGGL((gemm_kernel<T, OutT, AMODE, EPI, TA, TB, X3>), dim3(tiles, splits), dim3(256), 0, s, a);
    VITSEG_LAUNCH_CHECK("gemm");
    return VITSEG_OK;
}

// out[r][c4] = epi(sum_s partial[s][r][c4] + bias): the K slices of the CLS rows, summed in slice order (deterministic).
// The epilogue is the tile kernels' one, including the training forms: hidden dropout on the residual branch (RESADD),
// the saved GELU derivative (GELU with aux, 16-bit) and the multiplication by it (DGELU, R = 16-bit derivative rows).
template <int EPI, typename OutT>
__global__ __launch_bounds__(256) void thin_reduce_kernel(const float* __restrict__ partial, const float* __restrict__ bias,
                                                          const float* __restrict__ R, OutT* __restrict__ C, int rows, int N,
                                                          int ldc, int splits, OutT* __restrict__ aux, DropArgs drop,
                                                          unsigned row0) {
    const int n4 = N >> 2;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * n4) return;
    const int r = i / n4, c = (i - r * n4) * 4;
    const size_t slab = (size_t)rows * N;
    f32x4 acc = *(const f32x4*)(partial + (size_t)r * N + c);
    for (int sIdx = 1; sIdx < splits; ++sIdx) {
        const f32x4 v = *(const f32x4*)(partial + sIdx * slab + (size_t)r * N + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += v[e];
    }
    f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
    if (bias) b4 = *(const f32x4*)(bias + c);
    f32x4 res = {0.f, 0.f, 0.f, 0.f};
    if (EPI == EPI_RESADD) res = *(const f32x4*)(R + (size_t)r * ldc + c);
    if constexpr (EPI == EPI_DGELU) {
        const uint2 d = *(const uint2*)((const OutT*)R + (size_t)r * ldc + c);
        res[0] = H16<OutT>::lo(d.x);
        res[1] = H16<OutT>::hi(d.x);
        res[2] = H16<OutT>::lo(d.y);
        res[3] = H16<OutT>::hi(d.y);
    }
    f32x4 der = {0.f, 0.f, 0.f, 0.f};
    const unsigned key = drop.thresh ? drop_key(drop.seed, drop.stream, row0 + (unsigned)r) : 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float x = acc[e] + b4[e];
        if (EPI == EPI_GELU) {
            // as the tile kernels of that format
            if (sizeof(OutT) == 4) x = gelu_erf(x);
            else if (aux) { const GeluPair gp = gelu_erf_pair_fast(x); x = gp.g; der[e] = gp.d; }
            else x = gelu_erf_fast(x);
        }
        if (EPI == EPI_RESADD) {
            if (drop.thresh) x = drop_keep(key, (unsigned)(c + e), drop.thresh) ? x * drop.scale : 0.f;
            x = res[e] + x;
        }
        if (EPI == EPI_DGELU) x *= res[e];
        acc[e] = x;
    }
    if constexpr (sizeof(OutT) == 4) {
        *(f32x4*)(C + (size_t)r * ldc + c) = acc;
    } else {
        uint2 h;
        h.x = H16<OutT>::pack2(acc[0], acc[1]);
        h.y = H16<OutT>::pack2(acc[2], acc[3]);
        *(uint2*)(C + (size_t)r * ldc + c) = h;
        if (EPI == EPI_GELU && aux) {
            h.x = H16<OutT>::pack2(der[0], der[1]);
            h.y = H16<OutT>::pack2(der[2], der[3]);
            *(uint2*)(aux + (size_t)r * ldc + c) = h;
        }
    }
}

template <typename OutT>
int launch_thin_reduce(const GemmArgs& a, int epi, int splits, hipStream_t s) {
    const int rows = a.thin_rows, body = a.M - rows;
    const int blocks = (rows * (a.N / 4) + 255) / 256;
    const float* R = nullptr;
    if (a.R) R = epi == EPI_DGELU ? (const float*)((const OutT*)a.R + (size_t)body * a.ldc) : a.R + (size_t)body * a.ldc;
    OutT* C = (OutT*)a.C + (size_t)body * a.ldc;
    OutT* aux = a.aux ? (OutT*)a.aux + (size_t)body * a.ldc : nullptr;
    const unsigned row0 = (unsigned)(a.row_base + body);
#define VITSEG_THIN(E)                                                                                                 \
    hipLaunchKernelGGL((thin_reduce_kernel<E, OutT>), dim3(blocks), dim3(256), 0, s, a.thin_scratch, a.bias, R, C, rows, \
                       a.N, a.ldc, splits, aux, a.drop, row0)
    switch (epi) {
        case EPI_BIAS: VITSEG_THIN(EPI_BIAS); break;
        case EPI_GELU: VITSEG_THIN(EPI_GELU); break;
        case EPI_DGELU:
            if constexpr (sizeof(OutT) == 4) {
                set_error("thin_reduce: dGELU epilogue is 16-bit only");
                return VITSEG_EINVAL;
            } else {
                VITSEG_THIN(EPI_DGELU);
            }
            break;
        default: VITSEG_THIN(EPI_RESADD);
    }
#undef VITSEG_THIN
    VITSEG_LAUNCH_CHECK("thin_reduce");
    return VITSEG_OK;
}

}  // namespace

// THE table of the tile kernel's N-form instantiations: a combination that is not a row here does not exist (EINVAL under the
// caller's name `who`).  The T-form rows (fp32 backward) are launch_gemm_tile_bwd's.
int launch_gemm_tile(GemmType type, bool out_f32, int amode, int epi, int x3, const GemmArgs& a, hipStream_t s, const char* who) {
#define ROW(ID, T, OutT, AMODE, EPI, X3) \
    if (type == ID && out_f32 == (sizeof(OutT) == 4) && amode == AMODE && epi == EPI && x3 == X3) return launch_one<T, OutT, AMODE, EPI, 0, 0, X3>(a, s);
#define ROW_X3(AMODE, EPI) ROW(GT_F32, float, float, AMODE, EPI, 0) ROW(GT_F32, float, float, AMODE, EPI, 1) ROW(GT_F32, float, float, AMODE, EPI, 2)
#define ROW_H16(AMODE, EPI) ROW(GT_BF16, bf16_t, bf16_t, AMODE, EPI, 0) ROW(GT_F16, f16_t, f16_t, AMODE, EPI, 0)
#define ROW_H16_F32(AMODE, EPI) ROW(GT_BF16, bf16_t, float, AMODE, EPI, 0) ROW(GT_F16, f16_t, float, AMODE, EPI, 0)
    // fp32, plain or on the fp16 pipe (x3)
    ROW_X3(A_PLAIN, EPI_BIAS) ROW_X3(A_PLAIN, EPI_GELU) ROW_X3(A_PLAIN, EPI_RESADD) ROW(GT_F32, float, float, A_PLAIN, EPI_RELU, 0)
    ROW_X3(A_PATCH, EPI_POS) ROW_X3(A_CONV3, EPI_RELU)
    // 16-bit operands; output in the operand type (feeds the next MFMA) or fp32 (residual stream, head, K slices)
    ROW_H16(A_PLAIN, EPI_BIAS) ROW_H16(A_PLAIN, EPI_GELU) ROW_H16(A_PLAIN, EPI_DGELU)
    ROW_H16_F32(A_PLAIN, EPI_RESADD) ROW_H16_F32(A_PLAIN, EPI_BIAS) ROW_H16_F32(A_CONV3, EPI_RELU) ROW_H16_F32(A_CONV3, EPI_BIAS)
#undef ROW_H16_F32
#undef ROW_H16
#undef ROW_X3
#undef ROW
    set_error("%s: unsupported amode/epilogue %d/%d", who, amode, epi);
    return VITSEG_EINVAL;
}

// fp32 backward: dgrad (W in T-form; plain or * gelu'), wgrad (both in T-form), dgrad of the 3x3 conv
int launch_gemm_tile_bwd(int amode, int ta, int tb, int epi, const GemmArgs& a, hipStream_t s) {
    if (amode == A_PLAIN && !ta && tb && epi == EPI_BIAS) return launch_one<float, float, A_PLAIN, EPI_BIAS, 0, 1>(a, s);
    if (amode == A_PLAIN && !ta && tb && epi == EPI_DGELU) return launch_one<float, float, A_PLAIN, EPI_DGELU, 0, 1>(a, s);
    if (amode == A_PLAIN && ta && tb && epi == EPI_BIAS) return launch_one<float, float, A_PLAIN, EPI_BIAS, 1, 1>(a, s);
    if (amode == A_CONV3 && !ta && !tb && epi == EPI_BIAS) return launch_one<float, float, A_CONV3, EPI_BIAS, 0, 0>(a, s);
    set_error("gemm_bwd: unsupported combination amode %d ta %d tb %d epi %d", amode, ta, tb, epi);
    return VITSEG_EINVAL;
}

// fp32 / x3: slices of 32-element K steps, epilogue without the training forms.  16-bit operands: 64-element steps, fp32
// partials, output in the consumer's format (EPI_RESADD writes fp32), and the training epilogues (aux, dropout) run in the
// reducing kernel, not in the slices.
int launch_thin_rows(GemmType type, int x3, const GemmArgs& a, int epi, int slices, hipStream_t s) {
    const int rows = a.thin_rows, body = a.M - rows;
    GemmArgs t = a;
    t.A = (const char*)a.A + (size_t)body * a.lda * (type == GT_F32 ? 4 : 2);
    t.M = rows;
    t.bias = nullptr;
    t.R = nullptr;
    t.C = a.thin_scratch;
    t.ldc = a.N;
    t.splitk = slices;
    t.split_stride = (size_t)rows * a.N;
    t.thin_scratch = nullptr;
    if (type != GT_F32) {
        t.aux = nullptr;
        t.drop = DropArgs{};
    }
    if (int rc = launch_gemm_tile(type, true, A_PLAIN, EPI_BIAS, x3, t, s, "gemm (K slices)")) return rc;
    if (type == GT_F32 || epi == EPI_RESADD) return launch_thin_reduce<float>(a, epi, slices, s);
    return type == GT_F16 ? launch_thin_reduce<f16_t>(a, epi, slices, s) : launch_thin_reduce<bf16_t>(a, epi, slices, s);
}

}  // namespace vitseg
