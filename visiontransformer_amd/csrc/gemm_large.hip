// =====================================================================================================
// bf16 GEMM, large-M variant: block 256(M) x 128(N), BK = 64, 8 waves as 4(M) x 2(N) (64x64 per wave,
// the same per-wave work as the 128x128 kernel), ONE block per CU, 3-stage LDS ring (3 x 48 KiB).
//
// Why a second shape: at bf16 rates the 128x128 / 2-blocks-per-CU kernel stages 64 B/clk/CU, i.e. it needs
// the whole L2 bandwidth of the chip (34 TB/s) at full MFMA rate, and its single-tile prefetch exposes the
// L2/MALL latency (measured: 30 % MFMA busy, 790 TF/s asymptote, 1260 TF/s with the loads removed).  This
// tile stages 25 % fewer bytes per FLOP and keeps TWO K steps in flight: the global_load_lds of step kt+2
// are issued right after the barrier that publishes step kt and are only waited for (counted
// `s_waitcnt vmcnt(6)`: the 6 DMA pieces of step kt+1 may stay outstanding) two compute phases later.
// M = B*Np + B: the B*Np patch rows are whole 256-row tiles at 512x512; the CLS rows make one thin tile
// that is scheduled first and in which only the first wave row computes.
#include "gemm_tiles.hpp"

namespace vitseg {

// LBN = 128: waves 4(M) x 2(N), 64x64 per wave, 3-stage ring (3 x 48 KiB), 85 FLOP per staged byte.
// LBN = 256: waves 2(M) x 4(N), 128x64 per wave (128 accumulator registers), 2-stage ring (2 x 64 KiB),
//            128 FLOP per staged byte -- half the L2->LDS traffic of the 128x128 kernel, which is what bounds it.
template <typename T, typename OutT, int AMODE, int EPI, int LBN>
__global__ __launch_bounds__(512) void gemm_bf16_large_kernel(const GemmArgs p) {
    constexpr int CE = 8, BKE = 64, BK = BKF;
    constexpr int STAGES = LBN == 128 ? 3 : 2;
    constexpr int WAVES = 8;
    constexpr int MI = LBN == 128 ? 2 : 4, NI = 2;      // 32x32 MFMA tiles per wave
    constexpr int WROWS = MI * 32;                       // rows per wave
    constexpr int APW = LBM / 8 / WAVES;                 // A DMA pieces per wave (8 rows each)
    constexpr int WPW = LBN / 8 / WAVES;                 // W DMA pieces per wave
    extern __shared__ __attribute__((aligned(16))) float lds_raw[];  // [stage][A 256 rows | W LBN rows][32 words]
    auto stageA = [&](int st) { return lds_raw + st * (LBM + LBN) * BK; };
    auto stageW = [&](int st) { return lds_raw + st * (LBM + LBN) * BK + LBM * BK; };

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform: scalar branches below
    const int wm = LBN == 128 ? wave >> 1 : wave >> 2;
    const int wn = LBN == 128 ? wave & 1 : wave & 3;
    const int tiles_n = (p.N + LBN - 1) / LBN, tiles_m = (p.M + LBM - 1) / LBM;
    int t = xcd_remap(blockIdx.x, gridDim.x);
    const int GN = p.gn ? p.gn : (LBN == 128 ? ((size_t)p.K * sizeof(T) <= 2048 ? 8 : 4) : 4);
    const bool thin_last = p.M - (tiles_m - 1) * LBM <= 64 && tiles_m > 1;
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
    const int m0 = tile_m * LBM, n0 = tile_n * LBN;
    const bool computes = (p.M - m0 > 64) || wm == 0;  // thin tile: only the first 64 rows exist

    // ---- DMA assignment: per K step 32 A pieces + LBN/8 W pieces of 1 KiB (8 rows each) ----
    const T* asrc[APW];
    const T* wsrc[WPW];
    int ay[APW], ax[APW];
#pragma unroll
    for (int i = 0; i < APW; ++i) {
        const int row = (wave * APW + i) * 8 + (lane >> 3);
        const int cpos = (lane & 7) ^ ((row >> 1) & 7);
        const int m = min(m0 + row, p.M - 1);
        if (AMODE == A_PLAIN) {
            asrc[i] = (const T*)p.A + (size_t)m * p.lda + cpos * CE;
            ay[i] = ax[i] = 0;
        } else {
            const int bimg = m / p.Np, tt = m - bimg * p.Np;
            ay[i] = tt / p.g;
            ax[i] = tt - ay[i] * p.g;
            asrc[i] = (const T*)p.A + (size_t)m * p.D + cpos * CE;
        }
    }
#pragma unroll
    for (int i = 0; i < WPW; ++i) {
        const int row = (wave * WPW + i) * 8 + (lane >> 3);
        const int cpos = (lane & 7) ^ ((row >> 1) & 7);
        wsrc[i] = (const T*)p.W + (size_t)min(n0 + row, p.N - 1) * p.ldw + cpos * CE;
    }
    auto issue = [&](int kt, int st) {
        const int k0 = kt * BKE;
        int d0 = k0, ky = 1, kx = 1;
        if (AMODE == A_CONV3) {
            const int tap = k0 / p.D;
            d0 = k0 - tap * p.D;
            ky = tap / 3;
            kx = tap - ky * 3;
        }
#pragma unroll
        for (int i = 0; i < APW; ++i) {
            const T* ga;
            if (AMODE == A_PLAIN) {
                ga = asrc[i] + k0;
            } else {
                const int yy = ay[i] + ky - 1, xx = ax[i] + kx - 1;
                const bool in = (unsigned)yy < (unsigned)p.g && (unsigned)xx < (unsigned)p.g;
                ga = in ? asrc[i] + ((ptrdiff_t)(ky - 1) * p.g + (kx - 1)) * p.D + d0 : (const T*)p.zeros + (lane & 7) * CE;
            }
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)ga,
                                             (__attribute__((address_space(3))) void*)(stageA(st) + (wave * APW + i) * 8 * BK),
                                             16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < WPW; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc[i] + k0),
                                             (__attribute__((address_space(3))) void*)(stageW(st) + (wave * WPW + i) * 8 * BK),
                                             16, 0, 0);
    };

    f32x16 acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
    const int li = lane & 31, lh = lane >> 5;
    const int sw = (li >> 1) & 7;
    const int a_off = (wm * WROWS + li) * BK, b_off = (wn * NI * 32 + li) * BK;
    f32x4 a[2][MI], b[2][NI];
    auto lfrag = [&](int st, int j, int slot) {
        const int ch = (((2 * j + lh) ^ sw) << 2);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) a[slot][mi] = *(const f32x4*)&stageA(st)[a_off + mi * 32 * BK + ch];
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) b[slot][ni] = *(const f32x4*)&stageW(st)[b_off + ni * 32 * BK + ch];
    };
    auto mfmas = [&](int slot) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
                acc[mi][ni] = H16<T>::mfma(__builtin_bit_cast(bf16x8, a[slot][mi]),
                                           __builtin_bit_cast(bf16x8, b[slot][ni]), acc[mi][ni]);
    };

    const int KT = p.K / BKE;
    // Ring of STAGES buffers: while step kt is computed, steps kt+1 .. kt+STAGES-2 are in flight.  The loop is
    // rotated around the barrier (group 3 of step kt runs after the barrier that publishes step kt+1, under the
    // first fragment reads of step kt+1); sched_barrier pins "next group's ds_reads, then this group's MFMAs".
    issue(0, 0);
    if (STAGES == 3 && KT > 1) issue(1, 1);
    if (STAGES == 3 && KT > 1)
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");  // 6 = DMA pieces per wave per step at LBN = 128
    else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (STAGES == 2 && KT > 1) issue(1, 1);
    if (STAGES == 3 && KT > 2) issue(2, 2);
    int st = 0;
    if (computes) lfrag(0, 0, 0);
    for (int kt = 0; kt < KT; ++kt) {
        const int stn = st == STAGES - 1 ? 0 : st + 1;
        if (computes) {
            lfrag(st, 1, 1);
            __builtin_amdgcn_sched_barrier(0);
            mfmas(0);
            __builtin_amdgcn_sched_barrier(0);
            lfrag(st, 2, 0);
            __builtin_amdgcn_sched_barrier(0);
            mfmas(1);
            __builtin_amdgcn_sched_barrier(0);
            lfrag(st, 3, 1);
            __builtin_amdgcn_sched_barrier(0);
            mfmas(0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (kt + 1 < KT) {
            // step kt+1 has landed once only the pieces of later steps are outstanding (in-order retire);
            // lgkmcnt(0): this wave's reads of stage st are complete before anyone refills it
            if (STAGES == 3 && kt + 2 < KT)
                asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");
            else
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (kt + STAGES < KT) issue(kt + STAGES, st);
            if (computes) {
                lfrag(stn, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (computes) mfmas(1);
        st = stn;
    }

    // ---- epilogue: per-wave LDS staging (16 KiB = 64 rows x 64 cols fp32 at a time), row-vector stores ----
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (!computes) return;
    float* wl = lds_raw + wave * 4096;
    const int rr = lane >> 4, c4 = (lane & 15) * 4;
    OutT* C = (OutT*)p.C;
#pragma unroll
    for (int nh = 0; nh < NI / 2; ++nh) {   // 64-column halves of the wave tile
    const int gcol = n0 + wn * NI * 32 + nh * 64 + c4;
    f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
    if (p.bias && gcol < p.N) bias4 = *(const f32x4*)(p.bias + gcol);
#pragma unroll
    for (int half = 0; half < MI / 2; ++half) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    wl[(mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * 64 + ni * 32 + li] = acc[half * 2 + mi][nh * 2 + ni][r];
        // all LDS reads (and residual loads) first, stores last: in a kernel that contains LDS-DMA hipcc waits
        // vmcnt(0) before every use of a ds_read result, which would serialise the stores one by one
        f32x4 v[16], extra[16];
#pragma unroll
        for (int ps = 0; ps < 16; ++ps) {
            const int row = ps * 4 + rr;
            v[ps] = *(const f32x4*)&wl[row * 64 + c4];
            if (EPI == EPI_RESADD) {
                const int grow = min(m0 + wm * WROWS + half * 64 + row, p.M - 1);
                extra[ps] = *(const f32x4*)(p.R + (size_t)grow * p.ldc + min(gcol, p.N - 4));
            }
            if (EPI == EPI_DGELU) {  // training: R = the saved 16-bit gelu'(pre-activation)
                const int grow = min(m0 + wm * WROWS + half * 64 + row, p.M - 1);
                const uint2 u = *(const uint2*)((const T*)p.R + (size_t)grow * p.ldc + min(gcol, p.N - 4));
                extra[ps][0] = H16<T>::lo(u.x);
                extra[ps][1] = H16<T>::hi(u.x);
                extra[ps][2] = H16<T>::lo(u.y);
                extra[ps][3] = H16<T>::hi(u.y);
            }
        }
        if (gcol < p.N) {
#pragma unroll
            for (int ps = 0; ps < 16; ++ps) {
                const int grow = m0 + wm * WROWS + half * 64 + ps * 4 + rr;
                const size_t o = (size_t)grow * p.ldc + gcol;
                f32x4 pre = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float x = v[ps][e] + bias4[e];
                    if (EPI == EPI_GELU) {
                        if (p.aux) { const GeluPair gp = gelu_erf_pair_fast(x); x = gp.g; pre[e] = gp.d; }   // pre: gelu'(u), saved for the backward
                        else x = gelu_erf_fast(x);
                    }
                    if (EPI == EPI_RELU) x = fmaxf(x, 0.f);
                    if (EPI == EPI_RESADD && p.drop.thresh)
                        x = drop_keep(drop_key(p.drop.seed, p.drop.stream, grow + p.row_base), gcol + e, p.drop.thresh)
                                ? x * p.drop.scale : 0.f;
                    if (EPI == EPI_RESADD) x = extra[ps][e] + x;
                    if (EPI == EPI_DGELU) x *= extra[ps][e];
                    v[ps][e] = x;
                }
                if (EPI == EPI_GELU && p.aux && grow < p.M) {  // training: keep gelu'(pre-activation) for the backward
                    uint2 h;
                    h.x = H16<T>::pack2(pre[0], pre[1]);
                    h.y = H16<T>::pack2(pre[2], pre[3]);
                    *(uint2*)((T*)p.aux + o) = h;
                }
                if (grow < p.M) {
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
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-private buffer is reused by the next half
    }
    }
}

template <typename T, typename OutT, int AMODE, int EPI, int LBN = 128>
int launch_large(GemmArgs a, hipStream_t s) {
    if (a.ldw == 0) a.ldw = a.K;
    if (!a.gn) a.gn = env_gn();
    const int tiles = ((a.M + LBM - 1) / LBM) * ((a.N + LBN - 1) / LBN);
    const size_t smem = (size_t)(LBN == 128 ? 3 : 2) * (LBM + LBN) * BKF * sizeof(float);  // 144 / 128 KiB
    int dev = 0;
    static bool attr_set[64] = {};   // the attribute is per device
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!attr_set[dev]) {
        hipError_t e = hipFuncSetAttribute((const void*)gemm_bf16_large_kernel<T, OutT, AMODE, EPI, LBN>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(gemm_bf16_large)");
        attr_set[dev] = true;
    }
    hipLaunchKernelGGL((gemm_bf16_large_kernel<T, OutT, AMODE, EPI, LBN>), dim3(tiles), dim3(512), smem, s, a);
    VITSEG_LAUNCH_CHECK("gemm_bf16_large");
    return VITSEG_OK;
}

// the table of this kernel's instantiations; output: the operand type, fp32 for the residual stream and the head conv
template <typename T>
static int launch_large_t(int amode, int epi, int lbn, const GemmArgs& a, hipStream_t s, const char* who) {
#define ROW(OutT, AMODE, EPI, LBN) if (amode == AMODE && epi == EPI && lbn == LBN) return launch_large<T, OutT, AMODE, EPI, LBN>(a, s);
#define ROW2(OutT, EPI) ROW(OutT, A_PLAIN, EPI, 128) ROW(OutT, A_PLAIN, EPI, 256)
    ROW2(T, EPI_BIAS) ROW2(T, EPI_GELU) ROW2(T, EPI_DGELU) ROW2(float, EPI_RESADD)
    ROW(float, A_CONV3, EPI_RELU, 128) ROW(float, A_CONV3, EPI_BIAS, 128)   // EPI_BIAS: training, dgrad of the 3x3 conv
#undef ROW2
#undef ROW
    set_error("%s: unsupported amode/epilogue %d/%d (256x%d tiles)", who, amode, epi, lbn);
    return VITSEG_EINVAL;
}

int launch_gemm_large(bool f16, int amode, int epi, int lbn, const GemmArgs& a, hipStream_t s, const char* who) {
    return f16 ? launch_large_t<f16_t>(amode, epi, lbn, a, s, who) : launch_large_t<bf16_t>(amode, epi, lbn, a, s, who);
}

}  // namespace vitseg
