// The GEMM router: which kernel file takes C[M,N] = epi(A[M,K] . W[N,K]^T + bias).  Host code only; the launchers of the kernel
// files (gemm_tiles.hpp, kernels.hpp) launch their own kernel only.  The order of the tests below is the behaviour.
#include "gemm_tiles.hpp"

namespace vitseg {
namespace {

// Slice counts as functions of the shape alone; the tests below add what depends on the arguments.  gemm_slices() reports these.
// > 0: a (small) GEMM of this shape goes through K slices as a whole (kernels.hpp whole_split)
int whole_split_shape(int M, int N, int K, int kstep) { return K % kstep == 0 ? whole_split(M, N, K, kstep) : 0; }

// > 0: trailing rows of a GEMM with this K may go through the split-K side launch, on that many slices of >= 4 K steps
int thin_slices(int K, int kstep) {
    if (K < 256 || K % kstep != 0) return 0;
    const int sl = K / kstep / 4;
    return sl > THIN_MAX_SPLITS ? THIN_MAX_SPLITS : sl < 1 ? 1 : sl;
}

// > 0: the whole (small) GEMM goes through K slices + the reducing epilogue kernel
int whole_split_applies(const GemmArgs& a, int epi, int kstep) {
    const int sp = whole_split_shape(a.M, a.N, a.K, kstep);
    const bool ok = sp && a.thin_scratch && (size_t)sp * a.M * a.N <= a.thin_capacity && !a.drop.thresh &&
                    !a.aux && a.splitk <= 1 && a.ldc % 4 == 0 && (epi == EPI_BIAS || epi == EPI_GELU || epi == EPI_RESADD);
    return ok ? sp : 0;
}

// > 0: the trailing rows of `a` go through the split-K side launch (see GemmArgs::thin_scratch) on that many slices
// kstep 64 (16-bit operands): the reducing epilogue also covers dropout, the saved GELU derivative and dGELU (training)
int thin_split_applies(const GemmArgs& a, int epi, int kstep) {
    const bool h16 = kstep == 64;
    const int sl = thin_slices(a.K, kstep);
    const bool ok = sl && a.thin_scratch && a.thin_rows > 0 && a.thin_rows <= THIN_MAX_ROWS && a.M > a.thin_rows &&
                    (size_t)sl * a.thin_rows * a.N <= a.thin_capacity && (a.M - a.thin_rows) % BM == 0 &&
                    (h16 || (!a.drop.thresh && !a.aux)) && a.splitk <= 1 && a.ldc % 4 == 0 &&
                    (epi == EPI_BIAS || epi == EPI_GELU || epi == EPI_RESADD || (h16 && epi == EPI_DGELU));
    return ok ? sl : 0;
}

// A weight gradient on `splits` K slices (grid.y): partials in `scratch`, then the fixed-order reduce into a.C (deterministic)
template <typename F>
int sliced(GemmArgs a, int splits, float* scratch, hipStream_t s, F launch) {
    float* out = (float*)a.C;
    if (splits > 1) {
        a.C = scratch;
        a.splitk = splits;
    }
    a.split_stride = (size_t)a.M * a.N;
    if (int rc = launch(a)) return rc;
    return splits > 1 ? launch_splitk_reduce(scratch, out, (size_t)a.M * a.N / 4, splits, s) : VITSEG_OK;
}

enum H16Kernel { HK_NONE, HK_TILE, HK_LARGE, HK_XL, HK_P8, HK_H16P };

struct H16Route {
    H16Kernel body;   // kernel of the first body_rows rows (HK_NONE: a whole-split GEMM has tail rows only)
    int body_rows;
    int tail_rows;    // the rows after them, on a side launch of the 128x128 kernel:
    int slices;       //   > 0: before the body, as K slices + the reducing epilogue; 0: after it, with the body's epilogue
    int colsum_rows;  // leading rows whose column-sum partials the 8-phase kernel writes (GemmArgs::colsum_*)
};

}  // namespace

// x3 = 1: both fp32 operands are split into half pairs on the fly; 2: W is the pre-split shadow arena
// (vitseg_cast_params_split), only A is split in the kernel.  3 fp16 MFMAs per product (see gemm_tile, X3)
int launch_gemm_f32(const GemmArgs& a_in, int amode, int epi, hipStream_t s, int x3) {
    if (x3 != 1 && x3 != 2) x3 = 0;
    GemmArgs a = a_in;
    if (amode == A_PLAIN) {
        if (const int sp = whole_split_applies(a_in, epi, 32)) {  // small batch: every row through K slices
            a.thin_rows = a_in.M;
            return launch_thin_rows(GT_F32, x3, a, epi, sp, s);
        }
        if (const int sl = thin_split_applies(a_in, epi, 32)) {
            // the CLS rows first (tiny, split over K), then the whole-tile body: an exact number of rounds of blocks
            if (int rc = launch_thin_rows(GT_F32, x3, a_in, epi, sl, s)) return rc;
            a.M = a_in.M - a_in.thin_rows;
        }
    }
    a.thin_scratch = nullptr;
    VITSEG_CHECK_ARG(a.M > 0 && a.N > 0 && a.K > 0 && a.K % 4 == 0, VITSEG_EINVAL, "gemm_f32: bad M/N/K %d %d %d", a.M, a.N, a.K);
    VITSEG_CHECK_ARG(a.N % 4 == 0 && a.ldc % 4 == 0, VITSEG_ESHAPE, "gemm: N=%d and ldc=%d must be multiples of 4", a.N, a.ldc);
    if (amode == A_PLAIN) {
        VITSEG_CHECK_ARG(a.lda % 4 == 0, VITSEG_EINVAL, "gemm_f32: lda %% 4");
        if (!x3 && gemm_f32p_applies(a, epi)) return launch_gemm_f32p(a, epi, s);   // large shapes: persistent 256x128 kernel
    } else if (amode == A_PATCH && epi == EPI_POS) {
        VITSEG_CHECK_ARG(a.P % 4 == 0, VITSEG_ESHAPE, "patch size must be a multiple of 4");
    } else if (amode == A_CONV3 && epi == EPI_RELU) {
        VITSEG_CHECK_ARG(a.D % 4 == 0, VITSEG_ESHAPE, "hidden size must be a multiple of 4");
    }
    static const char* const who[3] = {"gemm_f32", "gemm_f32 (x3)", "gemm_f32 (x3, split W)"};
    return launch_gemm_tile(GT_F32, true, amode, epi, x3, a, s, who[x3]);
}

// Backward GEMMs in fp32 (no transposed copies, see gemm_tile):
//   dgrad  dX[M,K]  = dY[M,N] . W[N,K]        -> A N-form, B T-form;  epi: plain or * gelu'(R)
//   wgrad  dW[N,K]  = dY[M,N]^T . X[M,K]      -> A T-form, B T-form;  plain
// In GemmArgs terms M/N are always the OUTPUT rows/cols and K the reduction length.
int launch_gemm_f32_bwd(const GemmArgs& a, int amode, int ta, int tb, int epi, hipStream_t s) {
    VITSEG_CHECK_ARG(a.M > 0 && a.N > 0 && a.K > 0, VITSEG_EINVAL, "gemm_bwd: bad M/N/K %d %d %d", a.M, a.N, a.K);
    VITSEG_CHECK_ARG(a.N % 4 == 0 && a.ldc % 4 == 0 && a.lda % 4 == 0 && a.ldw % 4 == 0, VITSEG_ESHAPE,
                     "gemm_bwd: leading dimensions must be multiples of 4");
    VITSEG_CHECK_ARG(ta || a.K % 4 == 0, VITSEG_ESHAPE, "gemm_bwd: K %% 4");
    VITSEG_CHECK_ARG(!ta || a.M % 4 == 0, VITSEG_ESHAPE, "gemm_bwd: M %% 4 for a T-form A");
    return launch_gemm_tile_bwd(amode, ta, tb, epi, a, s);
}

// dW[M,N] = A^T . W (both T-form) with split-K through `scratch` (>= wgrad_scratch_floats floats; ldc == N)
int launch_wgrad_f32(GemmArgs a, float* scratch, hipStream_t s) {
    const int splits = wgrad_splits(a.M, a.N, a.K, 32);
    VITSEG_CHECK_ARG(splits <= 1 || (a.ldc == a.N && scratch), VITSEG_EINVAL, "wgrad: split-K needs a dense output and scratch");
    return sliced(a, splits, scratch, s, [&](const GemmArgs& g) { return launch_gemm_f32_bwd(g, A_PLAIN, 1, 1, EPI_BIAS, s); });
}

// ---- 16-bit operands (A and W), fp32 accumulate.  Output type follows the consumer: 16-bit for tensors that feed the
// next MFMA (q|k|v, MLP hidden), fp32 for the residual stream and the head features. ----
// Reads opt() and device_num_cus(), launches nothing.  Argument errors of the body are reported from here.
static int route_h16(const GemmArgs& a_in, int amode, int epi, H16Route& r) {
    r = H16Route{HK_NONE, 0, 0, 0, 0};
    const bool want_cs = a_in.colsum_out && a_in.colsum_scratch && epi == EPI_DGELU;
    const auto persistent = [&](const GemmArgs& g) {   // gemm_h16p.hip: bias epilogue, short K (VITSEG_NO_H16P=1: gemm_p8.hip)
        r.body = gemm_h16p_applies(g, epi) ? HK_H16P : HK_P8;
        r.body_rows = g.M;
        r.colsum_rows = want_cs ? g.M : 0;
        return VITSEG_OK;
    };
    GemmArgs a = a_in;
    if (amode == A_PLAIN) {
        if (const int sp = whole_split_applies(a_in, epi, 64)) {  // small batch: every row through K slices
            r.tail_rows = a_in.M;
            r.slices = sp;
            return VITSEG_OK;
        }
        // A ragged last row tile (the CLS rows) is free when it fits into the persistent kernel's last, partly empty round
        // (batch 32: 384 + 3 tiles of the N = 768 linears over 256 CUs): no side launch, no reducing kernel.
        if (a_in.M % 256 != 0 && a_in.M % 256 <= 128 && gemm_p8_applies(a_in, epi) &&
            gemm_p8_rounds(a_in.M, a_in.N) == gemm_p8_rounds(a_in.M - a_in.M % 256, a_in.N) && !opt(OPT_NO_RAGGED_P8))
            return persistent(a_in);
        const int sl = (a_in.M - a_in.thin_rows) % LBM == 0 ? thin_split_applies(a_in, epi, 64) : 0;
        if (sl) {
            r.tail_rows = a_in.thin_rows;  // CLS rows: split-K side launch (GemmArgs)
            r.slices = sl;
            a.M = a_in.M - a_in.thin_rows;
        }
    }
    VITSEG_CHECK_ARG(a.M > 0 && a.N > 0 && a.K > 0, VITSEG_EINVAL, "gemm_bf16: bad M/N/K %d %d %d", a.M, a.N, a.K);
    VITSEG_CHECK_ARG(a.K % 64 == 0, VITSEG_ESHAPE, "gemm_bf16: K=%d must be a multiple of 64", a.K);
    VITSEG_CHECK_ARG(a.N % 4 == 0 && a.ldc % 4 == 0, VITSEG_ESHAPE, "gemm: N=%d and ldc=%d must be multiples of 4", a.N, a.ldc);
    if (amode == A_PLAIN && gemm_p8_applies(a, epi)) {
        // persistent 256x256 kernel.  A ragged last row tile would cost every CU a whole extra round
        // (M = 65 600: 257 x 12 tiles over 256 CUs = 13 rounds for 12.05 rounds of work), so up to 128 trailing rows
        // (the CLS rows) go through the 128x128 kernel as a second, tiny launch with the same epilogue.
        const int tail = a.M % 256;
        if (tail != 0 && tail <= 128) {
            r.tail_rows = tail;
            a.M -= tail;
        }
        return persistent(a);
    }
    // the 256x128 / 3-stage kernel and the 128x128 / 2-stage kernel measure within a few % of each other on the
    // model's shapes (both ~790 TF/s asymptote); the large one is used where its deeper prefetch helps: long K
    const long force = opt(OPT_BF16_TILES);  // 1 small / 2 large / 3 xl for experiments
    const bool xl = force ? force == 3 : (a.M >= 8192 && a.N >= 2048);
    const bool large = force ? force == 2 : (!xl && a.M >= 4096 && a.K >= 2048);
    r.body_rows = a.M;
    if (amode == A_PLAIN) {
        VITSEG_CHECK_ARG(a.lda % 8 == 0, VITSEG_EINVAL, "gemm_bf16: lda %% 8");
        r.body = xl ? HK_XL : large ? HK_LARGE : HK_TILE;
        if (epi == EPI_BIAS || epi == EPI_GELU || epi == EPI_DGELU || epi == EPI_RESADD) return VITSEG_OK;
    } else if (amode == A_CONV3 && (epi == EPI_RELU || epi == EPI_BIAS)) {  // EPI_BIAS: training, dgrad of the 3x3 conv
        VITSEG_CHECK_ARG(a.D % 64 == 0 && a.zeros, VITSEG_ESHAPE, "%s must be a multiple of 64",
                         epi == EPI_RELU ? "hidden size" : "channel count");
        r.body = large ? HK_LARGE : HK_TILE;
        return VITSEG_OK;
    }
    set_error("gemm_bf16: unsupported amode/epilogue %d/%d", amode, epi);
    return VITSEG_EINVAL;
}

int launch_gemm_bf16(const GemmArgs& a_in, int amode, int epi, hipStream_t s, bool f16) {
    H16Route r;
    if (int rc = route_h16(a_in, amode, epi, r)) return rc;
    const GemmType type = f16 ? GT_F16 : GT_BF16;
    const bool out_f32 = epi == EPI_RESADD || amode == A_CONV3;
    GemmArgs a = a_in;
    if (r.slices) {
        a.thin_rows = r.tail_rows;
        if (int rc = launch_thin_rows(type, 0, a, epi, r.slices, s)) return rc;
    }
    a.M = r.body_rows;
    a.thin_scratch = nullptr;
    if (!r.colsum_rows) a.colsum_scratch = nullptr;
    int rc = VITSEG_OK;
    switch (r.body) {
        case HK_NONE: break;
        case HK_P8: rc = launch_gemm_p8(a, epi, s, f16); break;
        case HK_H16P: rc = launch_gemm_h16p(a, s, f16); break;
        case HK_XL: rc = launch_gemm_large(f16, amode, epi, 256, a, s, "gemm_bf16"); break;
        case HK_LARGE: rc = launch_gemm_large(f16, amode, epi, 128, a, s, "gemm_bf16"); break;
        case HK_TILE: rc = launch_gemm_tile(type, out_f32, amode, epi, 0, a, s, "gemm_bf16");
    }
    if (rc) return rc;
    if (r.tail_rows && !r.slices) {   // the rows after the persistent kernel's whole tiles: same epilogue, 128x128 kernel
        GemmArgs t = a;
        const auto row = [&](const void* p, size_t esz) { return (char*)p + (size_t)r.body_rows * a.ldc * esz; };
        t.M = r.tail_rows;
        t.row_base = a.row_base + r.body_rows;
        t.A = (const char*)a.A + (size_t)r.body_rows * a.lda * 2;
        if (a.aux) t.aux = row(a.aux, 2);
        if (a.R) t.R = (const float*)row(a.R, epi == EPI_RESADD ? 4 : 2);   // EPI_DGELU: 16-bit operand
        t.C = row(a.C, out_f32 ? 4 : 2);
        if ((rc = launch_gemm_tile(type, out_f32, A_PLAIN, epi, 0, t, s, "gemm_bf16"))) return rc;
    }
    if (!a_in.colsum_out) return VITSEG_OK;
    VITSEG_CHECK_ARG(a_in.colsum_scratch && !f16, VITSEG_EINVAL, "gemm: column sums need bf16 + scratch");
    if (r.colsum_rows > 0)   // per-tile partials are in the scratch; add the rows the persistent kernel did not cover and reduce
        return launch_colsum_finish_fused((const bf16_t*)a_in.C + (size_t)r.colsum_rows * a_in.ldc, a_in.M - r.colsum_rows,
                                          2 * ((r.colsum_rows + 255) / 256), a_in.colsum_out, a_in.colsum_scratch, a_in.N,
                                          a_in.ldc, s);
    return launch_colsum(a_in.C, 1, a_in.colsum_out, a_in.colsum_scratch, a_in.M, a_in.N, a_in.ldc, s);
}

// dW[M,N] (fp32, dense) = A^T . W with A = [K][M], W = [K][N] bf16 row-major; split-K through `scratch`.
int launch_wgrad_bf16_tt(GemmArgs a, float* scratch, hipStream_t s) {
    VITSEG_CHECK_ARG(a.M % 8 == 0 && a.N % 8 == 0 && a.lda % 8 == 0 && a.ldw % 8 == 0 && a.ldc == a.N && a.zeros,
                     VITSEG_ESHAPE, "wgrad_bf16_tt: M, N and the leading dimensions must be multiples of 8");
    if (wgrad_p8_applies(a)) return launch_wgrad_p8(a, scratch, s);   // 256x256 tiles, 8-phase stream (gemm_p8.hip)
    const int splits = wgrad_bf16_splits(a.M, a.N, a.K, false);
    VITSEG_CHECK_ARG(splits <= 1 || scratch, VITSEG_EINVAL, "wgrad_bf16_tt: split-K needs scratch");
    return sliced(a, splits, scratch, s, [&](const GemmArgs& g) { return launch_gemm_tt(g, s); });
}

// bf16 training GEMMs with a bf16 output (N-form: dgrad multiplies by a transposed bf16 copy of the weight):
// epi EPI_BIAS (plain dgrad), EPI_GELU (forward, `aux` = bf16 pre-activation) or EPI_DGELU (R = bf16 pre-activation).
// Same tile selection as inference (256x256 for wide outputs, 256x128 for long K, else 128x128).
int launch_gemm_bf16_train(const GemmArgs& a, int epi, hipStream_t s) {
    VITSEG_CHECK_ARG(a.M > 0 && a.N > 0 && a.K > 0 && a.K % 64 == 0, VITSEG_ESHAPE, "gemm_bf16_train: K=%d %% 64", a.K);
    VITSEG_CHECK_ARG(a.N % 4 == 0 && a.ldc % 4 == 0 && a.lda % 8 == 0, VITSEG_ESHAPE, "gemm_bf16_train: alignment");
    if (epi == EPI_BIAS || epi == EPI_GELU || epi == EPI_DGELU) return launch_gemm_bf16(a, A_PLAIN, epi, s, false);
    set_error("gemm_bf16_train: unsupported epilogue %d", epi);
    return VITSEG_EINVAL;
}

// The slice count of one K-sliced path for a dense [M, N] output reduced over K (include/vitseg.h vitseg_dbg_gemm_slices); 0 where
// the path does not take that shape.  Host arithmetic through the functions the launches above call.
int gemm_slices(int path, int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    GemmArgs g{};   // a weight gradient as vitseg_op_wgrad_bf16 lays it out
    g.M = M; g.N = N; g.K = K; g.lda = M; g.ldw = N; g.ldc = N;
    const bool tt_ok = M % 8 == 0 && N % 8 == 0;
    switch (path) {
        case VITSEG_SLICES_WHOLE_F32: return whole_split_shape(M, N, K, 32);
        case VITSEG_SLICES_WHOLE_H16: return whole_split_shape(M, N, K, 64);
        case VITSEG_SLICES_THIN_F32: return thin_slices(K, 32);
        case VITSEG_SLICES_THIN_H16: return thin_slices(K, 64);
        case VITSEG_SLICES_WGRAD_F32: return wgrad_splits(M, N, K, 32);
        case VITSEG_SLICES_WGRAD_BF16_TT: return tt_ok && !wgrad_p8_applies(g) ? wgrad_bf16_splits(M, N, K, false) : 0;
        case VITSEG_SLICES_WGRAD_BF16_P8: return tt_ok && wgrad_p8_applies(g) ? wgrad_bf16_splits(M, N, K, true) : 0;
    }
    return 0;
}

}  // namespace vitseg
