// The forward walks of the model (forward.hpp): the large-batch route and the small-batch route (small.hpp), and the
// route decision between them.  Inference (vitseg_api.hip) and the training step's forward (vitseg_train.hip) call them.
#include "kernels.hpp"
#include "profile.hpp"
#include "forward.hpp"

namespace vitseg {

using namespace plan;

long small_max_rows() {
    const long v = opt(OPT_SMALL_MAX_ROWS);
    return v > 0 ? v : SMALL_MAX_ROWS;
}

bool small_applies(const vitseg_config* cfg, int batch, int precision) {
    Shape s;
    if (precision == VITSEG_F32X3 || opt(OPT_NO_SMALL) || check_config(cfg, &s)) return false;
    const long rows = (long)batch * s.N;
    if (!(rows < small_max_rows() && s.D % 64 == 0 && s.I % 32 == 0 && s.I > s.D && s.S % 4 == 0)) return false;
    // 16-bit operands (inference): whole 64-value K steps per chunk, the sequence lengths of the key-split attention kernel (it
    // writes the 16-bit context), and fewer rows than fp32 -- the large-batch 16-bit kernels (256 x 256 tiles) catch up at
    // batch 16 of 197 tokens and at batch 4 of 785 (profiles/r05_h16_route_probe.txt)
    const long lim16 = opt(OPT_SMALL_MAX_ROWS) > 0 ? opt(OPT_SMALL_MAX_ROWS) : small_max_rows_16(s.N);   // (the option: probes of the limit)
    if (precision != VITSEG_F32 && !(s.I % 64 == 0 && attn_small_infer(s.Np) && rows < lim16)) return false;
    // ... and K chunks of the split linears (o_proj: K = D, fc2: K = I) that are whole 64-value steps: gemm_f32s counts a 16-bit
    // K in pairs and needs chunks of 32 pairs (D = 448 splits into 2 chunks of 224 values, D = 320 into 2 of 160)
    if (precision != VITSEG_F32 && ((s.D / small_splits(s.D, s.D)) % 64 || (s.I / small_splits(s.D, s.I)) % 64)) return false;
    return true;
}

namespace {

const float* wt(const Fwd& f, int t, int layer = 0) { return f.params + tensor_offset(*f.lay, t, layer); }

// weight operand of a GEMM: the fp32 arena, its 16-bit shadow or its pre-split form (same element offsets)
const void* wg(const Fwd& f, int t, int layer = 0) {
    const size_t off = tensor_offset(*f.lay, t, layer);
    if (f.x3 == 2) return (const float*)f.params_lp + off;
    return f.h16 ? (const void*)((const unsigned short*)f.params_lp + off) : (const void*)(f.params + off);
}

// dropout sites: 0 embeddings, 1 attention probabilities, 2 attention output, 3 MLP output (modeling_vit.py:159,184,276,283)
DropArgs drop(const Fwd& f, int layer, int site) { return drop_args(f.drop_p, f.drop_seed, (unsigned)(layer * 8 + site)); }

// embeddings (a2 + a3): the patch GEMM gathers straight from the NCHW image (+ bias + position embedding), the CLS rows,
// the embedding dropout; mode: launch_gemm_f32's operand mode
int embed_gemm(const Fwd& f, float* X, int mode) {
    const Shape& s = f.s;
    const int Mp = f.batch * s.Np;
    GemmArgs g{};
    g.A = f.x; g.W = f.x3 == 2 ? wg(f, VITSEG_T_PATCH_W) : (const void*)wt(f, VITSEG_T_PATCH_W);  // fp32 (or pre-split) weights
    g.bias = wt(f, VITSEG_T_PATCH_B); g.R = f.pos; g.C = X;
    g.M = Mp; g.N = s.D; g.K = s.Kp; g.lda = 0; g.ldc = s.D;
    g.S = s.S; g.P = s.P; g.g = s.g; g.Np = s.Np; g.Cin = s.Cin; g.D = s.D;
    {
        ProfScope ps(f.prof.patch, 2.0 * g.M * g.N * g.K, f.st);
        if (int rc = launch_gemm_f32(g, A_PATCH, EPI_POS, f.st, mode)) return rc;
    }
    if (int rc = launch_cls_rows(wt(f, VITSEG_T_CLS), f.pos, X, f.batch, s.Np, s.D, f.st)) return rc;
    if (f.drop_p > 0.f) return launch_dropout_rows(X, X, 0, Mp + f.batch, s.D, drop(f, 0, 0), f.st);
    return VITSEG_OK;
}

// seg_head.0 (a10 + a11): the 3x3 conv (+ bias, ReLU) as an implicit GEMM over the token-major map hf, into F
int head_conv_gemm(const Fwd& f) {
    const Shape& s = f.s;
    const int Mp = f.batch * s.Np, D = s.D;
    GemmArgs g{};
    g.A = f.hf; g.W = wg(f, VITSEG_T_HEAD0_W); g.bias = wt(f, VITSEG_T_HEAD0_B); g.C = f.F;
    g.M = Mp; g.N = MID; g.K = 9 * D; g.lda = 0; g.ldc = MID;
    g.g = s.g; g.Np = s.Np; g.D = D;
    g.zeros = f.zeros;
    if (f.h16) {
        hipError_t e = hipMemsetAsync((void*)f.zeros, 0, 256, f.st);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(zero page)");
    }
    ProfScope ps(f.prof.conv3, 2.0 * g.M * g.N * g.K, f.st);
    if (f.conv_dma && !f.h16 && !f.x3 && D % 32 == 0 && opt(OPT_CONV_DMA) && (size_t)(Mp + 128) * D * 4 < 0x7fffffffull) {
        // (switch conv_dma, off by default) fp32: the same fmaf chain per output (k = (ky, kx, d): bit-identical to the
        // implicit GEMM) with the operands through the LDS-DMA ring of gemm_f32s -- taps outside the image are out-of-range
        // offsets that read as zeros.  Measured at the headline size (profiles/r05_notes.md): 0.94 -> 0.85 ms per forward,
        // but 1 794 MB of L2 misses per launch against 978 MB: nine taps x two 128-column tiles re-read the map through
        // the Infinity Cache.  Not the default: more traffic for 0.2 % of the step.
        SGemm c{};
        c.A = (const float*)f.hf; c.W = wt(f, VITSEG_T_HEAD0_W); c.bias = wt(f, VITSEG_T_HEAD0_B); c.C = f.F;
        c.M = Mp; c.N = MID; c.K = D; c.lda = D; c.ldw = 9 * D; c.ldc = MID; c.splits = 1;
        c.g = s.g; c.Np = s.Np;
        return launch_gemm_f32s(c, SE_RELU, SA_CONV3_ALL, f.st);
    }
    return f.h16 ? launch_gemm_bf16(g, A_CONV3, EPI_RELU, f.st, f.h16 == 2) : launch_gemm_f32(g, A_CONV3, EPI_RELU, f.st, f.x3);
}

// seg_head.2 (the 1x1 conv on F) into the low-res logits Z
int head_1x1(const Fwd& f) {
    const Shape& s = f.s;
    const size_t Mp = (size_t)f.batch * s.Np;
    ProfScope ps(f.prof.head1x1, (double)Mp * MID * 4 + (double)f.batch * s.C * s.Np * 4, f.st);
    return launch_head1x1(f.F, wt(f, VITSEG_T_HEAD2_W), wt(f, VITSEG_T_HEAD2_B), f.Z, f.batch, s.Np, s.C, f.st);
}

// bilinear upsample (+ sigmoid -> argmax) (a12 + a14) into whichever outputs were asked for
int upsample(const Fwd& f) {
    const Shape& s = f.s;
    if (!f.logits && !f.mask) return VITSEG_OK;
    const double px = (double)f.batch * s.S * s.S;
    ProfScope ps(f.prof.upsample, (f.logits ? px * s.C * 4 : 0.0) + (f.mask ? px : 0.0) + (double)f.batch * s.C * s.Np * 4, f.st);
    return launch_upsample(f.Z, f.logits, f.mask, f.batch, s.C, s.g, s.S, f.st);
}

}  // namespace

// ---- the large-batch route: the GEMM router (gemm_dispatch.hip) and its tile kernels (fp32 / fp32x3 / 16-bit operands), LayerNorm launches of their own ----
int walk_large(const Fwd& f) {
    const Shape& s = f.s;
    const int Mp = f.batch * s.Np, Mt = Mp + f.batch, D = s.D, I = s.I;
    hipStream_t st = f.st;
    int rc;
    // 16-bit modes: the image and the patch weights are fp32 either way; the split-operand kernel (fp32-grade products on
    // the fp16 pipe) does this GEMM in 0.16 ms instead of 0.36 ms
    if ((rc = embed_gemm(f, f.layer(0).xin, f.h16 ? 1 : f.x3))) return rc;
    const int thin_rows = f.thin_rows ? thin_cls_rows(Mp, f.batch) : 0;
    auto gemm = [&](const void* A, int w, int b, int l, const float* R, void* C, int N, int K, int epi, int kind,
                    DropArgs dr = DropArgs{}, void* aux = nullptr) {
        GemmArgs g{};
        g.A = A; g.W = wg(f, w, l); g.bias = wt(f, b, l); g.R = R; g.C = C; g.aux = aux; g.drop = dr;
        g.M = Mt; g.N = N; g.K = K; g.lda = K; g.ldc = N;
        if (f.whole_split || thin_rows) {
            g.thin_rows = thin_rows;
            g.thin_scratch = f.scratch;
            g.thin_capacity = f.scratch_floats;
        }
        ProfScope ps(kind, 2.0 * g.M * g.N * g.K, st);
        if (f.fc1_train && epi == EPI_GELU) return launch_gemm_bf16_train(g, EPI_GELU, st);
        return f.h16 ? launch_gemm_bf16(g, A_PLAIN, epi, st, f.h16 == 2) : launch_gemm_f32(g, A_PLAIN, epi, st, f.x3);
    };
    auto lnorm = [&](const float* X, int w, int b, int l, void* H, int rows) {
        ProfScope ps(f.prof.ln, (double)rows * D * (f.h16 ? 6 : 8), st);
        return launch_layernorm(X, wt(f, w, l), wt(f, b, l), H, rows, D, f.eps, f.h16, st);
    };
    const bool mlp1 = f.prof.mlp_one_scope;
    for (int l = 0; l < s.L; ++l) {
        const LayerIO io = f.layer(l);
        if ((rc = lnorm(io.xin, VITSEG_T_LN1_W, VITSEG_T_LN1_B, l, io.h1, Mt))) return rc;
        if ((rc = gemm(io.h1, VITSEG_T_WQKV, VITSEG_T_BQKV, l, nullptr, io.qkv, 3 * D, D, EPI_BIAS, f.prof.qkv))) return rc;
        {
            ProfScope ps(f.prof.attn, 4.0 * f.batch * s.A * (double)s.N * s.N * 64, st);
            const DropArgs dr = drop(f, l, 1);
            if (io.dropw && (rc = launch_attn_dropmask((unsigned*)io.dropw, f.batch, s.Np, s.A, dr, st))) return rc;
            rc = f.h16 ? launch_attention_bf16(io.qkv, io.ctx, io.lse, f.batch, s.Np, s.A, dr, st, f.h16 == 2, io.dropw)
                       : launch_attention_f32((const float*)io.qkv, (float*)io.ctx, io.lse, f.batch, s.Np, s.A, dr, st, f.x3 != 0);
            if (rc) return rc;
        }
        if ((rc = gemm(io.ctx, VITSEG_T_WO, VITSEG_T_BO, l, io.xin, io.xmid, D, D, EPI_RESADD, f.prof.oproj, drop(f, l, 2))))
            return rc;
        if ((rc = lnorm(io.xmid, VITSEG_T_LN2_W, VITSEG_T_LN2_B, l, io.h2, Mt))) return rc;
        ProfScope ps(mlp1 ? f.prof.fc1 : -1, 4.0 * Mt * D * I, st);
        if ((rc = gemm(io.h2, VITSEG_T_W1, VITSEG_T_B1, l, nullptr, io.uact, I, D, EPI_GELU, mlp1 ? -1 : f.prof.fc1, DropArgs{},
                       io.upre)))
            return rc;
        if ((rc = gemm(io.uact, VITSEG_T_W2, VITSEG_T_B2, l, io.xmid, io.xout, D, I, EPI_RESADD, mlp1 ? -1 : f.prof.fc2,
                       drop(f, l, 3))))
            return rc;
    }
    // the final LayerNorm on the patch rows only (CLS is dropped, classes.py:250)
    if ((rc = lnorm(f.layer(s.L - 1).xout, VITSEG_T_LNF_W, VITSEG_T_LNF_B, 0, f.hf, Mp))) return rc;
    if ((rc = head_conv_gemm(f)) || (rc = head_1x1(f))) return rc;
    return upsample(f);
}

// ---- the small-batch route (small.hpp): fewer than small_max_rows() token rows ---------------------------------------
// 7 launches per layer: QKV GEMM (+bias) | attention | o_proj chunks | chunk sum + bias + residual + LayerNorm |
// fc1 GEMM (+bias, GELU) | fc2 chunks | chunk sum + bias + residual + the next LayerNorm.
// h16 (inference, VITSEG_BF16 / VITSEG_F16): the four linears of every block multiply 16-bit operands (weights from the 16-bit
// arena, LayerNorm output / attention context / MLP hidden written in that format by their producers) on the wide MFMA of the
// same kernels, the attention products too (q, k, P, v rounded in registers, fp32 softmax); the residual stream, q | k | v as
// stored, the patch embedding and the head stay fp32.
// Training keeps every block's input, dropout applied by the rows kernels (hidden dropout) and the attention kernels.
int walk_small(const Fwd& f) {
    const Shape& s = f.s;
    const int Mp = f.batch * s.Np, Mt = Mp + f.batch, D = s.D;
    hipStream_t st = f.st;
    float* part = f.scratch;
    const size_t dstride = (size_t)Mt * D;   // slab stride of the D-wide chunk sums
    int rc;
    auto linear = [&](const void* A, int K, int w, int b, int l, void* C, int N, int epi, void* aux, int kind) {
        SGemm g{};
        g.A = (const float*)A; g.W = (const float*)wg(f, w, l); g.bias = wt(f, b, l); g.C = (float*)C; g.aux = (float*)aux;
        g.h16 = f.h16;   // (A is 16-bit too: its producer wrote it so)
        g.M = Mt; g.N = N; g.K = K; g.lda = K; g.ldw = K; g.ldc = N;
        g.splits = epi == SE_PARTIAL ? small_splits(N, K) : 1;
        g.split_stride = dstride;
        ProfScope ps(kind, 2.0 * g.M * g.N * g.K, st);
        return launch_gemm_f32s(g, epi, SA_PLAIN, st);
    };
    // X = Xres + dropout(chunk sums + bias) (embed: the position embedding and the CLS rows instead of Xres), then the
    // LayerNorm of rows [0, ln_rows) into H in format h_fmt
    auto rows = [&](float* X, const float* Xres, int splits, const float* bias, DropArgs dr, int lnw, int lnb, int ln_layer,
                    void* H, int ln_rows, int h_fmt, bool embed) {
        SRows r{};
        r.h_fmt = h_fmt;
        r.X = X; r.Xres = Xres == X ? nullptr : Xres; r.partial = part; r.split_stride = dstride; r.splits = splits;
        r.bias = bias; r.drop = dr;
        r.pos = f.pos; r.cls = wt(f, VITSEG_T_CLS); r.lnw = wt(f, lnw, ln_layer); r.lnb = wt(f, lnb, ln_layer); r.H = (float*)H;
        r.rows = Mt; r.Mp = Mp; r.Np = s.Np; r.D = D; r.ln_rows = ln_rows; r.embed = embed ? 1 : 0;
        r.eps = f.eps;
        ProfScope ps(f.prof.ln, (double)Mt * D * 4 * (2 + splits) + (double)ln_rows * D * 4, st);
        return launch_resln(r, st);
    };
    // ---- embeddings (a2 + a3): patch projection chunks, then bias + position embedding + CLS rows + dropout + LayerNorm 1
    // of layer 0 (patch sizes the gathering DMA does not cover -- P = 4: 48 values per patch -- take the large-batch
    // route's launches)
    const LayerIO io0 = f.layer(0);
    if ((s.P == 8 || s.P == 16 || s.P == 32) && s.Kp % 32 == 0) {
        SGemm g{};
        g.A = f.x; g.W = wt(f, VITSEG_T_PATCH_W); g.C = part;
        g.M = Mp; g.N = D; g.K = s.Kp; g.lda = 0; g.ldw = s.Kp; g.ldc = D;
        g.splits = small_splits(D, s.Kp); g.split_stride = dstride;
        g.g = s.g; g.Np = s.Np; g.S = s.S; g.P = s.P; g.Cin = s.Cin;
        {
            ProfScope ps(f.prof.patch, 2.0 * g.M * g.N * g.K, st);
            if ((rc = launch_gemm_f32s(g, SE_PARTIAL, SA_PATCH, st))) return rc;
        }
        if ((rc = rows(io0.xin, nullptr, g.splits, wt(f, VITSEG_T_PATCH_B), drop(f, 0, 0), VITSEG_T_LN1_W, VITSEG_T_LN1_B, 0,
                       io0.h1, Mt, f.h16, true)))
            return rc;
    } else {
        if ((rc = embed_gemm(f, io0.xin, 0))) return rc;
        ProfScope ps(f.prof.ln, (double)Mt * D * 8, st);
        if ((rc = launch_layernorm(io0.xin, wt(f, VITSEG_T_LN1_W), wt(f, VITSEG_T_LN1_B), io0.h1, Mt, D, f.eps, f.h16, st)))
            return rc;
    }
    for (int l = 0; l < s.L; ++l) {
        const LayerIO io = f.layer(l);
        if ((rc = linear(io.h1, D, VITSEG_T_WQKV, VITSEG_T_BQKV, l, io.qkv, 3 * D, SE_BIAS, nullptr, f.prof.qkv))) return rc;
        {
            ProfScope ps(f.prof.attn, 4.0 * f.batch * s.A * (double)s.N * s.N * 64, st);
            // by the SHAPE only (a row's bits must not depend on the batch): the key-split kernel for the lengths f.attn_small
            // names, attention_f32 for the others (small.hpp attn_small_infer / attn_small_train)
            // (the 16-bit form of the route exists for the key-split kernel's lengths only: small_applies)
            const DropArgs dr = drop(f, l, 1);
            rc = f.attn_small(s.Np) ? launch_attention_small((const float*)io.qkv, (float*)io.ctx, f.batch, s.Np, s.A, st, io.lse, dr, f.h16)
                                    : launch_attention_f32((const float*)io.qkv, (float*)io.ctx, io.lse, f.batch, s.Np, s.A, dr, st);
            if (rc) return rc;
        }
        if ((rc = linear(io.ctx, D, VITSEG_T_WO, VITSEG_T_BO, l, part, D, SE_PARTIAL, nullptr, f.prof.oproj))) return rc;
        if ((rc = rows(io.xmid, io.xin, small_splits(D, D), wt(f, VITSEG_T_BO, l), drop(f, l, 2), VITSEG_T_LN2_W, VITSEG_T_LN2_B, l,
                       io.h2, Mt, f.h16, false)))
            return rc;
        if ((rc = linear(io.h2, D, VITSEG_T_W1, VITSEG_T_B1, l, io.uact, s.I, SE_GELU, io.upre, f.prof.fc1))) return rc;
        if ((rc = linear(io.uact, s.I, VITSEG_T_W2, VITSEG_T_B2, l, part, D, SE_PARTIAL, nullptr, f.prof.fc2))) return rc;
        // the final LayerNorm covers the patch rows only (CLS is dropped, classes.py:250) and writes fp32 (the head reads fp32)
        const bool last = l + 1 == s.L;
        if ((rc = last ? rows(io.xout, io.xmid, small_splits(D, s.I), wt(f, VITSEG_T_B2, l), drop(f, l, 3), VITSEG_T_LNF_W,
                              VITSEG_T_LNF_B, 0, f.hf, Mp, 0, false)
                       : rows(io.xout, io.xmid, small_splits(D, s.I), wt(f, VITSEG_T_B2, l), drop(f, l, 3), VITSEG_T_LN1_W,
                              VITSEG_T_LN1_B, l + 1, f.layer(l + 1).h1, Mt, f.h16, false)))
            return rc;
    }
    // ---- seg_head (a10 + a11)
    if (f.head_one_chain) {
        if (D % 32 == 0) {   // the implicit GEMM's chain per output on 32-row tiles (more blocks for the 216 dependent K steps)
            SGemm g{};
            g.A = (const float*)f.hf; g.W = wt(f, VITSEG_T_HEAD0_W); g.bias = wt(f, VITSEG_T_HEAD0_B); g.C = f.F;
            g.M = Mp; g.N = MID; g.K = D; g.lda = D; g.ldw = 9 * D; g.ldc = MID; g.splits = 1;
            g.g = s.g; g.Np = s.Np;
            ProfScope ps(f.prof.conv3, 2.0 * g.M * g.N * 9 * g.K, st);
            rc = launch_gemm_f32s(g, SE_RELU, SA_CONV3_ALL, st);
        } else {
            rc = head_conv_gemm(f);
        }
        if (rc || (rc = head_1x1(f))) return rc;
    } else {   // the 3x3 conv as nine shifted GEMMs (one tap per chunk), then ReLU + the 1x1 conv
        SGemm g{};
        g.A = (const float*)f.hf; g.W = wt(f, VITSEG_T_HEAD0_W); g.C = part;
        g.M = Mp; g.N = MID; g.K = D; g.lda = D; g.ldw = 9 * D; g.ldc = MID;
        g.splits = 9; g.split_stride = (size_t)Mp * MID;
        g.g = s.g; g.Np = s.Np;
        {
            ProfScope ps(f.prof.conv3, 2.0 * g.M * g.N * 9 * g.K, st);
            if ((rc = launch_gemm_f32s(g, SE_PARTIAL, SA_CONV3, st))) return rc;
        }
        ProfScope ps(f.prof.head1x1, (double)Mp * MID * 4 * 9 + (double)f.batch * s.C * s.Np * 4, st);
        if ((rc = launch_headfin(part, g.split_stride, wt(f, VITSEG_T_HEAD0_B), wt(f, VITSEG_T_HEAD2_W), wt(f, VITSEG_T_HEAD2_B),
                                 f.Z, f.batch, s.Np, s.C, st)))
            return rc;
    }
    return upsample(f);
}

// The small route's slab floats: the D-wide K-chunk slabs of o_proj / fc2 / the patch embedding (forward) or of the o_proj /
// fc1 / QKV input gradients (backward), and the nine tap slabs of the 3x3 head conv (inference: its output; the training
// backward: its input gradient -- the training forward takes the conv as one chain)
size_t small_slab_floats(const Shape& s, size_t Mt, size_t Mp, SmallRole role) {
    size_t n = 0;
    auto need = [&](size_t v) { n = v > n ? v : n; };
    auto slabs = [&](int K) { return (size_t)small_splits(s.D, K) * Mt * s.D; };
    need(slabs(s.D));
    need(slabs(s.I));
    if (role == SMALL_TRAIN_BWD) {
        need(slabs(3 * s.D));
        need((size_t)9 * Mp * s.D);
    } else {
        need(slabs(s.Kp));
        if (role == SMALL_INFER) need((size_t)9 * Mp * MID);
    }
    return n;
}

}  // namespace vitseg
