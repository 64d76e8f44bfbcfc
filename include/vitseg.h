/*
 * vitseg.h -- C ABI of libvitseg.so: the MI355X (gfx950) implementation of the
 * ViT-encoder + conv-segmentation-head hot path of mtumalan/VisionTransformer.
 *
 * The reference has no FFI of its own (it is pure Python on PyTorch); its
 * boundary for this path is the Python class surface
 *     ViTSegmentationModel.__init__/forward      /root/reference/model/CE/classes.py:221-262
 *     LightningViTModel.training_step/...        /root/reference/model/CE/classes.py:264-297
 *     inference post-processing                  /root/reference/model/CE/testViTModel.py:119-126
 * Every entry point below replaces the arithmetic behind one of those calls;
 * the Python mirror of the class surface lives in visiontransformer_amd/ and
 * binds these symbols with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *  - plain C types only; no exceptions cross the boundary.
 *  - every function returns 0 on success or a negative VITSEG_E* code; a
 *    human-readable message is kept per thread (vitseg_last_error()).
 *  - the caller owns ALL device memory (parameters, activations, workspace).
 *    No hipMalloc/hipFree/synchronise happens inside a call; all work is
 *    enqueued on the `stream` argument (a hipStream_t passed as void*).
 *  - parameters live in ONE fp32 arena whose layout this library defines
 *    (vitseg_param_offset); data pointers must be 16-byte aligned.
 *  - token rows inside the workspace are laid out "patches first":
 *    row b*Np + t for patch token t of image b, row B*Np + b for the CLS token.
 */
#ifndef VITSEG_H
#define VITSEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VITSEG_VERSION 110 /* 0.1.1: vitseg_op_attention_bwd_bf16 gained dbias_qkv and a larger scratch (round 4); the
                              small-batch ops (round 5).  Bindings should compare vitseg_version() with the header they were
                              written against. */

enum vitseg_status {
    VITSEG_OK = 0,
    VITSEG_EINVAL = -1,     /* bad argument / null pointer / misalignment */
    VITSEG_ESHAPE = -2,     /* shape the reference would reject (ValueError) or this build cannot run */
    VITSEG_EWORKSPACE = -3, /* workspace too small */
    VITSEG_EHIP = -4        /* a HIP runtime call / launch failed */
};

/* Constructor arguments of ViTSegmentationModel (classes.py:222) + the values
 * the reference hard-codes in its ViTConfig (classes.py:224-235). */
typedef struct vitseg_config {
    int32_t num_classes;       /* C */
    int32_t patch_size;        /* P  (multiple of 4) */
    int32_t hidden_size;       /* D  (multiple of 4) */
    int32_t num_layers;        /* L */
    int32_t num_heads;         /* A;  D / A must be 64 in this build */
    int32_t image_size;        /* S  (reference: 224) */
    int32_t intermediate_size; /* I  (reference: 3072; multiple of 4; a multiple of 64 for VITSEG_BF16 /
                                * VITSEG_F16, whose GEMMs step K in 64-value slices: other values give VITSEG_ESHAPE
                                * from vitseg_query_workspace, vitseg_train_workspace and every entry point) */
    int32_t num_channels;      /* 3 */
    float layer_norm_eps;      /* 1e-12, configuration_vit.py:58; any finite value >= 0 (timm checkpoints: 1e-6), else VITSEG_EINVAL */
} vitseg_config;

/* Parameter tensors, in arena order.  Per-layer tensors take a layer index. */
enum vitseg_tensor {
    VITSEG_T_CLS = 0,   /* [D]            backbone.embeddings.cls_token */
    VITSEG_T_POS,       /* [N, D]         backbone.embeddings.position_embeddings (row 0 = CLS) */
    VITSEG_T_PATCH_W,   /* [D, 3*P*P]     ...patch_embeddings.projection.weight, K order (c,py,px) */
    VITSEG_T_PATCH_B,   /* [D] */
    VITSEG_T_LN1_W,     /* [D]            layers.i.layernorm_before */
    VITSEG_T_LN1_B,
    VITSEG_T_WQKV,      /* [3D, D]        rows: q_proj, k_proj, v_proj weights stacked */
    VITSEG_T_BQKV,      /* [3D] */
    VITSEG_T_WO,        /* [D, D]         attention.o_proj */
    VITSEG_T_BO,
    VITSEG_T_LN2_W,     /* [D]            layernorm_after */
    VITSEG_T_LN2_B,
    VITSEG_T_W1,        /* [I, D]         mlp.fc1 */
    VITSEG_T_B1,
    VITSEG_T_W2,        /* [D, I]         mlp.fc2 */
    VITSEG_T_B2,
    VITSEG_T_LNF_W,     /* [D]            backbone.layernorm */
    VITSEG_T_LNF_B,
    VITSEG_T_HEAD0_W,   /* [256, 3, 3, D] seg_head.0.weight permuted (out, ky, kx, in) */
    VITSEG_T_HEAD0_B,   /* [256] */
    VITSEG_T_HEAD2_W,   /* [C, 256]       seg_head.2.weight */
    VITSEG_T_HEAD2_B,   /* [C] */
    VITSEG_T_COUNT
};

/* Precision of the encoder arithmetic. */
enum vitseg_precision {
    VITSEG_F32 = 0, /* fp32 storage, fp32-input MFMA (exact fmaf chains): the parity path */
    VITSEG_BF16 = 1, /* bf16 operands / fp32 accumulate MFMA, fp32 residual stream and softmax */
    VITSEG_F16 = 2,  /* IEEE-half operands, otherwise as VITSEG_BF16; inference only (BASELINE configs[4]) */
    VITSEG_F32X3 = 3 /* fp32 storage everywhere; GEMM operands split into (hi, lo) half pairs while staged and multiplied
                        with 3 fp16 MFMAs per product (22-bit operand significands, fp32 accumulate); attention,
                        LayerNorm, softmax as VITSEG_F32.  Inference only.  Domain: GEMM / attention operand values
                        must lie inside the half range (|x| < 65504), larger ones become inf and surface as NaN. */
};

/* Workspace buffers whose contents are defined after vitseg_forward returns
 * (used by the parity tests to read intermediate stages). */
enum vitseg_buffer {
    VITSEG_BUF_TOKENS = 0, /* fp32 [B*Np + B, D] residual stream after the last layer */
    VITSEG_BUF_LOWRES,     /* fp32 [B, C, g, g]  low-resolution logits (seg_head output) */
    VITSEG_BUF_COUNT
};

int vitseg_version(void);
const char* vitseg_last_error(void);
/* Dispatcher switches for A/B measurements and tests (which kernel family takes a GEMM, precomputed dropout words on or
 * off, ...): process-wide, read by the launch path with one atomic load.  Names (case-insensitive): no_f32p, no_p8,
 * no_h16p, no_ragged_p8, no_dropmask, dropw_limit_mb, upsample_global, bf16_tiles, f32p_noinl, gn, no_mask2, no_small,
 * small_variant, small_max_rows, conv_dma.  Each starts from the environment variable VITSEG_<NAME> as it was when the library was loaded (the launch
 * path itself never calls getenv): a numeric value is taken as is (VITSEG_NO_P8=0 leaves the switch off), an empty or
 * non-numeric value of an on/off switch means 1.
 * The reference has no counterpart: its dispatch is ATen's. */
int vitseg_set_option(const char* name, long long value);
int vitseg_get_option(const char* name, long long* value);

/* ---- parameter arena (replaces nn.Module parameter storage, classes.py:222-244) ---- */
int vitseg_param_count(const vitseg_config* cfg, size_t* n_floats);
int vitseg_param_offset(const vitseg_config* cfg, int tensor, int layer, size_t* offset_floats, size_t* numel);

/* fp32 arena -> bf16 shadow arena (same offsets, 2 bytes/elt); needed before a VITSEG_BF16 forward. */
int vitseg_cast_params_bf16(const float* params, void* params_bf16, size_t n_floats, void* stream);
/* fp32 arena -> split arena for VITSEG_F32X3 (optional; same size and offsets as the fp32 arena: every 4 values become
 * 4 hi halves | 4 scaled lo halves).  Passed in the params_bf16 slot it spares the GEMMs the weight half of the
 * operand splitting; with NULL there they split the fp32 weights themselves. */
int vitseg_cast_params_split(const float* params, void* params_split, size_t n_floats, void* stream);
/* same for IEEE half (VITSEG_F16); the shadow arena is passed in the params_bf16 slot of vitseg_forward */
int vitseg_cast_params_f16(const float* params, void* params_f16, size_t n_floats, void* stream);

/* Which kernels vitseg_forward takes for a call of this shape (host arithmetic, no GPU work): 1 = the small-batch route (fp32 below
 * 16 384 token rows: the reference's batch 4 x 224x224 and the worker's single image; bf16 / fp16 below 3 200 rows at up to 400
 * tokens, 2 400 at the other key-split lengths), 0 = the large-batch kernels; negative: a vitseg_status.  Results are bit-identical
 * for every batch size INSIDE one route; the two routes sum in different orders (both within the parity gate). */
int vitseg_forward_route(const vitseg_config* cfg, int batch, int precision);
/* ---- forward (replaces ViTSegmentationModel.forward, classes.py:246-262, and the
 *      sigmoid->argmax post-processing of testViTModel.py:122-126) ---- */
int vitseg_query_workspace(const vitseg_config* cfg, int batch, int precision, size_t* bytes);
int vitseg_workspace_offset(const vitseg_config* cfg, int batch, int precision, int buffer, size_t* offset_bytes,
                            size_t* bytes);

/* x: fp32 NCHW [batch, 3, S, S] on device.  logits (fp32 [batch, C, S, S]) and mask
 * (uint8 [batch, S, S], = argmax_c sigmoid(logits), first maximal index) may each be NULL.
 * params_bf16 (the 16-bit shadow arena in the format of `precision`) is only read when precision != VITSEG_F32. */
int vitseg_forward(const vitseg_config* cfg, const float* params, const void* params_bf16, const float* x, int batch,
                   int precision, float* logits, uint8_t* mask, void* workspace, size_t workspace_bytes, void* stream);

/* ---- other input sizes (Hugging Face ViTModel.forward(..., interpolate_pos_encoding=True)) ----
 * The same calls for an input of side image_size_in through the arena of cfg: the arena, its layout
 * (vitseg_param_offset) and its [1 + g0^2, D] position table keep cfg's geometry (g0 = cfg->image_size / P); the
 * activations, x, logits and mask take the input's (S = image_size_in, g1 = S / P).  When g1 != g0 the forward first
 * resamples the table into the workspace (vitseg_pos_interp) and the embeddings add that one; when g1 == g0 every call
 * here is exactly its plain form (same workspace size and offsets, same launches, same bits).  image_size_in must be a
 * positive multiple of P whose derived configuration passes the usual checks (VITSEG_ESHAPE otherwise).
 * vitseg_forward_route takes a cfg whose image_size is the input's: the route depends on the activations only. */
int vitseg_query_workspace_at(const vitseg_config* cfg, int image_size_in, int batch, int precision, size_t* bytes);
int vitseg_workspace_offset_at(const vitseg_config* cfg, int image_size_in, int batch, int precision, int buffer,
                               size_t* offset_bytes, size_t* bytes);
int vitseg_forward_at(const vitseg_config* cfg, int image_size_in, const float* params, const void* params_bf16,
                      const float* x, int batch, int precision, float* logits, uint8_t* mask, void* workspace,
                      size_t workspace_bytes, void* stream);
/* The resampling on its own: pos_out [1 + g1^2, D] from pos_in [1 + g0^2, D] -- row 0 (CLS) copied, the g0 x g0 grid
 * through F.interpolate(size=(g1, g1), mode="bicubic", align_corners=False) per channel (A = -0.75, taps clamped to the
 * grid), each output summed in a fixed order.  vitseg_pos_interp_bwd is its adjoint: dpos_in [1 + g0^2, D] (overwritten)
 * from dpos_out [1 + g1^2, D], two separable passes (x, then y) through scratch (>= g1 * g0 * D floats), no atomics:
 * reproducible bit for bit. */
int vitseg_pos_interp(const float* pos_in, float* pos_out, int g0, int g1, int D, void* stream);
int vitseg_pos_interp_bwd(const float* dpos_out, float* dpos_in, float* scratch, int g0, int g1, int D, void* stream);

/* ---- single-operator entry points (same kernels the forward uses; exported so each
 *      stage can be checked against the oracle in isolation) ---- */
int vitseg_op_layernorm_f32(const float* x, const float* w, const float* b, float* y, int rows, int D, float eps,
                            void* stream);
/* C[M,N] = epi(A[M,K] . W[N,K]^T + bias); epi: 0 none, 1 erf-GELU, 2 + R[M,N] (R may alias C), 3 ReLU */
int vitseg_op_linear_f32(const float* A, const float* W, const float* bias, const float* R, float* C, int M, int N,
                         int K, int epilogue, void* stream);
/* the same with the training forms of the fp32 forward: aux (optional, epilogue 1) receives the pre-activation
 * A.W^T + bias; dropout_p > 0 (epilogue 2): C = R + dropout(A.W^T + bias) with the counter-based mask of
 * (dropout_seed, dropout_stream, row, column), as vitseg_forward_train applies it (reference: hidden dropout,
 * transformers/models/vit/modeling_vit.py:276,283). */
int vitseg_op_linear_f32_ex(const float* A, const float* W, const float* bias, const float* R, float* C, float* aux,
                            int M, int N, int K, int epilogue, float dropout_p, uint32_t dropout_seed,
                            uint32_t dropout_stream, void* stream);
/* qkv: [B*Np + B, 3*A*64] rows as in the workspace; ctx: [B*Np + B, A*64] */
int vitseg_op_attention_f32(const float* qkv, float* ctx, int batch, int num_patches, int num_heads, void* stream);
/* ---- the small-batch fp32 route (fewer than 2048 token rows per forward; vitseg_forward takes it by itself) ----
 * One linear layer as that route computes it.  The reduction is cut into vitseg_small_splits(N, K) chunks -- a function of
 * the layer's shape only, so an output's bits do not depend on M -- each chunk one fp32 fmaf chain, the chunk sums added in
 * chunk order, then the bias.
 * epilogue 0 / 1 (bias / bias + exact GELU; needs vitseg_small_splits(N, K) == 1): C[M, N] written directly.
 * vitseg_op_linear_resln_f32_small (the o_proj / fc2 step of a pre-LN block, modeling_vit.py:266-286): chunk slabs into
 * `scratch` (>= vitseg_small_splits(N, K) * M * N floats), then ONE row kernel: X += chunk sums + bias (in place),
 * H = LayerNorm(X; lnw, lnb, eps). */
int vitseg_small_splits(int N, int K);
int vitseg_op_linear_f32_small(const float* A, const float* W, const float* bias, float* C, int M, int N, int K, int epilogue,
                               void* stream);
int vitseg_op_linear_resln_f32_small(const float* A, const float* W, const float* bias, float* X, const float* lnw,
                                     const float* lnb, float* H, float* scratch, size_t scratch_floats, int M, int N, int K,
                                     float eps, void* stream);
/* the activation gradient of a linear layer as the small-batch training step computes it (the reference trains at batch 4 x
 * 224x224, model/CE/trainCurrentViTmodel.py:57):  dX[M, Kd] = dY[M, Nd] . W[Nd, Kd]  with the nn.Linear weight read as it lies
 * (the reduction runs down its rows).  epilogue 0: plain (K-chunk slabs in `scratch`, >= vitseg_small_splits(Kd, Nd) * M * Kd
 * floats, summed in chunk order); epilogue 5: dX *= gelu'(R) with R[M, Kd] the saved pre-activation (the wide form). */
int vitseg_op_dgrad_f32_small(const float* dY, const float* W, const float* R, float* dX, float* scratch, size_t scratch_floats,
                              int M, int Nd, int Kd, int epilogue, void* stream);
/* ... and its weight gradient  dW[Nd, Kd] = dY[M, Nd]^T . X[M, Kd]  (both operands token-major as they lie; the M token rows are
 * the reduction, one fp32 fmaf chain in row order) */
int vitseg_op_wgrad_f32_small(const float* dY, const float* X, float* dW, int M, int Nd, int Kd, void* stream);
/* diagnostics: vitseg_op_linear_f32_small with per-block time stamps written by the kernel (8 words per block: s_memrealtime
 * at entry / exit, s_memtime at entry / after the prologue / after the K loop / at exit, HW_ID, XCC_ID; `stamps` must hold
 * 8 words per launched block) and `lds_pad` extra bytes of LDS per block (limits the blocks per CU).  tools/small_stamps.py. */
int vitseg_dbg_linear_f32_small(const float* A, const float* W, const float* bias, float* C, int M, int N, int K, int epilogue,
                                unsigned long long* stamps, int lds_pad, void* stream);
/* the 16-bit form of that route's linears (vitseg_forward takes it for VITSEG_BF16 / VITSEG_F16 below 16 384 token rows when the
 * sequence length is one of the key-split attention kernel's): A [M, K] and W [N, K] as raw bf16 (f16 = 0) or IEEE half bits, the
 * same kernels on v_mfma_f32_32x32x16_*, fp32 accumulate.  epilogue 0: C fp32 = acc + bias; 1: C 16-bit = gelu(acc + bias) (the
 * next GEMM's operand); 2 (any shape): the vitseg_small_splits(N, K) chunk slabs into scratch, C fp32 = chunk sums in chunk order
 * + bias (scratch: (splits + 1) * M * N floats). */
int vitseg_op_linear_h16_small(const void* A, const void* W, const float* bias, void* C, int M, int N, int K, int epilogue, int f16,
                               float* scratch, size_t scratch_floats, void* stream);
/* attention core for short sequences (same arguments and layout as vitseg_op_attention_f32) */
int vitseg_op_attention_f32_small(const float* qkv, float* ctx, int batch, int num_patches, int num_heads, void* stream);
/* its 16-bit form (what the route runs under VITSEG_BF16 / VITSEG_F16): fp32 q | k | v in; q, k, the probabilities and v rounded
 * to bf16 (f16 = 0) or IEEE half in registers and multiplied on v_mfma_f32_32x32x16_*, fp32 accumulate and softmax; ctx16
 * [Mt, D] written as 16-bit values (o_proj's operand) */
int vitseg_op_attention_h16_small(const float* qkv, void* ctx16, int batch, int num_patches, int num_heads, int f16, void* stream);
/* bf16 operands (A, W as raw bf16 bits), fp32 accumulate; bias and R fp32.  C is bf16 for epilogues 0/1
 * (tensors that feed the next MFMA) and fp32 for epilogue 2 (the residual stream). */
int vitseg_op_linear_bf16(const void* A, const void* W, const float* bias, const float* R, void* C, int M, int N,
                          int K, int epilogue, void* stream);
int vitseg_op_attention_bf16(const void* qkv, void* ctx, int batch, int num_patches, int num_heads, void* stream);
/* fp32 in / fp32 out through the split-operand fp16 MFMA path of VITSEG_F32X3 (same arguments as linear_f32) */
int vitseg_op_linear_f32x3(const float* A, const float* W, const float* bias, const float* R, float* C, int M, int N,
                           int K, int epilogue, void* stream);
int vitseg_op_attention_f32x3(const float* qkv, float* ctx, int batch, int num_patches, int num_heads, void* stream);
/* IEEE-half variants of the two above (operands as raw fp16 bits) */
int vitseg_op_linear_f16(const void* A, const void* W, const float* bias, const float* R, void* C, int M, int N, int K,
                         int epilogue, void* stream);
int vitseg_op_attention_f16(const void* qkv, void* ctx, int batch, int num_patches, int num_heads, void* stream);
/* The 16-bit linear layer with every epilogue / dispatch option the training path uses (exported so the parity
 * tests can reach each shape-selected tile variant): epilogue 0 bias, 1 bias+GELU (aux != NULL: also stores
 * gelu'(pre-activation) in the 16-bit format -- what the backward multiplies by), 2 residual R fp32 [M,N] +
 * dropout(acc + bias) with fp32 output, 5 acc * R with R = that saved 16-bit derivative [M,N].  f16: IEEE half instead of bf16.  thin_rows > 0: the last thin_rows rows (the CLS rows of the
 * patches-first layout) go through the split-K side launch (scratch: fp32 partials).  dropout_p > 0 (epilogue 2):
 * keep(seed, stream, row, col) of csrc/common.hpp, i.e. hidden dropout of modeling_vit.py:276,283. */
int vitseg_op_linear_h16_ex(const void* A, const void* W, const float* bias, const void* R, void* C, void* aux, int M,
                            int N, int K, int epilogue, int f16, int thin_rows, float* scratch, size_t scratch_floats,
                            float dropout_p, uint32_t dropout_seed, uint32_t dropout_stream, float* colsum_out,
                            float* colsum_scratch, void* stream);
/* colsum_out (epilogue 5, bf16; optional): the column sums of C [N] -- the bias gradient the backward needs next -- produced
 * from the GEMM epilogue's per-tile partial sums; colsum_scratch: vitseg_op_colsum_scratch_floats(M, N) floats. */
size_t vitseg_op_colsum_scratch_floats(int M, int N);
/* bf16 weight gradient dW[M,N] (fp32) = dY^T X with dY = [K tokens][M], X = [K tokens][N] bf16 row-major (the form
 * autograd's linear backward meets: both operands lie token-major, the reduction runs over the token rows); split over
 * the token rows, fp32 partials in `scratch` (>= vitseg_op_wgrad_bf16_scratch_floats floats), fixed-order reduce.
 * zeros: >= 256 zero bytes on the device. */
size_t vitseg_op_wgrad_bf16_scratch_floats(int M, int N, int K);
int vitseg_op_wgrad_bf16(const void* dY, const void* X, float* dW, float* scratch, const void* zeros, int M, int N, int K,
                         void* stream);
/* ---- the K-sliced GEMM paths, one entry each so that tests can reach and name them ----
 * vitseg_op_linear_f32_ex with the router's split-K arguments: x3 = 1 multiplies on the split-operand fp16 path (as
 * vitseg_op_linear_f32x3); scratch / scratch_floats: fp32 partials.  With scratch, a GEMM of at most 128 output tiles and
 * K >= 512 runs as a whole on K slices when the scratch holds slices * M * N floats; otherwise thin_rows > 0 sends the last
 * thin_rows (<= 64) rows after a body of whole 128-row tiles through the split-K side launch (K >= 256, K % 32 == 0) when the
 * scratch holds slices * thin_rows * N floats (16 * 64 * N always suffices).  A scratch that is too small is never written:
 * the GEMM runs unsliced. */
int vitseg_op_linear_f32_thin(const float* A, const float* W, const float* bias, const float* R, float* C, float* aux, int M,
                              int N, int K, int epilogue, int x3, int thin_rows, float* scratch, size_t scratch_floats,
                              float dropout_p, uint32_t dropout_seed, uint32_t dropout_stream, void* stream);
/* fp32 weight gradient dW[M,N] = dY^T X with dY = [K tokens][M], X = [K tokens][N] fp32 row-major, split over the token rows:
 * fp32 partials in `scratch` (>= vitseg_op_wgrad_f32_scratch_floats floats), fixed-order reduce.  M and N multiples of 4. */
size_t vitseg_op_wgrad_f32_scratch_floats(int M, int N, int K);
int vitseg_op_wgrad_f32(const float* dY, const float* X, float* dW, float* scratch, int M, int N, int K, void* stream);
/* diagnostics: the number of K slices the router cuts a GEMM with a dense [M, N] output and reduction length K into on one of
 * its sliced paths, 0 where that path does not take the shape (then the GEMM runs unsliced or on another path).  Host
 * arithmetic by the functions the launches call; launches nothing and needs no device (it then assumes 256 compute units).
 * WHOLE_*: the whole-GEMM split of small linears (32-deep K steps for fp32 / x3 operands, 64-deep for 16-bit ones); THIN_*:
 * the side launch of trailing rows (a function of K only); WGRAD_F32: vitseg_op_wgrad_f32; WGRAD_BF16_TT / _P8:
 * vitseg_op_wgrad_bf16 on the 128x128 kernel / on the 8-phase 256x256 kernel -- exactly one of the two is nonzero for a valid
 * shape, following the option no_p8. */
enum vitseg_slices_path {
    VITSEG_SLICES_WHOLE_F32 = 0, VITSEG_SLICES_WHOLE_H16 = 1, VITSEG_SLICES_THIN_F32 = 2, VITSEG_SLICES_THIN_H16 = 3,
    VITSEG_SLICES_WGRAD_F32 = 4, VITSEG_SLICES_WGRAD_BF16_TT = 5, VITSEG_SLICES_WGRAD_BF16_P8 = 6
};
int vitseg_dbg_gemm_slices(int path, int M, int N, int K);
/* lowres fp32 [B, C, g, g] -> logits fp32 [B, C, S, S] and/or mask uint8 [B, S, S] */
int vitseg_op_upsample_argmax(const float* lowres, float* logits, uint8_t* mask, int batch, int C, int g, int S,
                              void* stream);
/* the adjoint (what autograd derives for F.interpolate(..., mode="bilinear", align_corners=False), classes.py:260):
 * grad_logits fp32 [B, C, S, S] -> grad_lowres fp32 [B, C, g, g]; S a multiple of g; deterministic */
int vitseg_op_upsample_bwd(const float* grad_logits, float* grad_lowres, int batch, int C, int g, int S, void* stream);

/* ---- loss (replaces nn.CrossEntropyLoss()(logits, y), classes.py:268,280) ----
 * lowres: fp32 [B, C, g, g] low-resolution logits (VITSEG_BUF_LOWRES after vitseg_forward); target: class
 * indices [B, S, S], int64 (torch.long, as the reference passes them) or uint8.  Writes the mean loss to
 * *loss (device fp32).  scratch: >= vitseg_ce_scratch_bytes() device bytes.  grad_logits (optional, fp32
 * [B, C, S, S]) receives d loss / d logits.  Labels must lie in [0, C); these calls have no ignore_index: a pixel
 * with any other label (uint8 255, int64 -100 or C) makes the loss NaN and gets a NaN gradient (also in
 * vitseg_backward's fused loss).  ignore_index, class weights and label smoothing: the _opts calls below. */
size_t vitseg_ce_scratch_bytes(int batch, int S);
int vitseg_ce_loss(const float* lowres, const void* target, int target_is_u8, float* grad_logits, void* scratch,
                   float* loss, int batch, int C, int g, int S, void* stream);

/* ---- the other constructor arguments of nn.CrossEntropyLoss: F.cross_entropy(up, y, weight=w, ignore_index=ii,
 *      label_smoothing=eps, reduction="mean") on the same regenerated logits ----
 *   keep = (y != ii);  den = sum over kept pixels of w[y];
 *   loss = [ (1 - eps) sum_keep w[y] (lse - z_y) + (eps / C) sum_keep sum_c w[c] (lse - z_c) ] / den
 *   d loss / d z_c = keep [ (1 - eps) w[y] (p_c - 1[c = y]) + (eps / C) (p_c sum_k w[k] - w[c]) ] loss_scale / den
 * den depends on the targets: a count pass over them (fp64 per-block partials, fixed-order reduce, no atomics) leaves it
 * in `scratch` on the device before the loss / gradient kernel runs; the host never reads it.
 *  - a pixel whose label equals ignore_index contributes nothing; its grad_logits entries are written as 0.0f;
 *  - den == 0 (everything ignored, or every kept pixel has weight 0): the loss is NaN, kept pixels get NaN gradients,
 *    ignored pixels 0 -- torch's 0 / 0;
 *  - a label outside [0, C) that is not ignore_index: NaN loss and NaN gradient at that pixel, as in vitseg_ce_loss; it
 *    counts 1 in den, so every other pixel keeps its gradient;
 *  - with has_ignore_index = 0, class_weight = NULL and label_smoothing = 0 the results are bit for bit vitseg_ce_loss's.
 * C <= 255.  VITSEG_EINVAL before any launch: label_smoothing outside [0, 1], scratch NULL / not 8-byte aligned / smaller
 * than vitseg_ce_options_scratch_bytes, a null pointer. */
typedef struct vitseg_ce_options {
    int32_t has_ignore_index;  /* 0: no label is ignored (ignore_index is not read) */
    int32_t reserved;          /* 0 */
    int64_t ignore_index;      /* compared with the label widened to int64: 255 (uint8 void label), -100 (torch's default) */
    const float* class_weight; /* device fp32 [C], finite and >= 0; NULL = all ones */
    float label_smoothing;     /* eps, 0 <= eps <= 1 */
    void* scratch;             /* caller-owned device memory, >= vitseg_ce_options_scratch_bytes(batch, S); every word read
                                  is written within the call */
    size_t scratch_bytes;
} vitseg_ce_options;
size_t vitseg_ce_options_scratch_bytes(int batch, int S);
/* vitseg_ce_loss with the options; loss_scale multiplies grad_logits (not *loss), as in vitseg_backward.  opts == NULL:
 * exactly vitseg_ce_loss (the same launches), with loss_scale applied. */
int vitseg_ce_loss_opts(const float* lowres, const void* target, int target_is_u8, float* grad_logits, void* scratch,
                        float* loss, int batch, int C, int g, int S, const vitseg_ce_options* opts, float loss_scale,
                        void* stream);

/* ---- CE + soft Dice on the same regenerated logits (the region term of the binary trainer's loss, dice_loss of
 *      model/PAED/classes.py:608-620 with smooth 1e-6 flattened over the batch, applied per class to the softmax) ----
 *   up = the bilinear upsample of lowres (the taps and fma placement of vitseg_ce_loss);  p = softmax_c(up);  t = one-hot(y)
 *   keep = (y != ce->ignore_index), every pixel when ce is NULL or has_ignore_index = 0
 *   K = the classes counted: 0 .. C-1, or 1 .. C-1 with include_background = 0 (C >= 2 then)
 *   per class c in K, summed over the kept pixels of the whole batch:
 *     I_c = sum p_c t_c;  P_c = sum p_c;  T_c = sum t_c;  D_c = P_c + T_c + smooth
 *   dice = mean over c in K of [ 1 - (2 I_c + smooth) / D_c ]
 *   loss = ce_weight * CE + dice_weight * dice
 *     CE: what vitseg_ce_loss_opts computes for the same `ce` (vitseg_ce_loss when ce is NULL); class weights and label
 *     smoothing act on CE only, ignore_index on both terms.  ce_weight == 0: the CE term is not formed (no count pass, an
 *     exact 0, never 0 * NaN); dice_weight == 0: the Dice term is not formed (no sum pass) and grad_logits and terms[1]
 *     are, bit for bit, vitseg_ce_loss_opts's.
 *   a_c = -[2 t_c D_c - (2 I_c + smooth)] / (|K| D_c^2) for c in K on kept pixels, else 0
 *   d loss / d up_c = ce_weight * (the CE gradient above) + dice_weight * p_c (a_c - sum_k a_k p_k) * loss_scale
 * The gradient at one pixel depends on sums over the whole batch, so the call is three passes on one stream, no atomics,
 * no host read: a sum pass (the logits regenerated per pixel, fp64 per-block partials of I, P, T: wavefront shuffles, then
 * LDS; one block per 2048 pixels), a fixed-order reduce to 3 C device doubles, and one loss / gradient kernel (one thread
 * per pixel, one store per element of grad_logits); a finish kernel writes terms[3] = {loss, CE, dice} (device fp32; a
 * term that is not formed reads 0).  Results are bitwise reproducible and the same for int64 and uint8 targets.
 *  - a class absent from the targets (T_c = 0) is still counted;
 *  - everything ignored: I = P = T = 0, every dice_c = 1 - smooth / smooth = 0 (NaN when smooth == 0) and the Dice gradient
 *    is 0; CE is NaN as in vitseg_ce_loss_opts, so the total is NaN unless ce_weight == 0;
 *  - ignored pixels get 0.0f for every class, and nothing is read from under them;
 *  - a label outside [0, C) that is not ignore_index poisons the sums: loss, dice and every kept pixel's gradient are NaN.
 * `scratch` (the call's, >= vitseg_ce_scratch_bytes) holds the CE partials; dice->scratch (caller-owned device memory,
 * 8-byte aligned, >= vitseg_dice_options_scratch_bytes(batch, C, S); every word read is written within the call) the sums
 * and their partials.  C <= 255.  VITSEG_EINVAL before any launch: ce_weight, dice_weight or smooth negative or not
 * finite, both weights 0, include_background = 0 with C < 2, dice NULL, dice->scratch NULL / misaligned / too small, the
 * errors of vitseg_ce_loss_opts. */
typedef struct vitseg_dice_options {
    float ce_weight;            /* >= 0, finite */
    float dice_weight;          /* >= 0, finite; not both 0 */
    float smooth;               /* >= 0, finite; the reference's 1e-6 */
    int32_t include_background; /* 0: class 0 is not counted (C >= 2) */
    void* scratch;
    size_t scratch_bytes;
} vitseg_dice_options;
size_t vitseg_dice_options_scratch_bytes(int batch, int C, int S);
int vitseg_ce_dice_loss(const float* lowres, const void* target, int target_is_u8, float* grad_logits, void* scratch,
                        float* terms, int batch, int C, int g, int S, const vitseg_ce_options* ce,
                        const vitseg_dice_options* dice, float loss_scale, void* stream);

/* ---- training (replaces autograd behind LightningViTModel.training_step, classes.py:276-285, and
 *      torch.optim.Adam(lr=1e-5).step(), classes.py:296-297).  dropout_p (the reference trains with 0.1,
 *      classes.py:233-234) is applied at the four sites of HF ViT (embeddings, attention probabilities,
 *      attention output, MLP output) with a counter-based generator: the mask is a pure function of
 *      (dropout_seed, layer, site, element), so the SAME (p, seed) must be passed to vitseg_forward_train
 *      and vitseg_backward of one step; torch's RNG stream cannot be matched.  VITSEG_BF16 = mixed precision:
 *      bf16 MFMA operands (params_bf16 shadow arena, bf16 saved activations), fp32 master parameters,
 *      residual stream, LayerNorm / softmax statistics and gradients.
 * vitseg_forward_train saves every activation the backward needs inside `workspace`
 * (vitseg_train_workspace bytes; it must stay untouched until vitseg_backward has run) and optionally
 * writes the fp32 logits.  vitseg_backward takes EITHER integer targets (fused CE: writes the mean loss to
 * *loss) OR the gradient of an arbitrary loss w.r.t. the logits (fp32 [B, C, S, S]) and fills `grads`, an
 * arena-shaped fp32 buffer (same offsets as the parameters).  loss_scale multiplies the gradient of the fused CE loss
 * at its source (1 / accumulate_grad_batches in a gradient-accumulation loop, what Lightning applies to every micro-batch
 * loss); the value written to *loss is not scaled.
 * Training also needs num_classes <= 32 and hidden_size <= 1024 (the head and LayerNorm backward kernels); outside
 * that, vitseg_train_workspace, vitseg_forward_train and vitseg_backward return VITSEG_ESHAPE before any launch. */
int vitseg_train_workspace(const vitseg_config* cfg, int batch, int precision, size_t* bytes);
int vitseg_forward_train(const vitseg_config* cfg, const float* params, const void* params_bf16, const float* x,
                         int batch, int precision, float dropout_p, uint64_t dropout_seed, float* logits,
                         void* workspace, size_t workspace_bytes, void* stream);
int vitseg_backward(const vitseg_config* cfg, const float* params, const void* params_bf16, const float* x, int batch,
                    int precision, float dropout_p, uint64_t dropout_seed, const void* target, int target_is_u8,
                    const float* grad_logits, float* grads, float* loss, float loss_scale, void* const* bucket_events,
                    void* workspace, size_t workspace_bytes, void* stream);
/* Gradient buckets for overlapping the data-parallel all-reduce with the backward (the reference
 * trains single-process, this replaces what DDP would do behind trainer.fit, trainCurrentViTmodel.py:97-101).
 * The gradient arena splits into vitseg_grad_bucket_count() = L + 2 contiguous ranges in the order the backward
 * finishes them: 0 = final norm + seg_head, 1 .. L = encoder layers L-1 .. 0, L + 1 = embeddings.
 * vitseg_backward records bucket_events[i] (hipEvent_t, created by the caller; NULL array or NULL entries = skip)
 * on `stream` right after the last kernel that writes bucket i, so a communication stream can wait on it and
 * reduce that range while the rest of the backward still runs. */
/* The training calls for an input of side image_size_in (see vitseg_forward_at): the forward adds the resampled table,
 * the backward maps the position-embedding gradient back to the arena's grid (vitseg_pos_interp_bwd) before the
 * embeddings' gradient bucket is recorded; `grads` has the arena's layout.  With image_size_in == cfg->image_size
 * exactly the plain calls. */
int vitseg_train_workspace_at(const vitseg_config* cfg, int image_size_in, int batch, int precision, size_t* bytes);
int vitseg_forward_train_at(const vitseg_config* cfg, int image_size_in, const float* params, const void* params_bf16,
                            const float* x, int batch, int precision, float dropout_p, uint64_t dropout_seed, float* logits,
                            void* workspace, size_t workspace_bytes, void* stream);
int vitseg_backward_at(const vitseg_config* cfg, int image_size_in, const float* params, const void* params_bf16,
                       const float* x, int batch, int precision, float dropout_p, uint64_t dropout_seed, const void* target,
                       int target_is_u8, const float* grad_logits, float* grads, float* loss, float loss_scale,
                       void* const* bucket_events, void* workspace, size_t workspace_bytes, void* stream);
/* vitseg_backward / vitseg_backward_at (image_size_in == cfg->image_size: the plain geometry) whose fused CE loss takes
 * the options of vitseg_ce_loss_opts: ce_options is read by the fused-CE branch (target != NULL) only; together with
 * grad_logits it must be NULL (VITSEG_EINVAL).  ce_options == NULL: exactly the calls above.  The options' scratch is the
 * caller's, so the training workspace keeps its size and layout. */
int vitseg_backward_opts(const vitseg_config* cfg, int image_size_in, const float* params, const void* params_bf16,
                         const float* x, int batch, int precision, float dropout_p, uint64_t dropout_seed, const void* target,
                         int target_is_u8, const float* grad_logits, float* grads, float* loss, float loss_scale,
                         void* const* bucket_events, void* workspace, size_t workspace_bytes, void* stream,
                         const vitseg_ce_options* ce_options);
/* vitseg_backward_opts whose fused loss is vitseg_ce_dice_loss: with `dice` the fused branch (target != NULL) forms
 * ce_weight * CE + dice_weight * dice, writes {loss, CE, dice} to terms[3] (device fp32, required then) and the total to
 * *loss as well; nothing else in the walk changes.  dice == NULL: exactly vitseg_backward_opts (terms is not touched).
 * Together with grad_logits, dice must be NULL (VITSEG_EINVAL).  The Dice scratch is the caller's, so the training
 * workspace keeps its size and layout. */
int vitseg_backward_dice(const vitseg_config* cfg, int image_size_in, const float* params, const void* params_bf16,
                         const float* x, int batch, int precision, float dropout_p, uint64_t dropout_seed, const void* target,
                         int target_is_u8, const float* grad_logits, float* grads, float* loss, float loss_scale,
                         void* const* bucket_events, void* workspace, size_t workspace_bytes, void* stream,
                         const vitseg_ce_options* ce_options, const vitseg_dice_options* dice, float* terms);
int vitseg_grad_bucket_count(const vitseg_config* cfg);
int vitseg_grad_bucket_range(const vitseg_config* cfg, int bucket, size_t* offset_floats, size_t* n_floats);
/* ---- pre-processing (replaces transforms.Resize((S, S)) + transforms.ToTensor() on the PIL image,
 *      trainCurrentViTmodel.py:48-51 / testViTModel.py:92-97, and the mask side Resize(NEAREST) + value->class
 *      remap + F.interpolate(nearest), classes.py:76-83, 273-274).  Bit-exact with Pillow's 8-bit two-pass
 *      antialiased bilinear resampling (libImaging/Resample.c) and with its NEAREST (Geometry.c).
 * Host side (no GPU touched): vitseg_resize_taps = taps per output sample of one axis; vitseg_resize_coeffs fills
 * bounds[out][2] = (first source index, tap count) and kk[out][taps] (22-bit fixed point) for that axis;
 * vitseg_nearest_index fills the source index of every destination sample (mode 0 = Image.resize(NEAREST),
 * 1 = F.interpolate(mode='nearest')).  The caller uploads the tables once per (source size, S).
 * Device side: vitseg_preprocess_u8 turns n RGB images uint8 [n, H, W, 3] into fp32 [n, 3, S, S] in [0, 1];
 * x* tables (and scratch >= n * rows * S * 3 bytes) are needed when W != S, y* tables when H != S;
 * [row_first, row_first + rows) = the source rows the vertical pass touches (ybounds[0][0] .. last bound).
 * vitseg_resize_nearest_u8 gathers uint8 [n, H, W] -> [n, out_h, out_w] through the index tables and an optional
 * 256-entry LUT, writing uint8 or int64 (torch.long targets). */
int vitseg_resize_taps(int in_size, int out_size);
int vitseg_resize_coeffs(int in_size, int out_size, int32_t* bounds, int32_t* kk);
int vitseg_nearest_index(int in_size, int out_size, int mode, int32_t* idx);
int vitseg_preprocess_u8(const uint8_t* img, int n, int H, int W, int S, const int32_t* xbounds, const int32_t* xk, int xksize,
                         const int32_t* ybounds, const int32_t* yk, int yksize, int row_first, int rows, uint8_t* scratch,
                         float* out, void* stream);
int vitseg_resize_nearest_u8(const uint8_t* src, int n, int H, int W, const int32_t* yidx, const int32_t* xidx, int out_h,
                             int out_w, const uint8_t* lut, int out_is_i64, void* out, void* stream);
/* the same gather for int64 class-index maps (torch.long targets): LightningViTModel._resize_target,
 * model/CE/classes.py:273-274 = F.interpolate(y[:, None].float(), size, mode='nearest').long() with the mode-1 tables;
 * writes int64 (the reference's dtype) or uint8 (what vitseg_backward / vitseg_ce_loss read at a quarter of the bytes) */
int vitseg_resize_nearest_i64(const int64_t* src, int n, int H, int W, const int32_t* yidx, const int32_t* xidx, int out_h,
                              int out_w, int out_is_i64, void* out, void* stream);

/* ---- soft PAED loss for C classes (replaces softmax + one_hot + paed_loss_multiclass_soft and its autograd in the
 *      17-class LightningViTModel of model/PAED, classes.py:336-369, 449-478).  logits: fp32 [B, C, H, W]; target:
 *      class indices [B, H, W] (int64 or uint8); sigma = 3 and class_penalty = 1 are the reference's defaults.  Writes
 *      the scalar loss and, when grad_logits != NULL, d loss / d logits (fp32 [B, C, H, W]).  scratch:
 *      vitseg_paed_scratch_bytes() device bytes. */
size_t vitseg_paed_scratch_bytes(int batch, int C, int H, int W);
int vitseg_paed_multiclass_loss(const float* logits, const void* target, int target_is_u8, int batch, int C, int H, int W,
                                float sigma, int class_penalty, void* scratch, float* loss, float* grad_logits, void* stream);

/* ---- loss tail of the binary PAED trainer (replaces sigmoid + F.binary_cross_entropy + dice_loss + paed_loss_soft
 *      and their autograd in PAEDTrainer._forward_step_paed, model/PAED/classes.py:608-701).  logits fp32 [B, 1, H, W];
 *      mask fp32 0/1 [B, H, W] (already resized to the prediction); sdf_ext / sdf_int fp32 [B, sdf_h, sdf_w] (resized
 *      bilinearly on the fly).  out8 (device, 8 floats): loss = bce + 0.1 dice + 5 |paed|, bce, dice, paed, then the
 *      counts tp, fp, fn and #((p > 0.5) == mask) for the trainer's logged metrics.  grad_logits (optional) receives
 *      d loss / d logits.  scratch: vitseg_paed_binary_scratch_bytes() device bytes. */
size_t vitseg_paed_binary_scratch_bytes(int batch, int H, int W);
int vitseg_paed_binary_loss(const float* logits, const float* mask, const float* sdf_ext, const float* sdf_int, int sdf_h,
                            int sdf_w, int batch, int H, int W, void* scratch, float* out8, float* grad_logits,
                            void* stream);

/* ---- evaluation statistics (replaces the per-image numpy loops of datasetTestViTmodel.py:193-219) ----
 * pred: uint8 [n, S, S] class masks; gt: uint8 [n, gt_h, gt_w] label maps, nearest-resized on the fly through
 * yidx/xidx (device tables of S entries each; NULL when the sizes already match).  counts: int64 [n, 3, 256] =
 * per label value |gt == v & pred == v|, |gt == v|, |pred == v|; accuracy, IoU, Dice and the class sets follow from
 * these integers exactly. */
int vitseg_eval_counts(const uint8_t* pred, const uint8_t* gt, int n, int S, int gt_h, int gt_w, const int32_t* yidx,
                       const int32_t* xidx, int64_t* counts, void* stream);

/* ---- connected regions and their boxes (replaces get_bounding_boxes = scipy.ndimage.label + np.argwhere per label, called
 *      for every class present but 0: testViTModel.py:34-42,171-185, datasetTestViTmodel.py:27,315-318,
 *      model/PAED/ViTscriptTest.py:27,318-321) ----
 * A region is a maximal set of equal pixels of one image that is connected: connectivity 4 (the cross, scipy's default
 * structure) or 8 (the full 3x3).  Pixels equal to `background` (0..255; -1 = none) form no region.
 * mask uint8 [n, H, W] (any H, W >= 1, H * W < 2^31);
 * counts int32 [n]: regions per image (the true total, also when > max_regions);
 * regions int32 [n, max_regions, 8]: class, y_min, x_min, y_max, x_max, area, first, 0 -- box inclusive, first = raster
 *   index y * W + x of the region's first pixel; the first max_regions of each image in (class, first) order, which is
 *   the order of the reference's loop (np.unique classes, then scipy's label numbering); rows past the count are zero;
 *   16-byte aligned; may be NULL when max_regions == 0;
 * labels (optional) int32 [n, H, W]: region index in its image's list (full index, also past max_regions), -1 = background
 *   (scipy's label k of mask == c is offset_c + k - 1).
 * scratch: vitseg_regions_scratch_bytes(n, H, W) device bytes (about 24 bytes per pixel; every word read is written
 * within the call).  Results are integers from order-independent operations: the same bits on every call.
 * VITSEG_EINVAL: null pointer, connectivity not 4 / 8, background outside -1..255; VITSEG_ESHAPE: non-positive sizes,
 * H * W >= 2^31 or n > 65535; VITSEG_EWORKSPACE: scratch smaller than vitseg_regions_scratch_bytes (0 for a bad shape). */
size_t vitseg_regions_scratch_bytes(int n, int H, int W);
int vitseg_regions(const uint8_t* mask, int n, int H, int W, int connectivity, int background, int32_t* counts,
                   int32_t* regions, int max_regions, int32_t* labels, void* scratch, size_t scratch_bytes, void* stream);

/* ---- mask clean-up: small regions out, enclosed holes filled (the reference has no counterpart: its get_bounding_boxes
 *      labels the raw argmax; the usual host answer is skimage's remove_small_objects + scipy.ndimage.binary_fill_holes
 *      per class and image) ----
 * mask uint8 [n, H, W] -> out uint8 [n, H, W] (out != mask; mask is never written), two steps in this order:
 *  1. min_area > 1: every region (as above: a maximal `connectivity`-connected set of equal non-background pixels) of
 *     fewer than min_area pixels becomes `background`; a region of exactly min_area pixels stays.  0 and 1 change nothing.
 *  2. fill_holes != 0, on the result of step 1: a hole is a 4-connected component of background pixels that does not
 *     touch the image frame -- 4-connected whatever `connectivity` is (scipy's binary_fill_holes default structure).  A
 *     hole of at most max_hole_area pixels (0 = no limit) whose non-background 4-neighbours all carry one class c is
 *     filled with c; a hole bordered by two or more classes stays background.
 * background 0..255 (-1 is refused: clean-up needs one).
 * stats (optional) int32 [n, 8]: regions_removed, pixels_removed, holes_filled, pixels_filled, holes_mixed (left: two or
 *   more bordering classes), holes_over_area (left: above max_hole_area; a hole both over the limit and mixed counts here
 *   only), 0, 0.
 * scratch: vitseg_clean_scratch_bytes(n, H, W) device bytes (about 28 bytes per pixel; every word read is written within the
 * call).  Everything is an integer from order-independent operations: the same bits on every call, and an image gets the
 * same bits alone as in a batch.
 * Each with nothing launched -- VITSEG_EINVAL: a null mask / out / scratch, out == mask, connectivity not 4 / 8, background
 * outside 0..255, a negative min_area or max_hole_area; VITSEG_ESHAPE: non-positive sizes, H * W >= 2^31 or n > 65535;
 * VITSEG_EWORKSPACE: scratch smaller than vitseg_clean_scratch_bytes (0 for a bad shape). */
size_t vitseg_clean_scratch_bytes(int n, int H, int W);
int vitseg_clean_mask(const uint8_t* mask, uint8_t* out, int n, int H, int W, int connectivity, int background, int min_area,
                      int fill_holes, int max_hole_area, int32_t* stats /* [n, 8] or NULL */, void* scratch,
                      size_t scratch_bytes, void* stream);

/* ---- region-level detection statistics: the regions of a prediction matched against the regions of the ground truth, per
 *      class (the panoptic-quality construction of Kirillov et al. 2019, PQ = SQ * RQ, and coverage hit rates beside it; the
 *      reference draws the predicted regions and compares them with nothing; the usual host answer is scipy.ndimage.label
 *      twice per class and image and a loop over region pairs) ----
 * pred, gt uint8 [n, H, W] class maps; classes: K distinct label values in HOST memory, none of them the background or the
 * ignore label.  Regions are maximal 4- / 8-connected sets of equal pixels that are not `background` (0..255): those of
 * pred are exactly vitseg_regions' on the whole prediction.  ignore_label -1 (none) or 0..255: pixels with gt == ignore_label
 * are void -- they form no true region and count neither in a predicted region's area nor in any intersection; a predicted
 * region with no counted pixel does not exist for the statistics.
 * Per image and class c, P_i the predicted regions of class c, G_j the true ones: a_i = |P_i minus void|, b_j = |G_j|,
 * I_ij = |P_i n G_j|, U_ij = a_i + b_j - I_ij.
 *   match      (i, j) is matched iff I_ij * thr_den > thr_num * U_ij, thr_den / 2 <= thr_num < thr_den <= 1000: at or above
 *              one half a region has at most one partner.
 *   coverage   G_j is found iff |G_j n {pred == c}| * cov_den >= cov_num * b_j, P_i is confirmed iff
 *              |P_i n {gt == c}| * cov_den >= cov_num * a_i, 0 < cov_num <= cov_den <= 1000.
 *   q_ij       floor(I_ij * 2^32 / U_ij): the IoU of a matched pair in fixed point, so that its sum is exact.
 * stats int64 [n, K, 8]: n_gt, n_pred (regions with a_i > 0), tp (matched pairs), gt_found, pred_confirmed, the sums of q,
 *   of I and of U over the matched pairs.  fp = n_pred - tp, fn = n_gt - tp, PQ = (sum q / 2^32) / (tp + fp / 2 + fn / 2).
 * pred_info, gt_info (optional, either may be NULL) int32 [n, H, W, 2]: at the first pixel of every region of a class in
 *   `classes` (of pred: with a_i > 0) the pair (raster index of the matched partner's first pixel or -1, covered pixels);
 *   (-2, 0) at every other pixel.
 * scratch: vitseg_region_match_scratch_bytes(n, H, W) device bytes (about 75 bytes per pixel: the labelling of 2n planes, their
 * staged copy and a pair table of 2 * H * W slots per image; every word read is written within the call).  One enqueue on
 * `stream`, no allocation, no host synchronisation.  Everything is an integer from order-independent operations: the same
 * bits on every call, and an image gets the same bits alone as in a batch.
 * Each with nothing launched -- VITSEG_EINVAL: a null pred / gt / classes / stats / scratch, connectivity not 4 / 8,
 * background outside 0..255, ignore_label outside -1..255, equal to the background or in `classes`, a class outside 0..255,
 * equal to the background or repeated, a threshold outside the ranges above; VITSEG_ESHAPE: non-positive sizes,
 * H * W >= 2^31, n outside 1..32767 (the planes are labelled as a batch of 2n), K outside 1..256; VITSEG_EWORKSPACE: scratch
 * smaller than vitseg_region_match_scratch_bytes (0 for a bad shape). */
size_t vitseg_region_match_scratch_bytes(int n, int H, int W);
int vitseg_region_match(const uint8_t* pred, const uint8_t* gt, int n, int H, int W, const int32_t* classes, int K,
                        int connectivity, int background, int ignore_label, int thr_num, int thr_den, int cov_num,
                        int cov_den, int64_t* stats /* [n, K, 8] */, int32_t* pred_info /* [n, H, W, 2] or NULL */,
                        int32_t* gt_info /* [n, H, W, 2] or NULL */, void* scratch, size_t scratch_bytes, void* stream);

/* ---- exact Euclidean distance transforms and the signed-distance targets of binary masks (replaces
 *      segmentation.compute_sdf = scipy.ndimage.distance_transform_edt of ~mask and of mask, each divided by its maximum,
 *      model/PAED/segmentation.py:6-34, called per item by StructuralDamageDataset, model/PAED/classes.py:51-85) ----
 * mask uint8 [n, H, W]: a non-zero byte is a mask pixel (astype(bool)).  Per image, d2 = the exact squared distance to the
 * nearest feature pixel: the mask pixels for sdf_ext, the other pixels for sdf_int (feature pixels get 0).  An image with no
 * feature pixel for a field gets scipy's result, the distance to the virtual point (-1, 0): d2 = (y + 1)^2 + x^2.
 * sdf_ext, sdf_int float [n, H, W] (either may be NULL: that field is skipped):
 *   normalize = 0: (float) sqrt((double) d2), i.e. distance_transform_edt(~m) and (m) cast to float32;
 *   normalize = 1: that distance / (float) sqrt((double) max d2 of the image and field), IEEE float division, and 0
 *   everywhere when the maximum is 0 -- compute_sdf's result.
 * scratch: vitseg_sdf_scratch_bytes(n, H, W) device bytes (2 words per image; every word read is written within the call).
 * All arithmetic before the final conversion is integer: the same bits on every call, and per image the same bits in any
 * batch.  VITSEG_EINVAL: null mask or scratch, normalize not 0 / 1; VITSEG_ESHAPE: H or W outside 1..16384, n outside
 * 1..65535; VITSEG_EWORKSPACE: scratch smaller than vitseg_sdf_scratch_bytes (0 for a bad shape).  Nothing is launched
 * when a check fails. */
size_t vitseg_sdf_scratch_bytes(int n, int H, int W);
int vitseg_sdf(const uint8_t* mask, int n, int H, int W, int normalize, float* sdf_ext, float* sdf_int, void* scratch,
               size_t scratch_bytes, void* stream);

/* ---- boundary-distance statistics of class maps: the integers and fp64 sums behind PAED (the pixel average Euclidean
 *      distance of model/PAED/classes.py:209-258, there two Python loops over all pixel pairs), the Hausdorff distance, its
 *      percentiles (HD95) and the average symmetric distance ----
 * pred, gt uint8 [n, H, W] class maps of one size; classes: K label values 0..255 in HOST memory.  Per image and class c,
 * A = {gt == c} and P = {pred == c}; mode 0 (sets) takes them whole, mode 1 (borders) first replaces each by
 * S ^ binary_erosion(S) (cross structure, border_value 0: a pixel of S one of whose four neighbours is outside S or outside
 * the image).  d2_P(x) = the exact squared distance from pixel x to the nearest pixel of P.
 * stats_i int64 [n, K, 6] (device): n = |A|, m = |P|, max_d2_AP = max over A of d2_P, max_d2_PA = max over P of d2_A (their
 *   roots are the directed Hausdorff distances), d2_lo, d2_hi = the order statistics lo = pct_num (N - 1) / pct_den (integer
 *   division) and hi = min(lo + 1, N - 1) of the pooled multiset {d2_P(x): x in A} u {d2_A(x): x in P}, N = n + m; the
 *   percentile of the distances is sqrt(d2_lo) + (sqrt(d2_hi) - sqrt(d2_lo)) frac(pct_num (N - 1) / pct_den), as np.percentile.
 * stats_f double [n, K, 2] (device): sumAP = sum over A of sqrt((double) d2_P), sumPA = sum over P of sqrt((double) d2_A).
 * Empty sets (decided on the device): with n == 0 or m == 0 the maxima and order statistics are -1; the sums are 0 in mode 1;
 *   in mode 0 both sums are 0 when both sets are empty, and when one is empty the other's sum is sum sqrt(y^2 + x^2) over its
 *   pixels' (row, column) indices, the reference's rule (classes.py:230-235).
 * scratch: vitseg_distance_scratch_bytes(n, H, W) device bytes (about 10 bytes per pixel of the batch plus histograms and
 * partial sums; every word read is written within the call).  Classes are processed one after another on `stream`; no
 * allocation or synchronisation.  The integers come from order-independent integer operations and the sums are added in an
 * order fixed by H * W: the same bits on every call, and per image the same bits in any batch.
 * VITSEG_EINVAL: null pointer, mode not 0 / 1, a class value outside 0..255, not 0 <= pct_num <= pct_den <= 1000 (pct_den
 * >= 1); VITSEG_ESHAPE: H or W outside 1..16384, n outside 1..32767 (the planes are a batch of 2 n), K outside 1..256;
 * VITSEG_EWORKSPACE: scratch smaller than vitseg_distance_scratch_bytes (0 for a bad shape).  Nothing is launched when a
 * check fails. */
size_t vitseg_distance_scratch_bytes(int n, int H, int W);
int vitseg_distance_stats(const uint8_t* pred, const uint8_t* gt, int n, int H, int W, const int32_t* classes, int K, int mode,
                          int pct_num, int pct_den, int64_t* stats_i, double* stats_f, void* scratch, size_t scratch_bytes,
                          void* stream);

/* ---- skeletons of binary masks and the crack statistics on them: centre-line Dice (clDice), crack length and width
 *      (replaces CrackSeg.skeletonize = skimage.morphology.skeletonize per image on the host, model/PAED/segmentation.py:89-111) ----
 * The contract is the published algorithm, T. Y. Zhang and C. Y. Suen, "A Fast Parallel Algorithm for Thinning Digital
 * Patterns", CACM 1984: a non-zero byte is a mask pixel, pixels outside the image are background; neighbours clockwise from
 * north P2 = N .. P9 = NW; B = the set neighbours, A = the 0 -> 1 steps in P2, P3, ..., P9, P2; a pass is sub-iteration 1 then
 * 2, each deciding for all pixels from the state before it; a set pixel is deleted when 2 <= B <= 6, A = 1 and
 * (1) P2 P4 P6 = 0 and P4 P6 P8 = 0, (2) P2 P4 P8 = 0 and P2 P6 P8 = 0; the loop stops after the first pass that deleted
 * nothing.  Its quirks are part of the contract: an isolated 2 x 2 square vanishes, a full rectangle thins to a short
 * segment or a single pixel.
 * vitseg_skeleton: mask uint8 [n, H, W] -> skeleton uint8 [n, H, W] of 0 / 1 (it may alias nothing); passes (optional) int32
 *   [n]: the passes run per plane, counting the final one that deleted nothing.
 * route: 0 automatic, 1 resident (one workgroup per plane, the packed plane in LDS, one launch, NO host synchronisation;
 *   taken while 4 ((H + 2) (ceil(W / 32) + 1) + 4) bytes fit min(the device's shared memory per block, 160 KiB)), 2 global
 *   (packed planes in the scratch, one launch per sub-iteration; the host reads a convergence word every 16 passes, so this
 *   route SYNCHRONISES `stream`).  Route 0 takes the resident route whenever the plane fits it.
 * vitseg_skeleton_stats: pred, gt uint8 [n, H, W] class maps; classes: K label values 0..255 in HOST memory.  Per image and
 *   class c, G = {gt == c}, P = {pred == c}, S_X = the skeleton of X, d2_X(x) = the exact squared distance from a pixel x of X
 *   to the nearest pixel outside X (vitseg_sdf's "int" field before the root, its virtual point (-1, 0) included when X is the
 *   whole image).
 *   stats_i int64 [n, K, 10] (device): |G|, |P|, |S_G|, |S_P|, |S_G n P|, |S_P n G|, max d2_G over S_G, max d2_P over S_P
 *   (-1 when the skeleton is empty), the end points of S_G and of S_P (skeleton pixels with exactly one set 8-neighbour).
 *   stats_f double [n, K, 2] (device): the sum over S_G of sqrt((double) d2_G), the same over S_P.
 *   Classes are processed one after another on `stream`, 2 n planes at a time.
 * scratch: the matching *_scratch_bytes(n, H, W, route) device bytes, with the same route (every word read is written within
 * the call).  The integers come from order-independent integer operations and the sums are added in an order fixed by H * W:
 * the same bits on every call and by either route, and per image the same bits in any batch.
 * VITSEG_EINVAL: null pointer (passes excepted), route outside 0..2, a class value outside 0..255; VITSEG_ESHAPE: H or W
 * outside 1..16384, n outside 1..32767, K outside 1..256, route 1 for a plane that does not fit; VITSEG_EWORKSPACE: scratch
 * smaller than its size function (0 for a bad shape or route).  Nothing is launched when a check fails. */
size_t vitseg_skeleton_scratch_bytes(int n, int H, int W, int route);
int vitseg_skeleton(const uint8_t* mask, int n, int H, int W, int route, uint8_t* skeleton, int32_t* passes, void* scratch,
                    size_t scratch_bytes, void* stream);
size_t vitseg_skeleton_stats_scratch_bytes(int n, int H, int W, int route);
int vitseg_skeleton_stats(const uint8_t* pred, const uint8_t* gt, int n, int H, int W, const int32_t* classes, int K,
                          int route, int64_t* stats_i, double* stats_f, void* scratch, size_t scratch_bytes, void* stream);

/* ---- per-region measurements: moments, perimeter, frame contact and, for chosen classes, each region's own skeleton length
 *      and widths (the usual host answer is skimage.measure.regionprops plus a skeleton and a distance transform per label,
 *      one image at a time) ----
 * mask uint8 [n, H, W] class map.  The regions, their (class, first) order, counts (the true total, also above max_regions)
 * and labels are exactly vitseg_regions' for the same connectivity (4 / 8) and background (0..255 or -1): the same labelling
 * launches run.  props int64 [n, max_regions, VITSEG_PROPS_FIELDS]: one row per region for the first max_regions regions of
 * each image, rows past the count zero (may be NULL when max_regions == 0):
 *    0..6  class, first, area, y_min, x_min, y_max, x_max (box inclusive, first = raster index of the first pixel);
 *    7..11 sum_y, sum_x, sum_yy, sum_xx, sum_xy: the sums over the region's pixels of y, x, y^2, x^2, x y (row, column);
 *    12    perimeter: the (pixel, side) pairs whose 4-neighbour lies outside the image or has another value -- the outline
 *          length in pixel sides, holes included;
 *    13    frame_pixels: pixels with y in {0, H - 1} or x in {0, W - 1}, each once; > 0: the frame cuts the region off;
 *    14    max_d2: the maximum of d2 over the region's pixels (the squared inscribed radius);
 *    15    skel_len: skeleton pixels inside the region;   16  end_points: those with exactly one set 8-neighbour in the skeleton;
 *    17    skel_max_d2: the maximum of d2 over the skeleton pixels, -1 when skel_len = 0;
 *    18    skel_width_q16: the sum over the skeleton pixels of llrint(sqrt((double) d2) * 65536.0), a fixed-point sum (exact
 *          and independent of the order, as q of vitseg_region_match);   19  0, reserved.
 * Fields 14..18 are measured for the regions whose class is in `classes` (K distinct values 0..255 in HOST memory, none the
 * background; NULL allowed when K == 0) and are -1 for every other region.  For a class c, X = {mask == c} of the image: the
 * skeleton is vitseg_skeleton's of X (same kernels, same `route`, route 2 synchronises `stream` as documented there) and
 * d2(x) the exact squared distance from x in X to the nearest pixel outside X (vitseg_sdf's "int" field before the root,
 * virtual point (-1, 0) when X is the whole image: the field of vitseg_skeleton_stats).  A skeleton pixel belongs to the region
 * that contains it.  Under connectivity 8 two regions of one class never share a 3 x 3 neighbourhood, so this is each
 * region's own skeleton and own distance field.  Under connectivity 4 two diagonally touching regions of one class are
 * thinned and measured as the one plane they share: the thinning sees them as one 8-connected figure, and each region gets
 * the skeleton pixels and the distances that fall inside it.  K == 0 launches no skeleton or distance work, and `route`
 * is then only range-checked.
 * scratch: vitseg_region_props_scratch_bytes(n, H, W, K, route) device bytes (vitseg_regions' plus 4 bytes per pixel, with
 * K > 0 7 more and the thinning's; every word read is written within the call).  Classes are processed one after another on
 * `stream`; no allocation, no host synchronisation except route 2's.  Every value is an integer from order-independent
 * integer operations: the same bits on every call and by either route, and per image the same bits in any batch.  Regions
 * with index >= max_regions are skipped: nothing is written outside props.
 * VITSEG_EINVAL: null mask / counts / scratch, null props with max_regions > 0, negative max_regions, connectivity not 4 / 8,
 * background outside -1..255, route outside 0..2, null classes with K > 0, a class outside 0..255, repeated or equal to the
 * background; VITSEG_ESHAPE: H or W outside 1..16384, n outside 1..32767, K outside 0..256, route 1 (with K > 0) for a plane
 * that does not fit; VITSEG_EWORKSPACE: scratch smaller than the size function (0 for a bad shape).  Nothing is launched when
 * a check fails. */
#define VITSEG_PROPS_FIELDS 20
size_t vitseg_region_props_scratch_bytes(int n, int H, int W, int K, int route);
int vitseg_region_props(const uint8_t* mask, int n, int H, int W, int connectivity, int background,
                        const int32_t* classes /* host, K values, may be NULL when K == 0 */, int K, int route,
                        int32_t* counts /* [n] */, int64_t* props /* [n, max_regions, 20] */, int max_regions,
                        int32_t* labels /* [n, H, W] or NULL */, void* scratch, size_t scratch_bytes, void* stream);

/* ---- confidence: per-pixel scores of a stated mask, per-region score rows and a calibration histogram, re-generated from
 *      the low-resolution head output (the full-size logits are never written; the host answer is predict_mask's logits, then
 *      torch.sigmoid, gather, the rounding and index_add_ / bincount by label) ----
 * lowres fp32 [n, C, g, g] (vitseg_forward_lowres; g == S is the identity of the taps: full-size logits are scored as they
 * stand); mask uint8 [n, S, S], the class map whose confidence is asked for -- the decoder tail's, or a cleaned one.
 * Per pixel, c = mask[pixel] and v_k = the bilinear value of class k with the decoder tail's arithmetic (scale g / S, taps
 * src = max(scale * (d + 0.5) - 0.5, 0), row = fma(a, wx0, b * wx1), v = fma(top, wy0, bot * wy1)):
 *   VITSEG_CONF_PROB    p = sigmoid(v_c), the sigmoid as ATen computes it for fp32: on the tail's own mask this is
 *                       logits.sigmoid().max(dim=1).values;
 *   VITSEG_CONF_MARGIN  p = min(max(sigmoid(v_c) - sigmoid(max_{k != c} v_k), 0), 1): the lead over the best other class, 0
 *                       where the stated class did not win (C >= 2);
 *   c >= C              p = 0, and lowres is not indexed.
 *   q = (int) rintf(p * 65535.0f): the product rounded once in fp32, then to nearest even; 0 <= q <= 65535.
 * Every step is a single correctly rounded fp32 operation, so a CPU restatement holds bit for bit (tests/confidence_ref.py).
 * Outputs, any subset (none: VITSEG_EINVAL):
 *   conf fp32 [n, S, S] = p;   conf_q uint16 [n, S, S] = q;
 *   scores int64 [n, max_regions, 4], with labels int32 [n, S, S] = vitseg_regions' label plane of the same mask (negative:
 *     no region; an index >= max_regions is skipped, nothing is written outside scores): per region the row
 *     (pixels, sum_q, max_deficit, n_low), max_deficit = the maximum of 65535 - q over the region, n_low = the pixels with
 *     q < low_q (0..65536).  A zero row means "no pixel": the rows past the count stay zero.
 *   hist int64 [n, bins, 3], with gt uint8 [n, S, S]: pixels with gt == ignore_label (-1: none, or 0..255) are void; per image
 *     and bin = (q * bins) >> 16 (bins 1..256) the row (pixels, pixels with mask == gt, sum_q).
 * scores and hist are cleared by the call (one memset each), then ONE kernel runs on `stream`: no allocation, no scratch, no
 * host synchronisation.  The accumulators are 64-bit integer atomicAdd / atomicMax, order-independent: the same bits on every
 * call, and per image the same bits in any batch.
 * Each with a vitseg_last_error text and nothing launched -- VITSEG_EINVAL: null lowres or mask, no output, scores without
 * labels, hist without gt, kind not 0 / 1, margin with C < 2, and for the output that reads them: negative max_regions, low_q
 * outside 0..65536, bins outside 1..256, ignore_label outside -1..255; VITSEG_ESHAPE: C outside 1..255, n outside 1..65535,
 * S outside 1..16384, g outside 1..S. */
enum vitseg_conf_kind { VITSEG_CONF_PROB = 0, VITSEG_CONF_MARGIN = 1 };
int vitseg_confidence(const float* lowres /* [n, C, g, g] */, const uint8_t* mask /* [n, S, S] */, int n, int C, int g, int S,
                      int kind, float* conf /* [n, S, S] or NULL */, uint16_t* conf_q /* [n, S, S] or NULL */,
                      const int32_t* labels /* [n, S, S] or NULL */, int64_t* scores /* [n, max_regions, 4] or NULL */,
                      int max_regions, int low_q, const uint8_t* gt /* [n, S, S] or NULL */, int ignore_label,
                      int64_t* hist /* [n, bins, 3] or NULL */, int bins, void* stream);

/* one Adam step over a flat fp32 buffer (torch.optim.Adam semantics, weight_decay 0, amsgrad off: torch's L2 weight decay,
 * g += weight_decay * p, is not implemented, and FusedAdam refuses a nonzero weight_decay);
 * step is 1-based; gradients are multiplied by grad_scale first (1/world for summed all-reduce). */
int vitseg_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n_floats, float lr,
                     float beta1, float beta2, float eps, int step, float grad_scale, void* stream);
/* the same with torch.optim.AdamW's decoupled weight decay (params *= 1 - lr * weight_decay in front of the update, not
 * torch.optim.Adam's L2 form): what PAEDTrainer.configure_optimizers builds (model/PAED/classes.py:536-548,
 * AdamW(lr=1e-4), weight_decay 1e-2 by default) */
int vitseg_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n_floats, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);

/* fp32 GEMM with explicit operand forms, exported for the parity tests of the backward GEMMs:
 * C[M,N] = A . W with A N-form [M][K] (ta = 0) or T-form [K][M] (ta = 1), W N-form [N][K] (tb = 0) or
 * T-form [K][N] (tb = 1); epilogue 0 = plain, 5 = multiply by gelu'(R[M,N]). */
int vitseg_op_gemm_f32(const float* A, const float* W, const float* R, float* C, int M, int N, int K, int ta, int tb,
                       int epilogue, void* stream);
int vitseg_op_attention_bwd_f32(const float* qkv, const float* dctx, float* ctx_out, float* lse_out, float* scratch,
                                float* dqkv, int batch, int num_patches, int num_heads, void* stream);
/* the same pair for short sequences, as the fp32 training step of the small-batch route runs it (num_patches + 1 <= 400:
 * the reference's 197 tokens): key-split forward saving the log-sum-exp, then ONE backward launch (dq blocks | dk, dv blocks,
 * delta formed inside; no scratch).  dropout_p > 0: the counter-based mask of csrc/common.hpp on the probabilities. */
int vitseg_op_attention_bwd_f32_small(const float* qkv, const float* dctx, float* ctx_out, float* lse_out, float* dqkv,
                                      int batch, int num_patches, int num_heads, float dropout_p, uint32_t dropout_seed,
                                      uint32_t dropout_stream, void* stream);
/* bf16 attention core forward + backward (dropout_p > 0: the counter-based mask of csrc/common.hpp on the attention
 * probabilities, stream id = layer * 8 + 1); ctx_out bf16 [Mt, D], lse_out fp32 [B, A, Np + 1], dqkv bf16 [Mt, 3D].
 * dropmask_words (optional, vitseg_attention_dropmask_bytes; needs num_patches % 128 == 0 and dropout_p > 0): the keep
 * bits are generated once into this buffer and read by the three kernels -- the path vitseg_forward_train /
 * vitseg_backward take -- instead of being hashed per element in each of them; the masks are the same bits.
 * scratch: vitseg_attention_bwd_scratch_floats() floats (delta [B, A, Np + 1] + the per-block partial sums of the CLS
 * token's own gradients and of the column sums).
 * dbias_qkv (optional, fp32 [3 D]): the column sums of dqkv over all rows = the gradient of the fused q|k|v bias
 * (modeling_vit.py:207-222, qkv_bias=True), taken from the kernels' fp32 accumulators (patch rows) and the stored CLS rows. */
size_t vitseg_attention_dropmask_bytes(int batch, int num_patches, int num_heads);
size_t vitseg_attention_bwd_scratch_floats(int batch, int num_patches, int num_heads);
int vitseg_op_attention_bwd_bf16(const void* qkv, const void* dctx, void* ctx_out, float* lse_out, float* scratch,
                                 void* dqkv, int batch, int num_patches, int num_heads, float dropout_p,
                                 uint32_t dropout_seed, uint32_t dropout_stream, void* dropmask_words, float* dbias_qkv,
                                 void* stream);
/* scratch of vitseg_op_layernorm_bwd_f32: per-block partial sums of dw / db (the block count depends on rows and on the device) */
size_t vitseg_op_layernorm_bwd_scratch_floats(int rows, int D);
int vitseg_op_layernorm_bwd_f32(const float* x, const float* w, const float* g, const float* dres_in, float* dres_out,
                                float* dw, float* db, float* scratch, int rows, int D, float eps, void* stream);
/* the form the bf16 training step uses: g as bf16 [rows, D], the same fp32 arithmetic.  br_out != NULL (needs br_dbias): also
 * the gradient entering the NEXT dropped residual branch of the backward walk, as the bf16 operand of that branch's GEMMs --
 * br_out [rows, D] = bf16(mask * dres_out) (hidden dropout of csrc/common.hpp with the given stream id; dropout_p == 0: no mask)
 * and br_dbias [D] = the column sums of the ROUNDED values.  br_out == NULL: br_dbias must be NULL and dropout_p 0. */
int vitseg_op_layernorm_bwd_bf16(const float* x, const float* w, const void* g, const float* dres_in, float* dres_out,
                                 float* dw, float* db, float* scratch, int rows, int D, float eps, void* br_out, float* br_dbias,
                                 float dropout_p, uint32_t dropout_seed, uint32_t dropout_stream, void* stream);
/* the form the fp32 training step of the small-batch route uses (same arithmetic and bits for dres_out / dw / db): g arrives as
 * g_splits K-chunk slabs, g = slab 0 + slab 1 + ... (slab s at g + s * g_stride floats; 1 = plain); br_dbias != NULL: also the
 * gradient entering the NEXT dropped residual branch of the backward walk -- br_out = mask * dres_out (written only when
 * dropout_p > 0; hidden dropout of csrc/common.hpp with the given stream id), br_dbias [D] = its column sums (= column sums of
 * dres_out when dropout_p == 0): that branch's bias gradient.  scratch: vitseg_op_layernorm_bwd_scratch_floats(rows, D). */
int vitseg_op_layernorm_bwd_f32_small(const float* x, const float* w, const float* g, size_t g_stride, int g_splits,
                                      const float* dres_in, float* dres_out, float* dw, float* db, float* scratch, int rows,
                                      int D, float eps, float* br_out, float* br_dbias, float dropout_p, uint32_t dropout_seed,
                                      uint32_t dropout_stream, void* stream);

/* ---- helper kernels: the launches of the embeddings, the seg head and the training step around the encoder layers, one
 * entry per production call site, on caller-owned buffers (csrc/op_helpers.hip; tests/test_gpu_helpers.py).  Row layout as
 * everywhere: patch rows b * Np + t first, the CLS rows batch * Np + b after them.  Each entry builds the arguments of its
 * call site and makes that site's one launcher call.
 * patch_embed: X[batch * (g*g + 1), D] = patch projection of img [batch, Cin, g*P, g*P] (weights Wp [D, Cin*P*P]: fp32, or the
 * vitseg_cast_params_split form for x3 = 2) + bp + pos[1 + t], and the CLS rows cls + pos[0]; x3 as vitseg_op_linear_f32_thin
 * (0 fp32, 1 split operands, 2 pre-split weights); no dropout. */
int vitseg_op_patch_embed_f32(const float* img, const void* Wp, const float* bp, const float* pos, const float* cls, float* X,
                              int batch, int Cin, int P, int g, int D, int x3, void* stream);
/* 3x3 convolution, zero padding 1, as an implicit GEMM over the token-major map H [batch * g*g, channels]:
 * C [batch * g*g, N] = H (*) W, W [N, 9 * channels] with k = (ky, kx, channel).  relu != 0: + bias, ReLU (seg_head.0 forward;
 * x3 0 / 1 / 2 as above); relu == 0: the input-gradient form of the fp32 training step (bias may be NULL; x3 = 0). */
int vitseg_op_conv3x3_f32(const float* H, const void* W, const float* bias, float* C, int batch, int g, int channels, int N,
                          int relu, int x3, void* stream);
/* the same with 16-bit H and W (bf16, or IEEE half when f16 != 0) and an fp32 C; zeros: >= 128 zero bytes, the source of the
 * padding taps.  channels must be a multiple of 64.  relu == 0: the bf16 training step's input-gradient form. */
int vitseg_op_conv3x3_h16(const void* H, const void* W, const float* bias, float* C, const void* zeros, int batch, int g,
                          int channels, int N, int relu, int f16, void* stream);
/* seg_head.2: Z [batch, C, Np] = F [batch * Np, 256] . W2 [C, 256]^T + b2 */
int vitseg_op_head1x1(const float* F, const float* W2, const float* b2, float* Z, int batch, int num_patches, int C,
                      void* stream);
/* ... and its backward with the ReLU's: dFpre = (F > 0) * dZ . W2, dW2 = dZ^T F, db2 = sum dZ.  C <= 32 (VITSEG_ESHAPE). */
size_t vitseg_op_head1x1_bwd_scratch_floats(int batch, int num_patches, int C);
int vitseg_op_head1x1_bwd(const float* dZ, const float* F, const float* W2, float* dFpre, float* dW2, float* db2,
                          float* scratch, int batch, int num_patches, int C, void* stream);
/* out[N] = column sums of X [M, N] (leading dimension ld, a multiple of 4; fp32 or bf16), deterministic; scratch:
 * vitseg_op_colsum_scratch_floats(M, N) floats */
int vitseg_op_colsum(const void* X, int x_is_bf16, float* out, float* scratch, int M, int N, int ld, void* stream);
/* dpos [Np + 1, D] and dcls [D] from dX [batch * (Np + 1), D] */
int vitseg_op_embed_bwd(const float* dX, float* dpos, float* dcls, int batch, int num_patches, int D, void* stream);
/* im2col rows of the two convolutions (operands of their weight gradients): T [batch * g*g, 9 * D] of the token-major map H
 * (fp32 out of fp32 or bf16 H; bf16 out of bf16 H, D % 8 == 0), T [batch * (S/P)^2, Cin * P * P] of the NCHW image (fp32 or
 * rounded to bf16) */
int vitseg_op_im2col3x3(const void* H, int h_is_bf16, float* T, int batch, int g, int D, void* stream);
int vitseg_op_im2col3x3_bf16(const void* H, void* T, int batch, int g, int D, void* stream);
int vitseg_op_im2col_patch(const float* img, float* T, int batch, int Cin, int S, int P, void* stream);
int vitseg_op_im2col_patch_bf16(const float* img, void* T, int batch, int Cin, int S, int P, void* stream);
/* Wd [D, 9, 256] = W0 [256, 9, D] with the taps flipped: the weight of the input-gradient convolution of seg_head.0 */
int vitseg_op_conv_dgrad_weight(const float* W0, float* Wd, int D, void* stream);
/* bf16 out [C, Rpad] = in [R, C]^T (leading dimension ldin), zeros in columns R .. Rpad - 1 */
int vitseg_op_transpose_bf16(const void* in, void* out, int R, int C, int ldin, int Rpad, void* stream);
/* four bf16 matrices [R[k], C[k]] per layer, at elements src0[k] + layer * src_stride of arena, transposed into
 * out[layer][k] (dense, one after the other) */
int vitseg_op_transpose_layers_bf16(const void* arena, void* out, const size_t src0[4], const int R[4], const int C[4],
                                    size_t src_stride, int layers, void* stream);
/* dst = keep ? src * 1 / (1 - p) : 0 on [rows, cols] (cols % 4 == 0), the hidden-dropout mask of csrc/common.hpp on the
 * given stream id; dst fp32 (may be src) or bf16; 0 < dropout_p < 1 */
int vitseg_op_dropout_rows(const float* src, void* dst, int dst_bf16, int rows, int cols, float dropout_p, uint32_t dropout_seed,
                           uint32_t dropout_stream, void* stream);
/* vitseg_op_layernorm_f32 with a 16-bit output: out_fmt 1 = bf16, 2 = IEEE half */
int vitseg_op_layernorm_h16(const float* x, const float* w, const float* b, void* y, int rows, int D, float eps, int out_fmt,
                            void* stream);

/* ---- sliding-window inference: overlapping windows blended on the device ----
 * An image [H, W] larger than the model's input is covered by S x S windows `stride` apart; every window is one tile of
 * a batch through the model, and the tiles' low-resolution head outputs are blended into the full-size result.  The
 * reference has no counterpart: its scripts resize every image to the model's square (testViTModel.py:92-97), then
 * forward and sigmoid -> argmax (:122-126).
 *
 * Window grid of one axis (host arithmetic, no GPU touched):
 *   count = 1 + ceil((extent - S) / stride);  origin_i = min(i * stride, extent - S)   (the last window ends at the edge)
 * vitseg_window_count returns the count or a negative vitseg_status; vitseg_window_origins writes `count` origins.
 * VITSEG_ESHAPE (with a vitseg_last_error text): extent < S, stride < 1, stride > S, extent > 16384.
 * The tiles of a batch of n images are numbered image-major, then window row, then window column:
 *   tile = (image * ny + window_row) * nx + window_column.
 *
 * vitseg_window_gather: tiles [first, first + count) of that numbering as fp32 NCHW [count, 3, S, S].  src: fp32 NCHW
 * [n, 3, H, W] (src_is_u8 = 0: a plain copy) or uint8 HWC [n, H, W, 3] (src_is_u8 = 1: value / 255 with one correctly
 * rounded division, ToTensor, as vitseg_preprocess_u8 ends).  origins_y [ny] / origins_x [nx]: device int32 tables; no
 * alignment is assumed of the origins or of W.
 *
 * vitseg_forward_lowres: the forward walk of vitseg_forward_at (same routes, same workspace, same bits) that stops
 * before the upsample and leaves the head output in lowres, fp32 [batch, C, g, g] (g = image_size_in / P) -- the bytes
 * of VITSEG_BUF_LOWRES after vitseg_forward_at on the same input.
 *
 * vitseg_window_blend: lowres fp32 [n * ny * nx, C, g, g] (tile numbering as above) -> logits fp32 [n, C, H, W] and / or
 * mask uint8 [n, H, W] (either may be NULL; both NULL: VITSEG_EINVAL).  weights: device fp32 [S], all entries > 0; the
 * weight of a tile at its local pixel (ly, lx) is wt = weights[ly] * weights[lx].  For a pixel, a class and a covering
 * tile (origin <= coordinate < origin + S on both axes), v = the bilinear value at the tile-local coordinate with the
 * decoder tail's arithmetic (scale g / S, taps src = max(scale * (d + 0.5) - 0.5, 0), row = fma(a, wx0, b * wx1),
 * v = fma(top, wy0, bot * wy1)).  Then
 *   exactly one covering tile:  result = v;
 *   otherwise, over the covering tiles in increasing tile number from acc = 0, ws = 0:
 *     acc = fma(wt, v, acc);  ws = ws + wt;    result = acc / ws   (IEEE division).
 * Every operation is a single correctly rounded fp32 one, so a CPU restatement holds bit for bit (tests/window_ref.py).
 * mask = argmax_c sigmoid(result_c), the sigmoid as ATen computes it for fp32, first maximal index.
 * VITSEG_ESHAPE: C outside 1..255, S outside 1..4096, H or W outside S..16384, n outside 1..65535, g outside 1..S.
 * No global atomics and no scratch; every output element is written exactly once. */
int vitseg_window_count(int extent, int S, int stride);
int vitseg_window_origins(int extent, int S, int stride, int32_t* origins);
int vitseg_window_gather(const void* src, int src_is_u8, int n, int H, int W, int S, const int32_t* origins_y, int ny,
                         const int32_t* origins_x, int nx, int first, int count, float* tiles, void* stream);
int vitseg_forward_lowres(const vitseg_config* cfg, int image_size_in, const float* params, const void* params_bf16,
                          const float* x, int batch, int precision, float* lowres, void* workspace, size_t workspace_bytes,
                          void* stream);
int vitseg_window_blend(const float* lowres, const int32_t* origins_y, int ny, const int32_t* origins_x, int nx,
                        const float* weights, int n, int C, int g, int S, int H, int W, float* logits, uint8_t* mask,
                        void* stream);

/* ---- training augmentation: paired affine warp and colour jitter in one launch ----
 * A batch of images is warped bilinearly and colour-jittered into the fp32 [n, 3, oh, ow] model input, and up to two label
 * planes are warped by nearest tap, every plane with its own source size, output size and per-sample matrix table.  All
 * coordinate arithmetic is integer and every fp32 operation is a single correctly rounded one, so a CPU restatement holds
 * bit for bit (tests/augment_ref.py).
 *
 * Geometry.  Each sample has six int64 Q16 entries M = (m00, m01, m02, m10, m11, m12), which map the centre of output
 * pixel (x, y) to source coordinates
 *   U = (m00 (2x+1) + m01 (2y+1) + 2 m02 - 65536) >> 1,   V = (m10 (2x+1) + m11 (2y+1) + 2 m12 - 65536) >> 1
 * in int64 with an arithmetic (floor) shift; U / 65536 is the source x in pixel-index units, the identity is
 * (65536, 0, 0, 0, 65536, 0).  On load the kernel clamps m00, m01, m10, m11 to +-2^26 and m02, m12 to +-2^40, so no
 * table can overflow or index out of bounds, whatever it holds.
 *
 * Image taps.  ix = U >> 16, iy = V >> 16, fx = (U & 0xFFFF) >> 8, fy = (V & 0xFFFF) >> 8 (8-bit fractions); the weights
 * (256-fy)(256-fx), (256-fy) fx, fy (256-fx), fy fx go on the taps (iy, ix), (iy, ix+1), (iy+1, ix), (iy+1, ix+1) in that
 * order.  VITSEG_AUGMENT_CONSTANT: a tap outside the frame takes the channel's fill; VITSEG_AUGMENT_EDGE: tap indices are
 * clamped to the frame.
 *   VITSEG_AUGMENT_U8_NHWC   uint8 [n, H, W, 3]: S = the integer weighted sum (<= 255 * 65536, exact in fp32),
 *                            v = float(S) / 16711680.0f, one correctly rounded division: the identity gives v / 255 bitwise,
 *                            what vitseg_preprocess_u8 gives at equal size.  The fill is rintf(fill[c]) clamped to 0..255.
 *   VITSEG_AUGMENT_F32_NCHW  float32 [n, 3, H, W]: s = ((w00 p00 + w01 p01) + w10 p10) + w11 p11, v = s * 2^-16, every
 *                            product and sum rounded on its own.  The fill is fill[c] in the source's units.
 * Colour.  colour: device float32 [n, 12], a 3x4 matrix per sample:
 *   out_c = fminf(fmaxf(((c0 r + c1 g) + c2 b) + c3, 0), 1), every operation rounded on its own.
 * A null colour table skips the step: no multiply, no clamp.
 *
 * Masks.  num_masks = 0, 1 or 2 descriptors.  Nearest tap jx = (U + 32768) >> 16, jy = (V + 32768) >> 16 with the
 * descriptor's own matrix table; CONSTANT writes fill_label outside the frame, EDGE clamps.  Source uint8 or int64
 * [n, h, w], output uint8 or int64 [n, oh, ow] (a label is truncated to a byte as in vitseg_resize_nearest_*).
 *
 * matrix, colour and the descriptors' pointers are device memory; masks, fill (float[3], may be null with EDGE) are host
 * memory read during the call.  Before any launch, each with a vitseg_last_error message and nothing written:
 * VITSEG_ESHAPE for n <= 0, any extent < 1 or > 16384 or a batch beyond one launch; VITSEG_EINVAL for a null required
 * pointer, num_masks outside 0..2 or an unknown border / format flag.
 *
 * vitseg_augment_matrix (host arithmetic, no HIP call): the Q16 matrix of one (src_h, src_w) -> (dst_h, dst_w) pair from
 * a normalised 2x3 double affine a = (a00, a01, a02, a10, a11, a12), which maps the output's unit square onto the source's
 * ((x + 0.5) / dst_w  ->  (source x + 0.5) / src_w):
 *   rint(65536 [[Ws a00 / Wd, Ws a01 / Hd, Ws a02], [Hs a10 / Wd, Hs a11 / Hd, Hs a12]])
 * VITSEG_ESHAPE (nothing written) for an extent outside 1..16384 or an entry past the clamp bounds above (a NaN included). */
enum vitseg_augment_border { VITSEG_AUGMENT_CONSTANT = 0, VITSEG_AUGMENT_EDGE = 1 };
enum vitseg_augment_format { VITSEG_AUGMENT_U8_NHWC = 0, VITSEG_AUGMENT_F32_NCHW = 1 };
typedef struct vitseg_augment_mask {
    const void* src;       /* device: uint8 or int64 [n, h, w] */
    const int64_t* matrix; /* device: int64 [n, 6] */
    void* out;             /* device: uint8 or int64 [n, oh, ow] */
    int32_t src_is_i64, out_is_i64;
    int32_t h, w, oh, ow;
} vitseg_augment_mask;
int vitseg_augment_matrix(const double* affine, int src_h, int src_w, int dst_h, int dst_w, int64_t* matrix);
int vitseg_augment(const void* images, int image_format, int n, int H, int W, int oh, int ow, const int64_t* matrix,
                   const float* colour, float* out, const vitseg_augment_mask* masks, int num_masks, int border,
                   const float* fill, int64_t fill_label, void* stream);

/* ---- test-time augmentation: flipped, quarter-turned and rescaled views merged in one launch ----
 * The model runs on K views of a square batch, each forwarded on its own to the low-res head output
 * (vitseg_forward_lowres at the view's size), and the blend brings every view back to the image's frame, averages and
 * decides.  The reference has no counterpart: its scripts look at every image once (testViTModel.py:92-126).
 *
 * A view's op is 0..7: f = op >> 2 is a horizontal flip applied first, r = op & 3 the number of counter-clockwise quarter
 * turns:   view(X, op) = rot90(f ? flip(X, x axis) : X, r),   unview = its inverse
 * (op 4 the horizontal flip, op 6 the vertical flip, op 2 the half turn).  vitseg_tta_affine (host arithmetic, no HIP
 * call) writes the normalised 2x3 affine of view(., op) as vitseg_augment_matrix takes it; every entry is exact, so the
 * Q16 matrix of an equal-size pair has zero fractions and vitseg_augment with it is a bit-exact permutation.
 * VITSEG_EINVAL: a null pointer or an op outside 0..7.
 *
 * vitseg_tta_blend: views = K descriptors in host memory, read during the call; lowres = device fp32 [n, C, g, g] in the
 * view's OWN frame (the grids g may differ between views).  Output: merged fp32 [n, C, S, S] and / or mask uint8
 * [n, S, S] (either may be NULL; both NULL: VITSEG_EINVAL).  Per pixel (y, x), class c and view k, with U_k =
 * the bilinear upsample of lowres_k to S x S by the decoder tail's arithmetic (scale g_k / S, taps
 * src = max(scale * (d + 0.5) - 0.5, 0), row = fma(a, wx0, b * wx1) along the view's own x axis, fma(top, wy0, bot * wy1)):
 *   u_k = unview(U_k, op_k)[y, x], read at the view-frame position of (y, x) -- with x' = f ? S - 1 - x : x that is
 *         r = 0: (y, x')   r = 1: (S - 1 - x', y)   r = 2: (S - 1 - y, S - 1 - x')   r = 3: (x', S - 1 - y);
 *   t_k = u_k (mode 0: mean of logits)  or  sigmoid(u_k) as ATen computes it for fp32 (mode 1: mean of probabilities);
 *   K == 1:    result = t_1   (the weight plays no part);
 *   otherwise: acc = 0; in view order acc = fma(w_k, t_k, acc);  result = acc / Wsum   (IEEE division),
 *              Wsum = the fp32 sum of the weights, added in view order.
 *   mask = the first maximal index of sigmoid(result_c) (mode 0) or of result_c (mode 1).
 * Every operation is a single correctly rounded fp32 one, so a CPU restatement holds bit for bit (tests/tta_ref.py).
 * No atomics and no scratch; every output element is written exactly once; no per-view full-size tensor exists.
 * Each with a vitseg_last_error text and nothing launched -- VITSEG_EINVAL: a null pointer, K outside 1..16, an op outside
 * 0..7, a weight that is not finite and > 0 (or weights whose fp32 sum is not finite), mode not 0 / 1; VITSEG_ESHAPE:
 * C outside 1..255, S or a g outside 1..4096, n outside 1..65535. */
typedef struct vitseg_tta_view {
    const float* lowres; /* device: fp32 [n, C, g, g] */
    int32_t g;
    int32_t op;
    float weight;
} vitseg_tta_view;
int vitseg_tta_affine(int op, double* affine6);
int vitseg_tta_blend(const vitseg_tta_view* views, int K, int n, int C, int S, int mode, float* merged, uint8_t* mask,
                     void* stream);

/* ---- measurement hooks (bench.py's roofline object) ----
 * While enabled, vitseg_forward brackets every kernel launch of the hot path with a pair of
 * hipEvents on the launch stream; vitseg_forward_train / vitseg_backward bracket the GEMMs and
 * the attention kernels of the encoder layers (the VITSEG_K_TRAIN_* kinds).  vitseg_profile_collect synchronises those events (the only
 * call in this library that blocks) and returns, for one kernel kind, the summed device time,
 * the number of launches and the algorithmic work of those launches (FLOPs for the MFMA kinds,
 * HBM bytes for the bandwidth-bound kinds).  Process-global and not re-entrant: a debugging
 * facility, off by default. */
enum vitseg_kernel_kind {
    VITSEG_K_GEMM_BIAS = 0, /* gemm kernel, plain A, bias epilogue      (QKV projection) */
    VITSEG_K_GEMM_GELU,     /* gemm kernel, plain A, bias+GELU          (mlp.fc1) */
    VITSEG_K_GEMM_RESADD,   /* gemm kernel, plain A, bias+residual      (o_proj, mlp.fc2) */
    VITSEG_K_GEMM_PATCH,    /* gemm kernel, patchify loader, +pos       (patch embedding) */
    VITSEG_K_GEMM_CONV3,    /* gemm kernel, 3x3 im2col loader, ReLU     (seg_head.0) */
    VITSEG_K_ATTENTION,     /* flash attention core (patch queries) + CLS-query kernel */
    VITSEG_K_LAYERNORM,     /* bytes */
    VITSEG_K_HEAD1X1,       /* bytes */
    VITSEG_K_UPSAMPLE,      /* bytes */
    /* training step (vitseg_forward_train / vitseg_backward), encoder layers only: FLOPs */
    VITSEG_K_TRAIN_GEMM_FWD, /* the four forward linears of a layer */
    VITSEG_K_TRAIN_DGRAD,    /* activation-gradient GEMMs (incl. the weight transposes they consume) */
    VITSEG_K_TRAIN_WGRAD,    /* weight-gradient GEMMs (incl. their split-K reduction) */
    VITSEG_K_TRAIN_ATTN_FWD, /* attention forward (patch + CLS query kernels) */
    VITSEG_K_TRAIN_ATTN_BWD, /* attention backward (delta, dQ, dK/dV, CLS kernels) */
    VITSEG_K_COUNT
};
int vitseg_profile_enable(int on);
int vitseg_profile_collect(int kind, double* total_ms, int64_t* launches, double* work);

#ifdef __cplusplus
}
#endif
#endif /* VITSEG_H */
