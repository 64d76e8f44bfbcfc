// Single-launch entry points of the embedding, seg-head and training helper kernels (include/vitseg.h, "helper kernels"):
// what the forward walks (forward.hip) and the backward routes (vitseg_train.hip) launch around the encoder layers, callable on
// caller-owned buffers so that tests/test_gpu_helpers.py can hold each one to a reference of its own.  Every entry checks its
// arguments, fills the GemmArgs its production call site fills (or passes the arguments through) and makes that site's one
// launcher call; there is no arithmetic and no routing here.
#include "kernels.hpp"

using namespace vitseg;

extern "C" {

// forward.hip embed_gemm without the dropout: the A_PATCH / EPI_POS GEMM, then the CLS rows
int vitseg_op_patch_embed_f32(const float* img, const void* Wp, const float* bp, const float* pos, const float* cls, float* X,
                              int batch, int Cin, int P, int g, int D, int x3, void* stream) {
    VITSEG_CHECK_ARG(img && Wp && bp && pos && cls && X, VITSEG_EINVAL, "patch_embed: null pointer");
    VITSEG_CHECK_ARG(batch > 0 && Cin > 0 && P > 0 && g > 0 && D > 0, VITSEG_EINVAL, "patch_embed: bad geometry");
    VITSEG_CHECK_ARG(x3 >= 0 && x3 <= 2, VITSEG_EINVAL, "patch_embed: x3 %d", x3);
    GemmArgs a{};
    a.A = img; a.W = Wp; a.bias = bp; a.R = pos; a.C = X;
    a.M = batch * g * g; a.N = D; a.K = Cin * P * P; a.lda = 0; a.ldc = D;
    a.S = g * P; a.P = P; a.g = g; a.Np = g * g; a.Cin = Cin; a.D = D;
    if (int rc = launch_gemm_f32(a, A_PATCH, EPI_POS, (hipStream_t)stream, x3)) return rc;
    return launch_cls_rows(cls, pos, X, batch, g * g, D, (hipStream_t)stream);
}

// relu != 0: forward.hip head_conv_gemm (fp32 / x3); relu == 0: the fp32 routes' head_dgrad (vitseg_train.hip), no bias
int vitseg_op_conv3x3_f32(const float* H, const void* W, const float* bias, float* C, int batch, int g, int channels, int N,
                          int relu, int x3, void* stream) {
    VITSEG_CHECK_ARG(H && W && C, VITSEG_EINVAL, "conv3x3_f32: null pointer");
    VITSEG_CHECK_ARG(batch > 0 && g > 0 && channels > 0 && N > 0, VITSEG_EINVAL, "conv3x3_f32: bad geometry");
    VITSEG_CHECK_ARG(x3 >= 0 && x3 <= 2 && (relu || !x3), VITSEG_EINVAL, "conv3x3_f32: x3 %d (the gradient form is fp32 only)", x3);
    VITSEG_CHECK_ARG(channels % 4 == 0, VITSEG_ESHAPE, "conv3x3_f32: channels=%d must be a multiple of 4", channels);
    GemmArgs a{};
    a.A = H; a.W = W; a.bias = bias; a.C = C;
    a.M = batch * g * g; a.N = N; a.K = 9 * channels; a.lda = 0; a.ldc = N;
    a.g = g; a.Np = g * g; a.D = channels;
    if (relu) return launch_gemm_f32(a, A_CONV3, EPI_RELU, (hipStream_t)stream, x3);
    return launch_gemm_f32_bwd(a, A_CONV3, 0, 0, EPI_BIAS, (hipStream_t)stream);
}

// 16-bit operands, fp32 output: head_conv_gemm (relu != 0; bf16 or f16) and the bf16 route's head_dgrad (relu == 0)
int vitseg_op_conv3x3_h16(const void* H, const void* W, const float* bias, float* C, const void* zeros, int batch, int g,
                          int channels, int N, int relu, int f16, void* stream) {
    VITSEG_CHECK_ARG(H && W && C && zeros, VITSEG_EINVAL, "conv3x3_h16: null pointer");
    VITSEG_CHECK_ARG(batch > 0 && g > 0 && channels > 0 && N > 0, VITSEG_EINVAL, "conv3x3_h16: bad geometry");
    GemmArgs a{};
    a.A = H; a.W = W; a.bias = bias; a.C = C;
    a.M = batch * g * g; a.N = N; a.K = 9 * channels; a.lda = 0; a.ldc = N;
    a.g = g; a.Np = g * g; a.D = channels;
    a.zeros = zeros;
    return launch_gemm_bf16(a, A_CONV3, relu ? EPI_RELU : EPI_BIAS, (hipStream_t)stream, f16 != 0);
}

int vitseg_op_head1x1(const float* F, const float* W2, const float* b2, float* Z, int batch, int num_patches, int C,
                      void* stream) {
    VITSEG_CHECK_ARG(batch > 0 && num_patches > 0 && C > 0, VITSEG_EINVAL, "head1x1: bad geometry");
    return launch_head1x1(F, W2, b2, Z, batch, num_patches, C, (hipStream_t)stream);
}

size_t vitseg_op_head1x1_bwd_scratch_floats(int batch, int num_patches, int C) {
    return batch > 0 && num_patches > 0 && C > 0 ? head1x1_bwd_scratch_floats(batch, num_patches, C) : 0;
}

int vitseg_op_head1x1_bwd(const float* dZ, const float* F, const float* W2, float* dFpre, float* dW2, float* db2,
                          float* scratch, int batch, int num_patches, int C, void* stream) {
    VITSEG_CHECK_ARG(dZ && F && W2 && dFpre && dW2 && db2 && scratch, VITSEG_EINVAL, "head1x1_bwd: null pointer");
    VITSEG_CHECK_ARG(batch > 0 && num_patches > 0 && C > 0, VITSEG_EINVAL, "head1x1_bwd: bad geometry");
    return launch_head1x1_bwd(dZ, F, W2, dFpre, dW2, db2, scratch, batch, num_patches, C, (hipStream_t)stream);
}

// scratch: vitseg_op_colsum_scratch_floats(M, N) floats; the kernels read four adjacent columns of a row as one vector
int vitseg_op_colsum(const void* X, int x_is_bf16, float* out, float* scratch, int M, int N, int ld, void* stream) {
    VITSEG_CHECK_ARG(X && out && scratch, VITSEG_EINVAL, "colsum: null pointer");
    VITSEG_CHECK_ARG(M > 0 && N > 0 && ld >= N, VITSEG_EINVAL, "colsum: bad M/N/ld %d %d %d", M, N, ld);
    VITSEG_CHECK_ARG(ld % 4 == 0, VITSEG_ESHAPE, "colsum: ld=%d must be a multiple of 4", ld);
    return launch_colsum(X, x_is_bf16, out, scratch, M, N, ld, (hipStream_t)stream);
}

int vitseg_op_embed_bwd(const float* dX, float* dpos, float* dcls, int batch, int num_patches, int D, void* stream) {
    VITSEG_CHECK_ARG(dX && dpos && dcls, VITSEG_EINVAL, "embed_bwd: null pointer");
    VITSEG_CHECK_ARG(batch > 0 && num_patches > 0 && D > 0, VITSEG_EINVAL, "embed_bwd: bad geometry");
    return launch_embed_bwd(dX, dpos, dcls, batch, num_patches, D, (hipStream_t)stream);
}

int vitseg_op_im2col3x3(const void* H, int h_is_bf16, float* T, int batch, int g, int D, void* stream) {
    VITSEG_CHECK_ARG(H && T, VITSEG_EINVAL, "im2col3x3: null pointer");
    VITSEG_CHECK_ARG(batch > 0 && g > 0 && D > 0, VITSEG_EINVAL, "im2col3x3: bad geometry");
    VITSEG_CHECK_ARG(D % 4 == 0, VITSEG_ESHAPE, "im2col3x3: D=%d must be a multiple of 4", D);
    return launch_im2col3x3(H, h_is_bf16, T, batch, g, D, (hipStream_t)stream);
}

int vitseg_op_im2col3x3_bf16(const void* H, void* T, int batch, int g, int D, void* stream) {
    VITSEG_CHECK_ARG(H && T, VITSEG_EINVAL, "im2col3x3_bf16: null pointer");
    VITSEG_CHECK_ARG(batch > 0 && g > 0 && D > 0, VITSEG_EINVAL, "im2col3x3_bf16: bad geometry");
    return launch_im2col3x3_bf16(H, T, batch, g, D, (hipStream_t)stream);
}

int vitseg_op_im2col_patch(const float* img, float* T, int batch, int Cin, int S, int P, void* stream) {
    VITSEG_CHECK_ARG(img && T, VITSEG_EINVAL, "im2col_patch: null pointer");
    VITSEG_CHECK_ARG(batch > 0 && Cin > 0 && P > 0 && S >= P && S % P == 0, VITSEG_EINVAL, "im2col_patch: bad geometry");
    VITSEG_CHECK_ARG(P % 4 == 0, VITSEG_ESHAPE, "im2col_patch: P=%d must be a multiple of 4", P);
    return launch_im2col_patch(img, T, batch, Cin, S, P, (hipStream_t)stream);
}

int vitseg_op_im2col_patch_bf16(const float* img, void* T, int batch, int Cin, int S, int P, void* stream) {
    VITSEG_CHECK_ARG(img && T, VITSEG_EINVAL, "im2col_patch_bf16: null pointer");
    VITSEG_CHECK_ARG(batch > 0 && Cin > 0 && P > 0 && S >= P && S % P == 0, VITSEG_EINVAL, "im2col_patch_bf16: bad geometry");
    VITSEG_CHECK_ARG(P % 4 == 0, VITSEG_ESHAPE, "im2col_patch_bf16: P=%d must be a multiple of 4", P);
    return launch_im2col_patch_bf16(img, T, batch, Cin, S, P, (hipStream_t)stream);
}

int vitseg_op_conv_dgrad_weight(const float* W0, float* Wd, int D, void* stream) {
    VITSEG_CHECK_ARG(W0 && Wd && D > 0, VITSEG_EINVAL, "conv_dgrad_weight: bad arguments");
    return launch_conv_dgrad_weight(W0, Wd, D, (hipStream_t)stream);
}

int vitseg_op_transpose_bf16(const void* in, void* out, int R, int C, int ldin, int Rpad, void* stream) {
    VITSEG_CHECK_ARG(in && out, VITSEG_EINVAL, "transpose_bf16: null pointer");
    VITSEG_CHECK_ARG(R > 0 && C > 0 && ldin >= C && Rpad >= R, VITSEG_EINVAL, "transpose_bf16: bad R/C/ldin/Rpad %d %d %d %d", R, C,
                     ldin, Rpad);
    return launch_transpose_bf16(in, out, R, C, ldin, Rpad, (hipStream_t)stream);
}

int vitseg_op_transpose_layers_bf16(const void* arena, void* out, const size_t src0[4], const int R[4], const int C[4],
                                    size_t src_stride, int layers, void* stream) {
    VITSEG_CHECK_ARG(arena && out && src0 && R && C && layers > 0, VITSEG_EINVAL, "transpose_layers_bf16: bad arguments");
    for (int k = 0; k < 4; ++k) VITSEG_CHECK_ARG(R[k] > 0 && C[k] > 0, VITSEG_EINVAL, "transpose_layers_bf16: matrix %d is empty", k);
    return launch_transpose_layers_bf16(arena, out, src0, R, C, src_stride, layers, (hipStream_t)stream);
}

int vitseg_op_dropout_rows(const float* src, void* dst, int dst_bf16, int rows, int cols, float dropout_p, uint32_t dropout_seed,
                           uint32_t dropout_stream, void* stream) {
    VITSEG_CHECK_ARG(src && dst && rows > 0 && cols > 0, VITSEG_EINVAL, "dropout_rows: bad arguments");
    VITSEG_CHECK_ARG(dropout_p > 0.f && dropout_p < 1.f, VITSEG_EINVAL, "dropout_rows: dropout_p %f", dropout_p);
    return launch_dropout_rows(src, dst, dst_bf16, rows, cols, drop_args(dropout_p, dropout_seed, dropout_stream),
                               (hipStream_t)stream);
}

int vitseg_op_layernorm_h16(const float* x, const float* w, const float* b, void* y, int rows, int D, float eps, int out_fmt,
                            void* stream) {
    VITSEG_CHECK_ARG(out_fmt == 1 || out_fmt == 2, VITSEG_EINVAL, "layernorm_h16: out_fmt %d", out_fmt);
    return launch_layernorm(x, w, b, y, rows, D, eps, out_fmt, (hipStream_t)stream);
}

}  // extern "C"
