/*
 * vitseg_hardloss.h -- hard-pixel losses on the fused path, focal cross-entropy and online hard example mining (OHEM): a
 * family header of libvitseg.so's C ABI.
 *
 * A family header declares the entry points of one feature beside vitseg.h, which stays as it is: it includes vitseg.h
 * (here for vitseg_ce_options and vitseg_config), keeps its conventions (extern "C", 0 or a negative VITSEG_E* code, the
 * message through vitseg_last_error(), the caller owns all device memory, work is enqueued on `stream`, a hipStream_t passed
 * as void*) and carries a version of its own.  The Python side states the family once in visiontransformer_amd/_ext.py
 * (EXT_LATER), and tests compare that table with this file.
 *
 * ---- semantics ----
 * up = the bilinear upsample of lowres (the taps and fma placement of vitseg_ce_loss);  lse, p = softmax_c(up),
 * keep = (y != ignore_index) and the class weights w are those of vitseg_ce_loss_opts (ce_opts == NULL: nothing ignored,
 * all weights 1).  Per kept ("valid") pixel i, in fp32:
 *   ce_i = max(lse - up_y, +0)          the online log-sum-exp gives ssum >= 1, so ce >= 0 already: the max only turns -0
 *                                       into +0, and the bit pattern of ce_i is monotone in its value
 *   q_i  = -expm1f(-ce_i)               1 - p_y without the cancellation at p_y -> 1
 * Focal (Lin et al. 2017), gamma >= 0:
 *   f_i = w[y_i] q_i^gamma ce_i
 *   d f_i / d up_c = w[y_i] m_i (p_c - 1[c = y_i]),   m_i = q_i^gamma + gamma (1 - q_i) ce_i q_i^(gamma - 1)
 *   q_i == 0 with gamma > 0: q_i^gamma and m_i are 0 (no 0 * inf is formed);  gamma == 0: m_i = 1 and f_i = w ce_i.
 * OHEM (OhemCrossEntropy of HRNet / mmsegmentation), decided on the device in 64-bit integers:
 *   n_valid = the number of valid pixels of the call
 *   k   = min(n_valid, max(min_kept, ceil(n_valid * keep_q16 / 65536)))
 *   tau = min(loss_thresh, ce_(k)),  ce_(k) the k-th largest ce_i among the valid pixels;  k == 0: tau = loss_thresh
 *   H   = { i valid : ce_i >= tau }     every pixel tied at tau is in H, so H depends on no order
 * The ranking is by the unweighted, unmodulated ce_i (f is monotone in it).  loss_thresh is a CE value: for a probability
 * threshold t pass (float)(-log(t)); +inf is no threshold.  With OHEM off (loss_thresh = +inf, min_kept = 0, keep_q16 = 0) H
 * is every valid pixel.  The selection is over the call's batch (per rank under data parallelism).
 * Loss and gradient:
 *   den = sum_H w[y];   loss = sum_H f_i / den;
 *   grad_logits = [i in H] w[y_i] m_i (p_c - 1[c = y_i]) loss_scale / den
 *  - ignored pixels and valid pixels outside H get 0.0f written for every class;
 *  - den == 0: NaN loss, as in vitseg_ce_loss_opts;
 *  - a label outside [0, C) that is not ignore_index: ce_i is the canonical quiet NaN (0x7fc00000), which ranks above
 *    every finite loss and is in H; the loss and that pixel's gradient are NaN and it counts 1 in den;
 *  - gamma == 0 with OHEM off and no optional output: exactly the launches of vitseg_ce_loss_opts (vitseg_ce_loss when
 *    ce_opts is NULL) and their bits.
 * Everything runs on one stream with no host read and no float atomics (the histograms and n_valid are integer atomics, the
 * sums fp64 per-block partials added in a fixed order): the same bits on every call, for int64 and uint8 targets.
 *  - focal only: a count pass over the targets with its one-block reduce, the loss / gradient kernel (one thread per
 *    pixel, carrying m_i) and the finish kernel: the launches of vitseg_ce_loss_opts;
 *  - with OHEM: pass A (one thread per pixel regenerates the logits, writes ce_i to an fp32 plane [B, S, S] in the scratch,
 *    counts n_valid and histograms the top 11 bits of ce_i's 31 key bits), a one-block scan (k, the bin, prefix and
 *    remaining rank kept in a device state row), two more histogram / scan rounds of 10 bits over the plane alone, a sum
 *    pass over plane and targets, a one-block fixed-order reduce that also writes *loss and stats, and the gradient kernel
 *    (one thread per pixel, one store per element of grad_logits, logits regenerated for pixels in H only; skipped when
 *    grad_logits is NULL).
 * Optional outputs (device memory, either may be NULL):
 *   pixel_loss fp32 [B, S, S]: ce_i; ignored pixels hold -1.0f, the sentinel that cannot rank;
 *   stats int64[4] = { n_valid, k, |H|, the bits of tau };  with OHEM off { n_valid, 0, n_valid, 0 } (tau = +0).
 * hard->scratch: caller-owned device memory, 8-byte aligned, >= vitseg_hard_loss_scratch_bytes(batch, S); every word read is
 * written within the call.  `scratch` is the call's, >= vitseg_ce_scratch_bytes(batch, S).  ce_opts->scratch is checked as
 * vitseg_ce_loss_opts checks it.  C <= 255, batch * S * S < 2^31.
 * VITSEG_EINVAL before any launch: hard NULL, gamma negative or not finite, loss_thresh NaN or negative, min_kept < 0,
 * keep_q16 outside 0..65536, hard->scratch NULL / misaligned / too small, label smoothing set in ce_opts, batch * S * S
 * >= 2^31, the errors of vitseg_ce_loss_opts.
 */
#ifndef VITSEG_HARDLOSS_H
#define VITSEG_HARDLOSS_H

#include "vitseg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITSEG_HARDLOSS_VERSION 100

typedef struct vitseg_hard_options {
    float gamma;          /* focal exponent, finite and >= 0; 0: plain CE terms */
    float loss_thresh;    /* OHEM threshold as a CE value, >= 0; +inf: none */
    int64_t min_kept;     /* OHEM floor: at least this many of the hardest pixels, >= 0 */
    int32_t keep_q16;     /* OHEM floor as a fraction of the valid pixels: rint(fraction * 65536), 0..65536 */
    int32_t reserved;     /* 0 */
    void* scratch;
    size_t scratch_bytes;
} vitseg_hard_options;

int vitseg_hardloss_version(void);
size_t vitseg_hard_loss_scratch_bytes(int batch, int S);
int vitseg_hard_ce_loss(const float* lowres, const void* target, int target_is_u8, float* grad_logits, void* scratch,
                        float* loss, int batch, int C, int g, int S, const vitseg_ce_options* ce_opts,
                        const vitseg_hard_options* hard, float loss_scale, float* pixel_loss, int64_t* stats, void* stream);
/* vitseg_backward_opts whose fused loss is vitseg_hard_ce_loss: with `hard` the fused branch (target != NULL) forms the
 * loss above and writes `stats` (device int64[4] or NULL); nothing else in the walk changes.  hard == NULL: exactly
 * vitseg_backward_opts (stats is not touched).  Together with grad_logits, hard must be NULL (VITSEG_EINVAL).  The scratch
 * is the caller's, so the training workspace keeps its size and layout. */
int vitseg_backward_hard(const vitseg_config* cfg, int image_size_in, const float* params, const void* params_bf16,
                         const float* x, int batch, int precision, float dropout_p, uint64_t dropout_seed, const void* target,
                         int target_is_u8, const float* grad_logits, float* grads, float* loss, float loss_scale,
                         void* const* bucket_events, void* workspace, size_t workspace_bytes, void* stream,
                         const vitseg_ce_options* ce_options, const vitseg_hard_options* hard, int64_t* stats);

#ifdef __cplusplus
}
#endif

#endif /* VITSEG_HARDLOSS_H */
