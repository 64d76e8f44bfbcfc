/*
 * vitseg_cldice.h -- the soft-clDice loss on the fused path (Shit et al., "clDice -- a novel topology-preserving loss
 * function for tubular structure segmentation", CVPR 2021): a family header of libvitseg.so's C ABI, after the pattern of
 * vitseg_hardloss.h (it includes vitseg.h, keeps its conventions and carries a version of its own; the Python side states
 * the family in visiontransformer_amd/_ext.py, EXT_LATER).
 *
 * ---- semantics ----
 * All plane arithmetic is fp32 on [n, H, W] planes of finite values.  Pixels outside the frame do not take part
 * (max_pool2d's implicit -inf padding).
 *   erode(I)[y,x]  = min(m_col, m_row)
 *                    m_col = min over (y-1,x),(y,x),(y+1,x)     in-frame taps only
 *                    m_row = min over (y,x-1),(y,x),(y,x+1)     in-frame taps only
 *   dilate(I)[y,x] = max over the in-frame 3x3 window
 *   open(I)        = dilate(erode(I))
 *   soft_skel(I, iters):
 *       skel = relu(I - open(I))
 *       repeat iters times:
 *           I = erode(I)
 *           D = relu(I - open(I))
 *           skel = skel + relu(D - skel*D)
 * Every product, difference and sum is rounded on its own (no contracted fma).  This is the published soft_skel
 * (soft_erode = min(-max_pool2d(-x,(3,1)), -max_pool2d(-x,(1,3))), soft_dilate = max_pool2d(x,(3,3))); min, max and
 * single-rounded arithmetic are exact operations, so the device skeleton equals torch's fp32 CPU result bit for bit.
 *
 * For a class c: p = the softmax probability plane of c, y = the 0/1 plane (target == c); at a void pixel (ignore_index;
 * 255 in truth_u8) both are 0 and that pixel receives gradient 0.  sp = soft_skel(p), st = soft_skel(y).  The sums run over
 * the whole call's batch (per rank under data parallelism) in fp64: per image in a fixed order, and the per-image sums are
 * added in ascending order of their value, so the order of the images in the batch does not change a bit either.
 *   tprec = (sum sp y + s) / (sum sp + s)
 *   tsens = (sum st p + s) / (sum st + s)
 *   cl_c  = 1 - 2 tprec tsens / (tprec + tsens)
 * s = smooth > 0 (the published 1.0).  cldice = the mean of cl_c over the listed classes: per class, as this library's Dice
 * term is; the published code pools the foreground channels into one pair of sums instead.
 *   loss = ce_weight CE + dice_weight dice + cldice_weight cldice
 *
 * The gradient is autograd's, including where values tie:
 *   relu'(0) = 0;
 *   a pooling window hands its gradient to the FIRST extremal tap in row-major window order (m_col: up, centre, down;
 *   m_row: left, centre, right; the 3x3 window: dy-major, then dx);
 *   min(m_col, m_row) gives the whole gradient to the smaller one and half to each when they are equal.
 * The adjoint is a gather: each input pixel collects from the outputs whose chosen tap it is.  No float atomics: the same
 * bits on every call.  Through the softmax: d / d up_j = p_j (g_j - sum_c g_c p_c), g_c = d loss / d p_c for a listed
 * class and 0 otherwise, formed inside the one store per element of grad_logits.
 *
 * ---- launches (one stream, no host read) ----
 *   planes   one thread per pixel: p_c of the listed classes regenerated from lowres (the arithmetic of vitseg_ce_loss),
 *            p and y written, 0 at void pixels;
 *   stage j  (j = 0 .. iters+1, for p and for y) one stencil launch: I_{j+1} = erode(I_j) and, from the window of I_j
 *            already loaded, D_{j-1} = relu(I_{j-1} - dilate(I_j)) and the running skeleton skel_{j-1}.  For p every
 *            stage plane and every running skeleton is kept for the adjoint; for y three planes rotate;
 *   sums     per-block fp64 partials of sum sp y, sum sp, sum st p, sum st; one block per (sum, class, image) adds them
 *            in a fixed order; one block finishes: tprec, tsens, cl_c, the term, and per class the three scalars of
 *            d cl / d sp = alpha y + beta and d cl / d p (direct) = gamma st;
 *   adjoint  k = iters .. 0, three launches each: the pointwise step through skel_k and D_k, which also packs every pixel's
 *            chosen taps into 2 bytes, the gather through the dilation, the gather through the erosion (each reads the
 *            packed choices of its 9 or 5 outputs instead of their windows); the last leaves the g_c planes;
 *   the loss kernel of vitseg_ce_dice_loss in a third instantiation that reads the g planes.
 * Scratch of the term (vitseg_cldice_scratch_bytes): a header of sums and coefficients, 2 bytes per plane pixel of packed choices and
 * (2 iters + 12) fp32 planes of K * batch * S * S each.  Every word read is written within the call.  Limits: 0 <= iters <= 64, K * batch * S * S < 2^31.
 */
#ifndef VITSEG_CLDICE_H
#define VITSEG_CLDICE_H

#include "vitseg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITSEG_CLDICE_VERSION 100
#define VITSEG_CLDICE_MAX_ITERS 64

int vitseg_cldice_version(void);

/* skel = soft_skel(p, iters) of arbitrary finite fp32 planes [n, H, W], any H, W >= 1; n * H * W < 2^31.  scratch: device
 * memory, 8-byte aligned, >= vitseg_soft_skeleton_scratch_bytes(n, H, W) (three planes; 0 for a shape out of range).
 * skel must not overlap p.  VITSEG_EINVAL: a null pointer, n / H / W < 1, n * H * W >= 2^31, iters outside 0..64. */
size_t vitseg_soft_skeleton_scratch_bytes(int n, int H, int W);
int vitseg_soft_skeleton(const float* p, int n, int H, int W, int iters, float* skel, void* scratch, void* stream);

/* The loss of one class on given planes, with its gradient: prob fp32 [n, H, W]; truth_u8 [n, H, W]: 1 = the class, 255 =
 * void, anything else = not the class.  terms: device float[4] = {loss, tprec, tsens, 0}, loss = cl of the semantics above.
 * grad_prob (optional, fp32 [n, H, W]) = grad_scale * d loss / d prob, an exact +0 at void pixels.  scratch: 8-byte
 * aligned, >= vitseg_soft_cldice_scratch_bytes(n, H, W, iters).  VITSEG_EINVAL: a null pointer (grad_prob excepted), a
 * shape as above, iters outside 0..64, smooth not finite or <= 0. */
size_t vitseg_soft_cldice_scratch_bytes(int n, int H, int W, int iters);
int vitseg_soft_cldice(const float* prob, const uint8_t* truth_u8, int n, int H, int W, int iters, float smooth,
                       float grad_scale, void* scratch, float* terms, float* grad_prob, void* stream);

typedef struct vitseg_cldice_options {
    float weight;           /* cldice_weight, finite and >= 0; 0: the term is left out (the launches of vitseg_ce_dice_loss) */
    float smooth;           /* s, finite and > 0 */
    int32_t iters;          /* 0 .. VITSEG_CLDICE_MAX_ITERS */
    int32_t K;              /* the number of listed classes, 1 .. C */
    const int32_t* classes; /* host int32[K], distinct, each in [0, C) */
    void* scratch;          /* device, 8-byte aligned */
    size_t scratch_bytes;   /* >= vitseg_cldice_scratch_bytes(batch, K, S, iters) */
    float* prob_planes;     /* optional device fp32 [K, batch, S, S] out: p of the listed classes, 0 at void pixels */
    float* class_terms;     /* optional device float[3 K] out: {cl_c, tprec, tsens} per listed class */
} vitseg_cldice_options;

size_t vitseg_cldice_scratch_bytes(int batch, int K, int S, int iters);

/* vitseg_ce_dice_loss plus the term.  terms: device float[4] = {loss, CE, dice, cldice}.  dice_opts may be NULL (ce_weight
 * 1, no Dice term); with cld both of its weights may be 0.  cld NULL or cld->weight == 0: the launches and the bits of
 * vitseg_ce_dice_loss (of vitseg_ce_loss_opts when dice_opts is NULL too), and cldice = 0.  Focal / OHEM with clDice are not
 * built.  VITSEG_EINVAL before any launch: the errors of vitseg_ce_dice_loss, weight negative or not finite, smooth not
 * finite or <= 0, iters outside 0..64, K outside 1..C, classes NULL, a class repeated or outside [0, C), scratch NULL /
 * misaligned / too small, K * batch * S * S >= 2^31. */
int vitseg_ce_cldice_loss(const float* lowres, const void* target, int target_is_u8, float* grad_logits, void* scratch,
                          float* terms, int batch, int C, int g, int S, const vitseg_ce_options* ce_opts,
                          const vitseg_dice_options* dice_opts, const vitseg_cldice_options* cld, float loss_scale,
                          void* stream);

/* vitseg_backward_dice whose fused loss is vitseg_ce_cldice_loss: terms is the device float[4] above; dice may be NULL.
 * cld == NULL and dice != NULL: exactly vitseg_backward_dice's walk (terms[3] = 0 is written as well).  Together with
 * grad_logits, cld must be NULL (VITSEG_EINVAL).  The scratch is the caller's, so the training workspace keeps its size
 * and layout. */
int vitseg_backward_cldice(const vitseg_config* cfg, int image_size_in, const float* params, const void* params_bf16,
                           const float* x, int batch, int precision, float dropout_p, uint64_t dropout_seed,
                           const void* target, int target_is_u8, const float* grad_logits, float* grads, float* loss,
                           float loss_scale, void* const* bucket_events, void* workspace, size_t workspace_bytes,
                           void* stream, const vitseg_ce_options* ce_options, const vitseg_dice_options* dice,
                           const vitseg_cldice_options* cld, float* terms);

#ifdef __cplusplus
}
#endif

#endif /* VITSEG_CLDICE_H */
