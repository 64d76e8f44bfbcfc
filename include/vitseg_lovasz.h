/*
 * vitseg_lovasz.h -- the Lovasz-Softmax loss on the fused path (Berman, Triki and Blaschko, "The Lovasz-Softmax loss: a
 * tractable surrogate for the optimization of the intersection-over-union measure in neural networks", CVPR 2018): a family
 * header of libvitseg.so's C ABI, after the pattern of vitseg_cldice.h (it includes vitseg.h, keeps its conventions and
 * carries a version of its own; the Python side states the family in visiontransformer_amd/_ext.py, EXT_LATER).
 *
 * ---- semantics ----
 * For a listed class c over one segment:
 *   segment   the whole call's batch (per_image = 0, L = B S S pixels, pixel index = its index in [B, S, S]) or one image
 *             (per_image = 1, L = S S, pixel index = its index in the image);
 *   y_i       1 if target == c, else 0 (a label outside [0, C) that is not ignored is no class: y_i = 0 for every c, and the
 *             CE term of the call is NaN as in the plain call);
 *   p_i       the softmax probability of c, regenerated from lowres as expf(z_c - lse), the loss kernel's own expression;
 *   void      pixels of ignore_index (255 in truth_u8) are absent: they take no rank and receive an exact +0;
 *   error     e_i = y_i ? 1 - p_i : p_i, one fp32 subtraction or none;
 *   order     errors descending, equal errors by ascending pixel index within the segment: torch.sort(e, descending=True,
 *             stable=True).  The order is that of the bit patterns: with b the 32 bits of e, u = b ^ 0x80000000 for b >= 0 and
 *             ~b otherwise ascends with the value, and the sort key is ~u ascending (so -0 ranks after +0, where torch calls
 *             them equal; an error of the fused call is never -0).  A NaN error is made the canonical quiet NaN 0x7fc00000
 *             and ranks first; it poisons that class's loss and the total.  Void pixels carry the key 0xffffffff, which no
 *             error has;
 *   counts    G = sum y over the segment; at 1-based rank r: F = the number of y = 1 among ranks <= r, U = G + (r - F);
 *   dJ        1 / U                       when y = 1
 *             (G - F) / ((U - 1) * U)     when y = 0, and 1 when U - 1 = 0
 *             the integers G - F, U - 1, U converted to fp64, every fp64 operation rounded on its own (no fma).  This is
 *             Berman's lovasz_grad written in integers;
 *   L_c       sum over the ranks of (double)e_(r) * dJ_r in fp64: per thread in rank order over 8 ranks, per tile of
 *             VITSEG_LOVASZ_TILE ranks in a fixed tree, the tiles in the fixed order of the CE partials;
 *   present   present_only = 1 (the published classes='present'): a class with G = 0 in the segment is left out.  The term of
 *             a segment is the mean of L_c over the K' classes that remain (added in the order listed, divided by K'), 0
 *             when K' = 0; present_only = 0: K' = K.  per_image: the term is the sum over the B images in batch order of
 *             their segment terms, divided by B.  K' is counted on the device; there is no host read;
 *   total     loss = ce_weight CE + dice_weight dice + weight lovasz;
 *   g planes  g_c(i) = (float)(coef * dJ * (y_i ? -1 : +1)), coef = ((double)weight * (double)gscale) / K' and, per_image,
 *             that / B, in fp64 (gscale = loss_scale); +0 at void pixels and in every plane of a class left out;
 *   softmax   d / d up_j = p_j (g_j - sum_c g_c p_c) inside the one store per element of grad_logits: the arithmetic of
 *             vitseg_ce_cldice_loss's loss kernel, unchanged.
 * No float atomics anywhere: the same bits on every call.  With per_image an image's L_c has the same bits alone as in a
 * batch.  Without it the result depends on the order of the batch through the tie rule (equal errors rank by pixel index,
 * and the index runs over the batch); nothing more is promised.
 *
 * ---- launches (one stream, no host read) ----
 * n segments of L keys lie side by side: n = K, L = B S S, or n = K B, L = S S; either way key (k, b, y, x) is element
 * ((k B + b) S + y) S + x.
 *   planes    one thread per pixel: per listed class the 32-bit key and the payload (pixel index, y in bit 31);
 *   sort      four LSD passes of 8 bits, three launches each: per tile of VITSEG_LOVASZ_TILE keys a digit histogram; per
 *             (segment, digit) an exclusive scan over the tiles and the digit's total; the scatter: a key goes to its
 *             digit's base + the count of the digit in earlier tiles + its rank among equal digits in index order inside
 *             the tile (ballots and a popcount below the lane within a wave, waves in a fixed order through LDS; no return
 *             value of an atomic is used; integer LDS atomics form the histogram alone);
 *   ranks     per tile the count of y in sorted order; a scan per segment, which leaves G; one block forms K' and coef;
 *             the rank pass forms F, U, dJ per rank, writes g_c at the pixel the payload names and leaves an fp64 partial of
 *             e dJ per tile; one block per segment adds its partials; one block finishes: the mean, extra and class_terms;
 *   the loss kernel and the finish kernel of vitseg_ce_cldice_loss, as they are.
 * Scratch (vitseg_lovasz_scratch_bytes): 20 bytes per plane pixel (two key and two payload arrays and the g planes), 1 KiB +
 * 12 bytes per tile of histograms, counts and partials, and a small header.  Every word read is written within the call.
 * Limits: K batch S S < 2^31, C <= 255 (the fused losses' own limit).
 */
#ifndef VITSEG_LOVASZ_H
#define VITSEG_LOVASZ_H

#include "vitseg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITSEG_LOVASZ_VERSION 100
#define VITSEG_LOVASZ_TILE 2048

int vitseg_lovasz_version(void);

/* The sort on a caller's planes: n independent segments of L pixels.  prob fp32 [n, L]; truth_u8 [n, L]: 1 = the class,
 * 255 = void, anything else = not the class.  terms: device float[n] = L_c of each segment.  grad_prob (optional, fp32 [n, L])
 * = (float)((double)grad_scale * dJ * (y ? -1 : +1)) = grad_scale * d L_c / d prob, an exact +0 at void pixels.  order
 * (optional, int32 [n, L]): the pixel at each rank, -1 past the valid ones.  scratch: device, 8-byte aligned, >=
 * vitseg_lovasz_planes_scratch_bytes(n, L) (0 for a shape out of range).  VITSEG_EINVAL: a null pointer (grad_prob and order
 * excepted), n < 1, L < 1, n * L >= 2^31, scratch misaligned, grad_scale not finite. */
size_t vitseg_lovasz_planes_scratch_bytes(int n, int L);
int vitseg_lovasz_planes(const float* prob, const uint8_t* truth_u8, int n, int L, float grad_scale, void* scratch,
                         float* terms, float* grad_prob, int32_t* order, void* stream);

typedef struct vitseg_lovasz_options {
    float weight;           /* lovasz_weight, finite and >= 0; 0: the term is left out (the launches of vitseg_ce_dice_loss) */
    int32_t K;              /* the number of listed classes, 1 .. C */
    const int32_t* classes; /* host int32[K], distinct, each in [0, C) */
    int32_t per_image;      /* 0: one segment per class over the batch; 1: one per class and image */
    int32_t present_only;   /* 1: a class absent from a segment is left out of its mean; 0: every listed class counts */
    void* scratch;          /* device, 8-byte aligned */
    size_t scratch_bytes;   /* >= vitseg_lovasz_scratch_bytes(batch, K, S) */
    float* prob_planes;     /* optional device fp32 [K, batch, S, S] out: p of the listed classes, 0 at void pixels */
    float* grad_planes;     /* optional device fp32 [K, batch, S, S] out: the g planes */
    float* class_terms;     /* optional device float out: L_c per segment, [K] or, per_image, [K, batch] */
} vitseg_lovasz_options;

size_t vitseg_lovasz_scratch_bytes(int batch, int K, int S);

/* vitseg_ce_dice_loss plus the term.  terms: device float[4] = {loss, CE, dice, lovasz}.  dice_opts may be NULL (ce_weight 1,
 * no Dice term); with lovasz both of its weights may be 0.  lovasz NULL or lovasz->weight == 0: the launches and the bits of
 * vitseg_ce_dice_loss (of vitseg_ce_loss_opts when dice_opts is NULL too), and lovasz = 0.  The term with clDice or with focal
 * / OHEM is not built.  VITSEG_EINVAL before any launch: the errors of vitseg_ce_dice_loss, weight negative or not finite,
 * K outside 1..C, classes NULL, a class repeated or outside [0, C), per_image / present_only not 0 or 1, scratch NULL /
 * misaligned / too small, K * batch * S * S >= 2^31. */
int vitseg_ce_lovasz_loss(const float* lowres, const void* target, int target_is_u8, float* grad_logits, void* scratch,
                          float* terms, int batch, int C, int g, int S, const vitseg_ce_options* ce_opts,
                          const vitseg_dice_options* dice_opts, const vitseg_lovasz_options* lovasz, float loss_scale,
                          void* stream);

/* vitseg_backward_dice whose fused loss is vitseg_ce_lovasz_loss: terms is the device float[4] above; dice may be NULL.
 * lovasz == NULL and dice != NULL: exactly vitseg_backward_dice's walk (terms[3] = 0 is written as well).  Together with
 * grad_logits, lovasz must be NULL (VITSEG_EINVAL).  The scratch is the caller's, so the training workspace keeps its size
 * and layout. */
int vitseg_backward_lovasz(const vitseg_config* cfg, int image_size_in, const float* params, const void* params_bf16,
                           const float* x, int batch, int precision, float dropout_p, uint64_t dropout_seed,
                           const void* target, int target_is_u8, const float* grad_logits, float* grads, float* loss,
                           float loss_scale, void* const* bucket_events, void* workspace, size_t workspace_bytes,
                           void* stream, const vitseg_ce_options* ce_options, const vitseg_dice_options* dice,
                           const vitseg_lovasz_options* lovasz, float* terms);

#ifdef __cplusplus
}
#endif

#endif /* VITSEG_LOVASZ_H */
