/*
 * vitseg_decide.h -- a class decided by threshold, with hysteresis, from the low-res head output: a family header of
 * libvitseg.so's C ABI.
 *
 * A family header declares the entry points of one feature beside vitseg.h, which stays as it is: it includes vitseg.h,
 * keeps its conventions (extern "C", 0 or a negative VITSEG_E* code, the message through vitseg_last_error(), the caller
 * owns all device memory, work is enqueued on `stream`, a hipStream_t passed as void*), carries a version of its own and
 * uses only int, size_t, int32_t, int64_t, uint8_t, pointers to them and void*.  The Python side states the family once in
 * visiontransformer_amd/_ext.py (EXT_LATER), and tests compare that table with this file.
 *
 * ---- the mask of one class cut at a threshold of its score map, e.g. the one vitseg_pr_counts' curve is best at, or by
 *      hysteresis as crack and edge pipelines decide (the usual host answer: sigmoid of the full-size logits and
 *      skimage.filters.apply_hysteresis_threshold per image) ----
 * lowres fp32 [n, C, g, g]: the low-res head output (g == S: full-size logits as they stand).
 * q_i is the 16-bit score vitseg_confidence gives pixel i under a mask that states class `cls` everywhere, kind
 * VITSEG_CONF_PROB or VITSEG_CONF_MARGIN: the plane vitseg_pr_counts bins, bit for bit.
 * Thresholds: 0 <= low_q <= high_q <= 65536; 65536 is reached by no pixel.
 *   weak(i)    q_i >= low_q
 *   strong(i)  q_i >= high_q
 *   kept(i)    weak(i), and the maximal `connectivity`-connected (4 or 8) set of weak pixels that contains i also contains a
 *              strong pixel.
 * With low_q == high_q kept == strong: the plain threshold.  That call is a single launch without labelling, asks for 0
 * scratch bytes (pass hysteresis = 0 to the size query) and `scratch` may be NULL; no byte of it is read or written.
 * mask uint8 [n, S, S]:
 *   mask_i = value                                where kept(i);
 *   mask_i = off                                  elsewhere when base is NULL;
 *   mask_i = base_i == value ? off : base_i       elsewhere with base uint8 [n, S, S]: "class `value` is decided by this rule,
 *                                                 every other class by whoever wrote base" (the form for a many-class model
 *                                                 over its argmax mask).
 * counts int64 [n, 3] or NULL, zeroed by the call: per image (weak pixels, strong pixels, kept pixels), summed by 64-bit
 * integer atomics after a pre-reduction over each wave and then each workgroup.
 * Everything is an integer: the same bits on every call, and an image gets the same bits alone as in a batch.  No allocation,
 * no host synchronisation.
 * scratch: vitseg_decide_scratch_bytes(n, S, hysteresis) device bytes, hysteresis = (low_q != high_q); 0 for a bad shape.
 * Each with nothing launched -- VITSEG_EINVAL: a null lowres or mask, mask == base, kind not 0 / 1, the margin with C < 2, cls
 * outside 0..C-1, a threshold outside 0..65536 or low_q > high_q, connectivity not 4 / 8, value or off outside 0..255 or
 * value == off, a null scratch with a positive size; VITSEG_ESHAPE: C outside 1..255, n outside 1..65535, S outside 1..16384,
 * g outside 1..S; VITSEG_EWORKSPACE: scratch smaller than vitseg_decide_scratch_bytes.
 */
#ifndef VITSEG_DECIDE_H
#define VITSEG_DECIDE_H

#include "vitseg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITSEG_DECIDE_VERSION 100

int vitseg_decide_version(void);
size_t vitseg_decide_scratch_bytes(int n, int S, int hysteresis /* 0 when low_q == high_q */);
int vitseg_decide(const float* lowres /* [n, C, g, g] */, int n, int C, int g, int S, int cls, int kind /* vitseg_conf_kind */,
                  int high_q, int low_q, int connectivity /* 4 | 8 */, const uint8_t* base /* [n, S, S] or NULL */, int value,
                  int off, uint8_t* mask /* [n, S, S] */, int64_t* counts /* [n, 3] or NULL */, void* scratch,
                  size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VITSEG_DECIDE_H */
