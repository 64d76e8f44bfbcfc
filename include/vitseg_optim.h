/*
 * vitseg_optim.h -- the fine-tuning optimiser (Adam / AdamW over the parameter arena with groups, global-norm clipping,
 * non-finite step skip and a weight EMA): a family header of libvitseg.so's C ABI.
 *
 * A family header declares the entry points of one feature beside vitseg.h, which stays as it is: it includes vitseg.h,
 * keeps its conventions (extern "C", 0 or a negative VITSEG_E* code, the message through vitseg_last_error(), the caller
 * owns all device memory, work is enqueued on `stream`, a hipStream_t passed as void*), carries a version of its own and
 * uses only int, size_t, float, int32_t, int64_t, uint8_t, pointers to them and void*.  The Python side states the family
 * once in visiontransformer_amd/_ext.py (EXT_LATER), and tests compare that table with this file.
 *
 * ---- what vitseg_adam_step / vitseg_adamw_step (vitseg.h: one learning rate and one decay for the whole arena) cannot
 *      express: parameter groups, torch.nn.utils.clip_grad_norm_, a skipped step, an EMA of the weights ----
 * The entry points know nothing of a model configuration.  They see
 *   the arena: n_floats, a multiple of VITSEG_OPTIM_CHUNK = 64.  Every arena tensor starts on a 64-float boundary
 *     (vitseg_param_offset), so a 64-float chunk never straddles two tensors; a tensor's padding belongs to its chunks;
 *   chunk_group uint8 [n_floats / 64] (device): the group of every chunk;
 *   table float [n_groups, 2] (device), 1 <= n_groups <= 256: (lr_mult, wd_mult) of every group.  lr_mult = 0: the group is
 *     FROZEN -- its chunks are neither loaded nor stored by any kernel here, and their gradients (a NaN included) do not
 *     count in the norm.  A chunk whose byte is >= n_groups is treated as frozen.  vitseg_optim_check_groups checks a HOST
 *     copy of both arrays when they are built (the launching calls cannot look at device memory without a host read);
 *   state: VITSEG_OPTIM_STATE_BYTES = 32 device bytes, eight 4-byte words, all zero before the first step:
 *     word 0  int32  step     applied steps
 *     word 1  int32  skipped  steps skipped so far
 *     word 2  float  norm     L2 norm of grad_scale * g over the non-frozen chunks at the last step (0 when none was asked for)
 *     word 3  float  coef     the last clip coefficient min(1, max_norm / (norm + 1e-6)); 1 without clipping; 0 when the step
 *                             was skipped
 *     word 4  float  bc1      1 - beta1^step of the last applied step (fp64, rounded once)
 *     word 5  float  rbc2     1 / sqrt(1 - beta2^step) of the last applied step (fp64, rounded once)
 *     word 6  int32  applied  1: the last step was applied, 0: it was skipped
 *     word 7  reserved (0)
 *   scratch: vitseg_optim_scratch_bytes(n_floats, n_groups) device bytes: one fp32 partial sum per VITSEG_OPTIM_PARTIAL
 *     floats of the arena, then 256 rows (step_size, decay, live, 0) of the groups.  Every word read is written within the
 *     step.
 * One optimiser step is two or three calls on one stream, with no host read, no atomics and no wait of one block for another:
 *   vitseg_optim_grad_norm (only when the step clips or may skip): partial p = the fp32 sum of (grad_scale * g)^2 over floats
 *     [p * 8192, (p + 1) * 8192) outside frozen chunks, by a fixed pairwise tree (13 levels; the grid is ceil(n_floats / 8192)
 *     blocks whatever the device), written with an ordinary store: the same bits on every call;
 *   vitseg_optim_prepare: one block, always.  With VITSEG_OPTIM_NORM it sums the partials in fp64 in a fixed order (thread t of
 *     256 takes t, t + 256, ...; the 256 sums are then added in index order) and sets norm; with VITSEG_OPTIM_CLIP coef =
 *     min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_, L2), else coef = 1; with VITSEG_OPTIM_SKIP a norm that
 *     is not finite skips the step: skipped += 1, coef = 0, applied = 0 and nothing else changes.  Otherwise step += 1 and, in
 *     fp64 rounded once to fp32, bc1, rbc2 and per group step_size = lr * lr_mult / bc1, decay = 1 - lr * lr_mult *
 *     weight_decay * wd_mult.  lr and weight_decay arrive by value on every call;
 *   vitseg_optim_step: one launch over the arena with the arithmetic of vitseg_adamw_step element for element (same
 *     operation order, no contraction), gr = g * (grad_scale * coef), step_size and decay those of the element's group.  With
 *     ema != NULL also ema = ema_decay * ema + (1 - ema_decay) * p_new in the same pass.  After a skipped step it stores
 *     nothing.  g is never written.
 * VITSEG_EINVAL, with nothing launched: a null pointer (ema may be NULL), n_floats = 0 or not a multiple of 64, n_groups
 * outside 1..256, flags outside 0..7, VITSEG_OPTIM_CLIP or VITSEG_OPTIM_SKIP without VITSEG_OPTIM_NORM, a negative or NaN
 * weight_decay or lr, max_norm <= 0 (or NaN) with VITSEG_OPTIM_CLIP, beta1 / beta2 outside [0, 1), eps < 0, ema_decay outside
 * [0, 1) with an ema; vitseg_optim_check_groups: a negative, NaN or infinite lr_mult or wd_mult, a chunk byte >= n_groups.
 * VITSEG_EWORKSPACE: scratch smaller than vitseg_optim_scratch_bytes (0 for a refused n_floats or n_groups).
 */
#ifndef VITSEG_OPTIM_H
#define VITSEG_OPTIM_H

#include "vitseg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITSEG_OPTIM_VERSION 100
#define VITSEG_OPTIM_CHUNK 64         /* floats per chunk of chunk_group */
#define VITSEG_OPTIM_PARTIAL 8192     /* floats per fp32 partial sum of vitseg_optim_grad_norm */
#define VITSEG_OPTIM_MAX_GROUPS 256
#define VITSEG_OPTIM_STATE_BYTES 32
/* flags of vitseg_optim_prepare */
#define VITSEG_OPTIM_NORM 1           /* the partials of this step's vitseg_optim_grad_norm are in scratch */
#define VITSEG_OPTIM_CLIP 2           /* clip the global norm to max_norm */
#define VITSEG_OPTIM_SKIP 4           /* skip the step when the norm is not finite */

int vitseg_optim_version(void);
size_t vitseg_optim_scratch_bytes(size_t n_floats, int n_groups);
int vitseg_optim_check_groups(const float* table_host /* [n_groups, 2] */, int n_groups,
                              const uint8_t* chunk_group_host /* [n_chunks] or NULL */, size_t n_chunks);
int vitseg_optim_grad_norm(const float* grads, size_t n_floats, const uint8_t* chunk_group, const float* table, int n_groups,
                           float grad_scale, void* scratch, size_t scratch_bytes, void* stream);
int vitseg_optim_prepare(void* state, const float* table, int n_groups, size_t n_floats, int flags, float lr, float beta1,
                         float beta2, float weight_decay, float max_norm, void* scratch, size_t scratch_bytes, void* stream);
int vitseg_optim_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema /* or NULL */,
                      size_t n_floats, const uint8_t* chunk_group, const void* state, float beta1, float beta2, float eps,
                      float grad_scale, float ema_decay, const void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VITSEG_OPTIM_H */
