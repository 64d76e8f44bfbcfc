/*
 * vitseg_curves.h -- the precision-recall counts of a probability map over all thresholds, with a pixel tolerance: a family
 * header of libvitseg.so's C ABI.
 *
 * A family header declares the entry points of one feature beside vitseg.h, which stays as it is: it includes vitseg.h,
 * keeps its conventions (extern "C", 0 or a negative VITSEG_E* code, the message through vitseg_last_error(), the caller
 * owns all device memory, work is enqueued on `stream`, a hipStream_t passed as void*), carries a version of its own and
 * uses only int, size_t, int32_t, int64_t, uint8_t, pointers to them and void*.  The Python side states the family once in
 * visiontransformer_amd/_ext.py (EXT_LATER), and tests compare that table with this file.
 *
 * ---- what the crack benchmarks (CrackTree, CrackForest, DeepCrack) lead with: the curve behind ODS, OIS and AP, where a
 *      predicted crack pixel within a few pixels of a true one is not an error (the usual host answer: sigmoid of the full-size
 *      logits, a grey dilation by a disc, a distance transform and three bincounts per image) ----
 * lowres fp32 [n, C, g, g]: the low-res head output (g == S: full-size logits as they stand); gt uint8 [n, S, S].
 * q_i is the 16-bit score vitseg_confidence gives pixel i under a mask that states class `cls` everywhere, kind
 * VITSEG_CONF_PROB or VITSEG_CONF_MARGIN: the same arithmetic, bit for bit.  bin(q) = (q * bins) >> 16.
 * valid(i): gt_i != ignore_label (-1: every pixel is valid).  pos(i): valid and gt_i == cls.
 * D = {(dy, dx) : dy^2 + dx^2 <= tol2}, the Euclidean disc of squared radius tol2 (0..256).
 * counts int64 [n, bins, 3], zeroed by the call, per image and bin b:
 *   [b, 0] pred   the valid pixels i with bin(q_i) = b;
 *   [b, 1] hit    those of them with a pos pixel j, i - j in D;
 *   [b, 2] found  the pos pixels j with bin(max{q_i : i valid, inside the frame, i - j in D}) = b (j itself is in the set).
 * Threshold k means "positive iff bin >= k", that is q >= ceil(k 65536 / bins): the sums of the rows k.. are the predicted
 * pixels, the predicted pixels near a true one and the true pixels near a predicted one.  With tol2 = 0 hit and found are the
 * same plane and the curve is the plain pixel curve; that call runs without halo and without dilation.
 * Everything is an integer and every sum a 64-bit integer atomic: the same bits on every call, and an image gets the same
 * bits alone as in a batch.  One launch; no allocation, no host synchronisation.
 * scratch: vitseg_pr_counts_scratch_bytes(n, S, tol2) device bytes.  The score plane and its dilation live in the workgroup's
 * LDS, so this version asks for 0 bytes and `scratch` may then be NULL; no byte of it is read or written.
 * Each with nothing launched -- VITSEG_EINVAL: a null lowres, gt or counts, kind not 0 / 1, the margin with C < 2, cls
 * outside 0..C-1, bins outside 1..1024, tol2 outside 0..256, ignore_label outside -1..255, a null scratch with a positive
 * size; VITSEG_ESHAPE: C outside 1..255, n outside 1..65535, S outside 1..16384, g outside 1..S; VITSEG_EWORKSPACE: scratch
 * smaller than vitseg_pr_counts_scratch_bytes (0 for a bad shape).
 */
#ifndef VITSEG_CURVES_H
#define VITSEG_CURVES_H

#include "vitseg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITSEG_CURVES_VERSION 100
#define VITSEG_CURVES_MAX_BINS 1024
#define VITSEG_CURVES_MAX_TOL2 256 /* a tolerance of 16 px */

int vitseg_curves_version(void);
size_t vitseg_pr_counts_scratch_bytes(int n, int S, int tol2);
int vitseg_pr_counts(const float* lowres /* [n, C, g, g] */, const uint8_t* gt /* [n, S, S] */, int n, int C, int g, int S,
                     int cls, int kind /* vitseg_conf_kind */, int bins, int tol2, int ignore_label /* -1: none */,
                     int64_t* counts /* [n, bins, 3] */, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VITSEG_CURVES_H */
