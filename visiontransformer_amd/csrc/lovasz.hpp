// The Lovasz-Softmax term (lovasz.hip; include/vitseg_lovasz.h) as launch_fused_loss (loss_tail.hip) sees it: it leaves what
// the clDice term leaves, a CldTerm (cldice.hpp), so ce_cldice_kernel and ce_finish_kernel run on it as they are.
#pragma once
#include "../../include/vitseg_lovasz.h"
#include "cldice.hpp"

namespace vitseg {

size_t lovasz_scratch_bytes(int B, int K, int S);
// the argument checks of the options alone (VITSEG_EINVAL)
int check_lovasz_options(const vitseg_lovasz_options& c, int B, int C, int S);

// the chain for checked options (weight != 0): planes, the sort, ranks, finish; want_grad: the g planes
int launch_lovasz_term(const float* Z, const void* target, int target_is_u8, const CeOpt& o, int B, int C, int g, int S,
                       const vitseg_lovasz_options& c, bool want_grad, float gscale, hipStream_t s, CldTerm* out);

}  // namespace vitseg
