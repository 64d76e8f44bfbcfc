// Host-side launcher of the hard-pixel losses (hardloss.hip; include/vitseg_hardloss.h), for vitseg_train.hip's fused branch.
#pragma once
#include "kernels.hpp"
#include "../../include/vitseg_hardloss.h"

namespace vitseg {

size_t hard_loss_scratch_bytes(int B, int S);
// the argument checks of the options alone (VITSEG_EINVAL), for callers that launch other work first; ce may be null
int check_hard_options(const vitseg_hard_options& h, const vitseg_ce_options* ce, int B, int C, int S);
// partial: the call's CE scratch (ce_partial_count doubles).  G, pixel_loss and stats may be null.
int launch_hard_ce_loss(const float* Z, const void* target, int target_is_u8, float* G, double* partial, float* loss, int B,
                        int C, int g, int S, const vitseg_ce_options* ce, const vitseg_hard_options& h, hipStream_t s,
                        float gscale, float* pixel_loss, long long* stats);

}  // namespace vitseg
