// The hard-pixel losses (hardloss.hip; include/vitseg_hardloss.h) as launch_fused_loss (loss_tail.hip) sees them.
#pragma once
#include "../../include/vitseg_hardloss.h"
#include "kernels.hpp"

namespace vitseg {

struct CeOpt;   // loss_pixel.hpp: the CE options as the kernels take them
CeOpt ce_opt_of(const vitseg_ce_options* ce, bool with_smoothing = true);   // ce may be null: no option set
// the count pass over the targets (loss_tail.hip), shared by the CE options and the focal loss: partial[0 .. n) the per-block
// sums of the kept pixels' weights, n = ceil(npx / CE_COUNT_PPB); with_valid: partial[n .. 2 n) the per-block numbers of kept
// pixels as well
int launch_ce_count(const void* target, int target_is_u8, const CeOpt& o, double* partial, size_t npx, int C, bool with_valid,
                    hipStream_t s);

size_t hard_loss_scratch_bytes(int B, int S);
// the argument checks of the hard options alone (VITSEG_EINVAL)
int check_hard_options(const vitseg_hard_options& h, int B, int C, int S);
bool hard_ohem_on(const vitseg_hard_options& h);
// the focal / OHEM chain for checked options (f.hard is set; f.ce, f.pixel_loss and f.stats may be null).  partial: the call's
// CE scratch (ce_partial_count doubles).  G may be null.
int launch_hard_loss(const float* Z, const void* target, int target_is_u8, float* G, double* partial, float* loss, int B, int C,
                     int g, int S, const FusedLoss& f, hipStream_t s, float gscale);

}  // namespace vitseg
