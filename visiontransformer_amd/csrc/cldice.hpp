// The soft-clDice term (cldice.hip; include/vitseg_cldice.h) as launch_fused_loss (loss_tail.hip) sees it.
#pragma once
#include "../../include/vitseg_cldice.h"
#include "kernels.hpp"

namespace vitseg {

struct CeOpt;   // loss_pixel.hpp

// class -> 1 + its index among the listed classes (0: not listed), a kernel argument of the loss kernel; list: the listed
// classes in order, of the plane pass
struct CldClassMap {
    unsigned char slot[256];
};
struct CldClassList {
    unsigned char cls[256];
};

size_t cldice_scratch_bytes(int B, int K, int S, int iters);
// the argument checks of the options alone (VITSEG_EINVAL)
int check_cldice_options(const vitseg_cldice_options& c, int B, int C, int S);

// what the chain leaves on the device for the loss and the finish kernels
struct CldTerm {
    const double* extra;    // [0] weight * cldice, [1] cldice
    const float* gplanes;   // fp32 [K, B, S, S]: d (weight * cldice) / d p_c * gscale (null without the gradient)
    CldClassMap map;
};
// the chain for checked options (weight != 0): planes, stages, sums, finish and, want_grad, the adjoint
int launch_cldice_term(const float* Z, const void* target, int target_is_u8, const CeOpt& o, int B, int C, int g, int S,
                       const vitseg_cldice_options& c, bool want_grad, float gscale, hipStream_t s, CldTerm* out);

}  // namespace vitseg
