// Hard-pixel losses on the fused path (include/vitseg_hardloss.h): focal cross-entropy and online hard example mining on the
// logits regenerated from the low-res head output.  The per-pixel pieces (Pixel, the label rule, the CE gradient term, the block
// and fixed-order sums) are loss_pixel.hpp's, shared with loss_tail.hip; launch_fused_loss there decides when this chain runs.
//
//   ce_i = max(lse - up_y, +0);  q_i = -expm1f(-ce_i);  f_i = w[y] q_i^gamma ce_i;  m_i = q_i^gamma + gamma (1 - q_i) ce_i q_i^(gamma-1)
//   H = { i valid : ce_i >= tau },  tau = min(loss_thresh, k-th largest ce);  loss = sum_H f / sum_H w[y]
//
// Focal alone: loss_tail.hip's count pass + hard_count_finish_kernel (den and n_valid from the targets), hard_focal_kernel (one thread
// per pixel, loss partials and the gradient), hard_focal_finish_kernel.
// With OHEM the gradient of one pixel depends on a rank over the whole batch, so the call is a chain on one stream:
//   A.     hard_plane_kernel     one thread per pixel and step, 4096 pixels per block: ce_i to the fp32 plane (ignored
//                                pixels: -1.0f, sign bit set, which no round matches), n_valid, the histogram of the top 11
//                                of ce_i's 31 key bits;
//   scan   hard_scan_kernel      one block: k from n_valid, the bin that holds rank k counted from the top, prefix and remaining
//                                rank in the state row; leaves the histogram zeroed;
//   rounds hard_hist_kernel + hard_scan_kernel, twice: the next 10 bits over the plane alone, as distance.hip's select (step 5
//                                of its header).  After the last scan the prefix is ce_(k)'s bit pattern and tau is settled;
//   sum    hard_sum_kernel       plane + targets: fp64 per-block partials of sum_H w[y], sum_H f_i and |H|;
//   reduce hard_reduce_kernel    one block, ce_fixed_order_sum of the three; writes den, *loss and stats (the finish);
//   grad   hard_grad_kernel      one thread per pixel, one store per element of G; membership from the plane, tau and den
//                                from the state row; the logits are regenerated for pixels of H only.
// Keys: ce >= +0 or the canonical quiet NaN, so the bit pattern read as an unsigned integer is monotone in the value and NaN
// ranks above +inf.  Histograms and n_valid are integer atomics, the sums fp64 partials in a fixed order: the same bits on
// every call.
#include "hardloss.hpp"
#include "loss_pixel.hpp"

namespace vitseg {
namespace {

constexpr unsigned HARD_NAN = 0x7fc00000u;        // ce of a label outside [0, C) that is not ignored
constexpr unsigned HARD_IGNORED = 0xbf800000u;    // -1.0f: an ignored pixel's entry of the plane
constexpr int HARD_PPB = CE_COUNT_PPB;            // pixels per block of the count and sum passes (4 per thread)
constexpr int HARD_HIST_PPB = 4096;               // pixels per block of pass A and of a histogram round (16 per thread): one
                                                  // flush of the block's bins per 4096 pixels, not per 256
constexpr int HARD_BINS0 = 2048, HARD_BINS = 1024;   // 11 + 10 + 10 key bits
// state row (long long [16]): 0 n_valid | 1 k | 2 prefix | 3 remaining rank (<= 0: nothing to select) | 4 bits of tau | 5 |H|
//                             | 8 den (double) | 9 sum_H f (double)
constexpr int ST_NVALID = 0, ST_K = 1, ST_PREFIX = 2, ST_RANK = 3, ST_TAU = 4, ST_NHARD = 5, ST_DEN = 8, ST_FSUM = 9;
constexpr size_t HARD_STATE_BYTES = 256;

struct Layout {
    size_t state, hist, cpart, spart, plane, total;
    unsigned nc, ns;
};
Layout layout(int B, int S) {
    const size_t npx = (size_t)B * S * S;
    Layout l;
    l.nc = l.ns = (unsigned)((npx + HARD_PPB - 1) / HARD_PPB);
    size_t o = 0;
    l.state = o;  o += HARD_STATE_BYTES;
    l.hist = o;   o += up256(HARD_BINS0 * sizeof(unsigned));
    l.cpart = o;  o += up256((size_t)2 * l.nc * sizeof(double));
    l.spart = o;  o += up256((size_t)3 * l.ns * sizeof(double));
    l.plane = o;  o += up256(npx * sizeof(float));
    l.total = o;
    return l;
}

// q^gamma and m of the header from ce; gamma == 0: both 1 (no pow of anything); q == 0 with gamma > 0: both 0, not 0 * inf
__device__ __forceinline__ void focal_terms(float ce, float gamma, float& mod, float& m) {
    mod = 1.f;
    m = 1.f;
    if (gamma == 0.f) return;
    const float q = -expm1f(-ce);
    if (q == 0.f) {
        mod = 0.f;
        m = 0.f;
        return;
    }
    const float p1 = powf(q, gamma - 1.f);   // one pow: q^gamma = q q^(gamma - 1)
    mod = q * p1;
    m = mod + gamma * (1.f - q) * ce * p1;
}

// lse - picked as the key the selection ranks: -0 becomes +0, any NaN the canonical one (a negative value cannot occur:
// the online log-sum-exp has ssum >= 1)
__device__ __forceinline__ float hard_ce(float lse, float picked, bool bad) {
    float ce = lse - picked;
    if (!(ce > 0.f)) ce = ce == 0.f ? 0.f : __uint_as_float(HARD_NAN);
    return bad ? __uint_as_float(HARD_NAN) : ce;
}

// ---- focal alone ----

// den and n_valid from the two rows of the count pass (launch_ce_count, with_valid)
__global__ __launch_bounds__(1024) void hard_count_finish_kernel(const double* __restrict__ partial, int n, long long* __restrict__ st) {
    __shared__ double red[1024];
    ce_fixed_order_sum(partial, n, red);
    const double den = red[0];
    __syncthreads();   // red[0] is read above by every thread before the second sum overwrites it
    ce_fixed_order_sum(partial + n, n, red);
    if (threadIdx.x == 0) {
        ((double*)st)[ST_DEN] = den;
        st[ST_NVALID] = (long long)red[0];   // a sum of ones below 2^31: exact
    }
}

// the weighted CE with the focal factors: one thread per pixel
template <typename TargetT>
__global__ __launch_bounds__(256) void hard_focal_kernel(const float* __restrict__ Z, const TargetT* __restrict__ target,
                                                         float* __restrict__ G, float* __restrict__ plane,
                                                         double* __restrict__ partial, const long long* __restrict__ st, CeOpt o,
                                                         float gamma, int B, int C, int g, int S, float gscale) {
    __shared__ float wsh[256];
    __shared__ double red[4];
    ce_stage_weights(wsh, o.weight, C);
    const size_t npx = (size_t)B * S * S;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    double local = 0.0;
    if (idx < npx) {
        const Label l = classify_label((long long)target[idx], o, C);
        const Pixel px(Z, idx, C, g, S);
        const size_t gbase = (size_t)px.b * C * S * S + idx % ((size_t)S * S);   // element (b, 0, Y, X) of G
        if (l.kept) {   // the kept pixels first, the zeros of the ignored ones behind them (ce_loss_opts_kernel, loss_tail.hip)
            float lse, picked, mod, m;
            px.lse_picked(l.t, lse, picked);
            const float ce = hard_ce(lse, picked, l.bad);
            focal_terms(ce, gamma, mod, m);
            const float wy = l.bad ? 1.f : wsh[l.t];
            local = (double)(wy * mod) * (double)ce;
            if (plane) plane[idx] = ce;
            if (G) {
                const float inv = gscale / (float)((const double*)st)[ST_DEN];   // den == 0: inf, and 0 * inf = NaN
                const float a = wy * m;
                for (int c = 0; c < C; ++c) {
                    const float pc = expf(px.logit(c) - lse);
                    G[gbase + (size_t)c * S * S] = l.bad ? NAN : ce_grad(a, pc, c == l.t, inv);
                }
            }
        } else {
            if (plane) plane[idx] = __uint_as_float(HARD_IGNORED);
            if (G)
                for (int c = 0; c < C; ++c) G[gbase + (size_t)c * S * S] = 0.0f;
        }
    }
    const double sum = block_sum4(local, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

__global__ __launch_bounds__(1024) void hard_focal_finish_kernel(const double* __restrict__ partial, int n,
                                                                 const long long* __restrict__ st, float* __restrict__ loss,
                                                                 long long* __restrict__ stats) {
    __shared__ double red[1024];
    ce_fixed_order_sum(partial, n, red);
    if (threadIdx.x == 0) {
        *loss = (float)(red[0] * (1.0 / ((const double*)st)[ST_DEN]));   // den == 0: 0 * inf = NaN, torch's 0 / 0
        if (stats) {   // OHEM off: every valid pixel is hard, tau = +0
            stats[0] = st[ST_NVALID];
            stats[1] = 0;
            stats[2] = st[ST_NVALID];
            stats[3] = 0;
        }
    }
}

// ---- OHEM ----

// pass A: one thread per pixel and step; a block walks 4096 consecutive pixels in 16 steps
template <typename TargetT>
__global__ __launch_bounds__(256) void hard_plane_kernel(const float* __restrict__ Z, const TargetT* __restrict__ target,
                                                         float* __restrict__ plane, unsigned* __restrict__ hist,
                                                         long long* __restrict__ st, CeOpt o, int B, int C, int g, int S) {
    __shared__ unsigned h[HARD_BINS0];
    __shared__ unsigned nvalid;
    for (int b = threadIdx.x; b < HARD_BINS0; b += 256) h[b] = 0;
    if (threadIdx.x == 0) nvalid = 0;
    __syncthreads();
    const size_t npx = (size_t)B * S * S;
    const size_t base = (size_t)blockIdx.x * HARD_HIST_PPB + threadIdx.x;
    unsigned mine = 0;   // valid pixels of this wavefront, counted by its first lane
    for (int k = 0; k < HARD_HIST_PPB / 256; ++k) {
        const size_t idx = base + (size_t)k * 256;
        bool valid = false;
        if (idx < npx) {
            const Label l = classify_label((long long)target[idx], o, C);
            if (!l.kept) {
                plane[idx] = __uint_as_float(HARD_IGNORED);
            } else {
                const Pixel px(Z, idx, C, g, S);
                float lse, picked;
                px.lse_picked(l.t, lse, picked);
                const float ce = hard_ce(lse, picked, l.bad);
                plane[idx] = ce;
                atomicAdd(&h[__float_as_uint(ce) >> 20], 1u);   // the sign bit is clear: a bin below 2048
                valid = true;
            }
        }
        mine += (unsigned)__popcll(__ballot(valid));
    }
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&nvalid, mine);
    __syncthreads();
    for (int b = threadIdx.x; b < HARD_BINS0; b += 256)
        if (h[b]) atomicAdd(&hist[b], h[b]);
    if (threadIdx.x == 0 && nvalid) atomicAdd((unsigned long long*)&st[ST_NVALID], (unsigned long long)nvalid);
}

// rounds 1 and 2: among the keys whose bits above `hs` equal the prefix, count the next 10 bits
__global__ __launch_bounds__(256) void hard_hist_kernel(const float* __restrict__ plane, unsigned* __restrict__ hist,
                                                        const long long* __restrict__ st, size_t npx, int hs) {
    __shared__ unsigned h[HARD_BINS];
    if (st[ST_RANK] <= 0) return;   // k == 0: tau is the threshold
    const unsigned prefix = (unsigned)st[ST_PREFIX];
    for (int b = threadIdx.x; b < HARD_BINS; b += 256) h[b] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * HARD_HIST_PPB + threadIdx.x;
#pragma unroll 4
    for (int k = 0; k < HARD_HIST_PPB / 256; ++k) {
        const size_t idx = base + (size_t)k * 256;
        if (idx < npx) {
            const unsigned key = __float_as_uint(plane[idx]);   // an ignored pixel's sign bit matches no prefix
            if ((key >> hs) == prefix) atomicAdd(&h[(key >> (hs - 10)) & (HARD_BINS - 1)], 1u);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < HARD_BINS; b += 256)
        if (h[b]) atomicAdd(&hist[b], h[b]);
}

// one block of 1024 threads.  Round 0 turns n_valid into k; every round finds the bin that holds rank `rank` counted from
// the largest key down, appends it to the prefix and leaves the rank within that bin.  The histogram is left zeroed.
__global__ __launch_bounds__(1024) void hard_scan_kernel(unsigned* __restrict__ hist, long long* __restrict__ st, float loss_thresh,
                                                         long long min_kept, int keep_q16, int round) {
    __shared__ unsigned sc[HARD_BINS0];
    __shared__ long long res[2];
    const int t = threadIdx.x;
    const int nb = round == 0 ? HARD_BINS0 : HARD_BINS;
    long long rank, prefix = 0, k = 0;
    if (round == 0) {
        const long long n = st[ST_NVALID];
        const long long want = (n * (long long)keep_q16 + 65535) >> 16;   // ceil(n keep_q16 / 65536), n < 2^31
        k = min(n, max(min_kept, want));
        rank = k;
    } else {
        rank = st[ST_RANK];
        prefix = st[ST_PREFIX];
    }
    if (round != 0 && rank <= 0) return;   // nothing was counted: the histogram is still zero
    for (int j = t; j < nb; j += 1024) {   // reversed, so that the inclusive scan counts the keys at or above a bin
        sc[j] = hist[nb - 1 - j];
        hist[nb - 1 - j] = 0;
    }
    __syncthreads();   // (also: every thread has read the state row before thread 0 rewrites it)
    const unsigned thresh_bits = __float_as_uint(loss_thresh);
    if (rank <= 0) {   // round 0 with k == 0
        if (t == 0) {
            st[ST_K] = 0;
            st[ST_RANK] = 0;
            st[ST_TAU] = thresh_bits;
        }
        return;
    }
    const bool two = nb > 1024;
    for (int d = 1; d < nb; d <<= 1) {
        const unsigned a0 = t >= d ? sc[t - d] : 0u;
        const unsigned a1 = two ? sc[t + 1024 - d] : 0u;   // d <= 1024
        __syncthreads();
        sc[t] += a0;
        if (two) sc[t + 1024] += a1;
        __syncthreads();
    }
    for (int j = t; j < nb; j += 1024) {
        const long long incl = sc[j], excl = j ? sc[j - 1] : 0;
        if (excl < rank && rank <= incl) {   // exactly one j: rank <= the number of keys under the prefix
            res[0] = (prefix << (round == 0 ? 11 : 10)) | (long long)(nb - 1 - j);
            res[1] = rank - excl;
        }
    }
    __syncthreads();
    if (t == 0) {
        st[ST_PREFIX] = res[0];
        st[ST_RANK] = res[1];
        if (round == 0) st[ST_K] = k;
        if (round == 2) st[ST_TAU] = min((unsigned)res[0], thresh_bits);   // both >= +0: the smaller pattern is the smaller value
    }
}

__device__ __forceinline__ bool hard_member(unsigned key, unsigned tau) { return !(key >> 31) && key >= tau; }

template <typename TargetT>
__global__ __launch_bounds__(256) void hard_sum_kernel(const float* __restrict__ plane, const TargetT* __restrict__ target,
                                                       const long long* __restrict__ st, CeOpt o, float gamma,
                                                       double* __restrict__ partial, size_t npx, int C) {
    __shared__ float wsh[256];
    __shared__ double red[3][4];
    ce_stage_weights(wsh, o.weight, C);
    const unsigned tau = (unsigned)st[ST_TAU];
    const size_t base = (size_t)blockIdx.x * HARD_PPB + threadIdx.x;
    double lw = 0.0, lf = 0.0, ln = 0.0;
#pragma unroll
    for (int k = 0; k < HARD_PPB / 256; ++k) {
        const size_t idx = base + (size_t)k * 256;
        if (idx < npx) {
            const float ce = plane[idx];
            if (hard_member(__float_as_uint(ce), tau)) {
                const Label l = classify_label((long long)target[idx], o, C);   // (a member of H is not ignored)
                const float wy = l.bad ? 1.f : wsh[l.t];
                float mod, m;
                focal_terms(ce, gamma, mod, m);
                lw += (double)wy;
                lf += (double)(wy * mod) * (double)ce;
                ln += 1.0;
            }
        }
    }
    const double sw = block_sum4(lw, red[0]), sf = block_sum4(lf, red[1]), sn = block_sum4(ln, red[2]);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = sw;
        partial[gridDim.x + blockIdx.x] = sf;
        partial[2 * (size_t)gridDim.x + blockIdx.x] = sn;
    }
}

// the three fixed-order sums and the finish: den for the gradient kernel, *loss, stats
__global__ __launch_bounds__(1024) void hard_reduce_kernel(const double* __restrict__ partial, int n, long long* __restrict__ st,
                                                           float* __restrict__ loss, long long* __restrict__ stats) {
    __shared__ double red[1024];
    ce_fixed_order_sum(partial, n, red);
    const double den = red[0];
    __syncthreads();
    ce_fixed_order_sum(partial + n, n, red);
    const double fsum = red[0];
    __syncthreads();
    ce_fixed_order_sum(partial + 2 * (size_t)n, n, red);
    if (threadIdx.x == 0) {
        const long long nhard = (long long)red[0];
        ((double*)st)[ST_DEN] = den;
        ((double*)st)[ST_FSUM] = fsum;
        st[ST_NHARD] = nhard;
        *loss = (float)(fsum * (1.0 / den));   // den == 0: 0 * inf = NaN
        if (stats) {
            stats[0] = st[ST_NVALID];
            stats[1] = st[ST_K];
            stats[2] = nhard;
            stats[3] = st[ST_TAU];
        }
    }
}

template <typename TargetT>
__global__ __launch_bounds__(256) void hard_grad_kernel(const float* __restrict__ Z, const TargetT* __restrict__ target,
                                                        const float* __restrict__ plane, float* __restrict__ G,
                                                        const long long* __restrict__ st, CeOpt o, float gamma, int B, int C,
                                                        int g, int S, float gscale) {
    __shared__ float wsh[256];
    ce_stage_weights(wsh, o.weight, C);
    const size_t npx = (size_t)B * S * S;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npx) return;
    const size_t plane_px = (size_t)S * S;
    const size_t gbase = (idx / plane_px) * C * plane_px + idx % plane_px;
    const float ce = plane[idx];
    if (!hard_member(__float_as_uint(ce), (unsigned)st[ST_TAU])) {   // ignored, or valid and easy
        for (int c = 0; c < C; ++c) G[gbase + (size_t)c * plane_px] = 0.0f;
        return;
    }
    const Label l = classify_label((long long)target[idx], o, C);   // (a member of H is not ignored)
    const Pixel px(Z, idx, C, g, S);
    float lse, picked, mod, m;
    px.lse_picked(l.t, lse, picked);
    focal_terms(ce, gamma, mod, m);
    const float inv = gscale / (float)((const double*)st)[ST_DEN];
    const float a = (l.bad ? 1.f : wsh[l.t]) * m;
    for (int c = 0; c < C; ++c) {
        const float pc = expf(px.logit(c) - lse);
        G[gbase + (size_t)c * plane_px] = l.bad ? NAN : ce_grad(a, pc, c == l.t, inv);
    }
}

}  // namespace

bool hard_ohem_on(const vitseg_hard_options& h) { return !(h.loss_thresh == INFINITY && h.min_kept == 0 && h.keep_q16 == 0); }

size_t hard_loss_scratch_bytes(int B, int S) {
    if (B < 1 || S < 1 || (size_t)B * S * S >= ((size_t)1 << 31)) return 0;
    return layout(B, S).total;
}

int check_hard_options(const vitseg_hard_options& h, int B, int C, int S) {
    VITSEG_CHECK_ARG(h.gamma >= 0.f && h.gamma < INFINITY, VITSEG_EINVAL, "hard loss: gamma %f is negative or not finite",
                     (double)h.gamma);   // (a NaN fails both)
    VITSEG_CHECK_ARG(h.loss_thresh >= 0.f, VITSEG_EINVAL, "hard loss: loss_thresh %f is negative or NaN", (double)h.loss_thresh);
    VITSEG_CHECK_ARG(h.min_kept >= 0, VITSEG_EINVAL, "hard loss: min_kept %lld < 0", (long long)h.min_kept);
    VITSEG_CHECK_ARG(h.keep_q16 >= 0 && h.keep_q16 <= 65536, VITSEG_EINVAL, "hard loss: keep_q16 %d outside 0..65536", h.keep_q16);
    VITSEG_CHECK_ARG(B >= 1 && S >= 1 && (size_t)B * S * S < ((size_t)1 << 31), VITSEG_EINVAL,
                     "hard loss: %d x %d x %d pixels (1 .. 2^31 - 1)", B, S, S);
    VITSEG_CHECK_ARG(C >= 1 && C <= 255, VITSEG_EINVAL, "hard loss: %d classes (1..255)", C);
    VITSEG_CHECK_ARG(h.scratch && ((uintptr_t)h.scratch & 7) == 0, VITSEG_EINVAL, "hard loss: scratch is null or not 8-byte aligned");
    VITSEG_CHECK_ARG(h.scratch_bytes >= hard_loss_scratch_bytes(B, S), VITSEG_EINVAL, "hard loss: scratch %zu < required %zu",
                     h.scratch_bytes, hard_loss_scratch_bytes(B, S));
    return VITSEG_OK;
}

int launch_hard_loss(const float* Z, const void* target, int target_is_u8, float* G, double* partial, float* loss, int B, int C,
                     int g, int S, const FusedLoss& f, hipStream_t s, float gscale) {
    const vitseg_hard_options& h = *f.hard;
    const size_t npx = (size_t)B * S * S;
    const Layout l = layout(B, S);
    char* base = (char*)h.scratch;
    long long* st = (long long*)(base + l.state);
    unsigned* hist = (unsigned*)(base + l.hist);
    double* cpart = (double*)(base + l.cpart);
    double* spart = (double*)(base + l.spart);
    float* plane = f.pixel_loss ? f.pixel_loss : (float*)(base + l.plane);
    const unsigned nb = (unsigned)((npx + 255) / 256);
    const unsigned nh = (unsigned)((npx + HARD_HIST_PPB - 1) / HARD_HIST_PPB);
    const CeOpt o = ce_opt_of(f.ce, false);
    if (!hard_ohem_on(h)) {
        if (int rc = launch_ce_count(target, target_is_u8, o, cpart, npx, C, true, s)) return rc;
        hipLaunchKernelGGL(hard_count_finish_kernel, dim3(1), dim3(1024), 0, s, cpart, (int)l.nc, st);
        VITSEG_LAUNCH_CHECK("hard count finish");
        with_target_type(target, target_is_u8, [&](auto* t) {
            hipLaunchKernelGGL(hard_focal_kernel<target_t<decltype(t)>>, dim3(nb), dim3(256), 0, s, Z, t, G, f.pixel_loss, partial, st, o,
                               h.gamma, B, C, g, S, gscale);
        });
        VITSEG_LAUNCH_CHECK("hard focal");
        hipLaunchKernelGGL(hard_focal_finish_kernel, dim3(1), dim3(1024), 0, s, partial, (int)nb, st, loss, f.stats);
        VITSEG_LAUNCH_CHECK("hard focal finish");
        return VITSEG_OK;
    }
    // the state row and the histogram are adjacent: n_valid and every bin start at 0 (each scan leaves the bins zeroed again)
    hipError_t e = hipMemsetAsync(base + l.state, 0, l.cpart - l.state, s);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(hard loss state)");
    with_target_type(target, target_is_u8, [&](auto* t) {
        hipLaunchKernelGGL(hard_plane_kernel<target_t<decltype(t)>>, dim3(nh), dim3(256), 0, s, Z, t, plane, hist, st, o, B, C, g, S);
    });
    VITSEG_LAUNCH_CHECK("hard plane");
    const float thresh = h.loss_thresh == 0.f ? 0.f : h.loss_thresh;   // -0 -> +0
    for (int round = 0; round < 3; ++round) {
        if (round) {
            hipLaunchKernelGGL(hard_hist_kernel, dim3(nh), dim3(256), 0, s, plane, hist, st, npx, 30 - 10 * round);
            VITSEG_LAUNCH_CHECK("hard histogram");
        }
        hipLaunchKernelGGL(hard_scan_kernel, dim3(1), dim3(1024), 0, s, hist, st, thresh, (long long)h.min_kept, h.keep_q16, round);
        VITSEG_LAUNCH_CHECK("hard scan");
    }
    with_target_type(target, target_is_u8, [&](auto* t) {
        hipLaunchKernelGGL(hard_sum_kernel<target_t<decltype(t)>>, dim3(l.ns), dim3(256), 0, s, plane, t, st, o, h.gamma, spart, npx, C);
    });
    VITSEG_LAUNCH_CHECK("hard sum");
    hipLaunchKernelGGL(hard_reduce_kernel, dim3(1), dim3(1024), 0, s, spart, (int)l.ns, st, loss, f.stats);
    VITSEG_LAUNCH_CHECK("hard reduce");
    if (G) {
        with_target_type(target, target_is_u8, [&](auto* t) {
            hipLaunchKernelGGL(hard_grad_kernel<target_t<decltype(t)>>, dim3(nb), dim3(256), 0, s, Z, t, plane, G, st, o, h.gamma, B, C, g,
                               S, gscale);
        });
        VITSEG_LAUNCH_CHECK("hard gradient");
    }
    return VITSEG_OK;
}

}  // namespace vitseg

extern "C" {

int vitseg_hardloss_version(void) { return VITSEG_HARDLOSS_VERSION; }

size_t vitseg_hard_loss_scratch_bytes(int batch, int S) { return vitseg::hard_loss_scratch_bytes(batch, S); }

int vitseg_hard_ce_loss(const float* lowres, const void* target, int target_is_u8, float* grad_logits, void* scratch, float* loss,
                        int batch, int C, int g, int S, const vitseg_ce_options* ce_opts, const vitseg_hard_options* hard,
                        float loss_scale, float* pixel_loss, int64_t* stats, void* stream) {
    VITSEG_CHECK_ARG(batch >= 1 && C >= 1 && g >= 1 && S >= g, VITSEG_EINVAL, "hard_ce_loss: bad shape");
    VITSEG_CHECK_ARG(hard, VITSEG_EINVAL, "hard_ce_loss: the hard options are null");
    vitseg::FusedLoss f;
    f.ce = ce_opts;
    f.hard = hard;
    f.pixel_loss = pixel_loss;
    f.stats = (long long*)stats;
    return vitseg::launch_fused_loss(lowres, target, target_is_u8, grad_logits, (double*)scratch, loss, batch, C, g, S, f,
                                     (hipStream_t)stream, loss_scale);
}

}  // extern "C"
