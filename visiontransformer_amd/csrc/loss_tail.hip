// The fused losses on the upsampled logits: cross-entropy, its options (ignore_index, class weights, label smoothing) and the
// soft-Dice term, and the one host launcher of every fused loss (launch_fused_loss; the focal / OHEM chain is hardloss.hip).
// The logits are re-generated from the low-res map (the exact bilinear arithmetic of upsample_kernel, decoder_tail.hip)
// instead of being read back from HBM, so a loss costs one pass over the targets.  The per-pixel pieces: loss_pixel.hpp.
#include <float.h>

#include "cldice.hpp"
#include "hardloss.hpp"
#include "kernels.hpp"
#include "loss_pixel.hpp"
#include "lovasz.hpp"

namespace vitseg {
namespace {

// nn.CrossEntropyLoss() (model/CE/classes.py:268,280): mean over B*S*S pixels of logsumexp_c(logit) - logit[target].
// Optionally writes G = d loss / d logits = (softmax - onehot) gscale / (B*S*S) (fp32 [B, C, S, S]) for the backward pass;
// gscale: the upstream d(total loss) / d(this loss), e.g. 1 / accumulation.  Deterministic: per-block partial sums in fp64,
// reduced in a fixed order by ce_finish_kernel.  No weights, no denominator read, no LDS beyond red[4]: the loss of the
// measured training step, and for that reason the one loss kernel whose control flow is still written out here: built from
// Pixel, lse_step and block_sum4 it computes the same bits from differently allocated registers, and its device code is
// held byte for byte.  It shares the label rule and the bilinear expression.  ignore_index is not supported here
// (ce_loss_opts_kernel).
template <typename TargetT>
__global__ __launch_bounds__(256) void ce_loss_kernel(const float* __restrict__ Z, const TargetT* __restrict__ target,
                                                      float* __restrict__ G, double* __restrict__ partial, int B, int C,
                                                      int g, int S, float gscale) {
    __shared__ double red[4];
    const size_t npx = (size_t)B * S * S;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    double local = 0.0;
    if (idx < npx) {
        const int X = (int)(idx % S), Y = (int)((idx / S) % S), b = (int)(idx / ((size_t)S * S));
        const float scale = (float)g / (float)S;
        int y0, y1, x0, x1;
        float wy0, wy1, wx0, wx1;
        taps(Y, scale, g, y0, y1, wy0, wy1);
        taps(X, scale, g, x0, x1, wx0, wx1);
        const Label l = classify_label((long long)target[idx], C);
        auto logit = [&](int c) {
            const float* zt = Z + (((size_t)b * C + c) * g + y0) * g;
            const float* zb = Z + (((size_t)b * C + c) * g + y1) * g;
            return bilinear_fma(zt, zb, x0, x1, wx0, wx1, wy0, wy1);
        };
        float m = -INFINITY, ssum = 0.f, picked = 0.f;
        for (int c = 0; c < C; ++c) {  // online logsumexp
            const float v = logit(c);
            if (c == l.t) picked = v;
            const float mn = fmaxf(m, v);
            ssum = ssum * expf(m - mn) + expf(v - mn);
            m = mn;
        }
        const float lse = m + logf(ssum);
        local = l.bad ? (double)NAN : (double)(lse - picked);
        if (G) {
            const float inv = gscale / (float)npx;
            for (int c = 0; c < C; ++c) {
                const float pc = expf(logit(c) - lse);
                G[(((size_t)b * C + c) * S + Y) * S + X] = l.bad ? NAN : (pc - (c == l.t ? 1.f : 0.f)) * inv;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- cross-entropy with options: F.cross_entropy(up, y, weight=w, ignore_index=ii, label_smoothing=eps) ----
//   keep = (y != ii);  den = sum_keep w[y];
//   loss = [ (1 - eps) sum_keep w[y] (lse - z_y) + (eps / C) sum_keep sum_c w[c] (lse - z_c) ] / den
//   dL/dz_c = keep [ (1 - eps) w[y] (p_c - 1[c = y]) + (eps / C) (p_c sum_k w[k] - w[c]) ] gscale / den
// The mean's denominator depends on the targets, and the gradient kernel needs it before it writes G: a count pass over
// the targets alone (ce_count_kernel: fp64 per-block partials of w[y] keep) and a fixed-order reduce to one device double
// (sum_rows_kernel) run first on the same stream -- no atomics, no host read.  A bad label (loss_pixel.hpp, Label) counts 1
// in den, as it does in the plain mean over B S S pixels, so that every other pixel keeps the gradient it would have had.
// The picked-class sum and the smoothing sum are reduced apart and each is divided by den, and each gradient term is scaled
// by 1 / den on its own, as torch forms them: with den == 0 the picked-class part is 0 * inf = NaN whatever the smoothing
// part holds (kept pixels of weight 0 under smoothing: NaN, not inf).
// With no label ignored, no weights and eps = 0 every product is by 1 or adds +0: the bits of ce_loss_kernel.

// VALID: the number of kept pixels beside their summed weights (the focal loss), partial[0 .. n) and partial[n .. 2 n)
template <typename TargetT, bool VALID>
__global__ __launch_bounds__(256) void ce_count_kernel(const TargetT* __restrict__ target, CeOpt o, double* __restrict__ partial,
                                                       size_t npx, int C) {
    __shared__ float wsh[256];
    __shared__ double red[VALID ? 2 : 1][4];
    ce_stage_weights(wsh, o.weight, C);
    const size_t base = (size_t)blockIdx.x * CE_COUNT_PPB + threadIdx.x;
    double local = 0.0, cnt = 0.0;
#pragma unroll
    for (int k = 0; k < CE_COUNT_PPB / 256; ++k) {   // consecutive lanes read consecutive targets
        const size_t idx = base + (size_t)k * 256;
        if (idx < npx) {
            const Label l = classify_label((long long)target[idx], o, C);
            local += !l.kept ? 0.0 : (l.bad ? 1.0 : (double)wsh[l.bad ? 0 : l.t]);
            if (VALID) cnt += !l.kept ? 0.0 : 1.0;
        }
    }
    const double a = block_sum4(local, red[0]);
    if (threadIdx.x == 0) partial[blockIdx.x] = a;
    if (VALID) {
        const double n = block_sum4(cnt, red[1]);
        if (threadIdx.x == 0) partial[gridDim.x + blockIdx.x] = n;
    }
}

// out[r] = the fixed-order sum of row r of partial [rows][n]; one block each (the denominator: one row; the Dice sums
// I | P | T: 3 C rows)
__global__ __launch_bounds__(1024) void sum_rows_kernel(const double* __restrict__ partial, int n, double* __restrict__ out) {
    __shared__ double red[1024];
    ce_fixed_order_sum(partial + (size_t)blockIdx.x * n, n, red);
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// ---- CE + soft Dice (include/vitseg.h, vitseg_ce_dice_loss) ----
//   I_c = sum_keep p_c t_c;  P_c = sum_keep p_c;  T_c = sum_keep t_c;  D_c = P_c + T_c + smooth  (c in K, the classes counted)
//   dice = mean_K [ 1 - (2 I_c + smooth) / D_c ]
//   a_c = -[2 t_c D_c - (2 I_c + smooth)] / (|K| D_c^2);  d dice / d z_c = p_c (a_c - sum_k a_k p_k)
// The sums run over the whole batch, so they are on the device before the gradient kernel starts: dice_sum_kernel leaves
// per-block fp64 partials, sum_rows_kernel adds them in the fixed order, and ce_dice_kernel reads the 3 C doubles.
// A block of the sum pass covers DICE_PPT * 256 = 2048 consecutive pixels, 8 per thread: the wavefront reduce of a class
// (two doubles and a count) is paid once per 8 pixels, and the partial table of 32 x 17 x 512^2 is 4096 blocks x 51 doubles
// = 1.6 MB where one block per 256 pixels would write 13 MB.  16 per thread would halve it again but holds 16 pixels' taps
// and lse in registers (9 each).
constexpr int DICE_PPT = 8;

template <typename TargetT>
__global__ __launch_bounds__(256) void dice_sum_kernel(const float* __restrict__ Z, const TargetT* __restrict__ target,
                                                       long long ignore, int has_ignore, double* __restrict__ partial,
                                                       unsigned nblk, int B, int C, int g, int S) {
    __shared__ double red[2][4][2];
    __shared__ int cred[2][4];
    const size_t npx = (size_t)B * S * S;
    const size_t base = (size_t)blockIdx.x * (256 * DICE_PPT) + threadIdx.x;
    const float scale = (float)g / (float)S;
    // per pixel, packed (Pixel would hold 13 registers each): the top-left tap's row, the two columns, the row step, the two
    // upper weights, the label
    const float* zp[DICE_PPT];
    int x0[DICE_PPT], x1[DICE_PPT], dy[DICE_PPT], t[DICE_PPT];   // t: -2 = not counted (ignored / past the end), -1 = bad label
    float wx1[DICE_PPT], wy1[DICE_PPT], m[DICE_PPT], ssum[DICE_PPT];
#pragma unroll
    for (int k = 0; k < DICE_PPT; ++k) {   // consecutive lanes read consecutive targets
        const size_t idx = base + (size_t)k * 256;
        zp[k] = Z;
        x0[k] = x1[k] = dy[k] = 0;
        wx1[k] = wy1[k] = 0.f;
        t[k] = -2;
        m[k] = -INFINITY;
        ssum[k] = 0.f;
        if (idx < npx) {
            const Label l = classify_label((long long)target[idx], CeOpt{nullptr, ignore, has_ignore, 0.f}, C);
            if (l.kept) {
                const int X = (int)(idx % S), Y = (int)((idx / S) % S), b = (int)(idx / ((size_t)S * S));
                int y0, y1;
                float w0;
                taps(Y, scale, g, y0, y1, w0, wy1[k]);
                taps(X, scale, g, x0[k], x1[k], w0, wx1[k]);
                zp[k] = Z + ((size_t)b * C * g + y0) * g;
                dy[k] = (y1 - y0) * g;
                t[k] = l.t;
            }
        }
    }
    const int plane = g * g;
    auto logit = [&](int k, int c) {   // Pixel::logit from the packed form (w0 = 1 - w1 as taps() forms it)
        const float* zt = zp[k] + (size_t)c * plane;
        return bilinear_fma(zt, zt + dy[k], x0[k], x1[k], __fsub_rn(1.f, wx1[k]), wx1[k], __fsub_rn(1.f, wy1[k]), wy1[k]);
    };
    for (int c = 0; c < C; ++c) {   // online logsumexp, every pixel of the thread in step
#pragma unroll
        for (int k = 0; k < DICE_PPT; ++k)
            if (t[k] != -2) lse_step(logit(k, c), m[k], ssum[k]);
    }
#pragma unroll
    for (int k = 0; k < DICE_PPT; ++k)   // m becomes lse; a bad label poisons P_c of every class
        m[k] = t[k] == -1 ? NAN : m[k] + logf(ssum[k]);
    for (int c = 0; c < C; ++c) {
        double accP = 0.0, accI = 0.0;
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < DICE_PPT; ++k)
            if (t[k] != -2) {
                const double pc = (double)expf(logit(k, c) - m[k]);
                accP += pc;
                if (t[k] == c) {
                    accI += pc;
                    ++cnt;
                }
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            accP += __shfl_xor(accP, o, 64);
            accI += __shfl_xor(accI, o, 64);
            cnt += __shfl_xor(cnt, o, 64);
        }
        const int par = c & 1;   // two sets of slots: one barrier per class
        if ((threadIdx.x & 63) == 0) {
            red[par][threadIdx.x >> 6][0] = accI;
            red[par][threadIdx.x >> 6][1] = accP;
            cred[par][threadIdx.x >> 6] = cnt;
        }
        __syncthreads();
        if (threadIdx.x < 2)
            partial[((size_t)threadIdx.x * C + c) * nblk + blockIdx.x] =
                (red[par][0][threadIdx.x] + red[par][1][threadIdx.x]) + (red[par][2][threadIdx.x] + red[par][3][threadIdx.x]);
        else if (threadIdx.x == 2)
            partial[((size_t)2 * C + c) * nblk + blockIdx.x] = (double)((cred[par][0] + cred[par][1]) + (cred[par][2] + cred[par][3]));
    }
}

struct DiceOpt {
    float cw, dw, smooth;   // ce_weight, dice_weight, smooth
    int c0;                 // first class counted (0, or 1 without the background)
    int use_ce, use_dice;   // the term is formed (its weight is not 0)
};
constexpr DiceOpt CE_ALONE{1.f, 0.f, 0.f, 0, 1, 0};

// The body of ce_loss_opts_kernel (!DICE) and ce_dice_kernel (DICE): the CE options and, DICE, the Dice gradient; one thread
// per pixel, one store per element of G.  den: the device double of the count pass, or (DICE only) null: no CE options,
// den_plain = B S S.  sums (DICE): I | P | T, C doubles each.  !DICE: den_plain, sums and d are not read, the CE term is
// formed and its gradient is not scaled by a ce_weight.  CLD (with DICE; d may leave either term out): the soft-clDice term's
// gradient by the softmax chain rule, p_j (g_j - sum_c g_c p_c), from the planes gcl [K, B, S, S] of g_c = d term / d p_c
// (cldice.hip; already scaled by the term's weight and gscale) of the classes cmap lists, inside the same one store.
template <typename TargetT, bool DICE, bool CLD = false>
__device__ __forceinline__ void ce_opts_pixel(const float* __restrict__ Z, const TargetT* __restrict__ target,
                                              float* __restrict__ G, double* __restrict__ partial,
                                              double* __restrict__ spartial, const double* __restrict__ den, double den_plain,
                                              const double* __restrict__ sums, const CeOpt& o, const DiceOpt& d, int B, int C,
                                              int g, int S, float gscale, const float* __restrict__ gcl = nullptr,
                                              const CldClassMap* cmap = nullptr) {
    __shared__ float wsh[256], a0sh[DICE ? 256 : 1], a1sh[DICE ? 256 : 1];   // a_c of a pixel whose label is not c / is c
    __shared__ double red[4], sred[4];
    const bool use_ce = !DICE || d.use_ce, use_dice = DICE && d.use_dice;
    if (use_dice && (int)threadIdx.x < C) {
        const int c = threadIdx.x;
        float a0 = 0.f, a1 = 0.f;
        if (c >= d.c0) {
            const double sm = (double)d.smooth, num = 2.0 * sums[c] + sm, D = sums[C + c] + sums[2 * C + c] + sm;
            const double kd = (double)(C - d.c0) * D * D;
            a0 = (float)(num / kd);
            a1 = (float)(-(2.0 * D - num) / kd);
        }
        a0sh[c] = a0;
        a1sh[c] = a1;
    }
    ce_stage_weights(wsh, o.weight, C);   // (ends in the barrier that publishes a0sh / a1sh as well)
    const size_t npx = (size_t)B * S * S;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    double local = 0.0, slocal = 0.0;   // the picked-class term and the smoothing term of this pixel
    const bool smooth = use_ce && o.eps > 0.f;
    if (idx < npx) {
        const PixelAt at(idx, S);
        const Label l = classify_label((long long)target[idx], o, C);
        // The kept pixels first, the ignored ones behind them: a wave then writes the zeros of its ignored lanes right after
        // the values of the kept ones, and the two partial writes of a line of G meet in the cache.
        if (l.kept) {
            const Pixel px(Z, at, C, g, S);
            float lse, picked;
            SmoothSums ss{wsh, smooth};
            px.lse_picked(l.t, lse, picked, ss);
            const float wy = l.bad ? 1.f : wsh[l.t];
            const float a = (1.f - o.eps) * wy;
            const float bsm = o.eps / (float)C;
            if (use_ce) {
                if (smooth) slocal = ce_smooth_term(bsm, lse, ss.sw, ss.swz);
                local = ce_picked_term(a, lse, picked, l.bad);
            }
            if (G) {
                float inv = 0.f, sap = 0.f;
                if (use_ce) inv = gscale / (float)(DICE && !den ? den_plain : *den);   // den == 0: inf, and 0 * inf = NaN as the arithmetic gives
                if (use_dice)   // sum_k a_k p_k (a bad label: its P_c, hence a_c, are NaN already)
                    for (int c = 0; c < C; ++c) sap += (c == l.t ? a1sh[c] : a0sh[c]) * expf(px.logit(c) - lse);
                float sgp = 0.f;   // sum_c g_c p_c over the listed classes
                if (CLD)
                    for (int c = 0; c < C; ++c)
                        if (const int slot = cmap->slot[c]) sgp += gcl[(size_t)(slot - 1) * npx + idx] * expf(px.logit(c) - lse);
                const float swf = (float)ss.sw;
                const float dwg = d.dw * gscale;
                for (int c = 0; c < C; ++c) {
                    const float pc = expf(px.logit(c) - lse);
                    float out = 0.f;
                    if (use_ce) {
                        float v = ce_grad(a, pc, c == l.t, inv);
                        if (smooth) v += ce_grad_smooth(bsm, pc, swf, wsh[c], inv);
                        out = DICE ? d.cw * v : v;
                    }
                    if (use_dice) {
                        const float dv = dwg * (pc * ((c == l.t ? a1sh[c] : a0sh[c]) - sap));
                        out = use_ce ? out + dv : dv;
                    }
                    if (CLD) {
                        const int slot = cmap->slot[c];
                        out += pc * ((slot ? gcl[(size_t)(slot - 1) * npx + idx] : 0.f) - sgp);
                    }
                    G[at.out_index(c, C, S)] = l.bad ? NAN : out;
                }
            }
        } else if (G) {   // contributes nothing; G arrives uninitialised, so its zeros are written
            for (int c = 0; c < C; ++c) G[at.out_index(c, C, S)] = 0.0f;
        }
    }
    if (!use_ce) return;   // (uniform over the grid) no CE partials: the finish kernel does not read them
    // both sums put, then thread 0 alone gets them (block_sum4 twice has every thread read red and sred)
    block_sum4_put(local, red);
    __syncthreads();
    if (smooth) block_sum4_put(slocal, sred);   // (uniform over the grid)
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = block_sum4_get(red);
        if (smooth) spartial[blockIdx.x] = block_sum4_get(sred);
    }
}

// The two kernels of that body, kept apart, each with the arguments it reads (as one template <TargetT, DICE> the CE-options
// kernel carried den_plain, sums and DiceOpt unread; both forms are measured in profiles/loss_refactor_probe.txt).
template <typename TargetT>
__global__ __launch_bounds__(256) void ce_loss_opts_kernel(const float* __restrict__ Z, const TargetT* __restrict__ target,
                                                           float* __restrict__ G, double* __restrict__ partial,
                                                           double* __restrict__ spartial, const double* __restrict__ den,
                                                           CeOpt o, int B, int C, int g, int S, float gscale) {
    ce_opts_pixel<TargetT, false>(Z, target, G, partial, spartial, den, 0.0, nullptr, o, CE_ALONE, B, C, g, S, gscale);
}
template <typename TargetT>
__global__ __launch_bounds__(256) void ce_dice_kernel(const float* __restrict__ Z, const TargetT* __restrict__ target,
                                                      float* __restrict__ G, double* __restrict__ partial,
                                                      double* __restrict__ spartial, const double* __restrict__ den,
                                                      double den_plain, const double* __restrict__ sums, CeOpt o, DiceOpt d,
                                                      int B, int C, int g, int S, float gscale) {
    ce_opts_pixel<TargetT, true>(Z, target, G, partial, spartial, den, den_plain, sums, o, d, B, C, g, S, gscale);
}

template <typename TargetT>
__global__ __launch_bounds__(256) void ce_cldice_kernel(const float* __restrict__ Z, const TargetT* __restrict__ target,
                                                        float* __restrict__ G, double* __restrict__ partial,
                                                        double* __restrict__ spartial, const double* __restrict__ den,
                                                        double den_plain, const double* __restrict__ sums, CeOpt o, DiceOpt d,
                                                        int B, int C, int g, int S, float gscale, const float* __restrict__ gcl,
                                                        CldClassMap cmap) {
    ce_opts_pixel<TargetT, true, true>(Z, target, G, partial, spartial, den, den_plain, sums, o, d, B, C, g, S, gscale, gcl, &cmap);
}

// terms of a vitseg_ce_cldice_loss call whose clDice term is left out: {loss, CE, dice, 0}; without the Dice options the
// finish kernel wrote the total alone, to terms[0]
__global__ void cld_terms_fill_kernel(float* __restrict__ terms, int have_dice, float* __restrict__ loss) {
    if (!have_dice) {
        terms[1] = terms[0];
        terms[2] = 0.f;
        if (loss) *loss = terms[0];
    }
    terms[3] = 0.f;
}

// The finish of the CE family, one block.  CE = (sum of partial + sum of spartial) / den, the two sums divided apart;
// spartial: the smoothing partials, or null (eps == 0: they were not written); den: a device double, or null: den_plain
// (= B S S, the plain mean).  1.0 / den_plain here and a host's 1.0 / (B S S) are the same correctly rounded fp64 division
// of the same operands: the same bits.  dice from the 3 C sums in fp64.  The total is cw CE + dw dice; a term that was not
// formed is an exact 0, and CE alone (CE_ALONE: cw = 1) is 1.0 * CE, the same double.  terms (optional) = {total, CE, dice};
// loss_out (optional): the total.  extra (optional): {weight cldice, cldice} of cldice.hip: the first joins the total, the
// second is terms[3].
__global__ __launch_bounds__(1024) void ce_finish_kernel(const double* __restrict__ partial, const double* __restrict__ spartial,
                                                         int n, const double* __restrict__ den, double den_plain,
                                                         const double* __restrict__ sums, int C, DiceOpt d,
                                                         float* __restrict__ terms, float* __restrict__ loss_out,
                                                         const double* __restrict__ extra = nullptr) {
    __shared__ double red[1024];
    double total = 0.0;
    if (d.use_ce) {
        const double inv = 1.0 / (den ? *den : den_plain);
        ce_fixed_order_sum(partial, n, red);
        total = red[0] * inv;   // den == 0: 0 * inf = NaN, torch's 0 / 0
        if (spartial) {
            __syncthreads();   // red[0] is read above by every thread before the second sum overwrites it
            ce_fixed_order_sum(spartial, n, red);
            total += red[0] * inv;
        }
    }
    if (threadIdx.x == 0) {
        double dice = 0.0;
        if (d.use_dice) {
            const double sm = (double)d.smooth;
            for (int c = d.c0; c < C; ++c) dice += 1.0 - (2.0 * sums[c] + sm) / (sums[C + c] + sums[2 * C + c] + sm);
            dice /= (double)(C - d.c0);
        }
        double loss = 0.0;
        if (d.use_ce) loss = (double)d.cw * total;
        if (d.use_dice) loss += (double)d.dw * dice;
        if (extra) loss += extra[0];
        if (terms) {
            terms[0] = (float)loss;
            terms[1] = (float)total;
            terms[2] = (float)dice;
            if (extra) terms[3] = (float)extra[1];
        }
        if (loss_out) *loss_out = (float)loss;
    }
}

size_t dice_block_count(int B, int S) { return ((size_t)B * S * S + 256 * DICE_PPT - 1) / (256 * DICE_PPT); }
size_t ce_count_partial_count(int B, int S) { return ((size_t)B * S * S + CE_COUNT_PPB - 1) / CE_COUNT_PPB; }

int check_ce_options(const vitseg_ce_options& o, int B, int C, int S) {
    VITSEG_CHECK_ARG(o.label_smoothing >= 0.f && o.label_smoothing <= 1.f, VITSEG_EINVAL,
                     "ce options: label_smoothing %f outside [0, 1]", (double)o.label_smoothing);   // (a NaN fails both)
    VITSEG_CHECK_ARG(C >= 1 && C <= 255, VITSEG_EINVAL, "ce options: %d classes (1..255)", C);
    VITSEG_CHECK_ARG(o.scratch && ((uintptr_t)o.scratch & 7) == 0, VITSEG_EINVAL, "ce options: scratch is null or not 8-byte aligned");
    VITSEG_CHECK_ARG(o.scratch_bytes >= ce_opts_scratch_bytes(B, S), VITSEG_EINVAL, "ce options: scratch %zu < required %zu",
                     o.scratch_bytes, ce_opts_scratch_bytes(B, S));
    return VITSEG_OK;
}

int check_dice_options(const vitseg_dice_options& d, int B, int C, int S, bool other_term = false) {
    auto weight_ok = [](float v) { return v >= 0.f && v <= FLT_MAX; };   // (a NaN fails both)
    VITSEG_CHECK_ARG(weight_ok(d.ce_weight) && weight_ok(d.dice_weight), VITSEG_EINVAL,
                     "dice options: ce_weight %f / dice_weight %f must be finite and >= 0", (double)d.ce_weight, (double)d.dice_weight);
    VITSEG_CHECK_ARG(other_term || d.ce_weight != 0.f || d.dice_weight != 0.f, VITSEG_EINVAL, "dice options: both weights are 0");
    VITSEG_CHECK_ARG(weight_ok(d.smooth), VITSEG_EINVAL, "dice options: smooth %f must be finite and >= 0", (double)d.smooth);
    VITSEG_CHECK_ARG(C >= 1 && C <= 255, VITSEG_EINVAL, "dice options: %d classes (1..255)", C);
    VITSEG_CHECK_ARG(d.include_background || C >= 2, VITSEG_EINVAL, "dice options: include_background = 0 needs C >= 2");
    VITSEG_CHECK_ARG(d.scratch && ((uintptr_t)d.scratch & 7) == 0, VITSEG_EINVAL, "dice options: scratch is null or not 8-byte aligned");
    VITSEG_CHECK_ARG(d.scratch_bytes >= dice_scratch_bytes(B, C, S), VITSEG_EINVAL, "dice options: scratch %zu < required %zu",
                     d.scratch_bytes, dice_scratch_bytes(B, C, S));
    return VITSEG_OK;
}

}  // namespace

size_t ce_partial_count(int B, int S) { return ((size_t)B * S * S + 255) / 256; }
// scratch of the CE options: the denominator (one double in a 16-byte slot) | the count pass's per-block partials | the loss
// kernel's per-block partials of the smoothing term
size_t ce_opts_scratch_bytes(int B, int S) {
    return 16 + (ce_count_partial_count(B, S) + ce_partial_count(B, S)) * sizeof(double);
}
// scratch of the Dice term: the sums I | P | T (C doubles each) | the sum pass's per-block partials, [3][C][blocks]
size_t dice_scratch_bytes(int B, int C, int S) { return (size_t)3 * C * (1 + dice_block_count(B, S)) * sizeof(double); }

CeOpt ce_opt_of(const vitseg_ce_options* ce, bool with_smoothing) {
    return ce ? CeOpt{ce->class_weight, (long long)ce->ignore_index, ce->has_ignore_index != 0, with_smoothing ? ce->label_smoothing : 0.f}
              : CeOpt{nullptr, 0, 0, 0.f};
}

int launch_ce_count(const void* target, int target_is_u8, const CeOpt& o, double* partial, size_t npx, int C, bool with_valid,
                    hipStream_t s) {
    const unsigned nc = (unsigned)((npx + CE_COUNT_PPB - 1) / CE_COUNT_PPB);
    with_target_type(target, target_is_u8, [&](auto* t) {
        using T = target_t<decltype(t)>;
        if (with_valid)
            hipLaunchKernelGGL((ce_count_kernel<T, true>), dim3(nc), dim3(256), 0, s, t, o, partial, npx, C);
        else
            hipLaunchKernelGGL((ce_count_kernel<T, false>), dim3(nc), dim3(256), 0, s, t, o, partial, npx, C);
    });
    VITSEG_LAUNCH_CHECK("ce_count");
    return VITSEG_OK;
}

int check_fused_loss(const FusedLoss& f, int B, int C, int S) {
    VITSEG_CHECK_ARG(!(f.dice && f.hard), VITSEG_EINVAL, "fused loss: the dice and the hard options cannot be combined");
    VITSEG_CHECK_ARG(!(f.cldice && f.hard), VITSEG_EINVAL, "fused loss: focal / OHEM with the clDice term are not built");
    VITSEG_CHECK_ARG(!f.cldice || f.terms4, VITSEG_EINVAL, "fused loss: the clDice options need the four terms");
    VITSEG_CHECK_ARG(!(f.lovasz && (f.cldice || f.hard)), VITSEG_EINVAL,
                     "fused loss: the Lovasz term with clDice or with focal / OHEM is not built");
    VITSEG_CHECK_ARG(!f.lovasz || f.terms4, VITSEG_EINVAL, "fused loss: the Lovasz options need the four terms");
    if (f.lovasz)
        if (int rc = check_lovasz_options(*f.lovasz, B, C, S)) return rc;
    if (f.cldice)
        if (int rc = check_cldice_options(*f.cldice, B, C, S)) return rc;
    if (f.hard)
        if (int rc = check_hard_options(*f.hard, B, C, S)) return rc;
    if (f.dice)
        if (int rc = check_dice_options(*f.dice, B, C, S, (f.cldice && f.cldice->weight != 0.f) || (f.lovasz && f.lovasz->weight != 0.f))) return rc;
    if (f.ce)
        if (int rc = check_ce_options(*f.ce, B, C, S)) return rc;
    VITSEG_CHECK_ARG(!(f.hard && f.ce) || f.ce->label_smoothing == 0.f, VITSEG_EINVAL,
                     "hard loss: label smoothing %f cannot be combined with the focal / OHEM options", (double)f.ce->label_smoothing);
    return VITSEG_OK;
}

int launch_fused_loss(const float* Z, const void* target, int target_is_u8, float* G, double* partial, float* loss, int B, int C,
                      int g, int S, const FusedLoss& f, hipStream_t s, float gscale) {
    VITSEG_CHECK_ARG(Z && target && partial && (f.dice || f.terms4 ? f.terms : loss), VITSEG_EINVAL, "%s: null pointer",
                     f.terms4 ? "ce_cldice_loss" : f.dice ? "ce_dice_loss" : f.hard ? "hard loss" : "ce_loss");
    if (int rc = check_fused_loss(f, B, C, S)) return rc;
    const bool lov_on = f.lovasz && f.lovasz->weight != 0.f;   // it leaves what clDice leaves: the same loss and finish kernels
    const bool cld_on = (f.cldice && f.cldice->weight != 0.f) || lov_on;
    if (f.terms4 && !cld_on) {   // the term is left out: the launches of the call without it, then the fourth entry
        FusedLoss f3 = f;
        f3.cldice = nullptr;
        f3.lovasz = nullptr;
        f3.terms4 = false;
        if (int rc = launch_fused_loss(Z, target, target_is_u8, G, partial, f.dice ? loss : f.terms, B, C, g, S, f3, s, gscale)) return rc;
        hipLaunchKernelGGL(cld_terms_fill_kernel, dim3(1), dim3(1), 0, s, f.terms, f.dice ? 1 : 0, loss);
        VITSEG_LAUNCH_CHECK("cldice terms");
        return VITSEG_OK;
    }
    // the hard options at gamma 0 with OHEM off and no optional output ask for nothing beyond the CE below: its launches
    if (f.hard && (f.hard->gamma != 0.f || hard_ohem_on(*f.hard) || f.pixel_loss || f.stats))
        return launch_hard_loss(Z, target, target_is_u8, G, partial, loss, B, C, g, S, f, s, gscale);
    const size_t npx = (size_t)B * S * S;
    const unsigned nb = (unsigned)ce_partial_count(B, S), nc = (unsigned)ce_count_partial_count(B, S);
    const double den_plain = (double)npx;
    if (!f.ce && !f.dice && !cld_on) {
        with_target_type(target, target_is_u8, [&](auto* t) {
            hipLaunchKernelGGL(ce_loss_kernel<target_t<decltype(t)>>, dim3(nb), dim3(256), 0, s, Z, t, G, partial, B, C, g, S, gscale);
        });
        VITSEG_LAUNCH_CHECK("ce_loss");
        hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(1024), 0, s, partial, nullptr, (int)nb, nullptr, den_plain, nullptr, C,
                           CE_ALONE, nullptr, loss);
        VITSEG_LAUNCH_CHECK("ce_finish");
        return VITSEG_OK;
    }
    const DiceOpt d = f.dice ? DiceOpt{f.dice->ce_weight, f.dice->dice_weight, f.dice->smooth, f.dice->include_background ? 0 : 1,
                                       f.dice->ce_weight != 0.f, f.dice->dice_weight != 0.f}
                             : CE_ALONE;
    const CeOpt o = ce_opt_of(f.ce);
    double *den = nullptr, *spart = nullptr, *sums = nullptr;
    if (f.ce && d.use_ce) {   // the mean's denominator
        den = (double*)f.ce->scratch;
        double* cpart = (double*)((char*)f.ce->scratch + 16);
        spart = cpart + nc;
        if (int rc = launch_ce_count(target, target_is_u8, o, cpart, npx, C, false, s)) return rc;
        hipLaunchKernelGGL(sum_rows_kernel, dim3(1), dim3(1024), 0, s, cpart, (int)nc, den);
        VITSEG_LAUNCH_CHECK("ce_count_finish");
    }
    if (d.use_dice) {
        const unsigned nd = (unsigned)dice_block_count(B, S);
        sums = (double*)f.dice->scratch;
        double* dpart = sums + 3 * C;
        with_target_type(target, target_is_u8, [&](auto* t) {
            hipLaunchKernelGGL(dice_sum_kernel<target_t<decltype(t)>>, dim3(nd), dim3(256), 0, s, Z, t, o.ignore, o.has_ignore, dpart,
                               nd, B, C, g, S);
        });
        VITSEG_LAUNCH_CHECK("dice_sum");
        hipLaunchKernelGGL(sum_rows_kernel, dim3(3 * C), dim3(1024), 0, s, dpart, (int)nd, sums);
        VITSEG_LAUNCH_CHECK("dice_reduce");
    }
    CldTerm cld{};
    if (lov_on) {
        if (int rc = launch_lovasz_term(Z, target, target_is_u8, o, B, C, g, S, *f.lovasz, G != nullptr, gscale, s, &cld)) return rc;
    } else if (cld_on) {
        if (int rc = launch_cldice_term(Z, target, target_is_u8, o, B, C, g, S, *f.cldice, G != nullptr, gscale, s, &cld)) return rc;
    }
    with_target_type(target, target_is_u8, [&](auto* t) {
        using T = target_t<decltype(t)>;
        if (cld_on)
            hipLaunchKernelGGL(ce_cldice_kernel<T>, dim3(nb), dim3(256), 0, s, Z, t, G, partial, spart, den, den_plain, sums, o, d, B, C, g,
                               S, gscale, cld.gplanes, cld.map);
        else if (f.dice)
            hipLaunchKernelGGL(ce_dice_kernel<T>, dim3(nb), dim3(256), 0, s, Z, t, G, partial, spart, den, den_plain, sums,
                               o, d, B, C, g, S, gscale);
        else
            hipLaunchKernelGGL(ce_loss_opts_kernel<T>, dim3(nb), dim3(256), 0, s, Z, t, G, partial, spart, den, o, B, C, g, S, gscale);
    });
    VITSEG_LAUNCH_CHECK("ce_loss_opts");
    hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(1024), 0, s, partial, d.use_ce && o.eps > 0.f ? (const double*)spart : nullptr,
                       (int)nb, (const double*)den, den_plain, (const double*)sums, C, d, f.dice || cld_on ? f.terms : nullptr, loss,
                       cld_on ? cld.extra : nullptr);
    VITSEG_LAUNCH_CHECK("ce_finish");
    return VITSEG_OK;
}

}  // namespace vitseg
