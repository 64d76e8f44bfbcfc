// Decoder tail: seg_head.2 (1x1 conv), bilinear upsample, sigmoid -> argmax mask.
#include <float.h>
#include <stdlib.h>

#include "kernels.hpp"
#include "tail_math.hpp"

namespace vitseg {
namespace {

constexpr int MID = 256;  // seg_head.0 output channels, model/CE/classes.py:241

// seg_head.2 = Conv2d(256, C, 1) (model/CE/classes.py:243): Z[b, c, y, x] = F[b*Np + t, :] . W2[c, :] + b2[c].
// One wave per pixel row of F (256 floats = 64 lanes x 16 B); tiny (2*Np*256*C FLOP/image).
__global__ __launch_bounds__(256) void head1x1_kernel(const float* __restrict__ F, const float* __restrict__ W2,
                                                      const float* __restrict__ b2, float* __restrict__ Z, int B,
                                                      int Np, int C) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B * Np) return;
    const f32x4 f = ((const f32x4*)(F + (size_t)row * MID))[lane];
    const int b = row / Np, t = row - b * Np;
    for (int c = 0; c < C; ++c) {
        const f32x4 w = ((const f32x4*)(W2 + (size_t)c * MID))[lane];
        float s = (f[0] * w[0] + f[1] * w[1]) + (f[2] * w[2] + f[3] * w[3]);
        s = wave_sum(s);
        if (lane == 0) Z[((size_t)b * C + c) * Np + t] = s + b2[c];
    }
}

// F.interpolate(out, size=x.shape[2:], mode='bilinear', align_corners=False)
// (model/CE/classes.py:260) fused with the scripts' post-processing
// `logits.sigmoid()` -> `argmax(dim=class)` (model/CE/testViTModel.py:122-126).
//
// The taps, the fma placement (row = fma(a, wx0, b*wx1); out = fma(row_top, wy0, row_bot*wy1)) and ATen's fp32 sigmoid:
// tail_math.hpp (taps, sigmoid_aten), shared with the overlapping-window blend of window.hip.
// Bound: HBM writes (C*S*S*4 B logits and/or S*S B mask per image); the low-res input
// (C*g*g*4 B per image) stays in L2.  Thread = 4 consecutive x of one output row.

// Thread = a 4 (x) by UPR (y) block of output pixels: the x taps are computed once, and the two horizontally
// interpolated source rows (`top`, `bot`) are reused while consecutive output rows keep the same source rows (at
// 16x up-scaling 15 of 16 do; the test is wave-uniform because a wave covers one output row band).
// STAGED (a block = whole row bands of one image, launch_upsample decides): the few low-res rows the block's output rows
// interpolate between are copied to LDS for all classes FIRST, so the class loop issues no global reads.  With C = 17
// the kernel writes 581 MB per launch; a dependent global gather per class then waits behind the saturated write
// queues (17 serialized round trips of several us each: 3.3 TB/s) -- from LDS the loop is a pure store stream.
constexpr int UPR = 4;
template <bool STAGED>
__global__ __launch_bounds__(256) void upsample_kernel(const float* __restrict__ Z, float* __restrict__ logits,
                                                       uint8_t* __restrict__ mask, int B, int C, int g, int S) {
    extern __shared__ __attribute__((aligned(16))) float zs[];   // STAGED: [class][source row - ymin][g]
    // STAGED: pixels whose raw top-2 margin does not settle the sigmoid argmax are queued here and resolved densely after
    // the main pass (one lane per queued pixel) -- inside the main pass a single such pixel would send its whole wave
    // (256 pixels) through the exact-sigmoid loop over all classes, which made the mask cost 2x the logits stream
    __shared__ unsigned amb_n;
    __shared__ unsigned amb_px[STAGED ? 256 * UPR * 4 : 1];
    const int quads = S >> 2, bands = S / UPR;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const float scale = (float)g / (float)S;
    int ymin = 0, nr = 0, Yf = 0, bimg = 0;
    if (STAGED) {
        const int bpb = (int)blockDim.x / quads;                       // bands per block (whole number, same image; the block
        const size_t band0 = (size_t)blockIdx.x * bpb;                 // has quads * bpb <= 256 threads, launch_upsample)
        Yf = (int)(band0 % bands) * UPR;
        bimg = (int)(band0 / bands);
        if (threadIdx.x == 0) amb_n = 0;
        int ya, yb, yc, yd;
        float w0, w1;
        taps(Yf, scale, g, ya, yb, w0, w1);
        taps(Yf + bpb * UPR - 1, scale, g, yc, yd, w0, w1);
        ymin = ya;
        nr = yd - ya + 1;
        if (bimg < B) {
            const int per = nr * g;
            for (int i = threadIdx.x; i < C * per; i += (int)blockDim.x) {
                const int c = i / per, rem = i - c * per;
                zs[i] = Z[((size_t)bimg * C + c) * g * g + (size_t)ymin * g + rem];
            }
        }
        __syncthreads();
    }
    if (!STAGED && idx >= (size_t)B * bands * quads) return;   // STAGED grids are whole blocks (launch_upsample)
    const int xq = (int)(idx % quads);
    const int Y0 = (int)((idx / quads) % bands) * UPR;
    const int b = (int)(idx / ((size_t)quads * bands));
    int x0[4], x1[4];
    float wx0[4], wx1[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) taps(4 * xq + e, scale, g, x0[e], x1[e], wx0[e], wx1[e]);
    int y0[UPR], y1[UPR];
    float wy0[UPR], wy1[UPR];
#pragma unroll
    for (int r = 0; r < UPR; ++r) taps(Y0 + r, scale, g, y0[r], y1[r], wy0[r], wy1[r]);

    // argmax_c sigmoid(v_c) with first-index ties.  sigmoid is monotone, so the answer is the raw argmax m unless
    // an EARLIER class rounds to the same fp32 sigmoid.  That cannot happen when the top-1 logit t1 leads every
    // other class by a margin whose image under sigma is many ulps: |t1| <= 2 (sigma' >= 0.105) and margin >= 1e-4
    // -> the true sigmoids differ by >= 1e-5 ~ 170 ulp(1); |t1| <= 8 (sigma' >= 3.3e-4) and margin >= 4e-3 ->
    // >= 1.3e-6 ~ 22 ulp -- far beyond the <= 2 ulp error of ATen's 1/(1+exp(-x)).  Only the remaining (near-tie or
    // saturated) pixels evaluate the exact fp32 sigmoids (sigmoid_aten above); the result is identical on EVERY pixel.
    float t1[UPR][4], t2[UPR][4];
    int arg[UPR][4];
#pragma unroll
    for (int r = 0; r < UPR; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            t1[r][e] = -INFINITY;
            t2[r][e] = -INFINITY;
            arg[r][e] = 0;
        }
    auto hrow = [&](int c, int y) {  // source row y of class c interpolated along x at this thread's 4 columns
        const float* z = STAGED ? zs + (c * nr + (y - ymin)) * g : Z + (((size_t)b * C + c) * g + y) * g;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __fmaf_rn(z[x0[e]], wx0[e], __fmul_rn(z[x1[e]], wx1[e]));
        return v;
    };
    for (int c = 0; c < C; ++c) {
        f32x4 top = hrow(c, y0[0]), bot = hrow(c, y1[0]);
#pragma unroll
        for (int r = 0; r < UPR; ++r) {
            if (r > 0) {
                if (y0[r] != y0[r - 1]) top = (y0[r] == y1[r - 1]) ? bot : hrow(c, y0[r]);
                if (y1[r] != y1[r - 1]) bot = hrow(c, y1[r]);
            }
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __fmaf_rn(top[e], wy0[r], __fmul_rn(bot[e], wy1[r]));
            if (logits)   // streamed once, never re-read by this kernel: keep it out of the caches
                __builtin_nontemporal_store(v, (f32x4*)(logits + (((size_t)b * C + c) * S + Y0 + r) * S + 4 * xq));
            if (mask) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (v[e] > t1[r][e]) {  // strict: the first maximal class stays
                        t2[r][e] = t1[r][e];
                        t1[r][e] = v[e];
                        arg[r][e] = c;
                    } else {
                        t2[r][e] = fmaxf(t2[r][e], v[e]);
                    }
                }
            }
        }
    }
    if (mask) {
#pragma unroll
        for (int r = 0; r < UPR; ++r) {
            bool amb = false;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float at = fabsf(t1[r][e]), margin = t1[r][e] - t2[r][e];
                const bool a1 = !((at <= 2.0f && margin >= 1e-4f) || (at <= 8.0f && margin >= 4e-3f));
                if (STAGED && a1)   // resolved after the main pass (the raw argmax written below is overwritten)
                    amb_px[atomicAdd(&amb_n, 1u)] = (unsigned)(((Y0 + r - Yf) << 12) | (4 * xq + e));
                amb = amb || a1;
            }
            if (!STAGED && amb) {  // exact path: ATen's fp32 sigmoid restated (sigmoid_aten), first maximal class wins
                float best[4];
                for (int c = 0; c < C; ++c) {
                    const f32x4 top = hrow(c, y0[r]), bot = hrow(c, y1[r]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = __fmaf_rn(top[e], wy0[r], __fmul_rn(bot[e], wy1[r]));
                        const float sg = sigmoid_aten(v);
                        if (c == 0 || sg > best[e]) {
                            best[e] = sg;
                            arg[r][e] = c;
                        }
                    }
                }
            }
            uchar4 m4;
            m4.x = (unsigned char)arg[r][0];
            m4.y = (unsigned char)arg[r][1];
            m4.z = (unsigned char)arg[r][2];
            m4.w = (unsigned char)arg[r][3];
            *(uchar4*)(mask + ((size_t)b * S + Y0 + r) * S + 4 * xq) = m4;
        }
    }
    if (STAGED && mask) {
        __syncthreads();   // the queue is complete and this block's raw-argmax bytes are written
        const unsigned n_amb = amb_n;
        for (unsigned i = threadIdx.x; i < n_amb; i += blockDim.x) {
            const int Y = Yf + (int)(amb_px[i] >> 12), X = (int)(amb_px[i] & 0xfffu);
            int ya, yb, xa, xb;
            float wya, wyb, wxa, wxb;
            taps(Y, scale, g, ya, yb, wya, wyb);
            taps(X, scale, g, xa, xb, wxa, wxb);
            float best = 0.f;
            int barg = 0;
            for (int c = 0; c < C; ++c) {   // the same fma placement as the main pass, then ATen's fp32 sigmoid
                const float* zt = zs + (c * nr + (ya - ymin)) * g;
                const float* zb = zs + (c * nr + (yb - ymin)) * g;
                const float top = __fmaf_rn(zt[xa], wxa, __fmul_rn(zt[xb], wxb));
                const float bot = __fmaf_rn(zb[xa], wxa, __fmul_rn(zb[xb], wxb));
                const float sg = sigmoid_aten(__fmaf_rn(top, wya, __fmul_rn(bot, wyb)));
                if (c == 0 || sg > best) {
                    best = sg;
                    barg = c;
                }
            }
            mask[((size_t)bimg * S + Y) * S + X] = (unsigned char)barg;
        }
    }
}

// Mask-only output for TWO classes (BASELINE configs[4]: 1 byte per pixel, no logits tensor): the same result as
// upsample_kernel<true> on every pixel at a quarter of the arithmetic.  mask = 1 iff sigmoid(v1) > sigmoid(v0) (the first
// maximal class wins ties), v_c = the ATen-exact bilinear value of class c.  Bilinear interpolation is linear, so
// D = interp(z1 - z0) equals v1 - v0 up to fp32 rounding (|z| <= 8: < 6e-6 from a dozen roundings of values below 8).
// Where |D| clears the margin that settles the sigmoid comparison (upsample_kernel's rule: 1e-4 while every |z| <= 2,
// 4e-3 while <= 8; the block's low-res maximum bounds every interpolated value) plus that rounding slack, the sign of D
// is the answer: ONE plain interpolation instead of two exact ones and the top-2 bookkeeping.  Every other pixel is
// queued and resolved exactly as in upsample_kernel (ATen's fma placement, ATen's fp32 sigmoid, first maximum).
__global__ __launch_bounds__(256) void upsample_mask2_kernel(const float* __restrict__ Z, uint8_t* __restrict__ mask, int B,
                                                             int g, int S) {
    extern __shared__ __attribute__((aligned(16))) float zs[];   // [z0 | z1 | z1 - z0][source row - ymin][g]
    __shared__ unsigned amb_n, zmax_bits;
    __shared__ unsigned amb_px[256 * UPR * 4];
    const int quads = S >> 2, bands = S / UPR;
    const float scale = (float)g / (float)S;
    const int bpb = (int)blockDim.x / quads;
    const size_t band0 = (size_t)blockIdx.x * bpb;
    const int Yf = (int)(band0 % bands) * UPR, bimg = (int)(band0 / bands);
    if (threadIdx.x == 0) {
        amb_n = 0;
        zmax_bits = 0;
    }
    int ya, yb, yc, yd;
    float w0, w1;
    taps(Yf, scale, g, ya, yb, w0, w1);
    taps(Yf + bpb * UPR - 1, scale, g, yc, yd, w0, w1);
    const int ymin = ya, nr = yd - ya + 1, per = nr * g;
    __syncthreads();
    if (bimg < B) {
        unsigned mx = 0;
        for (int i = threadIdx.x; i < per; i += (int)blockDim.x) {
            const float a = Z[((size_t)bimg * 2 + 0) * g * g + (size_t)ymin * g + i];
            const float b = Z[((size_t)bimg * 2 + 1) * g * g + (size_t)ymin * g + i];
            zs[i] = a;
            zs[per + i] = b;
            zs[2 * per + i] = b - a;
            // |z| as an unsigned integer orders like the float; a NaN (exponent all ones, above every finite value) makes
            // the whole block take the exact path
            mx = max(mx, max(__float_as_uint(a) & 0x7fffffffu, __float_as_uint(b) & 0x7fffffffu));
        }
        atomicMax(&zmax_bits, mx);
    }
    __syncthreads();
    const float zmax = __uint_as_float(zmax_bits);
    // margin of upsample_kernel's rule + the rounding slack of D; no margin settles it once a logit may exceed 8
    const float thr = zmax <= 2.0f ? 1.1e-4f : (zmax <= 8.0f ? 4.01e-3f : INFINITY);
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int xq = (int)(idx % quads);
    const int Y0 = (int)((idx / quads) % bands) * UPR;
    if (bimg < B) {
        int x0[4], x1[4];
        float wx0[4], wx1[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) taps(4 * xq + e, scale, g, x0[e], x1[e], wx0[e], wx1[e]);
        const float* zd = zs + 2 * per;
        auto hrow = [&](int y) {
            const float* z = zd + (y - ymin) * g;
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaf(z[x0[e]], wx0[e], z[x1[e]] * wx1[e]);
            return v;
        };
        int py0 = -1, py1 = -1;
        f32x4 top = {0.f, 0.f, 0.f, 0.f}, bot = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < UPR; ++r) {
            int y0, y1;
            float wy0, wy1;
            taps(Y0 + r, scale, g, y0, y1, wy0, wy1);
            if (y0 != py0) top = (y0 == py1) ? bot : hrow(y0);
            if (y1 != py1) bot = hrow(y1);
            py0 = y0;
            py1 = y1;
            uchar4 m4;
            unsigned char cls[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = fmaf(top[e], wy0, bot[e] * wy1);
                cls[e] = d > 0.f ? 1 : 0;
                if (!(fabsf(d) >= thr))   // (a NaN difference is ambiguous too)
                    amb_px[atomicAdd(&amb_n, 1u)] = (unsigned)(((Y0 + r - Yf) << 12) | (4 * xq + e));
            }
            m4.x = cls[0]; m4.y = cls[1]; m4.z = cls[2]; m4.w = cls[3];
            *(uchar4*)(mask + ((size_t)bimg * S + Y0 + r) * S + 4 * xq) = m4;
        }
    }
    __syncthreads();   // the queue is complete and this block's provisional bytes are written
    const unsigned n_amb = amb_n;
    for (unsigned i = threadIdx.x; i < n_amb; i += blockDim.x) {
        const int Y = Yf + (int)(amb_px[i] >> 12), X = (int)(amb_px[i] & 0xfffu);
        int y0, y1, xa, xb;
        float wya, wyb, wxa, wxb;
        taps(Y, scale, g, y0, y1, wya, wyb);
        taps(X, scale, g, xa, xb, wxa, wxb);
        float sg[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {   // the fma placement of upsample_kernel, then ATen's fp32 sigmoid
            const float* zt = zs + c * per + (y0 - ymin) * g;
            const float* zb = zs + c * per + (y1 - ymin) * g;
            const float top = __fmaf_rn(zt[xa], wxa, __fmul_rn(zt[xb], wxb));
            const float bot = __fmaf_rn(zb[xa], wxa, __fmul_rn(zb[xb], wxb));
            sg[c] = sigmoid_aten(__fmaf_rn(top, wya, __fmul_rn(bot, wyb)));
        }
        mask[((size_t)bimg * S + Y) * S + X] = sg[1] > sg[0] ? 1 : 0;
    }
}

// nn.CrossEntropyLoss() on the upsampled logits (model/CE/classes.py:268,280): mean over B*S*S pixels of
// logsumexp_c(logit) - logit[target].  The logits are re-generated from the low-res map (same exact
// bilinear arithmetic as upsample_kernel) instead of being read back from HBM, so the loss costs one
// pass over the targets.  Optionally writes G = d loss / d logits = (softmax - onehot) / (B*S*S)
// (fp32 [B, C, S, S]) for the backward pass.  Deterministic: per-block partial sums in fp64, reduced in a
// fixed order by ce_finish_kernel.
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
        // a label outside [0, C) (uint8 255, the reference's ignore_index -100, C itself) is not a class: its pixel's loss
        // and gradient are NaN, so the mean loss is NaN rather than a plausible wrong number (ignore_index is not supported)
        const long long tl = (long long)target[idx];
        const bool bad = tl < 0 || tl >= C;
        const int t = bad ? -1 : (int)tl;
        auto logit = [&](int c) {
            const float* zt = Z + (((size_t)b * C + c) * g + y0) * g;
            const float* zb = Z + (((size_t)b * C + c) * g + y1) * g;
            const float top = __fmaf_rn(zt[x0], wx0, __fmul_rn(zt[x1], wx1));
            const float bot = __fmaf_rn(zb[x0], wx0, __fmul_rn(zb[x1], wx1));
            return __fmaf_rn(top, wy0, __fmul_rn(bot, wy1));
        };
        float m = -INFINITY, ssum = 0.f, picked = 0.f;
        for (int c = 0; c < C; ++c) {  // online logsumexp
            const float v = logit(c);
            if (c == t) picked = v;
            const float mn = fmaxf(m, v);
            ssum = ssum * expf(m - mn) + expf(v - mn);
            m = mn;
        }
        const float lse = m + logf(ssum);
        local = bad ? (double)NAN : (double)(lse - picked);
        if (G) {
            const float inv = gscale / (float)npx;   // gscale: the upstream d(total loss) / d(this loss), e.g. 1 / accumulation
            for (int c = 0; c < C; ++c) {
                const float pc = expf(logit(c) - lse);
                G[(((size_t)b * C + c) * S + Y) * S + X] = bad ? NAN : (pc - (c == t ? 1.f : 0.f)) * inv;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// (ce_fixed_order_sum below restates this reduction for the options path, so that this kernel's code stays as it is:
// an edit to the order here is mirrored there -- the options path at its defaults must give this kernel's bits)
__global__ __launch_bounds__(1024) void ce_finish_kernel(const double* __restrict__ partial, int n, double inv_count,
                                                         float* __restrict__ loss) {
    __shared__ double red[1024];
    // fixed assignment and order: 4 independent strided chains per thread (loads in flight), then a tree
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int i = threadIdx.x;
    for (; i + 3 * 1024 < n; i += 4 * 1024) {
        s0 += partial[i];
        s1 += partial[i + 1024];
        s2 += partial[i + 2 * 1024];
        s3 += partial[i + 3 * 1024];
    }
    for (; i < n; i += 1024) s0 += partial[i];
    red[threadIdx.x] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(red[0] * inv_count);
}

// ---- cross-entropy with options: F.cross_entropy(up, y, weight=w, ignore_index=ii, label_smoothing=eps) ----
//   keep = (y != ii);  den = sum_keep w[y];
//   loss = [ (1 - eps) sum_keep w[y] (lse - z_y) + (eps / C) sum_keep sum_c w[c] (lse - z_c) ] / den
//   dL/dz_c = keep [ (1 - eps) w[y] (p_c - 1[c = y]) + (eps / C) (p_c sum_k w[k] - w[c]) ] gscale / den
// The mean's denominator depends on the targets, and the gradient kernel needs it before it writes G: a count pass over
// the targets alone (ce_count_kernel: fp64 per-block partials of w[y] keep) and a fixed-order reduce to one device double
// (ce_count_finish_kernel) run first on the same stream -- no atomics, no host read.  A label outside [0, C) that is not
// the ignored one stays what it is in ce_loss_kernel (NaN loss, NaN gradient at its pixel) and counts 1 in den, as it does
// in the plain mean over B S S pixels, so that every other pixel keeps the gradient it would have had.
// The picked-class sum and the smoothing sum are reduced apart and each is divided by den, and each gradient term is scaled
// by 1 / den on its own, as torch forms them: with den == 0 the picked-class part is 0 * inf = NaN whatever the smoothing
// part holds (kept pixels of weight 0 under smoothing: NaN, not inf).
// With no label ignored, no weights and eps = 0 every product below is by 1 or adds +0: the bits of ce_loss_kernel.
constexpr int CE_COUNT_PER_THREAD = 4;   // targets per thread of the count pass (block = 1024 consecutive targets)

// (ce_fixed_order_sum, CeOpt and ce_stage_weights: tail_math.hpp, shared with hardloss.hip)

template <typename TargetT>
__global__ __launch_bounds__(256) void ce_count_kernel(const TargetT* __restrict__ target, CeOpt o, double* __restrict__ partial,
                                                       size_t npx, int C) {
    __shared__ float wsh[256];
    __shared__ double red[4];
    ce_stage_weights(wsh, o.weight, C);
    const size_t base = (size_t)blockIdx.x * (256 * CE_COUNT_PER_THREAD) + threadIdx.x;
    double local = 0.0;
#pragma unroll
    for (int k = 0; k < CE_COUNT_PER_THREAD; ++k) {   // consecutive lanes read consecutive targets
        const size_t idx = base + (size_t)k * 256;
        if (idx < npx) {
            const long long tl = (long long)target[idx];   // uint8 widened before the compare
            const bool ignored = o.has_ignore && tl == o.ignore;
            const bool bad = tl < 0 || tl >= C;
            local += ignored ? 0.0 : (bad ? 1.0 : (double)wsh[bad ? 0 : (int)tl]);
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) local += __shfl_xor(local, s, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(1024) void ce_count_finish_kernel(const double* __restrict__ partial, int n, double* __restrict__ den) {
    __shared__ double red[1024];
    ce_fixed_order_sum(partial, n, red);
    if (threadIdx.x == 0) *den = red[0];
}

// ce_loss_kernel with the options: same taps, same fma placement, same online log-sum-exp; one thread per pixel.
template <typename TargetT>
__global__ __launch_bounds__(256) void ce_loss_opts_kernel(const float* __restrict__ Z, const TargetT* __restrict__ target,
                                                           float* __restrict__ G, double* __restrict__ partial,
                                                           double* __restrict__ spartial, const double* __restrict__ den,
                                                           CeOpt o, int B, int C, int g, int S, float gscale) {
    __shared__ float wsh[256];
    __shared__ double red[4], sred[4];
    ce_stage_weights(wsh, o.weight, C);
    const size_t npx = (size_t)B * S * S;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    double local = 0.0, slocal = 0.0;   // the picked-class term and the smoothing term of this pixel
    const bool smooth = o.eps > 0.f;
    if (idx < npx) {
        const int X = (int)(idx % S), Y = (int)((idx / S) % S), b = (int)(idx / ((size_t)S * S));
        const long long tl = (long long)target[idx];
        if (o.has_ignore && tl == o.ignore) {   // contributes nothing; G arrives uninitialised, so its zeros are written
            if (G)
                for (int c = 0; c < C; ++c) G[(((size_t)b * C + c) * S + Y) * S + X] = 0.0f;
        } else {
            const float scale = (float)g / (float)S;
            int y0, y1, x0, x1;
            float wy0, wy1, wx0, wx1;
            taps(Y, scale, g, y0, y1, wy0, wy1);
            taps(X, scale, g, x0, x1, wx0, wx1);
            const bool bad = tl < 0 || tl >= C;
            const int t = bad ? -1 : (int)tl;
            auto logit = [&](int c) {
                const float* zt = Z + (((size_t)b * C + c) * g + y0) * g;
                const float* zb = Z + (((size_t)b * C + c) * g + y1) * g;
                const float top = __fmaf_rn(zt[x0], wx0, __fmul_rn(zt[x1], wx1));
                const float bot = __fmaf_rn(zb[x0], wx0, __fmul_rn(zb[x1], wx1));
                return __fmaf_rn(top, wy0, __fmul_rn(bot, wy1));
            };
            float m = -INFINITY, ssum = 0.f, picked = 0.f;
            // label smoothing: sum_c w[c] z_c and sum_c w[c] in fp64 (exact products, one rounding per add), so that
            // lse sum w - sum w z cancels no fp32 roundings
            double swz = 0.0, sw = 0.0;
            for (int c = 0; c < C; ++c) {  // online logsumexp
                const float v = logit(c);
                if (c == t) picked = v;
                const float mn = fmaxf(m, v);
                ssum = ssum * expf(m - mn) + expf(v - mn);
                m = mn;
                if (smooth) {
                    const double wc = (double)wsh[c];
                    swz += wc * (double)v;
                    sw += wc;
                }
            }
            const float lse = m + logf(ssum);
            const float wy = bad ? 1.f : wsh[t];
            const float a = (1.f - o.eps) * wy;          // weight of the picked-class term
            const float bsm = o.eps / (float)C;          // weight of each class's smoothing term
            local = (double)a * (double)(lse - picked);
            if (smooth) slocal = (double)bsm * ((double)lse * sw - swz);
            if (bad) local = (double)NAN;
            if (G) {
                const float inv = gscale / (float)*den;   // den == 0: inf, and 0 * inf = NaN as the arithmetic gives
                const float swf = (float)sw;
                for (int c = 0; c < C; ++c) {
                    const float pc = expf(logit(c) - lse);
                    float v = (a * (pc - (c == t ? 1.f : 0.f))) * inv;
                    if (smooth) v += (bsm * (pc * swf - wsh[c])) * inv;
                    G[(((size_t)b * C + c) * S + Y) * S + X] = bad ? NAN : v;
                }
            }
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) local += __shfl_xor(local, s, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local;
    __syncthreads();
    if (smooth) {   // (uniform over the grid)
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) slocal += __shfl_xor(slocal, s, 64);
        if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = slocal;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        if (smooth) spartial[blockIdx.x] = (sred[0] + sred[1]) + (sred[2] + sred[3]);
    }
}

// spartial: the smoothing partials, or null (eps == 0: they were not written)
__global__ __launch_bounds__(1024) void ce_finish_opts_kernel(const double* __restrict__ partial,
                                                              const double* __restrict__ spartial, int n,
                                                              const double* __restrict__ den, float* __restrict__ loss) {
    __shared__ double red[1024];
    const double inv = 1.0 / *den;
    ce_fixed_order_sum(partial, n, red);
    double total = red[0] * inv;   // den == 0: 0 * inf = NaN, torch's 0 / 0
    if (spartial) {
        __syncthreads();   // red[0] is read above by every thread before the second sum overwrites it
        ce_fixed_order_sum(spartial, n, red);
        total += red[0] * inv;
    }
    if (threadIdx.x == 0) *loss = (float)total;
}

// ---- CE + soft Dice (include/vitseg.h, vitseg_ce_dice_loss) ----
//   I_c = sum_keep p_c t_c;  P_c = sum_keep p_c;  T_c = sum_keep t_c;  D_c = P_c + T_c + smooth  (c in K, the classes counted)
//   dice = mean_K [ 1 - (2 I_c + smooth) / D_c ]
//   a_c = -[2 t_c D_c - (2 I_c + smooth)] / (|K| D_c^2);  d dice / d z_c = p_c (a_c - sum_k a_k p_k)
// The sums run over the whole batch, so they are on the device before the gradient kernel starts: dice_sum_kernel leaves
// per-block fp64 partials, dice_reduce_kernel adds them in the fixed order of ce_fixed_order_sum, and ce_dice_kernel (one
// thread per pixel, the CE arithmetic of ce_loss_opts_kernel restated) reads the 3 C doubles.
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
    // per pixel: the top-left tap's row, the two columns, the row step, the two upper weights, the label
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
            const long long tl = (long long)target[idx];   // uint8 widened before the compare
            if (!(has_ignore && tl == ignore)) {
                const int X = (int)(idx % S), Y = (int)((idx / S) % S), b = (int)(idx / ((size_t)S * S));
                int y0, y1;
                float w0;
                taps(Y, scale, g, y0, y1, w0, wy1[k]);
                taps(X, scale, g, x0[k], x1[k], w0, wx1[k]);
                zp[k] = Z + ((size_t)b * C * g + y0) * g;
                dy[k] = (y1 - y0) * g;
                t[k] = (tl < 0 || tl >= C) ? -1 : (int)tl;
            }
        }
    }
    const int plane = g * g;
    // the logit of ce_loss_kernel: the same taps, the same fma placement (w0 = 1 - w1 as taps() forms it)
    auto logit = [&](int k, int c) {
        const float* zt = zp[k] + (size_t)c * plane;
        const float* zb = zt + dy[k];
        const float wx0 = __fsub_rn(1.f, wx1[k]), wy0 = __fsub_rn(1.f, wy1[k]);
        const float top = __fmaf_rn(zt[x0[k]], wx0, __fmul_rn(zt[x1[k]], wx1[k]));
        const float bot = __fmaf_rn(zb[x0[k]], wx0, __fmul_rn(zb[x1[k]], wx1[k]));
        return __fmaf_rn(top, wy0, __fmul_rn(bot, wy1[k]));
    };
    for (int c = 0; c < C; ++c) {   // online logsumexp, every pixel of the thread in step
#pragma unroll
        for (int k = 0; k < DICE_PPT; ++k)
            if (t[k] != -2) {
                const float v = logit(k, c);
                const float mn = fmaxf(m[k], v);
                ssum[k] = ssum[k] * expf(m[k] - mn) + expf(v - mn);
                m[k] = mn;
            }
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

// sums[q * C + c] = the fixed-order sum of the nblk partials of quantity q (I, P, T) and class c; one block each
__global__ __launch_bounds__(1024) void dice_reduce_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ sums) {
    __shared__ double red[1024];
    ce_fixed_order_sum(partial + (size_t)blockIdx.x * nblk, nblk, red);
    if (threadIdx.x == 0) sums[blockIdx.x] = red[0];
}

struct DiceOpt {
    float cw, dw, smooth;   // ce_weight, dice_weight, smooth
    int c0;                 // first class counted (0, or 1 without the background)
    int use_ce, use_dice;   // the term is formed (its weight is not 0)
};

// ce_loss_opts_kernel with the Dice gradient: same taps, same fma placement, same online log-sum-exp, the CE terms formed
// by the same expressions; one thread per pixel, one store per element of G.  den: the device double of the count pass, or
// null (no CE options: den_plain = B S S).  sums: I | P | T, C doubles each.
template <typename TargetT>
__global__ __launch_bounds__(256) void ce_dice_kernel(const float* __restrict__ Z, const TargetT* __restrict__ target,
                                                      float* __restrict__ G, double* __restrict__ partial,
                                                      double* __restrict__ spartial, const double* __restrict__ den,
                                                      double den_plain, const double* __restrict__ sums, CeOpt o, DiceOpt d,
                                                      int B, int C, int g, int S, float gscale) {
    __shared__ float wsh[256], a0sh[256], a1sh[256];   // a_c of a pixel whose label is not c / is c
    __shared__ double red[4], sred[4];
    if (d.use_dice && (int)threadIdx.x < C) {
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
    const bool smooth = d.use_ce && o.eps > 0.f;
    if (idx < npx) {
        const int X = (int)(idx % S), Y = (int)((idx / S) % S), b = (int)(idx / ((size_t)S * S));
        const long long tl = (long long)target[idx];
        if (o.has_ignore && tl == o.ignore) {   // contributes nothing; G arrives uninitialised, so its zeros are written
            if (G)
                for (int c = 0; c < C; ++c) G[(((size_t)b * C + c) * S + Y) * S + X] = 0.0f;
        } else {
            const float scale = (float)g / (float)S;
            int y0, y1, x0, x1;
            float wy0, wy1, wx0, wx1;
            taps(Y, scale, g, y0, y1, wy0, wy1);
            taps(X, scale, g, x0, x1, wx0, wx1);
            const bool bad = tl < 0 || tl >= C;
            const int t = bad ? -1 : (int)tl;
            auto logit = [&](int c) {
                const float* zt = Z + (((size_t)b * C + c) * g + y0) * g;
                const float* zb = Z + (((size_t)b * C + c) * g + y1) * g;
                const float top = __fmaf_rn(zt[x0], wx0, __fmul_rn(zt[x1], wx1));
                const float bot = __fmaf_rn(zb[x0], wx0, __fmul_rn(zb[x1], wx1));
                return __fmaf_rn(top, wy0, __fmul_rn(bot, wy1));
            };
            float m = -INFINITY, ssum = 0.f, picked = 0.f;
            double swz = 0.0, sw = 0.0;
            for (int c = 0; c < C; ++c) {  // online logsumexp
                const float v = logit(c);
                if (c == t) picked = v;
                const float mn = fmaxf(m, v);
                ssum = ssum * expf(m - mn) + expf(v - mn);
                m = mn;
                if (smooth) {
                    const double wc = (double)wsh[c];
                    swz += wc * (double)v;
                    sw += wc;
                }
            }
            const float lse = m + logf(ssum);
            const float wy = bad ? 1.f : wsh[t];
            const float a = (1.f - o.eps) * wy;          // weight of the picked-class term
            const float bsm = o.eps / (float)C;          // weight of each class's smoothing term
            if (d.use_ce) {
                local = (double)a * (double)(lse - picked);
                if (smooth) slocal = (double)bsm * ((double)lse * sw - swz);
                if (bad) local = (double)NAN;
            }
            if (G) {
                float inv = 0.f, sap = 0.f;
                if (d.use_ce) inv = gscale / (float)(den ? *den : den_plain);   // den == 0: inf, and 0 * inf = NaN as the arithmetic gives
                if (d.use_dice)   // sum_k a_k p_k (a bad label: its P_c, hence a_c, are NaN already)
                    for (int c = 0; c < C; ++c) sap += (c == t ? a1sh[c] : a0sh[c]) * expf(logit(c) - lse);
                const float swf = (float)sw;
                const float dwg = d.dw * gscale;
                for (int c = 0; c < C; ++c) {
                    const float pc = expf(logit(c) - lse);
                    float out = 0.f;
                    if (d.use_ce) {
                        float v = (a * (pc - (c == t ? 1.f : 0.f))) * inv;
                        if (smooth) v += (bsm * (pc * swf - wsh[c])) * inv;
                        out = d.cw * v;
                    }
                    if (d.use_dice) {
                        const float dv = dwg * (pc * ((c == t ? a1sh[c] : a0sh[c]) - sap));
                        out = d.use_ce ? out + dv : dv;
                    }
                    G[(((size_t)b * C + c) * S + Y) * S + X] = bad ? NAN : out;
                }
            }
        }
    }
    if (!d.use_ce) return;   // (uniform over the grid) no CE partials: the finish kernel does not read them
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) local += __shfl_xor(local, s, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local;
    __syncthreads();
    if (smooth) {   // (uniform over the grid)
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) slocal += __shfl_xor(slocal, s, 64);
        if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = slocal;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        if (smooth) spartial[blockIdx.x] = (sred[0] + sred[1]) + (sred[2] + sred[3]);
    }
}

// terms = {ce_weight CE + dice_weight dice, CE, dice}; CE as ce_finish_opts_kernel (ce_finish_kernel without options) forms
// it, dice from the 3 C sums in fp64; a term that was not formed is an exact 0.  loss_out (optional): terms[0] once more.
__global__ __launch_bounds__(1024) void ce_dice_finish_kernel(const double* __restrict__ partial,
                                                              const double* __restrict__ spartial, int n,
                                                              const double* __restrict__ den, double den_plain,
                                                              const double* __restrict__ sums, int C, DiceOpt d,
                                                              float* __restrict__ terms, float* __restrict__ loss_out) {
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
        const float ce = (float)total;
        double loss = 0.0;
        if (d.use_ce) loss = (double)d.cw * total;
        if (d.use_dice) loss += (double)d.dw * dice;
        terms[0] = (float)loss;
        terms[1] = ce;
        terms[2] = (float)dice;
        if (loss_out) *loss_out = (float)loss;
    }
}

}  // namespace

size_t ce_partial_count(int B, int S) { return ((size_t)B * S * S + 255) / 256; }

int launch_ce_loss(const float* Z, const void* target, int target_is_u8, float* G, double* partial, float* loss, int B,
                   int C, int g, int S, hipStream_t s, float gscale) {
    VITSEG_CHECK_ARG(Z && target && partial && loss, VITSEG_EINVAL, "ce_loss: null pointer");
    const unsigned nb = (unsigned)ce_partial_count(B, S);
    if (target_is_u8)
        hipLaunchKernelGGL(ce_loss_kernel<uint8_t>, dim3(nb), dim3(256), 0, s, Z, (const uint8_t*)target, G, partial, B,
                           C, g, S, gscale);
    else
        hipLaunchKernelGGL(ce_loss_kernel<long long>, dim3(nb), dim3(256), 0, s, Z, (const long long*)target, G,
                           partial, B, C, g, S, gscale);
    VITSEG_LAUNCH_CHECK("ce_loss");
    hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(1024), 0, s, partial, (int)nb, 1.0 / ((double)B * S * S), loss);
    VITSEG_LAUNCH_CHECK("ce_finish");
    return VITSEG_OK;
}

// scratch of the options: the denominator (one double in a 16-byte slot) | the count pass's per-block partials | the loss
// kernel's per-block partials of the smoothing term
size_t ce_count_partial_count(int B, int S) {
    return ((size_t)B * S * S + 256 * CE_COUNT_PER_THREAD - 1) / (256 * CE_COUNT_PER_THREAD);
}
size_t ce_opts_scratch_bytes(int B, int S) {
    return 16 + (ce_count_partial_count(B, S) + ce_partial_count(B, S)) * sizeof(double);
}

int check_ce_options(const vitseg_ce_options& o, int B, int C, int S) {
    VITSEG_CHECK_ARG(o.label_smoothing >= 0.f && o.label_smoothing <= 1.f, VITSEG_EINVAL,
                     "ce options: label_smoothing %f outside [0, 1]", (double)o.label_smoothing);   // (a NaN fails both)
    VITSEG_CHECK_ARG(C >= 1 && C <= 255, VITSEG_EINVAL, "ce options: %d classes (1..255)", C);
    VITSEG_CHECK_ARG(o.scratch && ((uintptr_t)o.scratch & 7) == 0, VITSEG_EINVAL, "ce options: scratch is null or not 8-byte aligned");
    VITSEG_CHECK_ARG(o.scratch_bytes >= ce_opts_scratch_bytes(B, S), VITSEG_EINVAL, "ce options: scratch %zu < required %zu",
                     o.scratch_bytes, ce_opts_scratch_bytes(B, S));
    return VITSEG_OK;
}

int launch_ce_loss_opts(const float* Z, const void* target, int target_is_u8, float* G, double* partial, float* loss, int B,
                        int C, int g, int S, const vitseg_ce_options& opts, hipStream_t s, float gscale) {
    VITSEG_CHECK_ARG(Z && target && partial && loss, VITSEG_EINVAL, "ce_loss: null pointer");
    if (int rc = check_ce_options(opts, B, C, S)) return rc;
    const size_t npx = (size_t)B * S * S;
    const unsigned nb = (unsigned)ce_partial_count(B, S), nc = (unsigned)ce_count_partial_count(B, S);
    double* den = (double*)opts.scratch;
    double* cpart = (double*)((char*)opts.scratch + 16);
    double* spart = cpart + nc;
    const CeOpt o{opts.class_weight, (long long)opts.ignore_index, opts.has_ignore_index != 0, opts.label_smoothing};
    if (target_is_u8)
        hipLaunchKernelGGL(ce_count_kernel<uint8_t>, dim3(nc), dim3(256), 0, s, (const uint8_t*)target, o, cpart, npx, C);
    else
        hipLaunchKernelGGL(ce_count_kernel<long long>, dim3(nc), dim3(256), 0, s, (const long long*)target, o, cpart, npx, C);
    VITSEG_LAUNCH_CHECK("ce_count");
    hipLaunchKernelGGL(ce_count_finish_kernel, dim3(1), dim3(1024), 0, s, cpart, (int)nc, den);
    VITSEG_LAUNCH_CHECK("ce_count_finish");
    if (target_is_u8)
        hipLaunchKernelGGL(ce_loss_opts_kernel<uint8_t>, dim3(nb), dim3(256), 0, s, Z, (const uint8_t*)target, G, partial, spart, den,
                           o, B, C, g, S, gscale);
    else
        hipLaunchKernelGGL(ce_loss_opts_kernel<long long>, dim3(nb), dim3(256), 0, s, Z, (const long long*)target, G, partial,
                           spart, den, o, B, C, g, S, gscale);
    VITSEG_LAUNCH_CHECK("ce_loss_opts");
    hipLaunchKernelGGL(ce_finish_opts_kernel, dim3(1), dim3(1024), 0, s, partial,
                       opts.label_smoothing > 0.f ? (const double*)spart : nullptr, (int)nb, den, loss);
    VITSEG_LAUNCH_CHECK("ce_finish_opts");
    return VITSEG_OK;
}

// scratch of the Dice term: the sums I | P | T (C doubles each) | the sum pass's per-block partials, [3][C][blocks]
static size_t dice_block_count(int B, int S) { return ((size_t)B * S * S + 256 * DICE_PPT - 1) / (256 * DICE_PPT); }
size_t dice_scratch_bytes(int B, int C, int S) { return (size_t)3 * C * (1 + dice_block_count(B, S)) * sizeof(double); }

int check_dice_options(const vitseg_dice_options& d, const vitseg_ce_options* ce, int B, int C, int S) {
    auto weight_ok = [](float v) { return v >= 0.f && v <= FLT_MAX; };   // (a NaN fails both)
    VITSEG_CHECK_ARG(weight_ok(d.ce_weight) && weight_ok(d.dice_weight), VITSEG_EINVAL,
                     "dice options: ce_weight %f / dice_weight %f must be finite and >= 0", (double)d.ce_weight, (double)d.dice_weight);
    VITSEG_CHECK_ARG(d.ce_weight != 0.f || d.dice_weight != 0.f, VITSEG_EINVAL, "dice options: both weights are 0");
    VITSEG_CHECK_ARG(weight_ok(d.smooth), VITSEG_EINVAL, "dice options: smooth %f must be finite and >= 0", (double)d.smooth);
    VITSEG_CHECK_ARG(C >= 1 && C <= 255, VITSEG_EINVAL, "dice options: %d classes (1..255)", C);
    VITSEG_CHECK_ARG(d.include_background || C >= 2, VITSEG_EINVAL, "dice options: include_background = 0 needs C >= 2");
    VITSEG_CHECK_ARG(d.scratch && ((uintptr_t)d.scratch & 7) == 0, VITSEG_EINVAL, "dice options: scratch is null or not 8-byte aligned");
    VITSEG_CHECK_ARG(d.scratch_bytes >= dice_scratch_bytes(B, C, S), VITSEG_EINVAL, "dice options: scratch %zu < required %zu",
                     d.scratch_bytes, dice_scratch_bytes(B, C, S));
    return ce ? check_ce_options(*ce, B, C, S) : VITSEG_OK;
}

int launch_ce_dice_loss(const float* Z, const void* target, int target_is_u8, float* G, double* partial, float* terms,
                        float* loss_out, int B, int C, int g, int S, const vitseg_ce_options* ce,
                        const vitseg_dice_options& dice, hipStream_t s, float gscale) {
    VITSEG_CHECK_ARG(Z && target && partial && terms, VITSEG_EINVAL, "ce_dice_loss: null pointer");
    if (int rc = check_dice_options(dice, ce, B, C, S)) return rc;
    const size_t npx = (size_t)B * S * S;
    const unsigned nb = (unsigned)ce_partial_count(B, S), nc = (unsigned)ce_count_partial_count(B, S);
    const unsigned nd = (unsigned)dice_block_count(B, S);
    const DiceOpt d{dice.ce_weight, dice.dice_weight, dice.smooth, dice.include_background ? 0 : 1, dice.ce_weight != 0.f,
                    dice.dice_weight != 0.f};
    CeOpt o{nullptr, 0, 0, 0.f};
    double *den = nullptr, *cpart = nullptr, *spart = nullptr;
    if (ce) {
        o = CeOpt{ce->class_weight, (long long)ce->ignore_index, ce->has_ignore_index != 0, ce->label_smoothing};
        den = (double*)ce->scratch;
        cpart = (double*)((char*)ce->scratch + 16);
        spart = cpart + nc;
    }
    double* sums = (double*)dice.scratch;
    double* dpart = sums + 3 * C;
    if (ce && d.use_ce) {   // the mean's denominator, as launch_ce_loss_opts leaves it
        if (target_is_u8)
            hipLaunchKernelGGL(ce_count_kernel<uint8_t>, dim3(nc), dim3(256), 0, s, (const uint8_t*)target, o, cpart, npx, C);
        else
            hipLaunchKernelGGL(ce_count_kernel<long long>, dim3(nc), dim3(256), 0, s, (const long long*)target, o, cpart, npx, C);
        VITSEG_LAUNCH_CHECK("ce_count");
        hipLaunchKernelGGL(ce_count_finish_kernel, dim3(1), dim3(1024), 0, s, cpart, (int)nc, den);
        VITSEG_LAUNCH_CHECK("ce_count_finish");
    }
    if (d.use_dice) {
        if (target_is_u8)
            hipLaunchKernelGGL(dice_sum_kernel<uint8_t>, dim3(nd), dim3(256), 0, s, Z, (const uint8_t*)target, o.ignore, o.has_ignore,
                               dpart, nd, B, C, g, S);
        else
            hipLaunchKernelGGL(dice_sum_kernel<long long>, dim3(nd), dim3(256), 0, s, Z, (const long long*)target, o.ignore,
                               o.has_ignore, dpart, nd, B, C, g, S);
        VITSEG_LAUNCH_CHECK("dice_sum");
        hipLaunchKernelGGL(dice_reduce_kernel, dim3(3 * C), dim3(1024), 0, s, dpart, (int)nd, sums);
        VITSEG_LAUNCH_CHECK("dice_reduce");
    }
    const double den_plain = (double)B * S * S;
    const double* denp = d.use_ce ? den : nullptr;
    if (target_is_u8)
        hipLaunchKernelGGL(ce_dice_kernel<uint8_t>, dim3(nb), dim3(256), 0, s, Z, (const uint8_t*)target, G, partial, spart, denp,
                           den_plain, sums, o, d, B, C, g, S, gscale);
    else
        hipLaunchKernelGGL(ce_dice_kernel<long long>, dim3(nb), dim3(256), 0, s, Z, (const long long*)target, G, partial, spart,
                           denp, den_plain, sums, o, d, B, C, g, S, gscale);
    VITSEG_LAUNCH_CHECK("ce_dice");
    hipLaunchKernelGGL(ce_dice_finish_kernel, dim3(1), dim3(1024), 0, s, partial,
                       d.use_ce && o.eps > 0.f ? (const double*)spart : nullptr, (int)nb, denp, den_plain, sums, C, d, terms, loss_out);
    VITSEG_LAUNCH_CHECK("ce_dice_finish");
    return VITSEG_OK;
}

int launch_head1x1(const float* F, const float* W2, const float* b2, float* Z, int B, int Np, int C, hipStream_t s) {
    VITSEG_CHECK_ARG(F && W2 && b2 && Z, VITSEG_EINVAL, "head1x1: null pointer");
    hipLaunchKernelGGL(head1x1_kernel, dim3((B * Np + 3) / 4), dim3(256), 0, s, F, W2, b2, Z, B, Np, C);
    VITSEG_LAUNCH_CHECK("head1x1");
    return VITSEG_OK;
}

int launch_upsample(const float* Z, float* logits, uint8_t* mask, int B, int C, int g, int S, hipStream_t s) {
    VITSEG_CHECK_ARG(Z && (logits || mask), VITSEG_EINVAL, "upsample: null pointer");
    VITSEG_CHECK_ARG(S % 4 == 0 && C >= 1 && C <= 255, VITSEG_ESHAPE, "upsample: S %% 4 != 0 or C out of range");
    const size_t n = (size_t)B * (S / UPR) * (S / 4);
    const int quads = S / 4, bands = S / UPR;
    // staged variants: a block is a whole number of row bands of ONE image -- quads * bpb <= 256 threads, bpb | bands (S = 512:
    // 2 bands = 256 threads; S = 224: 4 bands = 224 threads) -- and the source rows of its output rows must fit the LDS
    int bpb = quads <= 256 ? 256 / quads : 0;
    while (bpb > 1 && bands % bpb) --bpb;
    // few images: smaller blocks rather than a grid of a few dozen (one 224x224 image: 14 blocks of 4 bands took 18 us)
    while (bpb > 1 && (long)B * bands / bpb < 2 * device_num_cus()) {
        int nb = bpb - 1;
        while (nb > 1 && bands % nb) --nb;
        if (quads * nb < 48) break;
        bpb = nb;
    }
    const bool whole = bpb >= 1 && quads * bpb >= 48;
    const int threads = whole ? quads * bpb : 256;
    const int rows_out = whole ? bpb * UPR : 0;
    const size_t nr_max = (size_t)((double)rows_out * g / S) + 3;
    const size_t smem = (size_t)C * nr_max * g * sizeof(float);
    const unsigned blocks_staged = whole ? (unsigned)((size_t)B * bands / bpb) : 0;
    if (whole && C == 2 && !logits && 3 * nr_max * g * sizeof(float) <= 32 * 1024 && !opt(OPT_UPSAMPLE_GLOBAL) &&
        !opt(OPT_NO_MASK2)) {   // mask-only, two classes: the class difference decides (upsample_mask2_kernel)
        hipLaunchKernelGGL(upsample_mask2_kernel, dim3(blocks_staged), dim3(threads), 3 * nr_max * g * sizeof(float), s, Z, mask, B,
                           g, S);
        VITSEG_LAUNCH_CHECK("upsample_mask2");
        return VITSEG_OK;
    }
    if (whole && smem <= 48 * 1024 && !opt(OPT_UPSAMPLE_GLOBAL))
        hipLaunchKernelGGL(upsample_kernel<true>, dim3(blocks_staged), dim3(threads), smem, s, Z, logits, mask, B, C, g, S);
    else
        hipLaunchKernelGGL(upsample_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, Z, logits, mask, B, C,
                           g, S);
    VITSEG_LAUNCH_CHECK("upsample");
    return VITSEG_OK;
}

}  // namespace vitseg
