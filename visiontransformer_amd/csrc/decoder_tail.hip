// Decoder tail: seg_head.2 (1x1 conv), bilinear upsample, sigmoid -> argmax mask.  (The losses on its output: loss_tail.hip.)
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

}  // namespace

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
