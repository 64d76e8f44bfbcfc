// The soft-clDice loss on the fused path (include/vitseg_cldice.h holds the semantics, the tie rules and the launch list).
//
// Planes are fp32 [n, H, W], n = K * B on the fused path; every kernel runs one thread per pixel and reads its stencil
// straight from global memory (the 3x3 / 5x5 neighbourhoods of a wave overlap in the cache).  Stage planes: I_0 = the input,
// I_{j+1} = erode(I_j); open(I_k) = dilate(I_{k+1}), so one launch per stage forms I_{j+1} and, from the same window of I_j,
// D_{j-1} = relu(I_{j-1} - dilate(I_j)) and the running skeleton skel_{j-1}.
// The adjoint of stage k (k = iters .. 0), with gs the gradient of the running skeleton:
//   point   u = D_k - skel_{k-1} D_k;  r = [u > 0] gs;  gs <- gs - r D_k;  gD = r - r skel_{k-1}  (k = 0: gD = gs);
//           GV = [I_k - O_k > 0] gD  (the gradient of I_k through the subtraction; that of O_k = dilate(I_{k+1}) is -GV)
//   dilate  T = A - sum of GV over the outputs whose first maximal tap this pixel is   (T = the whole gradient of I_{k+1};
//           A = what I_{k+1} collected as stage k+1's own input, absent at k = iters)
//   erode   A = GV + sum over the outputs of erode(I_k) that chose this pixel of T x {1, 1/2, 0}   (the gradient of I_k)
// after k = 0, A is d / d p; the direct term gamma st joins it there.
#include "cldice.hpp"
#include "loss_pixel.hpp"

// Every product, difference and sum of this file is rounded on its own.  hipcc contracts a * b + c into an fma by default, and
// the header's __fmul_rn / __fsub_rn / __fadd_rn are plain operators compiled under that default, so they fuse all the same
// (the skeleton then differs from torch's in a few pixels per thousand).  The pragma switches contraction off for the
// operators written in this file, and mul_rn / sub_rn / add_rn below are those operators: the stage kernel's device code
// has v_mul_f32 and v_sub_f32 where it had v_fma_f32.
#pragma clang fp contract(off)

namespace vitseg {
namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

constexpr int CLD_SUM_PPB = 1024;   // pixels per block of the sum pass (4 per thread)

__device__ __forceinline__ float relu(float v) { return v > 0.f ? v : 0.f; }

// erode(I) at (y, x) of the plane pl and which taps it chose: ct / rt = -1, 0, +1 (up / left, centre, down / right), the
// first minimal tap in that order; wc / wr: the share of m_col / m_row in the gradient of min(m_col, m_row)
struct Erode {
    float m, wc, wr;
    int ct, rt;
};
__device__ __forceinline__ Erode erode_at(const float* pl, int y, int x, int H, int W) {
    const float* p = pl + (size_t)y * W + x;
    const float c = p[0];
    Erode e;
    float mc = c, mr = c;
    e.ct = 0;
    e.rt = 0;
    if (y > 0) {
        mc = p[-W];
        e.ct = -1;
        if (c < mc) {
            mc = c;
            e.ct = 0;
        }
    }
    if (y + 1 < H) {
        const float d = p[W];
        if (d < mc) {
            mc = d;
            e.ct = 1;
        }
    }
    if (x > 0) {
        mr = p[-1];
        e.rt = -1;
        if (c < mr) {
            mr = c;
            e.rt = 0;
        }
    }
    if (x + 1 < W) {
        const float d = p[1];
        if (d < mr) {
            mr = d;
            e.rt = 1;
        }
    }
    e.m = mr < mc ? mr : mc;
    e.wc = mc < mr ? 1.f : (mc == mr ? 0.5f : 0.f);
    e.wr = 1.f - e.wc;
    return e;
}

// dilate(I) at (y, x): the first maximal in-frame tap of the 3x3 window, dy-major then dx; tap = (dy + 1) * 3 + (dx + 1)
__device__ __forceinline__ float dilate_at(const float* pl, int y, int x, int H, int W, int& tap) {
    float m = -INFINITY;
    tap = 4;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= W) continue;
            const float v = pl[(size_t)yy * W + xx];
            if (v > m) {
                m = v;
                tap = (dy + 1) * 3 + (dx + 1);
            }
        }
    }
    return m;
}

// where thread idx is: the plane's first element, the row and the column
// (all planes of a call hold fewer than 2^31 pixels: 32-bit divisions, a fraction of the 64-bit ones' instructions)
struct PlaneAt {
    size_t base;
    int y, x;
    __device__ __forceinline__ PlaneAt(size_t idx, int H, int W) {
        const unsigned hw = (unsigned)H * (unsigned)W, in = (unsigned)idx % hw;
        base = idx - in;
        y = (int)(in / (unsigned)W);
        x = (int)(in - (unsigned)y * (unsigned)W);
    }
};

// stage j: Inext = erode(Icur) (Inext may be null) and, with Iprev, skel_out = the running skeleton after D = relu(Iprev -
// dilate(Icur)) (skel_prev null: the first, skel = D).  skel_prev may be skel_out: each thread reads its own element first.
__global__ __launch_bounds__(256) void cld_stage_kernel(const float* Iprev, const float* __restrict__ Icur, const float* skel_prev,
                                                        float* __restrict__ Inext, float* skel_out, size_t total, int H, int W) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const PlaneAt at(idx, H, W);
    const float* pl = Icur + at.base;
    if (Inext) Inext[idx] = erode_at(pl, at.y, at.x, H, W).m;
    if (Iprev) {
        int tap;
        const float O = dilate_at(pl, at.y, at.x, H, W, tap);
        const float D = relu(sub_rn(Iprev[idx], O));
        float out = D;
        if (skel_prev) {
            const float sk = skel_prev[idx];
            out = add_rn(sk, relu(sub_rn(D, mul_rn(sk, D))));
        }
        skel_out[idx] = out;
    }
}

// ---- the planes ----

// p and y of the listed classes from the regenerated logits; 0 at void pixels
template <typename TargetT>
__global__ __launch_bounds__(256) void cld_planes_kernel(const float* __restrict__ Z, const TargetT* __restrict__ target, CeOpt o,
                                                         CldClassList list, int K, float* __restrict__ P0, float* __restrict__ Y0,
                                                         int B, int C, int g, int S) {
    const size_t npx = (size_t)B * S * S;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= npx) return;
    const Label l = classify_label((long long)target[idx], o, C);
    if (l.kept) {
        const Pixel px(Z, idx, C, g, S);
        float lse, picked;
        px.lse_picked(l.t, lse, picked);
        for (int k = 0; k < K; ++k) {
            const int c = list.cls[k];
            P0[(size_t)k * npx + idx] = expf(px.logit(c) - lse);
            Y0[(size_t)k * npx + idx] = c == l.t ? 1.f : 0.f;
        }
    } else {
        for (int k = 0; k < K; ++k) {
            P0[(size_t)k * npx + idx] = 0.f;
            Y0[(size_t)k * npx + idx] = 0.f;
        }
    }
}

// the same from given planes: truth 1 = the class, 255 = void
__global__ __launch_bounds__(256) void cld_planes_given_kernel(const float* __restrict__ prob, const unsigned char* __restrict__ truth,
                                                               float* __restrict__ P0, float* __restrict__ Y0, size_t total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const unsigned char t = truth[idx];
    P0[idx] = t == 255 ? 0.f : prob[idx];
    Y0[idx] = t == 1 ? 1.f : 0.f;
}

// ---- the sums ----

// per-block fp64 partials of sum sp y | sum sp | sum st p | sum st: partial[q][plane][block]; block = plane * nblk + its
// block within the plane, so that no block straddles two images
__global__ __launch_bounds__(256) void cld_sum_kernel(const float* __restrict__ Sp, const float* __restrict__ Y0,
                                                      const float* __restrict__ St, const float* __restrict__ P0,
                                                      double* __restrict__ partial, int hw, int n, unsigned nblk) {
    __shared__ double red[4][4];
    const unsigned plane = blockIdx.x / nblk, blk = blockIdx.x % nblk;
    const size_t pbase = (size_t)plane * hw;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
    for (int k = 0; k < CLD_SUM_PPB / 256; ++k) {
        const int i = (int)blk * CLD_SUM_PPB + k * 256 + threadIdx.x;
        if (i < hw) {
            const double sp = (double)Sp[pbase + i], st = (double)St[pbase + i];
            a0 += sp * (double)Y0[pbase + i];
            a1 += sp;
            a2 += st * (double)P0[pbase + i];
            a3 += st;
        }
    }
    block_sum4_put(a0, red[0]);
    block_sum4_put(a1, red[1]);
    block_sum4_put(a2, red[2]);
    block_sum4_put(a3, red[3]);
    __syncthreads();
    if (threadIdx.x < 4)
        partial[((size_t)threadIdx.x * n + plane) * nblk + blk] = block_sum4_get(red[threadIdx.x]);
}

// imgsum[q][plane] = the fixed-order sum of its row of partials; grid (n, 4)
__global__ __launch_bounds__(1024) void cld_image_sum_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ imgsum) {
    __shared__ double red[1024];
    const size_t row = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    ce_fixed_order_sum(partial + row * nblk, nblk, red);
    if (threadIdx.x == 0) imgsum[row] = red[0];
}

// v[0 .. n) ascending, in place (heap sort: one thread, n = the batch)
__device__ void sort_ascending(double* v, int n) {
    auto sift = [&](int root, int end) {
        for (;;) {
            int child = 2 * root + 1;
            if (child >= end) return;
            if (child + 1 < end && v[child] < v[child + 1]) ++child;
            if (!(v[root] < v[child])) return;
            const double t = v[root];
            v[root] = v[child];
            v[child] = t;
            root = child;
        }
    };
    for (int i = n / 2 - 1; i >= 0; --i) sift(i, n);
    for (int end = n - 1; end > 0; --end) {
        const double t = v[0];
        v[0] = v[end];
        v[end] = t;
        sift(0, end);
    }
}

// One block of 1024 threads (4 K <= 1020).  Thread q K + k adds the B per-image sums of (q, k) in ascending order of their
// value (the order of the batch does not matter); thread k forms class k's terms and coefficients; thread 0 the mean.
// coef[4 k ..] = {alpha, beta, gamma, 0} times scale = weight gscale / K.  extra = {weight cldice, cldice}.
__global__ __launch_bounds__(1024) void cld_finish_kernel(double* __restrict__ imgsum, int B, int K, double smooth, double weight,
                                                          double gscale, double* __restrict__ tot, float* __restrict__ coef,
                                                          double* __restrict__ extra, float* __restrict__ class_terms,
                                                          float* __restrict__ terms4) {
    __shared__ double cl[256];
    const int t = threadIdx.x;
    if (t < 4 * K) {
        double* v = imgsum + (size_t)t * B;
        sort_ascending(v, B);
        double a = 0.0;
        for (int i = 0; i < B; ++i) a += v[i];
        tot[t] = a;
    }
    __syncthreads();
    if (t < K) {
        const double spy = tot[t], sp = tot[K + t], stp = tot[2 * K + t], st = tot[3 * K + t];
        const double dp = sp + smooth, ds = st + smooth;
        const double tp = (spy + smooth) / dp, ts = (stp + smooth) / ds;
        const double sum = tp + ts;
        cl[t] = 1.0 - 2.0 * tp * ts / sum;
        const double dtp = -2.0 * ts * ts / (sum * sum), dts = -2.0 * tp * tp / (sum * sum);
        const double scale = weight * gscale / (double)K;
        coef[4 * t + 0] = (float)(scale * dtp / dp);
        coef[4 * t + 1] = (float)(-scale * dtp * tp / dp);
        coef[4 * t + 2] = (float)(scale * dts / ds);
        coef[4 * t + 3] = 0.f;
        if (class_terms) {
            class_terms[3 * t + 0] = (float)cl[t];
            class_terms[3 * t + 1] = (float)tp;
            class_terms[3 * t + 2] = (float)ts;
        }
        if (terms4 && t == 0) {
            terms4[1] = (float)tp;
            terms4[2] = (float)ts;
            terms4[3] = 0.f;
        }
    }
    __syncthreads();
    if (t == 0) {
        double m = 0.0;
        for (int k = 0; k < K; ++k) m += cl[k];
        m /= (double)K;
        extra[0] = weight * m;
        extra[1] = m;
        if (terms4) terms4[0] = (float)m;
    }
}

// ---- the adjoint ----

// What the two gathers of a stage need to know about a pixel as an OUTPUT, packed by the pointwise step that has both windows
// at hand anyway: bits 0-3 the first maximal tap of dilate(I_{k+1}) here, bits 4-5 / 6-7 the taps m_col / m_row of
// erode(I_k) chose here (+1), bits 8-9 the share of m_col (0: none, 1: half, 2: all).  A gather then reads 9 or 5 codes
// where it would regenerate 9 or 5 windows (81 and 25 loads; the first version's dilate gather alone was 29 % of the call).
__device__ __forceinline__ unsigned short pack_choice(int tap, const Erode& e) {
    const int wcode = e.wc == 1.f ? 2 : (e.wc == 0.5f ? 1 : 0);
    return (unsigned short)(tap | ((e.ct + 1) << 4) | ((e.rt + 1) << 6) | (wcode << 8));
}
__device__ __forceinline__ int code_tap(unsigned c) { return (int)(c & 15u); }
__device__ __forceinline__ int code_ct(unsigned c) { return (int)((c >> 4) & 3u) - 1; }
__device__ __forceinline__ int code_rt(unsigned c) { return (int)((c >> 6) & 3u) - 1; }
__device__ __forceinline__ float code_wc(unsigned c) { return 0.5f * (float)((c >> 8) & 3u); }

// the pointwise step of stage k (the header).  coef != null: k = iters, gs starts as alpha y + beta of the pixel's class
// (per_class pixels each).  skel_prev null: k = 0.
__global__ __launch_bounds__(256) void cld_adj_point_kernel(const float* __restrict__ Ik, const float* __restrict__ Ik1,
                                                            const float* __restrict__ skel_prev, float* __restrict__ gs,
                                                            float* __restrict__ GV, unsigned short* __restrict__ codes,
                                                            const float* __restrict__ coef, const float* __restrict__ Y0,
                                                            unsigned per_class, size_t total, int H, int W) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const PlaneAt at(idx, H, W);
    int tap;
    const float O = dilate_at(Ik1 + at.base, at.y, at.x, H, W, tap);
    const Erode e = erode_at(Ik + at.base, at.y, at.x, H, W);
    codes[idx] = pack_choice(tap, e);
    const float v = sub_rn(Ik[idx], O);
    const float D = relu(v);
    float g;
    if (coef) {
        const float* cf = coef + 4 * ((unsigned)idx / per_class);
        g = add_rn(mul_rn(cf[0], Y0[idx]), cf[1]);
    } else {
        g = gs[idx];
    }
    float gD = g;
    if (skel_prev) {
        const float sk = skel_prev[idx];
        const float u = sub_rn(D, mul_rn(sk, D));
        const float r = u > 0.f ? g : 0.f;
        gs[idx] = sub_rn(g, mul_rn(r, D));
        gD = sub_rn(r, mul_rn(r, sk));
    }
    GV[idx] = v > 0.f ? gD : 0.f;
}

// through O_k = dilate(I_{k+1}): this pixel collects -GV of every output whose first maximal tap it is
__global__ __launch_bounds__(256) void cld_adj_dilate_kernel(const unsigned short* __restrict__ codes, const float* __restrict__ GV,
                                                             const float* __restrict__ A, float* __restrict__ T, size_t total,
                                                             int H, int W) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const PlaneAt at(idx, H, W);
    float acc = A ? A[idx] : 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int oy = at.y + dy;
        if (oy < 0 || oy >= H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int ox = at.x + dx;
            if (ox < 0 || ox >= W) continue;
            const size_t q = at.base + (size_t)oy * W + ox;
            // this pixel is the output's tap (-dy, -dx)
            if (code_tap(codes[q]) == (1 - dy) * 3 + (1 - dx)) acc = sub_rn(acc, GV[q]);
        }
    }
    T[idx] = acc;
}

// through I_{k+1} = erode(I_k), plus the pixel's own GV.  coef != null: k = 0, the result is d / d p and the direct term
// gamma st joins it; truth (plane call): 255 = void, an exact +0.
__global__ __launch_bounds__(256) void cld_adj_erode_kernel(const unsigned short* __restrict__ codes, const float* __restrict__ T,
                                                            const float* __restrict__ GV, float* __restrict__ A,
                                                            const float* __restrict__ coef, const float* __restrict__ St,
                                                            const unsigned char* __restrict__ truth, unsigned per_class,
                                                            size_t total, int H, int W) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const PlaneAt at(idx, H, W);
    const int y = at.y, x = at.x;
    float acc = GV[idx];
    {
        const unsigned c = codes[idx];
        const float t = T[idx], wc = code_wc(c);
        if (code_ct(c) == 0) acc = add_rn(acc, mul_rn(t, wc));
        if (code_rt(c) == 0) acc = add_rn(acc, mul_rn(t, 1.f - wc));
    }
    if (y > 0) {   // the output above: this pixel is its lower tap
        const unsigned c = codes[idx - W];
        if (code_ct(c) == 1) acc = add_rn(acc, mul_rn(T[idx - W], code_wc(c)));
    }
    if (y + 1 < H) {
        const unsigned c = codes[idx + W];
        if (code_ct(c) == -1) acc = add_rn(acc, mul_rn(T[idx + W], code_wc(c)));
    }
    if (x > 0) {
        const unsigned c = codes[idx - 1];
        if (code_rt(c) == 1) acc = add_rn(acc, mul_rn(T[idx - 1], 1.f - code_wc(c)));
    }
    if (x + 1 < W) {
        const unsigned c = codes[idx + 1];
        if (code_rt(c) == -1) acc = add_rn(acc, mul_rn(T[idx + 1], 1.f - code_wc(c)));
    }
    if (coef) {
        acc = add_rn(acc, mul_rn(coef[4 * ((unsigned)idx / per_class) + 2], St[idx]));
        if (truth && truth[idx] == 255) acc = 0.f;
    }
    A[idx] = acc;
}

// ---- host ----

inline unsigned blocks256(size_t total) { return (unsigned)((total + 255) / 256); }

bool shape_ok(long long n, int H, int W) {
    return n >= 1 && H >= 1 && W >= 1 && (unsigned long long)n * (unsigned long long)H * (unsigned long long)W < (1ull << 31);
}

// soft_skel of I0 into skel: stage(j) = I_j for j >= 1 (distinct from I_{j-1} and I_{j+1}), skel_of(k) = where skel_k goes
template <typename StageOf, typename SkelOf>
int run_skeleton(const float* I0, int iters, StageOf stage, SkelOf skel_of, size_t total, int H, int W, hipStream_t s) {
    for (int j = 0; j <= iters + 1; ++j) {
        const float* Icur = j == 0 ? I0 : stage(j);
        const float* Iprev = j == 0 ? nullptr : (j == 1 ? I0 : stage(j - 1));
        float* Inext = j <= iters ? stage(j + 1) : nullptr;
        const float* skel_prev = j >= 2 ? skel_of(j - 2) : nullptr;
        float* skel_out = j >= 1 ? skel_of(j - 1) : nullptr;
        hipLaunchKernelGGL(cld_stage_kernel, dim3(blocks256(total)), dim3(256), 0, s, Iprev, Icur, skel_prev, Inext, skel_out, total, H,
                           W);
        VITSEG_LAUNCH_CHECK("cldice stage");
    }
    return VITSEG_OK;
}

struct Layout {
    size_t extra, coef, tot, imgsum, partial, codes, planes, plane_bytes, total;
    unsigned nblk;
};
Layout layout(size_t n, int K, int H, int W, int iters) {
    const size_t hw = (size_t)H * W;
    Layout l;
    l.nblk = (unsigned)((hw + CLD_SUM_PPB - 1) / CLD_SUM_PPB);
    size_t o = 0;
    l.extra = o;    o += 256;
    l.coef = o;     o += up256((size_t)4 * K * sizeof(float));
    l.tot = o;      o += up256((size_t)4 * K * sizeof(double));
    l.imgsum = o;   o += up256((size_t)4 * n * sizeof(double));
    l.partial = o;  o += up256((size_t)4 * n * l.nblk * sizeof(double));
    l.codes = o;    o += up256(n * hw * sizeof(unsigned short));
    l.planes = o;
    l.plane_bytes = up256(n * hw * sizeof(float));
    o += (size_t)(2 * iters + 12) * l.plane_bytes;
    l.total = o;
    return l;
}

// The chain on n = K * B planes of H x W whose P0 (p, 0 at void) and Y0 are written: skeletons, sums, finish and, want_grad,
// the adjoint, which leaves d / d p in the plane this returns through *gout.
struct Planes {
    char* base;
    Layout l;
    int iters;
    float* at(int i) const { return (float*)(base + l.planes + (size_t)i * l.plane_bytes); }
    float* P0() const { return at(0); }
    float* Y0() const { return at(1); }
    float* Ip(int j) const { return at(2 + (j - 1)); }                   // I_j of p, j = 1 .. iters + 1
    float* Sp(int k) const { return at(2 + (iters + 1) + k); }           // skel_k of p, k = 0 .. iters
    float* R(int j) const { return at(2 * iters + 4 + (j - 1) % 3); }    // I_j of y, three rotate
    float* St() const { return at(2 * iters + 7); }
    float* gs() const { return at(2 * iters + 8); }
    float* GV() const { return at(2 * iters + 9); }
    float* T() const { return at(2 * iters + 10); }
    float* A() const { return at(2 * iters + 11); }
    unsigned short* codes() const { return (unsigned short*)(base + l.codes); }
};

int run_chain(const Planes& pl, const float* P0, int B, int K, int H, int W, float smooth, float weight, float gscale, bool want_grad,
              float* class_terms, float* terms4, const unsigned char* truth, float* gout, hipStream_t s) {
    const int iters = pl.iters;
    const size_t n = (size_t)K * B, hw = (size_t)H * W, total = n * hw, per_class = (size_t)B * hw;
    const Layout& l = pl.l;
    if (int rc = run_skeleton(P0, iters, [&](int j) { return pl.Ip(j); }, [&](int k) { return pl.Sp(k); }, total, H, W, s)) return rc;
    if (int rc = run_skeleton(pl.Y0(), iters, [&](int j) { return pl.R(j); }, [&](int) { return pl.St(); }, total, H, W, s)) return rc;
    double* partial = (double*)(pl.base + l.partial);
    double* imgsum = (double*)(pl.base + l.imgsum);
    double* tot = (double*)(pl.base + l.tot);
    double* extra = (double*)(pl.base + l.extra);
    float* coef = (float*)(pl.base + l.coef);
    hipLaunchKernelGGL(cld_sum_kernel, dim3((unsigned)(n * l.nblk)), dim3(256), 0, s, pl.Sp(iters), pl.Y0(), pl.St(), P0, partial,
                       (int)hw, (int)n, l.nblk);
    VITSEG_LAUNCH_CHECK("cldice sums");
    hipLaunchKernelGGL(cld_image_sum_kernel, dim3((unsigned)n, 4), dim3(1024), 0, s, partial, (int)l.nblk, imgsum);
    VITSEG_LAUNCH_CHECK("cldice image sums");
    hipLaunchKernelGGL(cld_finish_kernel, dim3(1), dim3(1024), 0, s, imgsum, B, K, (double)smooth, (double)weight, (double)gscale, tot,
                       coef, extra, class_terms, terms4);
    VITSEG_LAUNCH_CHECK("cldice finish");
    if (!want_grad) return VITSEG_OK;
    const unsigned nb = blocks256(total);
    for (int k = iters; k >= 0; --k) {
        const float* Ik = k == 0 ? P0 : pl.Ip(k);
        const float* Ik1 = pl.Ip(k + 1);
        hipLaunchKernelGGL(cld_adj_point_kernel, dim3(nb), dim3(256), 0, s, Ik, Ik1, k > 0 ? (const float*)pl.Sp(k - 1) : nullptr, pl.gs(),
                           pl.GV(), pl.codes(), k == iters ? (const float*)coef : nullptr, (const float*)pl.Y0(), (unsigned)per_class, total,
                           H, W);
        VITSEG_LAUNCH_CHECK("cldice adjoint (point)");
        hipLaunchKernelGGL(cld_adj_dilate_kernel, dim3(nb), dim3(256), 0, s, (const unsigned short*)pl.codes(), (const float*)pl.GV(),
                           k == iters ? nullptr : (const float*)pl.A(), pl.T(), total, H, W);
        VITSEG_LAUNCH_CHECK("cldice adjoint (dilate)");
        hipLaunchKernelGGL(cld_adj_erode_kernel, dim3(nb), dim3(256), 0, s, (const unsigned short*)pl.codes(), (const float*)pl.T(),
                           (const float*)pl.GV(),
                           k == 0 && gout ? gout : pl.A(),
                           k == 0 ? (const float*)coef : nullptr, (const float*)pl.St(), k == 0 ? truth : nullptr, (unsigned)per_class, total, H,
                           W);
        VITSEG_LAUNCH_CHECK("cldice adjoint (erode)");
    }
    return VITSEG_OK;
}

}  // namespace

size_t cldice_scratch_bytes(int B, int K, int S, int iters) {
    if (K < 1 || iters < 0 || iters > VITSEG_CLDICE_MAX_ITERS || !shape_ok((long long)K * B, S, S) || B < 1) return 0;
    return layout((size_t)K * B, K, S, S, iters).total;
}

int check_cldice_options(const vitseg_cldice_options& c, int B, int C, int S) {
    VITSEG_CHECK_ARG(c.weight >= 0.f && c.weight < INFINITY, VITSEG_EINVAL, "cldice options: weight %f is negative or not finite",
                     (double)c.weight);   // (a NaN fails both)
    VITSEG_CHECK_ARG(c.smooth > 0.f && c.smooth < INFINITY, VITSEG_EINVAL, "cldice options: smooth %f must be finite and > 0",
                     (double)c.smooth);
    VITSEG_CHECK_ARG(c.iters >= 0 && c.iters <= VITSEG_CLDICE_MAX_ITERS, VITSEG_EINVAL, "cldice options: iters %d outside 0..%d", c.iters,
                     VITSEG_CLDICE_MAX_ITERS);
    VITSEG_CHECK_ARG(C >= 1 && C <= 255, VITSEG_EINVAL, "cldice options: %d classes (1..255)", C);
    VITSEG_CHECK_ARG(c.K >= 1 && c.K <= C, VITSEG_EINVAL, "cldice options: K = %d listed classes (1..%d)", c.K, C);
    VITSEG_CHECK_ARG(c.classes, VITSEG_EINVAL, "cldice options: classes is null");
    bool seen[256] = {};
    for (int k = 0; k < c.K; ++k) {
        const int cls = c.classes[k];
        VITSEG_CHECK_ARG(cls >= 0 && cls < C, VITSEG_EINVAL, "cldice options: class %d outside [0, %d)", cls, C);
        VITSEG_CHECK_ARG(!seen[cls], VITSEG_EINVAL, "cldice options: class %d is listed twice", cls);
        seen[cls] = true;
    }
    VITSEG_CHECK_ARG(B >= 1 && shape_ok((long long)c.K * B, S, S), VITSEG_EINVAL, "cldice options: %d x %d x %d x %d plane pixels (1 .. 2^31 - 1)",
                     c.K, B, S, S);
    VITSEG_CHECK_ARG(c.scratch && ((uintptr_t)c.scratch & 7) == 0, VITSEG_EINVAL, "cldice options: scratch is null or not 8-byte aligned");
    VITSEG_CHECK_ARG(c.scratch_bytes >= cldice_scratch_bytes(B, c.K, S, c.iters), VITSEG_EINVAL, "cldice options: scratch %zu < required %zu",
                     c.scratch_bytes, cldice_scratch_bytes(B, c.K, S, c.iters));
    return VITSEG_OK;
}

int launch_cldice_term(const float* Z, const void* target, int target_is_u8, const CeOpt& o, int B, int C, int g, int S,
                       const vitseg_cldice_options& c, bool want_grad, float gscale, hipStream_t s, CldTerm* out) {
    const int K = c.K;
    const size_t npx = (size_t)B * S * S;
    Planes pl{(char*)c.scratch, layout((size_t)K * B, K, S, S, c.iters), c.iters};
    CldClassList list = {};
    out->map = CldClassMap{};
    for (int k = 0; k < K; ++k) {
        list.cls[k] = (unsigned char)c.classes[k];
        out->map.slot[c.classes[k]] = (unsigned char)(k + 1);
    }
    float* P0 = c.prob_planes ? c.prob_planes : pl.P0();
    CeOpt oo = o;
    oo.weight = nullptr;   // the label rule alone
    with_target_type(target, target_is_u8, [&](auto* t) {
        hipLaunchKernelGGL(cld_planes_kernel<target_t<decltype(t)>>, dim3(blocks256(npx)), dim3(256), 0, s, Z, t, oo, list, K, P0, pl.Y0(), B,
                           C, g, S);
    });
    VITSEG_LAUNCH_CHECK("cldice planes");
    if (int rc = run_chain(pl, P0, B, K, S, S, c.smooth, c.weight, gscale, want_grad, c.class_terms, nullptr, nullptr, nullptr, s)) return rc;
    out->extra = (const double*)(pl.base + pl.l.extra);
    out->gplanes = want_grad ? pl.A() : nullptr;
    return VITSEG_OK;
}

}  // namespace vitseg

extern "C" {

using namespace vitseg;

int vitseg_cldice_version(void) { return VITSEG_CLDICE_VERSION; }

size_t vitseg_soft_skeleton_scratch_bytes(int n, int H, int W) {
    return shape_ok(n, H, W) ? 3 * up256((size_t)n * H * W * sizeof(float)) : 0;
}

int vitseg_soft_skeleton(const float* p, int n, int H, int W, int iters, float* skel, void* scratch, void* stream) {
    VITSEG_CHECK_ARG(p && skel && scratch, VITSEG_EINVAL, "soft_skeleton: null pointer");
    VITSEG_CHECK_ARG(((uintptr_t)scratch & 7) == 0, VITSEG_EINVAL, "soft_skeleton: scratch is not 8-byte aligned");
    VITSEG_CHECK_ARG(shape_ok(n, H, W), VITSEG_EINVAL, "soft_skeleton: %d x %d x %d pixels (1 .. 2^31 - 1)", n, H, W);
    VITSEG_CHECK_ARG(iters >= 0 && iters <= VITSEG_CLDICE_MAX_ITERS, VITSEG_EINVAL, "soft_skeleton: iters %d outside 0..%d", iters,
                     VITSEG_CLDICE_MAX_ITERS);
    const size_t total = (size_t)n * H * W, pb = up256(total * sizeof(float));
    char* base = (char*)scratch;
    return run_skeleton(p, iters, [&](int j) { return (float*)(base + (size_t)((j - 1) % 3) * pb); }, [&](int) { return skel; }, total, H, W,
                        (hipStream_t)stream);
}

size_t vitseg_soft_cldice_scratch_bytes(int n, int H, int W, int iters) {
    if (!shape_ok(n, H, W) || iters < 0 || iters > VITSEG_CLDICE_MAX_ITERS) return 0;
    return layout((size_t)n, 1, H, W, iters).total;
}

int vitseg_soft_cldice(const float* prob, const uint8_t* truth_u8, int n, int H, int W, int iters, float smooth, float grad_scale,
                       void* scratch, float* terms, float* grad_prob, void* stream) {
    VITSEG_CHECK_ARG(prob && truth_u8 && scratch && terms, VITSEG_EINVAL, "soft_cldice: null pointer");
    VITSEG_CHECK_ARG(((uintptr_t)scratch & 7) == 0, VITSEG_EINVAL, "soft_cldice: scratch is not 8-byte aligned");
    VITSEG_CHECK_ARG(shape_ok(n, H, W), VITSEG_EINVAL, "soft_cldice: %d x %d x %d pixels (1 .. 2^31 - 1)", n, H, W);
    VITSEG_CHECK_ARG(iters >= 0 && iters <= VITSEG_CLDICE_MAX_ITERS, VITSEG_EINVAL, "soft_cldice: iters %d outside 0..%d", iters,
                     VITSEG_CLDICE_MAX_ITERS);
    VITSEG_CHECK_ARG(smooth > 0.f && smooth < INFINITY, VITSEG_EINVAL, "soft_cldice: smooth %f must be finite and > 0", (double)smooth);
    hipStream_t s = (hipStream_t)stream;
    const size_t total = (size_t)n * H * W;
    Planes pl{(char*)scratch, layout((size_t)n, 1, H, W, iters), iters};
    hipLaunchKernelGGL(cld_planes_given_kernel, dim3(blocks256(total)), dim3(256), 0, s, prob, truth_u8, pl.P0(), pl.Y0(), total);
    VITSEG_LAUNCH_CHECK("cldice planes");
    return run_chain(pl, pl.P0(), n, 1, H, W, smooth, 1.f, grad_scale, grad_prob != nullptr, nullptr, terms, truth_u8, grad_prob, s);
}

size_t vitseg_cldice_scratch_bytes(int batch, int K, int S, int iters) { return cldice_scratch_bytes(batch, K, S, iters); }

int vitseg_ce_cldice_loss(const float* lowres, const void* target, int target_is_u8, float* grad_logits, void* scratch, float* terms,
                          int batch, int C, int g, int S, const vitseg_ce_options* ce_opts, const vitseg_dice_options* dice_opts,
                          const vitseg_cldice_options* cld, float loss_scale, void* stream) {
    VITSEG_CHECK_ARG(batch >= 1 && C >= 1 && g >= 1 && S >= g, VITSEG_EINVAL, "ce_cldice_loss: bad shape");
    FusedLoss f;
    f.ce = ce_opts;
    f.dice = dice_opts;
    f.cldice = cld;
    f.terms = terms;
    f.terms4 = true;
    return launch_fused_loss(lowres, target, target_is_u8, grad_logits, (double*)scratch, nullptr, batch, C, g, S, f, (hipStream_t)stream,
                             loss_scale);
}

}  // extern "C"
