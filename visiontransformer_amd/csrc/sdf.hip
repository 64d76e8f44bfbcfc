// Exact Euclidean distance transforms of binary masks and the signed-distance targets of the binary PAED dataset
// (model/PAED/classes.py:51-85 StructuralDamageDataset.__getitem__ -> segmentation.compute_sdf, segmentation.py:6-34:
// scipy.ndimage.distance_transform_edt of ~mask and of mask, each divided by its maximum).
//
// Meijster, Roerdink & Hesselink (2000), the separable linear-time EDT, for both polarities in the same launches.  The
// field "ext" has the mask pixels (non-zero bytes) as features, "int" the others; a feature pixel gets 0.  Three launches:
//  1. column   one thread per (image, column): down and up sweeps give g = distance to the nearest feature pixel in the
//              column, INF = H + W when the column has none.  g is kept as int32 bits in the field's output buffer.
//  2. row      one wave per block of R rows of one field: the rows of g are staged in LDS (uint16: g <= INF <= 32768),
//              then one lane per row builds the lower envelope of the parabolas (x - i)^2 + g(i)^2 over the columns i with
//              a finite g (stacks s[], t[] as packed uint16 pairs in LDS) and scans it back, writing d2 = the exact
//              squared distance as int32 bits over g.  The maximum d2 of each (image, field) is folded into one scratch
//              word by a wave max and atomicMax.  A row with no finite g belongs to an image without any feature pixel
//              (a feature pixel makes its whole column finite); it takes scipy's virtual feature at (-1, 0):
//              d2 = (y + 1)^2 + x^2.
//  3. finish   d = (float) sqrt((double) d2), as scipy takes the root in float64 and casts; normalised: d / max with
//              max = (float) sqrt((double) max_d2), IEEE float division, 0 everywhere when max_d2 == 0.
// Everything before the final conversion is integer arithmetic and the maximum is an order-independent atomicMax, so the
// results are the same bits on every call, and an image's result does not depend on the other images of the batch.
// With 1 <= H, W <= 16384 every squared distance and every Sep numerator lies below 2^30: int32 throughout.
#include <algorithm>

#include "kernels.hpp"

namespace vitseg {
namespace {

constexpr int SDF_MAX_SIDE = 16384;
constexpr int ROW_LDS_TARGET = 80 * 1024;   // two row blocks per CU when a block of R >= 1 rows fits

struct SdfOut {
    int* f[2];   // ext, int: g, then d2, as int32 bits in the float outputs; NULL = field skipped
};

__global__ __launch_bounds__(256) void sdf_column_kernel(const unsigned char* __restrict__ mask, SdfOut o, int H, int W) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const int INF = H + W;
    const size_t base = (size_t)blockIdx.y * H * W + x;
    const unsigned char* m = mask + base;
    int* ge = o.f[0] ? o.f[0] + base : nullptr;
    int* gi = o.f[1] ? o.f[1] + base : nullptr;
    int last_m = -INF, last_b = -INF;   // row of the last mask / non-mask pixel above; y - (-INF) >= INF
#pragma unroll 8
    for (int y = 0; y < H; ++y) {
        if (m[(size_t)y * W]) last_m = y;
        else last_b = y;
        if (ge) ge[(size_t)y * W] = min(y - last_m, INF);
        if (gi) gi[(size_t)y * W] = min(y - last_b, INF);
    }
    int next_m = H + INF, next_b = H + INF;
#pragma unroll 8
    for (int y = H - 1; y >= 0; --y) {
        if (m[(size_t)y * W]) next_m = y;
        else next_b = y;
        if (ge) ge[(size_t)y * W] = min(ge[(size_t)y * W], next_m - y);
        if (gi) gi[(size_t)y * W] = min(gi[(size_t)y * W], next_b - y);
    }
}

__device__ __forceinline__ int wave_max(int v) {
    for (int d = WAVE / 2; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

// block (row block, field slot, image); 64 threads, lane r < R owns row y0 + r.  LDS: g uint16 [R][Wp], then the stack /
// result words uint32 [R][Wp] (Wp = W | 1: odd strides keep the lanes' equal-column accesses on different banks).
__global__ __launch_bounds__(64) void sdf_row_kernel(SdfOut o, int* __restrict__ maxw, int H, int W, int R, int Wp,
                                                     int f0) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int field = f0 + blockIdx.y;
    int* d = o.f[field] + (size_t)blockIdx.z * H * W;
    const int y0 = blockIdx.x * R, rows = min(R, H - y0), lane = threadIdx.x, INF = H + W;
    unsigned short* G = reinterpret_cast<unsigned short*>(lds);
    unsigned* S = reinterpret_cast<unsigned*>(lds + (((size_t)R * Wp * 2 + 15) & ~(size_t)15));
    for (int r = 0; r < rows; ++r)
        for (int c = lane; c < W; c += WAVE) G[r * Wp + c] = (unsigned short)d[(size_t)(y0 + r) * W + c];
    __syncthreads();
    int mx = 0;
    if (lane < rows) {
        const unsigned short* g = G + lane * Wp;
        unsigned* st = S + lane * Wp;   // st[k] = s | t << 16 while the envelope is built; d2 of column x afterwards
        int k = -1, sk = 0, tk = 0, gk = 0;   // the top of the stack, in registers
        for (int u = 0; u < W; ++u) {
            const int gu = g[u];
            if (gu >= INF) continue;
            while (k >= 0 && (tk - sk) * (tk - sk) + gk * gk > (tk - u) * (tk - u) + gu * gu) {
                if (--k >= 0) {
                    const unsigned e = st[k];
                    sk = (int)(e & 0xffffu);
                    tk = (int)(e >> 16);
                    gk = g[sk];
                }
            }
            if (k < 0) {
                k = 0;
                sk = u;
                tk = 0;
                gk = gu;
                st[0] = (unsigned)u;
            } else {
                // Sep(sk, u) = floor((u^2 - sk^2 + g(u)^2 - g(sk)^2) / (2 (u - sk))).  Parabola sk survived the loop, so it is
                // not above parabola u at x = tk >= 0, which makes the numerator >= 2 tk (u - sk) >= 0: the unsigned
                // quotient is the floor (a truncating signed one would round a negative numerator the wrong way).
                const unsigned num = (unsigned)(u * u - sk * sk + gu * gu - gk * gk);
                const int w = 1 + (int)(num / (unsigned)(2 * (u - sk)));
                if (w < W) {
                    ++k;
                    sk = u;
                    tk = w;
                    gk = gu;
                    st[k] = (unsigned)u | ((unsigned)w << 16);
                }
            }
        }
        if (k < 0) {   // no feature pixel in the image: scipy's virtual feature at (-1, 0)
            const int yy = (y0 + lane + 1) * (y0 + lane + 1);
            for (int x = 0; x < W; ++x) st[x] = (unsigned)(yy + x * x);
            mx = yy + (W - 1) * (W - 1);
        } else {
            // slot x is written after the top was read; the entries still to be popped lie at k <= t[k] <= x - 1
            for (int x = W - 1; x >= 0; --x) {
                const int v = (x - sk) * (x - sk) + gk * gk;
                st[x] = (unsigned)v;
                mx = max(mx, v);
                if (x == tk && --k >= 0) {
                    const unsigned e = st[k];
                    sk = (int)(e & 0xffffu);
                    tk = (int)(e >> 16);
                    gk = g[sk];
                }
            }
        }
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r)
        for (int c = lane; c < W; c += WAVE) d[(size_t)(y0 + r) * W + c] = (int)S[r * Wp + c];
    mx = wave_max(mx);
    if (lane == 0) atomicMax(&maxw[blockIdx.z * 2 + field], mx);
}

// grid (pixel chunks of 1024, image, field slot): d2 -> float distance, optionally divided by the image's maximum
__global__ __launch_bounds__(256) void sdf_finish_kernel(SdfOut o, const int* __restrict__ maxw, int P, int normalize,
                                                         int f0) {
    const int field = f0 + blockIdx.z;
    int* d = o.f[field] + (size_t)blockIdx.y * P;
    const int mx2 = maxw[blockIdx.y * 2 + field];
    const float mx = (float)sqrt((double)mx2);
    for (int k = 0; k < 4; ++k) {
        const long long i = (long long)blockIdx.x * 1024 + k * 256 + threadIdx.x;
        if (i >= P) return;
        float v = (float)sqrt((double)d[i]);
        if (normalize) v = mx2 == 0 ? 0.0f : v / mx;
        reinterpret_cast<float*>(d)[i] = v;
    }
}

bool shape_ok(int n, int H, int W) {
    return n >= 1 && n <= 65535 && H >= 1 && H <= SDF_MAX_SIDE && W >= 1 && W <= SDF_MAX_SIDE;
}

size_t scratch_bytes(int n) { return up256((size_t)n * 2 * sizeof(int)); }

struct RowPlan {
    int R, Wp;
    size_t lds;
};

RowPlan row_plan(int W) {
    RowPlan p;
    p.Wp = W | 1;
    const size_t row = (size_t)p.Wp * 6;
    p.R = (int)std::max<size_t>(1, std::min<size_t>(WAVE, ROW_LDS_TARGET / row));
    p.lds = (((size_t)p.R * p.Wp * 2 + 15) & ~(size_t)15) + (size_t)p.R * p.Wp * 4;
    return p;
}

// the column and row launches: d2 of the fields f0 .. f0 + nf - 1 as int32 bits in o.f[], their maxima folded into maxw (zeroed
// by the caller)
int launch_d2(const unsigned char* mask, int n, int H, int W, const SdfOut& o, int f0, int nf, int* maxw, hipStream_t s) {
    hipLaunchKernelGGL(sdf_column_kernel, dim3((W + 255) / 256, n), dim3(256), 0, s, mask, o, H, W);
    VITSEG_LAUNCH_CHECK("sdf column");
    const RowPlan p = row_plan(W);
    if (p.lds > 65536) {
        const hipError_t e = hipFuncSetAttribute((const void*)sdf_row_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
        if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(sdf row)");
    }
    hipLaunchKernelGGL(sdf_row_kernel, dim3((H + p.R - 1) / p.R, nf, n), dim3(WAVE), p.lds, s, o, maxw, H, W, p.R, p.Wp, f0);
    VITSEG_LAUNCH_CHECK("sdf row");
    return VITSEG_OK;
}

}  // namespace

size_t sdf_scratch_bytes(int n, int H, int W) { return shape_ok(n, H, W) ? scratch_bytes(n) : 0; }

int launch_sdf(const unsigned char* mask, int n, int H, int W, int normalize, float* sdf_ext, float* sdf_int, void* scratch,
               size_t scratch_bytes_, hipStream_t s) {
    VITSEG_CHECK_ARG(mask && scratch, VITSEG_EINVAL, "sdf: null mask or scratch");
    VITSEG_CHECK_ARG(normalize == 0 || normalize == 1, VITSEG_EINVAL, "sdf: normalize must be 0 or 1, got %d", normalize);
    VITSEG_CHECK_ARG(shape_ok(n, H, W), VITSEG_ESHAPE, "sdf: bad shape n=%d H=%d W=%d (1 <= H, W <= %d, 1 <= n <= 65535)", n,
                     H, W, SDF_MAX_SIDE);
    const size_t need = scratch_bytes(n);
    VITSEG_CHECK_ARG(scratch_bytes_ >= need, VITSEG_EWORKSPACE, "sdf: scratch of %zu bytes, %zu needed", scratch_bytes_, need);
    const SdfOut o{{reinterpret_cast<int*>(sdf_ext), reinterpret_cast<int*>(sdf_int)}};
    const int f0 = sdf_ext ? 0 : 1, nf = (sdf_ext ? 1 : 0) + (sdf_int ? 1 : 0);
    if (nf == 0) return VITSEG_OK;
    int* maxw = (int*)scratch;
    hipError_t e = hipMemsetAsync(maxw, 0, (size_t)n * 2 * sizeof(int), s);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(sdf maxima)");
    const int rc = launch_d2(mask, n, H, W, o, f0, nf, maxw, s);
    if (rc != VITSEG_OK) return rc;
    const int P = H * W;
    hipLaunchKernelGGL(sdf_finish_kernel, dim3((P + 1023) / 1024, n, nf), dim3(256), 0, s, o, maxw, P, normalize, f0);
    VITSEG_LAUNCH_CHECK("sdf finish");
    return VITSEG_OK;
}

int launch_sdf_d2(const unsigned char* mask, int n, int H, int W, int* d2, int* maxw, hipStream_t s) {
    return launch_d2(mask, n, H, W, SdfOut{{d2, nullptr}}, 0, 1, maxw, s);
}

}  // namespace vitseg

extern "C" {

size_t vitseg_sdf_scratch_bytes(int n, int H, int W) { return vitseg::sdf_scratch_bytes(n, H, W); }

int vitseg_sdf(const uint8_t* mask, int n, int H, int W, int normalize, float* sdf_ext, float* sdf_int, void* scratch,
               size_t scratch_bytes, void* stream) {
    return vitseg::launch_sdf(mask, n, H, W, normalize, sdf_ext, sdf_int, scratch, scratch_bytes, (hipStream_t)stream);
}

}  // extern "C"
