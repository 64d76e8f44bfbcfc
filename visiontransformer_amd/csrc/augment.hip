// Training augmentation (include/vitseg.h "paired affine warp and colour jitter"): ONE launch warps a batch of images
// bilinearly, applies a per-sample 3x4 colour matrix and warps up to two label planes by nearest tap, every plane with its
// own per-sample Q16 affine table:
//   vitseg_augment_matrix   host arithmetic: normalised 2x3 double affine -> Q16 int64 matrix of one (source, output) size
//   vitseg_augment          the launch
// All coordinate arithmetic is int64 and every fp32 operation is a single correctly rounded one, so a numpy restatement
// holds bit for bit (tests/augment_ref.py).  The reference has no counterpart: its datasets are Resize + ToTensor alone.
//
// The kernel is memory-bound (12 B written, 3 B or 12 B gathered per output pixel).  Thread = 4 consecutive output x of one
// row, all three channels, one 16-byte store per channel.  Block = a 16-row x 64-pixel output tile of one sample, each of
// its four waves an 8-row x 32-pixel quarter (8 x 8 threads): whatever the rotation, the wave's taps fall into a compact
// patch of the source, 8 to 16 cache lines per load instruction.  (A wave laid along ONE output row reads a source COLUMN
// under a quarter turn, 64 lines per load: the first version of this kernel, 3.5x slower on a batch with quarter turns.)
// No LDS staging.  The blocks of a launch are dealt to the planes in order (image, mask 0, mask 1); which plane a block
// serves is block-uniform.
#include "kernels.hpp"

namespace vitseg {

constexpr int AUG_MAX_EXTENT = 16384, AUG_RUN = 4, AUG_TILE_H = 16, AUG_TILE_RUNS = 16;
constexpr long long AUG_LIN_MAX = 1LL << 26, AUG_OFF_MAX = 1LL << 40;

namespace {

struct AugPlane {
    const void* src;
    void* out;
    const long long* M;   // device int64 [n, 6]
    int H, W, oh, ow;
    unsigned gx, gy;      // tiles along x and y: ceil(ow / (AUG_RUN * AUG_TILE_RUNS)), ceil(oh / AUG_TILE_H)
    int src_wide;         // image: 1 = float32 NCHW, 0 = uint8 NHWC;  mask: 1 = int64, 0 = uint8
    int out_wide;         // mask: 1 = int64 out, 0 = uint8 out
    unsigned first_block; // the plane's first block of the launch (n * gx * gy blocks)
};

struct AugArgs {
    AugPlane img, mask[2];
    int nmask;
    int border;
    const float* colour;  // device float32 [n, 12] or null
    float fill[3];        // f32 source: the fill of a tap outside the frame
    int fill_u8[3];       // u8 source: the same as an integer 0..255
    long long fill_label;
};

__device__ __forceinline__ long long clampll(long long v, long long lim) { return v < -lim ? -lim : (v > lim ? lim : v); }

struct Affine {
    long long m00, m01, m02, m10, m11, m12;
    __device__ __forceinline__ void load(const long long* __restrict__ M) {
        m00 = clampll(M[0], AUG_LIN_MAX);
        m01 = clampll(M[1], AUG_LIN_MAX);
        m02 = clampll(M[2], AUG_OFF_MAX);
        m10 = clampll(M[3], AUG_LIN_MAX);
        m11 = clampll(M[4], AUG_LIN_MAX);
        m12 = clampll(M[5], AUG_OFF_MAX);
    }
    // |m00 (2x+1)| + |m01 (2y+1)| + |2 m02| + 65536 < 2^26 * 2^15 * 2 + 2^41 + 2^16 < 2^43: no overflow
    __device__ __forceinline__ void at(int x, int y, long long& U, long long& V) const {
        const long long tx = 2 * x + 1, ty = 2 * y + 1;
        U = (m00 * tx + m01 * ty + 2 * m02 - 65536) >> 1;
        V = (m10 * tx + m11 * ty + 2 * m12 - 65536) >> 1;
    }
};

__device__ __forceinline__ int clampi(long long v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }

// the thread's sample, row and first x in block `lb` of the plane; false: the run lies outside the plane
__device__ __forceinline__ bool locate(const AugPlane& p, unsigned lb, size_t& b, int& x0, int& y) {
    const unsigned bx = lb % p.gx, r = lb / p.gx, by = r % p.gy;
    b = r / p.gy;
    const unsigned w = threadIdx.x >> 6, l = threadIdx.x & 63;
    x0 = (int)(bx * AUG_TILE_RUNS + (w & 1) * 8 + (l & 7)) * AUG_RUN;
    y = (int)(by * AUG_TILE_H + (w >> 1) * 8 + (l >> 3));
    return x0 < p.ow && y < p.oh;
}

template <bool F32>
__device__ __forceinline__ void augment_image(const AugArgs& a, unsigned lb) {
    // every product and sum below is rounded on its own: no fused a * b + c.  (Plain operators, not __fmul_rn / __fadd_rn:
    // those are header functions compiled with contraction on, and an inlined pair of them is fused all the same.)
#pragma clang fp contract(off)
    const AugPlane& p = a.img;
    size_t b;
    int x0, y;
    if (!locate(p, lb, b, x0, y)) return;
    Affine A;
    A.load(p.M + b * 6);
    long long U, V;
    A.at(x0, y, U, V);   // one step in x adds 2 m00 to the numerator of U: exactly m00 to U, and m10 to V
    const int H = p.H, W = p.W;
    const size_t splane = (size_t)H * W;
    const float* __restrict__ sf = (const float*)p.src + b * 3 * splane;
    const unsigned char* __restrict__ su = (const unsigned char*)p.src + b * 3 * splane;
    float cm[12];
    if (a.colour) {
#pragma unroll
        for (int i = 0; i < 12; ++i) cm[i] = a.colour[b * 12 + i];
    }
    float res[3][AUG_RUN];
#pragma unroll
    for (int e = 0; e < AUG_RUN; ++e, U += A.m00, V += A.m10) {
        if (x0 + e >= p.ow) {
            res[0][e] = res[1][e] = res[2][e] = 0.f;
            continue;
        }
        const long long ix = U >> 16, iy = V >> 16;
        const int fx = (int)(U & 0xFFFF) >> 8, fy = (int)(V & 0xFFFF) >> 8;
        const int w00 = (256 - fy) * (256 - fx), w01 = (256 - fy) * fx, w10 = fy * (256 - fx), w11 = fy * fx;
        // taps (iy, ix), (iy, ix + 1), (iy + 1, ix), (iy + 1, ix + 1): in-frame flags (CONSTANT) or clamped indices (EDGE)
        int tx[2], ty[2];
        bool okx[2], oky[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            okx[k] = a.border == VITSEG_AUGMENT_EDGE || (ix + k >= 0 && ix + k < W);
            oky[k] = a.border == VITSEG_AUGMENT_EDGE || (iy + k >= 0 && iy + k < H);
            tx[k] = clampi(ix + k, W - 1);
            ty[k] = clampi(iy + k, H - 1);
        }
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (F32) {
                const float* pc = sf + (size_t)c * splane;
                const float p00 = oky[0] && okx[0] ? pc[(size_t)ty[0] * W + tx[0]] : a.fill[c];
                const float p01 = oky[0] && okx[1] ? pc[(size_t)ty[0] * W + tx[1]] : a.fill[c];
                const float p10 = oky[1] && okx[0] ? pc[(size_t)ty[1] * W + tx[0]] : a.fill[c];
                const float p11 = oky[1] && okx[1] ? pc[(size_t)ty[1] * W + tx[1]] : a.fill[c];
                float s = (float)w00 * p00 + (float)w01 * p01;
                s = s + (float)w10 * p10;
                s = s + (float)w11 * p11;
                v[c] = s * 1.52587890625e-05f;   // 2^-16
            } else {
                const int p00 = oky[0] && okx[0] ? su[((size_t)ty[0] * W + tx[0]) * 3 + c] : a.fill_u8[c];
                const int p01 = oky[0] && okx[1] ? su[((size_t)ty[0] * W + tx[1]) * 3 + c] : a.fill_u8[c];
                const int p10 = oky[1] && okx[0] ? su[((size_t)ty[1] * W + tx[0]) * 3 + c] : a.fill_u8[c];
                const int p11 = oky[1] && okx[1] ? su[((size_t)ty[1] * W + tx[1]) * 3 + c] : a.fill_u8[c];
                const int S = w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11;   // <= 255 * 65536: exact in fp32
                v[c] = __fdiv_rn((float)S, 16711680.0f);
            }
        }
        if (a.colour) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float s = cm[4 * c] * v[0] + cm[4 * c + 1] * v[1];
                s = s + cm[4 * c + 2] * v[2];
                s = s + cm[4 * c + 3];
                res[c][e] = fminf(fmaxf(s, 0.f), 1.f);
            }
        } else {
            res[0][e] = v[0];
            res[1][e] = v[1];
            res[2][e] = v[2];
        }
    }
    const size_t oplane = (size_t)p.oh * p.ow;
    float* o = (float*)p.out + b * 3 * oplane + (size_t)y * p.ow + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* oc = o + (size_t)c * oplane;
        if (x0 + AUG_RUN <= p.ow && ((uintptr_t)oc & 15) == 0) {
            const f32x4 v4 = {res[c][0], res[c][1], res[c][2], res[c][3]};
            *(f32x4*)oc = v4;
        } else {
#pragma unroll
            for (int e = 0; e < AUG_RUN; ++e)
                if (x0 + e < p.ow) oc[e] = res[c][e];
        }
    }
}

__device__ __forceinline__ void augment_mask(const AugArgs& a, const AugPlane& p, unsigned lb) {
    size_t b;
    int x0, y;
    if (!locate(p, lb, b, x0, y)) return;
    Affine A;
    A.load(p.M + b * 6);
    long long U, V;
    A.at(x0, y, U, V);
    const int H = p.H, W = p.W;
    const size_t sbase = b * (size_t)H * W, obase = (b * p.oh + y) * (size_t)p.ow;
#pragma unroll
    for (int e = 0; e < AUG_RUN; ++e, U += A.m00, V += A.m10) {
        const int x = x0 + e;
        if (x >= p.ow) break;
        const long long jx = (U + 32768) >> 16, jy = (V + 32768) >> 16;
        long long label;
        if (a.border == VITSEG_AUGMENT_CONSTANT && (jx < 0 || jx >= W || jy < 0 || jy >= H)) {
            label = a.fill_label;
        } else {
            const size_t si = sbase + (size_t)clampi(jy, H - 1) * W + clampi(jx, W - 1);
            label = p.src_wide ? ((const long long*)p.src)[si] : (long long)((const unsigned char*)p.src)[si];
        }
        if (p.out_wide)
            ((long long*)p.out)[obase + x] = label;
        else
            ((unsigned char*)p.out)[obase + x] = (unsigned char)label;
    }
}

__global__ __launch_bounds__(256) void augment_kernel(const AugArgs a) {
    const unsigned bid = blockIdx.x;
    if (a.nmask > 1 && bid >= a.mask[1].first_block) {
        augment_mask(a, a.mask[1], bid - a.mask[1].first_block);
    } else if (a.nmask > 0 && bid >= a.mask[0].first_block) {
        augment_mask(a, a.mask[0], bid - a.mask[0].first_block);
    } else if (a.img.src_wide) {
        augment_image<true>(a, bid);
    } else {
        augment_image<false>(a, bid);
    }
}

int check_extents(const char* what, int H, int W, int oh, int ow) {
    VITSEG_CHECK_ARG(H >= 1 && W >= 1 && H <= AUG_MAX_EXTENT && W <= AUG_MAX_EXTENT, VITSEG_ESHAPE,
                     "augment: %s source %dx%d outside 1..%d a side", what, H, W, AUG_MAX_EXTENT);
    VITSEG_CHECK_ARG(oh >= 1 && ow >= 1 && oh <= AUG_MAX_EXTENT && ow <= AUG_MAX_EXTENT, VITSEG_ESHAPE,
                     "augment: %s output %dx%d outside 1..%d a side", what, oh, ow, AUG_MAX_EXTENT);
    return VITSEG_OK;
}

}  // namespace

int augment_matrix(const double* a, int src_h, int src_w, int dst_h, int dst_w, int64_t* out) {
    VITSEG_CHECK_ARG(a && out, VITSEG_EINVAL, "augment_matrix: null pointer");
    if (int rc = check_extents("matrix", src_h, src_w, dst_h, dst_w)) return rc;
    const double Ws = src_w, Hs = src_h, Wd = dst_w, Hd = dst_h;
    const double e[6] = {Ws * a[0] / Wd, Ws * a[1] / Hd, Ws * a[2], Hs * a[3] / Wd, Hs * a[4] / Hd, Hs * a[5]};
    int64_t q[6];
    for (int i = 0; i < 6; ++i) {
        const double v = rint(65536.0 * e[i]);
        const double lim = (double)((i % 3 == 2) ? AUG_OFF_MAX : AUG_LIN_MAX);
        VITSEG_CHECK_ARG(v >= -lim && v <= lim, VITSEG_ESHAPE,   // (a NaN fails both comparisons)
                         "augment_matrix: entry %d = %g is outside the Q16 range +-2^%d", i, v, i % 3 == 2 ? 40 : 26);
        q[i] = (int64_t)v;
    }
    for (int i = 0; i < 6; ++i) out[i] = q[i];
    return VITSEG_OK;
}

int launch_augment(const void* images, int image_format, int n, int H, int W, int oh, int ow, const int64_t* matrix,
                   const float* colour, float* out, const vitseg_augment_mask* masks, int num_masks, int border,
                   const float* fill, int64_t fill_label, hipStream_t s) {
    VITSEG_CHECK_ARG(n >= 1, VITSEG_ESHAPE, "augment: %d samples", n);
    if (int rc = check_extents("image", H, W, oh, ow)) return rc;
    VITSEG_CHECK_ARG(num_masks >= 0 && num_masks <= 2, VITSEG_EINVAL, "augment: %d label planes (0..2)", num_masks);
    VITSEG_CHECK_ARG(num_masks == 0 || masks, VITSEG_EINVAL, "augment: null mask descriptors");
    for (int i = 0; i < num_masks; ++i)
        if (int rc = check_extents(i ? "mask 1" : "mask 0", masks[i].h, masks[i].w, masks[i].oh, masks[i].ow)) return rc;
    VITSEG_CHECK_ARG(images && matrix && out, VITSEG_EINVAL, "augment: null image, matrix or output pointer");
    VITSEG_CHECK_ARG(image_format == VITSEG_AUGMENT_U8_NHWC || image_format == VITSEG_AUGMENT_F32_NCHW, VITSEG_EINVAL,
                     "augment: unknown image format %d", image_format);
    VITSEG_CHECK_ARG(border == VITSEG_AUGMENT_CONSTANT || border == VITSEG_AUGMENT_EDGE, VITSEG_EINVAL,
                     "augment: unknown border mode %d", border);
    VITSEG_CHECK_ARG(border != VITSEG_AUGMENT_CONSTANT || fill, VITSEG_EINVAL, "augment: CONSTANT border without a fill");
    for (int i = 0; i < num_masks; ++i) {
        VITSEG_CHECK_ARG(masks[i].src && masks[i].matrix && masks[i].out, VITSEG_EINVAL, "augment: null pointer in mask %d", i);
        VITSEG_CHECK_ARG((masks[i].src_is_i64 | 1) == 1 && (masks[i].out_is_i64 | 1) == 1, VITSEG_EINVAL,
                         "augment: unknown label format in mask %d", i);
    }
    AugArgs a = {};
    unsigned long long blocks = 0;
    auto plane = [&](AugPlane& p, const void* src, void* dst, const int64_t* M, int h, int w, int ph, int pw, int sw, int dw) {
        p.src = src;
        p.out = dst;
        p.M = (const long long*)M;
        p.H = h;
        p.W = w;
        p.oh = ph;
        p.ow = pw;
        p.gx = (unsigned)((pw + AUG_RUN * AUG_TILE_RUNS - 1) / (AUG_RUN * AUG_TILE_RUNS));
        p.gy = (unsigned)((ph + AUG_TILE_H - 1) / AUG_TILE_H);
        p.src_wide = sw;
        p.out_wide = dw;
        p.first_block = (unsigned)blocks;
        blocks += (unsigned long long)n * p.gx * p.gy;
    };
    plane(a.img, images, out, matrix, H, W, oh, ow, image_format == VITSEG_AUGMENT_F32_NCHW, 0);
    for (int i = 0; i < num_masks && blocks <= 0x7fffffffULL; ++i)
        plane(a.mask[i], masks[i].src, masks[i].out, masks[i].matrix, masks[i].h, masks[i].w, masks[i].oh, masks[i].ow,
              masks[i].src_is_i64, masks[i].out_is_i64);
    VITSEG_CHECK_ARG(blocks <= 0x7fffffffULL, VITSEG_ESHAPE, "augment: %d samples of these sizes exceed one launch", n);
    a.nmask = num_masks;
    a.border = border;
    a.colour = colour;
    a.fill_label = fill_label;
    for (int c = 0; c < 3; ++c) {
        a.fill[c] = fill ? fill[c] : 0.f;
        const float r = rintf(a.fill[c]);
        a.fill_u8[c] = r >= 0.f ? (r <= 255.f ? (int)r : 255) : 0;   // (a NaN gives 0)
    }
    hipLaunchKernelGGL(augment_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    VITSEG_LAUNCH_CHECK("augment");
    return VITSEG_OK;
}

}  // namespace vitseg

extern "C" {

int vitseg_augment_matrix(const double* affine, int src_h, int src_w, int dst_h, int dst_w, int64_t* matrix) {
    return vitseg::augment_matrix(affine, src_h, src_w, dst_h, dst_w, matrix);
}

int vitseg_augment(const void* images, int image_format, int n, int H, int W, int oh, int ow, const int64_t* matrix,
                   const float* colour, float* out, const vitseg_augment_mask* masks, int num_masks, int border,
                   const float* fill, int64_t fill_label, void* stream) {
    return vitseg::launch_augment(images, image_format, n, H, W, oh, ow, matrix, colour, out, masks, num_masks, border, fill,
                                  fill_label, (hipStream_t)stream);
}

}  // extern "C"
