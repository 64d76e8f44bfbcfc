// Sliding-window inference (include/vitseg.h "overlapping windows"): an image larger than the model's input is covered by
// S x S windows `stride` apart (the last one of an axis shifted back to end at the edge), every window runs through the
// model as one tile, and the tiles' LOW-RES head outputs ([C, g, g] each) are blended into the full-size result:
//   vitseg_window_count / vitseg_window_origins   host arithmetic of the window grid
//   vitseg_window_gather                          image (fp32 NCHW or uint8 HWC) -> fp32 NCHW tiles
//   vitseg_window_blend                           low-res tiles -> logits [n, C, H, W] and / or mask [n, H, W]
// The blend upsamples each covering tile on the fly with the decoder tail's arithmetic (tail_math.hpp), so the per-tile
// full-resolution logits (C*S*S*4 bytes per tile) are never written or read back.  The reference has no counterpart: its
// scripts resize every image to the model's square (model/CE/testViTModel.py:92-97).
#include "kernels.hpp"
#include "tail_math.hpp"

namespace vitseg {

constexpr int WINDOW_MAX_EXTENT = 16384, WINDOW_MAX_S = 4096;

// windows along one axis: 1 + ceil((extent - S) / stride), or a negative status
int window_count(int extent, int S, int stride) {
    VITSEG_CHECK_ARG(S >= 1 && extent >= S, VITSEG_ESHAPE, "window: extent %d is shorter than the window %d", extent, S);
    VITSEG_CHECK_ARG(stride >= 1, VITSEG_ESHAPE, "window: stride %d < 1", stride);
    VITSEG_CHECK_ARG(stride <= S, VITSEG_ESHAPE, "window: stride %d exceeds the window %d (pixels would be left uncovered)", stride, S);
    VITSEG_CHECK_ARG(extent <= WINDOW_MAX_EXTENT, VITSEG_ESHAPE, "window: extent %d > %d", extent, WINDOW_MAX_EXTENT);
    return 1 + (extent - S + stride - 1) / stride;
}

namespace {

// [lo, hi] = the windows of one axis that cover coordinate p: origin <= p < origin + S.  The origins ascend, so the set is
// a run; lo > hi when nothing covers p (a table that is not a window grid).
__device__ __forceinline__ void cover_range(const int* __restrict__ o, int cnt, int S, int p, int& lo, int& hi) {
    int a = 0, b = cnt;   // first index with o[i] + S > p
    while (a < b) {
        const int m = (a + b) >> 1;
        if (o[m] + S > p) b = m; else a = m + 1;
    }
    lo = a;
    a = lo; b = cnt;      // first index with o[i] > p
    while (a < b) {
        const int m = (a + b) >> 1;
        if (o[m] > p) b = m; else a = m + 1;
    }
    hi = a - 1;
}

// tiles [first, first + count) of the image-major, window-row, window-column numbering as fp32 NCHW [count, 3, S, S].
// Block = 256 consecutive x of one tile row; U8: the source is uint8 HWC (a lane reads its pixel's 3 bytes, the wave a
// contiguous span) and is converted as ToTensor does (one correctly rounded division, as vitseg_preprocess_u8 ends).
template <bool U8>
__global__ __launch_bounds__(256) void window_gather_kernel(const void* __restrict__ src, float* __restrict__ out,
                                                            const int* __restrict__ oy, const int* __restrict__ ox, int ny,
                                                            int nx, int H, int W, int S, int first, int xchunks) {
    const unsigned bid = blockIdx.x;
    const int xc = (int)(bid % (unsigned)xchunks);
    const int yy = (int)((bid / (unsigned)xchunks) % (unsigned)S);
    const int lt = (int)(bid / ((unsigned)xchunks * (unsigned)S));
    const int xx = xc * 256 + (int)threadIdx.x;
    if (xx >= S) return;
    const int t = first + lt;
    const int kx = t % nx, ky = (t / nx) % ny, b = t / (nx * ny);
    // (clamped: the origin tables are the caller's device memory, which the host cannot check)
    const int y = min(max(oy[ky] + yy, 0), H - 1), x = min(max(ox[kx] + xx, 0), W - 1);
    const size_t plane = (size_t)S * S, o = (size_t)lt * 3 * plane + (size_t)yy * S + xx;
    if (U8) {
        const unsigned char* p = (const unsigned char*)src + (((size_t)b * H + y) * W + x) * 3;
        out[o] = __fdiv_rn((float)p[0], 255.0f);
        out[o + plane] = __fdiv_rn((float)p[1], 255.0f);
        out[o + 2 * plane] = __fdiv_rn((float)p[2], 255.0f);
    } else {
        const float* p = (const float*)src + ((size_t)b * 3 * H + y) * W + x;
        const size_t splane = (size_t)H * W;
        out[o] = p[0];
        out[o + plane] = p[splane];
        out[o + 2 * plane] = p[2 * splane];
    }
}

// Thread = 4 pixels of one output row; a block = blockDim.y rows x 4 * blockDim.x columns of one image (blockDim.x a
// multiple of 64: a wave lies in one row, so the window rows it walks are wave-uniform).
// VEC (W % 4 == 0: every row of both outputs starts 16-byte / 4-byte aligned): the 4 pixels are consecutive, one 16-byte
// logits store and one 4-byte mask store per class / row.  Otherwise the 4 pixels lie blockDim.x apart and every store
// is one element per lane, consecutive across the wave (256 contiguous bytes of logits per instruction).
// Per class: the covering tiles in increasing tile number (window row outer, window column inner), each tile's value by
// the decoder tail's taps and fma placement at the tile-local coordinate, then
//   one covering tile: the value itself;  else acc = fma(wt, v, acc), ws += wt over the tiles, result = acc / ws.
// The logits are written once and never re-read: non-temporal stores.  The mask: raw argmax where the top-2 margin
// settles the sigmoid comparison (argmax_settled), else the exact fp32 sigmoids of a second pass over the classes.
// No LDS staging of the low-res rows: every tap is a global read that hits L1 / L2 (the tiles of a block's rectangle are
// a few KB).
template <bool VEC>
__global__ __launch_bounds__(256) void window_blend_kernel(const float* __restrict__ Z, const int* __restrict__ oy,
                                                           const int* __restrict__ ox, const float* __restrict__ wtab,
                                                           float* __restrict__ logits, uint8_t* __restrict__ mask, int C,
                                                           int g, int S, int H, int W, int ny, int nx) {
    const int y = (int)(blockIdx.y * blockDim.y + threadIdx.y);
    const int b = (int)blockIdx.z;
    if (y >= H) return;
    const int xbase = (int)blockIdx.x * 4 * (int)blockDim.x;
    int px[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) px[e] = xbase + (VEC ? 4 * (int)threadIdx.x + e : e * (int)blockDim.x + (int)threadIdx.x);
    if (px[0] >= W) return;   // (VEC: W % 4 == 0, so the four pixels are inside together)
    const float scale = (float)g / (float)S;
    int kyl, kyh;
    cover_range(oy, ny, S, y, kyl, kyh);
    int kxl[4], kxh[4], kxmin = nx, kxmax = -1;
    bool inside[4], single[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        inside[e] = px[e] < W;
        cover_range(ox, nx, S, inside[e] ? px[e] : W - 1, kxl[e], kxh[e]);
        if (!inside[e]) { kxl[e] = nx; kxh[e] = -1; }   // covered by nothing: no reads, no stores
        kxmin = min(kxmin, kxl[e]);
        kxmax = max(kxmax, kxh[e]);
        single[e] = kyl == kyh && kxl[e] == kxh[e];
    }
    const size_t gg = (size_t)g * g;
    // the blended values of class c at the thread's 4 pixels
    auto blend = [&](int c, float* res) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f}, ws[4] = {0.f, 0.f, 0.f, 0.f}, one[4] = {0.f, 0.f, 0.f, 0.f};
        for (int ky = kyl; ky <= kyh; ++ky) {
            const int ly = y - oy[ky];
            if ((unsigned)ly >= (unsigned)S) continue;   // (only with origin tables that are no ascending window grid)
            int y0, y1;
            float wy0, wy1;
            taps(ly, scale, g, y0, y1, wy0, wy1);
            const float wrow = wtab[ly];
            for (int kx = kxmin; kx <= kxmax; ++kx) {
                const int o = ox[kx];
                const float* z = Z + ((((size_t)b * ny + ky) * nx + kx) * C + c) * gg;
                const float* zt = z + (size_t)y0 * g;
                const float* zb = z + (size_t)y1 * g;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int lx = px[e] - o;
                    if (!inside[e] || (unsigned)lx >= (unsigned)S) continue;   // this window does not cover the pixel
                    int x0, x1;
                    float wx0, wx1;
                    taps(lx, scale, g, x0, x1, wx0, wx1);
                    const float top = __fmaf_rn(zt[x0], wx0, __fmul_rn(zt[x1], wx1));
                    const float bot = __fmaf_rn(zb[x0], wx0, __fmul_rn(zb[x1], wx1));
                    const float v = __fmaf_rn(top, wy0, __fmul_rn(bot, wy1));
                    const float wt = __fmul_rn(wrow, wtab[lx]);
                    acc[e] = __fmaf_rn(wt, v, acc[e]);
                    ws[e] = __fadd_rn(ws[e], wt);
                    one[e] = v;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) res[e] = single[e] ? one[e] : __fdiv_rn(acc[e], ws[e]);
    };
    float t1[4], t2[4];
    int arg[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        t1[e] = -INFINITY;
        t2[e] = -INFINITY;
        arg[e] = 0;
    }
    for (int c = 0; c < C; ++c) {
        float v[4];
        blend(c, v);
        if (logits) {
            float* row = logits + (((size_t)b * C + c) * H + y) * W;
            if (VEC) {
                const f32x4 v4 = {v[0], v[1], v[2], v[3]};
                __builtin_nontemporal_store(v4, (f32x4*)(row + px[0]));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (inside[e]) __builtin_nontemporal_store(v[e], row + px[e]);
            }
        }
        if (mask) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (v[e] > t1[e]) {   // strict: the first maximal class stays
                    t2[e] = t1[e];
                    t1[e] = v[e];
                    arg[e] = c;
                } else {
                    t2[e] = fmaxf(t2[e], v[e]);
                }
            }
        }
    }
    if (!mask) return;
    bool amb = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) amb = amb || (inside[e] && !argmax_settled(t1[e], t1[e] - t2[e]));
    if (amb) {   // exact path: ATen's fp32 sigmoid of the same blended values, first maximal class wins
        float best[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < C; ++c) {
            float v[4];
            blend(c, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float sg = sigmoid_aten(v[e]);
                if (c == 0 || sg > best[e]) {
                    best[e] = sg;
                    arg[e] = c;
                }
            }
        }
    }
    uint8_t* mrow = mask + ((size_t)b * H + y) * W;
    if (VEC) {
        uchar4 m4;
        m4.x = (unsigned char)arg[0];
        m4.y = (unsigned char)arg[1];
        m4.z = (unsigned char)arg[2];
        m4.w = (unsigned char)arg[3];
        *(uchar4*)(mrow + px[0]) = m4;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (inside[e]) mrow[px[e]] = (unsigned char)arg[e];
    }
}

int check_window_grid(const char* what, int n, int H, int W, int S, int ny, int nx) {
    VITSEG_CHECK_ARG(n >= 1 && n <= 65535, VITSEG_ESHAPE, "%s: %d images (1..65535)", what, n);
    VITSEG_CHECK_ARG(S >= 1 && S <= WINDOW_MAX_S, VITSEG_ESHAPE, "%s: window %d outside 1..%d", what, S, WINDOW_MAX_S);
    VITSEG_CHECK_ARG(H >= S && W >= S && H <= WINDOW_MAX_EXTENT && W <= WINDOW_MAX_EXTENT, VITSEG_ESHAPE,
                     "%s: image %dx%d must be at least the window %d and at most %d a side", what, H, W, S, WINDOW_MAX_EXTENT);
    VITSEG_CHECK_ARG(ny >= 1 && nx >= 1 && ny <= H && nx <= W, VITSEG_ESHAPE, "%s: %d x %d windows on a %dx%d image", what, ny,
                     nx, H, W);
    VITSEG_CHECK_ARG((long long)n * ny * nx <= 0x7fffffffLL, VITSEG_ESHAPE, "%s: %lld tiles", what, (long long)n * ny * nx);
    return VITSEG_OK;
}

}  // namespace

int launch_window_gather(const void* src, int src_is_u8, int n, int H, int W, int S, const int* oy, int ny, const int* ox,
                         int nx, int first, int count, float* out, hipStream_t s) {
    VITSEG_CHECK_ARG(src && oy && ox && out, VITSEG_EINVAL, "window_gather: null pointer");
    if (int rc = check_window_grid("window_gather", n, H, W, S, ny, nx)) return rc;
    const long long tiles = (long long)n * ny * nx;
    VITSEG_CHECK_ARG(first >= 0 && count >= 1 && (long long)first + count <= tiles, VITSEG_EINVAL,
                     "window_gather: tiles [%d, +%d) of %lld", first, count, tiles);
    const int xchunks = (S + 255) / 256;
    const long long blocks = (long long)count * S * xchunks;
    VITSEG_CHECK_ARG(blocks <= 0x7fffffffLL, VITSEG_ESHAPE, "window_gather: %d tiles of %d rows in one call", count, S);
    if (src_is_u8)
        hipLaunchKernelGGL(window_gather_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, src, out, oy, ox, ny, nx, H, W, S,
                           first, xchunks);
    else
        hipLaunchKernelGGL(window_gather_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, src, out, oy, ox, ny, nx, H, W, S,
                           first, xchunks);
    VITSEG_LAUNCH_CHECK("window_gather");
    return VITSEG_OK;
}

int launch_window_blend(const float* lowres, const int* oy, int ny, const int* ox, int nx, const float* w, int n, int C, int g,
                        int S, int H, int W, float* logits, uint8_t* mask, hipStream_t s) {
    VITSEG_CHECK_ARG(lowres && oy && ox && w, VITSEG_EINVAL, "window_blend: null pointer");
    VITSEG_CHECK_ARG(logits || mask, VITSEG_EINVAL, "window_blend: both outputs are null");
    VITSEG_CHECK_ARG(C >= 1 && C <= 255, VITSEG_ESHAPE, "window_blend: %d classes (1..255)", C);
    VITSEG_CHECK_ARG(g >= 1 && g <= S, VITSEG_ESHAPE, "window_blend: grid %d for a window of %d", g, S);
    if (int rc = check_window_grid("window_blend", n, H, W, S, ny, nx)) return rc;
    const bool vec = W % 4 == 0 && (uintptr_t)logits % 16 == 0 && (uintptr_t)mask % 4 == 0;
    // threads along x: a whole number of waves covering the row 4 pixels per thread, at most 256; the rest of the block's
    // 256 threads go to further rows
    int tx = ((W + 3) / 4 + 63) / 64 * 64;
    if (tx > 256) tx = 256;
    const int ty = 256 / tx;
    const dim3 block(tx, ty), grid((W + 4 * tx - 1) / (4 * tx), (H + ty - 1) / ty, n);
    if (vec)
        hipLaunchKernelGGL(window_blend_kernel<true>, grid, block, 0, s, lowres, oy, ox, w, logits, mask, C, g, S, H, W, ny, nx);
    else
        hipLaunchKernelGGL(window_blend_kernel<false>, grid, block, 0, s, lowres, oy, ox, w, logits, mask, C, g, S, H, W, ny, nx);
    VITSEG_LAUNCH_CHECK("window_blend");
    return VITSEG_OK;
}

}  // namespace vitseg

extern "C" {

int vitseg_window_count(int extent, int S, int stride) { return vitseg::window_count(extent, S, stride); }

int vitseg_window_origins(int extent, int S, int stride, int32_t* origins) {
    const int cnt = vitseg::window_count(extent, S, stride);
    if (cnt < 0) return cnt;
    VITSEG_CHECK_ARG(origins, VITSEG_EINVAL, "window_origins: null pointer");
    for (int i = 0; i < cnt; ++i) {
        const long long o = (long long)i * stride;
        origins[i] = o < extent - S ? (int32_t)o : extent - S;   // the last window is shifted back to end at the edge
    }
    return VITSEG_OK;
}

int vitseg_window_gather(const void* src, int src_is_u8, int n, int H, int W, int S, const int32_t* origins_y, int ny,
                         const int32_t* origins_x, int nx, int first, int count, float* tiles, void* stream) {
    return vitseg::launch_window_gather(src, src_is_u8, n, H, W, S, origins_y, ny, origins_x, nx, first, count, tiles,
                                        (hipStream_t)stream);
}

int vitseg_window_blend(const float* lowres, const int32_t* origins_y, int ny, const int32_t* origins_x, int nx,
                        const float* weights, int n, int C, int g, int S, int H, int W, float* logits, uint8_t* mask,
                        void* stream) {
    return vitseg::launch_window_blend(lowres, origins_y, ny, origins_x, nx, weights, n, C, g, S, H, W, logits, mask,
                                       (hipStream_t)stream);
}

}  // extern "C"
