// The Lovasz-Softmax loss on the fused path (include/vitseg_lovasz.h holds the semantics and the launch list).
//
// n segments of L (key, payload) pairs lie side by side; a tile is LOV_TILE consecutive ranks of one segment and one block of
// 256 threads.  The sort is a segmented LSD radix sort, 8 bits a pass.  Per pass:
//   hist     hist[(seg, digit, tile)] = the count of the digit in the tile (integer LDS atomics: only a count results);
//   rowscan  per (seg, digit) the exclusive scan of its row over the tiles, in place, and the row's total;
//   scatter  every block scans the 256 totals of its segment (the digit bases) and ranks its keys: wave w owns the w-th
//            quarter of the tile and walks it 64 keys a round in index order; a key's rank among the equal digits of its
//            round is the popcount of its ballot peers below its lane, the rounds before it are a running count per (wave,
//            digit) in LDS that the wave alone reads and writes, and the waves are joined in wave order after a barrier.
//            Nothing depends on which wave or lane ran first: the same destination on every call.
// Then the ranks: ycount / yscan give every tile the count of y = 1 before it and G; the rank pass walks 8 consecutive ranks
// per thread.
#include "loss_pixel.hpp"
#include "lovasz.hpp"

// every fp64 product and quotient of dJ and of the sums is rounded on its own (the header's semantics; numpy's arithmetic)
#pragma clang fp contract(off)

namespace vitseg {
namespace {

using u32 = unsigned int;
using u64 = unsigned long long;

constexpr int LOV_TILE = VITSEG_LOVASZ_TILE;
constexpr int LOV_ROUNDS = LOV_TILE / 256;   // keys per thread
constexpr u32 LOV_VOID = 0xffffffffu;        // the key of a void pixel: after every error's key
constexpr int LOV_MAX_SEGMENTS = 1 << 20;
static_assert(LOV_TILE % 256 == 0 && LOV_ROUNDS == 8, "the rank pass walks 8 ranks per thread");

// ascending keys = descending errors by bit pattern; a NaN is the canonical quiet NaN and ranks first
__device__ __forceinline__ u32 error_key(float e) {
    u32 b = __float_as_uint(e);
    if (e != e) b = 0x7fc00000u;
    const u32 u = (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
    return ~u;
}
__device__ __forceinline__ float key_error(u32 key) {
    const u32 u = ~key;
    return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

// exclusive scan of one value per thread over a block of 256, in thread order; total: the block's sum
__device__ __forceinline__ u32 block_excl_scan256(u32 v, u32* wsum /* shared [4] */, u32& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u32 up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    u32 base = 0;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    total = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    __syncthreads();   // wsum may be written again
    return base + (inc - v);
}

// row[0 .. len) becomes its exclusive scan; returns the total (to every thread)
__device__ __forceinline__ u32 row_excl_scan(u32* __restrict__ row, int len, u32* wsum) {
    u32 carry = 0;
    for (int base = 0; base < len; base += 256) {
        const int i = base + (int)threadIdx.x;
        const u32 v = i < len ? row[i] : 0u;
        u32 total;
        const u32 ex = block_excl_scan256(v, wsum, total);
        if (i < len) row[i] = carry + ex;
        carry += total;
    }
    return carry;
}

// ---- the planes ----

template <typename TargetT>
__global__ __launch_bounds__(256) void lov_planes_kernel(const float* __restrict__ Z, const TargetT* __restrict__ target, CeOpt o,
                                                         CldClassList list, int K, u32* __restrict__ keys, u32* __restrict__ pay,
                                                         float* __restrict__ prob, int B, int C, int g, int S, int per_image) {
    const size_t npx = (size_t)B * S * S;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= npx) return;
    const u32 pos = per_image ? (u32)idx % ((u32)S * (u32)S) : (u32)idx;
    const Label l = classify_label((long long)target[idx], o, C);
    if (l.kept) {
        const Pixel px(Z, idx, C, g, S);
        float lse, picked;
        px.lse_picked(l.t, lse, picked);
        for (int k = 0; k < K; ++k) {
            const int c = list.cls[k];
            const float p = expf(px.logit(c) - lse);
            const bool y = c == l.t;
            keys[(size_t)k * npx + idx] = error_key(y ? 1.f - p : p);
            pay[(size_t)k * npx + idx] = pos | (y ? 0x80000000u : 0u);
            if (prob) prob[(size_t)k * npx + idx] = p;
        }
    } else {
        for (int k = 0; k < K; ++k) {
            keys[(size_t)k * npx + idx] = LOV_VOID;
            pay[(size_t)k * npx + idx] = pos;
            if (prob) prob[(size_t)k * npx + idx] = 0.f;
        }
    }
}

// the same from given planes: truth 1 = the class, 255 = void
__global__ __launch_bounds__(256) void lov_planes_given_kernel(const float* __restrict__ prob, const unsigned char* __restrict__ truth,
                                                               u32* __restrict__ keys, u32* __restrict__ pay, size_t total, u32 L) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const unsigned char t = truth[idx];
    const u32 pos = (u32)idx % L;
    const bool y = t == 1;
    const float p = prob[idx];
    keys[idx] = t == 255 ? LOV_VOID : error_key(y ? 1.f - p : p);
    pay[idx] = pos | (y && t != 255 ? 0x80000000u : 0u);
}

// ---- one radix pass ----

__global__ __launch_bounds__(256) void lov_hist_kernel(const u32* __restrict__ keys, u32* __restrict__ hist, u32 L, u32 ntile,
                                                       int shift) {
    __shared__ u32 cnt[256];
    const u32 seg = blockIdx.x / ntile, tile = blockIdx.x % ntile;
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const u32* k = keys + (size_t)seg * L;
#pragma unroll
    for (int r = 0; r < LOV_ROUNDS; ++r) {
        const u32 i = tile * LOV_TILE + r * 256 + threadIdx.x;
        if (i < L) atomicAdd(&cnt[(k[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[((size_t)seg * 256 + threadIdx.x) * ntile + tile] = cnt[threadIdx.x];
}

// grid n * 256: the row of (seg, digit)
__global__ __launch_bounds__(256) void lov_rowscan_kernel(u32* __restrict__ hist, u32* __restrict__ rowtot, int ntile) {
    __shared__ u32 wsum[4];
    const u32 total = row_excl_scan(hist + (size_t)blockIdx.x * ntile, ntile, wsum);
    if (threadIdx.x == 0) rowtot[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void lov_scatter_kernel(const u32* __restrict__ keys_in, const u32* __restrict__ pay_in,
                                                          u32* __restrict__ keys_out, u32* __restrict__ pay_out,
                                                          const u32* __restrict__ hist, const u32* __restrict__ rowtot, u32 L,
                                                          u32 ntile, int shift) {
    __shared__ u32 wcnt[4][256];   // per wave: the running count of each digit, then the wave's base in the segment
    __shared__ u32 wsum[4];
    const u32 seg = blockIdx.x / ntile, tile = blockIdx.x % ntile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 unused;
    const u32 dbase = block_excl_scan256(rowtot[(size_t)seg * 256 + threadIdx.x], wsum, unused);   // where the digit starts
#pragma unroll
    for (int w = 0; w < 4; ++w) wcnt[w][threadIdx.x] = 0;
    __syncthreads();
    const size_t sbase = (size_t)seg * L;
    const u64 below = (1ull << lane) - 1ull;
    u32 kk[LOV_ROUNDS], pp[LOV_ROUNDS], rk[LOV_ROUNDS];
#pragma unroll
    for (int r = 0; r < LOV_ROUNDS; ++r) {
        const u32 i = tile * LOV_TILE + wave * (LOV_TILE / 4) + r * 64 + lane;
        const bool valid = i < L;
        kk[r] = valid ? keys_in[sbase + i] : 0u;
        pp[r] = valid ? pay_in[sbase + i] : 0u;
        const u32 d = (kk[r] >> shift) & 255u;
        u64 peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const u64 m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const u32 before_lane = (u32)__popcll(peers & below);
        u32 before = 0;
        if (valid) before = wcnt[wave][d];
        __builtin_amdgcn_wave_barrier();
        if (valid && before_lane == 0) wcnt[wave][d] = before + (u32)__popcll(peers);   // one lane per digit of the round
        __builtin_amdgcn_wave_barrier();
        rk[r] = before + before_lane;
    }
    __syncthreads();
    {   // thread = digit: the waves in order, on top of the digit's base and the earlier tiles' count
        u32 run = dbase + hist[((size_t)seg * 256 + threadIdx.x) * ntile + tile];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const u32 c = wcnt[w][threadIdx.x];
            wcnt[w][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < LOV_ROUNDS; ++r) {
        const u32 i = tile * LOV_TILE + wave * (LOV_TILE / 4) + r * 64 + lane;
        if (i < L) {
            const u32 dest = wcnt[wave][(kk[r] >> shift) & 255u] + rk[r];
            if (dest < L) {   // always, when the histograms are those of these keys
                keys_out[sbase + dest] = kk[r];
                pay_out[sbase + dest] = pp[r];
            }
        }
    }
}

// ---- ranks ----

// ycnt[seg, tile] = the count of y = 1 among the tile's ranks
__global__ __launch_bounds__(256) void lov_ycount_kernel(const u32* __restrict__ pay, u32* __restrict__ ycnt, u32 L, u32 ntile) {
    __shared__ u32 wsum[4];
    const u32 seg = blockIdx.x / ntile, tile = blockIdx.x % ntile;
    const u32* p = pay + (size_t)seg * L;
    u32 c = 0;
#pragma unroll
    for (int r = 0; r < LOV_ROUNDS; ++r) {
        const u32 i = tile * LOV_TILE + r * 256 + threadIdx.x;
        if (i < L) c += p[i] >> 31;
    }
    u32 total;
    block_excl_scan256(c, wsum, total);
    if (threadIdx.x == 0) ycnt[blockIdx.x] = total;
}

// grid n: ycnt[seg, :] becomes the count of y = 1 before each tile; Gs[seg] = G
__global__ __launch_bounds__(256) void lov_yscan_kernel(u32* __restrict__ ycnt, u32* __restrict__ Gs, int ntile) {
    __shared__ u32 wsum[4];
    const u32 total = row_excl_scan(ycnt + (size_t)blockIdx.x * ntile, ntile, wsum);
    if (threadIdx.x == 0) Gs[blockIdx.x] = total;
}

// How the K (pooled) or K B (per image) segments form groups: group q (0, or the image) holds segment k * stride + q of
// every listed class k.
struct LovGroups {
    int K, groups, stride, present_only, per_image;
    __device__ __forceinline__ int seg(int k, int q) const { return k * stride + q; }
};

// one block: K' of every group, coef and whether the class counts, per segment
__global__ __launch_bounds__(256) void lov_coef_kernel(const u32* __restrict__ Gs, LovGroups gr, double weight, double gscale,
                                                       double* __restrict__ coef, int* __restrict__ on) {
    for (int q = threadIdx.x; q < gr.groups; q += 256) {
        int kp = 0;
        for (int k = 0; k < gr.K; ++k) kp += !gr.present_only || Gs[gr.seg(k, q)] > 0;
        double c = 0.0;
        if (kp > 0) {
            c = (weight * gscale) / (double)kp;
            if (gr.per_image) c = c / (double)gr.groups;
        }
        for (int k = 0; k < gr.K; ++k) {
            const int s = gr.seg(k, q);
            coef[s] = c;
            on[s] = !gr.present_only || Gs[s] > 0;
        }
    }
}

// The rank pass: thread t of tile's block walks ranks tile * LOV_TILE + 8 t .. + 7.  coefs null: plain_coef for every segment,
// every segment counts (the planes call).  gout (optional): g at the pixel the payload names; order (optional): the pixel
// at each rank.
__global__ __launch_bounds__(256) void lov_rank_kernel(const u32* __restrict__ keys, const u32* __restrict__ pay,
                                                       const u32* __restrict__ ycnt, const u32* __restrict__ Gs,
                                                       const double* __restrict__ coefs, const int* __restrict__ on,
                                                       double plain_coef, float* __restrict__ gout, int* __restrict__ order,
                                                       double* __restrict__ partial, u32 L, u32 ntile) {
    __shared__ u32 wsum[4];
    __shared__ double red[4];
    const u32 seg = blockIdx.x / ntile, tile = blockIdx.x % ntile;
    const size_t sbase = (size_t)seg * L;
    const u32 first = tile * LOV_TILE + threadIdx.x * LOV_ROUNDS;
    u32 kk[LOV_ROUNDS], pp[LOV_ROUNDS];
    u32 mine = 0;
#pragma unroll
    for (int j = 0; j < LOV_ROUNDS; ++j) {
        const u32 i = first + j;
        kk[j] = i < L ? keys[sbase + i] : LOV_VOID;
        pp[j] = i < L ? pay[sbase + i] : 0u;
        mine += pp[j] >> 31;
    }
    u32 unused;
    const u32 before = block_excl_scan256(mine, wsum, unused);
    const long long G = (long long)Gs[seg];
    long long F = (long long)ycnt[blockIdx.x] + before;
    const double coef = coefs ? coefs[seg] : plain_coef;
    const bool counts = on ? on[seg] != 0 : true;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < LOV_ROUNDS; ++j) {
        const u32 i = first + j;
        if (i >= L) break;
        const u32 pix = pp[j] & 0x7fffffffu;
        if (kk[j] == LOV_VOID) {   // void pixels rank after every error
            if (gout) gout[sbase + pix] = 0.f;
            if (order) order[sbase + i] = -1;
            continue;
        }
        const bool y = pp[j] >> 31;
        F += y;
        const long long U = G + ((long long)i + 1 - F);
        double dJ;
        if (y)
            dJ = 1.0 / (double)U;
        else if (U - 1 == 0)
            dJ = 1.0;
        else
            dJ = (double)(G - F) / ((double)(U - 1) * (double)U);
        acc += (double)key_error(kk[j]) * dJ;
        if (gout) {
            const double gd = coef * dJ;
            gout[sbase + pix] = counts ? (float)(y ? -gd : gd) : 0.f;
        }
        if (order) order[sbase + i] = (int)pix;
    }
    const double sum = block_sum4(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// grid n: Lc[seg] = the fixed-order sum of its tiles' partials; out (optional): the same as floats
__global__ __launch_bounds__(1024) void lov_segsum_kernel(const double* __restrict__ partial, int ntile, double* __restrict__ Lc,
                                                          float* __restrict__ out) {
    __shared__ double red[1024];
    ce_fixed_order_sum(partial + (size_t)blockIdx.x * ntile, ntile, red);
    if (threadIdx.x == 0) {
        Lc[blockIdx.x] = red[0];
        if (out) out[blockIdx.x] = (float)red[0];
    }
}

// one block: the mean over the classes that count per group, then over the groups; extra = {weight lovasz, lovasz}
__global__ __launch_bounds__(256) void lov_finish_kernel(const double* __restrict__ Lc, const int* __restrict__ on, LovGroups gr,
                                                         double weight, double* __restrict__ gterm, double* __restrict__ extra) {
    for (int q = threadIdx.x; q < gr.groups; q += 256) {
        double m = 0.0;
        int kp = 0;
        for (int k = 0; k < gr.K; ++k) {
            const int s = gr.seg(k, q);
            if (on[s]) {
                m += Lc[s];
                ++kp;
            }
        }
        gterm[q] = kp > 0 ? m / (double)kp : 0.0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int q = 0; q < gr.groups; ++q) t += gterm[q];
        if (gr.per_image) t = t / (double)gr.groups;
        extra[0] = weight * t;
        extra[1] = t;
    }
}

// ---- host ----

inline unsigned blocks256(size_t total) { return (unsigned)((total + 255) / 256); }

bool segments_ok(long long n, long long L) {
    return n >= 1 && n <= LOV_MAX_SEGMENTS && L >= 1 && (unsigned long long)n * (unsigned long long)L < (1ull << 31);
}

struct Layout {
    size_t extra, Gs, on, coef, Lc, gterm, rowtot, hist, ycnt, partial, keys[2], pay[2], gplanes, total;
    u32 ntile;
};
Layout layout(size_t n, size_t L, size_t groups) {
    Layout l;
    l.ntile = (u32)((L + LOV_TILE - 1) / LOV_TILE);
    const size_t tiles = n * l.ntile;
    size_t o = 0;
    l.extra = o;    o += 256;
    l.Gs = o;       o += up256(n * sizeof(u32));
    l.on = o;       o += up256(n * sizeof(int));
    l.coef = o;     o += up256(n * sizeof(double));
    l.Lc = o;       o += up256(n * sizeof(double));
    l.gterm = o;    o += up256(groups * sizeof(double));
    l.rowtot = o;   o += up256(n * 256 * sizeof(u32));
    l.hist = o;     o += up256(tiles * 256 * sizeof(u32));
    l.ycnt = o;     o += up256(tiles * sizeof(u32));
    l.partial = o;  o += up256(tiles * sizeof(double));
    for (int i = 0; i < 2; ++i) {
        l.keys[i] = o;  o += up256(n * L * sizeof(u32));
        l.pay[i] = o;   o += up256(n * L * sizeof(u32));
    }
    l.gplanes = o;  o += up256(n * L * sizeof(float));
    l.total = o;
    return l;
}

struct Buffers {
    char* base;
    Layout l;
    template <typename T>
    T* at(size_t off) const { return (T*)(base + off); }
};

// keys[0] / pay[0] hold the planes: four passes leave them sorted in place
int run_sort(const Buffers& b, size_t n, u32 L, hipStream_t s) {
    const u32 ntile = b.l.ntile;
    const unsigned tiles = (unsigned)(n * ntile);
    u32* hist = b.at<u32>(b.l.hist);
    u32* rowtot = b.at<u32>(b.l.rowtot);
    for (int pass = 0; pass < 4; ++pass) {
        const int in = pass & 1, shift = 8 * pass;
        const u32* ki = b.at<u32>(b.l.keys[in]);
        const u32* pi = b.at<u32>(b.l.pay[in]);
        hipLaunchKernelGGL(lov_hist_kernel, dim3(tiles), dim3(256), 0, s, ki, hist, L, ntile, shift);
        VITSEG_LAUNCH_CHECK("lovasz histogram");
        hipLaunchKernelGGL(lov_rowscan_kernel, dim3((unsigned)(n * 256)), dim3(256), 0, s, hist, rowtot, (int)ntile);
        VITSEG_LAUNCH_CHECK("lovasz row scan");
        hipLaunchKernelGGL(lov_scatter_kernel, dim3(tiles), dim3(256), 0, s, ki, pi, b.at<u32>(b.l.keys[in ^ 1]),
                           b.at<u32>(b.l.pay[in ^ 1]), (const u32*)hist, (const u32*)rowtot, L, ntile, shift);
        VITSEG_LAUNCH_CHECK("lovasz scatter");
    }
    return VITSEG_OK;
}

// the ranks of sorted keys[0] / pay[0]: G, (gr: K', coef,) the rank pass and L_c per segment (seg_out: as floats)
int run_ranks(const Buffers& b, size_t n, u32 L, const LovGroups* gr, double weight, double gscale, float* gout, int* order,
              float* seg_out, hipStream_t s) {
    const u32 ntile = b.l.ntile;
    const unsigned tiles = (unsigned)(n * ntile);
    const u32* keys = b.at<u32>(b.l.keys[0]);
    const u32* pay = b.at<u32>(b.l.pay[0]);
    u32* ycnt = b.at<u32>(b.l.ycnt);
    u32* Gs = b.at<u32>(b.l.Gs);
    double* coef = b.at<double>(b.l.coef);
    int* on = b.at<int>(b.l.on);
    double* partial = b.at<double>(b.l.partial);
    double* Lc = b.at<double>(b.l.Lc);
    hipLaunchKernelGGL(lov_ycount_kernel, dim3(tiles), dim3(256), 0, s, pay, ycnt, L, ntile);
    VITSEG_LAUNCH_CHECK("lovasz y count");
    hipLaunchKernelGGL(lov_yscan_kernel, dim3((unsigned)n), dim3(256), 0, s, ycnt, Gs, (int)ntile);
    VITSEG_LAUNCH_CHECK("lovasz y scan");
    if (gr) {
        hipLaunchKernelGGL(lov_coef_kernel, dim3(1), dim3(256), 0, s, (const u32*)Gs, *gr, weight, gscale, coef, on);
        VITSEG_LAUNCH_CHECK("lovasz coef");
    }
    hipLaunchKernelGGL(lov_rank_kernel, dim3(tiles), dim3(256), 0, s, keys, pay, (const u32*)ycnt, (const u32*)Gs,
                       gr ? (const double*)coef : nullptr, gr ? (const int*)on : nullptr, gscale, gout, order, partial, L, ntile);
    VITSEG_LAUNCH_CHECK("lovasz ranks");
    hipLaunchKernelGGL(lov_segsum_kernel, dim3((unsigned)n), dim3(1024), 0, s, (const double*)partial, (int)ntile, Lc, seg_out);
    VITSEG_LAUNCH_CHECK("lovasz segment sums");
    if (gr) {
        hipLaunchKernelGGL(lov_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)Lc, (const int*)on, *gr, weight,
                           b.at<double>(b.l.gterm), b.at<double>(b.l.extra));
        VITSEG_LAUNCH_CHECK("lovasz finish");
    }
    return VITSEG_OK;
}

}  // namespace

size_t lovasz_scratch_bytes(int B, int K, int S) {
    if (B < 1 || K < 1 || S < 1 || !segments_ok((long long)K * B, (long long)S * S)) return 0;
    // the pooled and the per-image layout differ in their tile counts: the larger of the two serves both
    const size_t a = layout((size_t)K, (size_t)B * S * S, 1).total, b = layout((size_t)K * B, (size_t)S * S, (size_t)B).total;
    return a > b ? a : b;
}

int check_lovasz_options(const vitseg_lovasz_options& c, int B, int C, int S) {
    VITSEG_CHECK_ARG(c.weight >= 0.f && c.weight < INFINITY, VITSEG_EINVAL, "lovasz options: weight %f is negative or not finite",
                     (double)c.weight);   // (a NaN fails both)
    VITSEG_CHECK_ARG(C >= 1 && C <= 255, VITSEG_EINVAL, "lovasz options: %d classes (1..255)", C);
    VITSEG_CHECK_ARG(c.K >= 1 && c.K <= C, VITSEG_EINVAL, "lovasz options: K = %d listed classes (1..%d)", c.K, C);
    VITSEG_CHECK_ARG(c.classes, VITSEG_EINVAL, "lovasz options: classes is null");
    bool seen[256] = {};
    for (int k = 0; k < c.K; ++k) {
        const int cls = c.classes[k];
        VITSEG_CHECK_ARG(cls >= 0 && cls < C, VITSEG_EINVAL, "lovasz options: class %d outside [0, %d)", cls, C);
        VITSEG_CHECK_ARG(!seen[cls], VITSEG_EINVAL, "lovasz options: class %d is listed twice", cls);
        seen[cls] = true;
    }
    VITSEG_CHECK_ARG((c.per_image == 0 || c.per_image == 1) && (c.present_only == 0 || c.present_only == 1), VITSEG_EINVAL,
                     "lovasz options: per_image %d / present_only %d must be 0 or 1", c.per_image, c.present_only);
    VITSEG_CHECK_ARG(B >= 1 && S >= 1 && segments_ok((long long)c.K * B, (long long)S * S), VITSEG_EINVAL,
                     "lovasz options: %d x %d x %d x %d plane pixels (1 .. 2^31 - 1, at most 2^20 segments)", c.K, B, S, S);
    VITSEG_CHECK_ARG(c.scratch && ((uintptr_t)c.scratch & 7) == 0, VITSEG_EINVAL, "lovasz options: scratch is null or not 8-byte aligned");
    VITSEG_CHECK_ARG(c.scratch_bytes >= lovasz_scratch_bytes(B, c.K, S), VITSEG_EINVAL, "lovasz options: scratch %zu < required %zu",
                     c.scratch_bytes, lovasz_scratch_bytes(B, c.K, S));
    return VITSEG_OK;
}

int launch_lovasz_term(const float* Z, const void* target, int target_is_u8, const CeOpt& o, int B, int C, int g, int S,
                       const vitseg_lovasz_options& c, bool want_grad, float gscale, hipStream_t s, CldTerm* out) {
    const int K = c.K;
    const size_t npx = (size_t)B * S * S;
    const size_t n = c.per_image ? (size_t)K * B : (size_t)K, L = c.per_image ? (size_t)S * S : npx;
    const LovGroups gr{K, c.per_image ? B : 1, c.per_image ? B : 1, c.present_only, c.per_image};
    Buffers b{(char*)c.scratch, layout(n, L, (size_t)gr.groups)};
    CldClassList list = {};
    out->map = CldClassMap{};
    for (int k = 0; k < K; ++k) {
        list.cls[k] = (unsigned char)c.classes[k];
        out->map.slot[c.classes[k]] = (unsigned char)(k + 1);
    }
    CeOpt oo = o;
    oo.weight = nullptr;   // the label rule alone
    with_target_type(target, target_is_u8, [&](auto* t) {
        hipLaunchKernelGGL(lov_planes_kernel<target_t<decltype(t)>>, dim3(blocks256(npx)), dim3(256), 0, s, Z, t, oo, list, K,
                           b.at<u32>(b.l.keys[0]), b.at<u32>(b.l.pay[0]), c.prob_planes, B, C, g, S, c.per_image);
    });
    VITSEG_LAUNCH_CHECK("lovasz planes");
    if (int rc = run_sort(b, n, (u32)L, s)) return rc;
    float* gout = nullptr;
    if (want_grad || c.grad_planes) gout = c.grad_planes ? c.grad_planes : b.at<float>(b.l.gplanes);
    if (int rc = run_ranks(b, n, (u32)L, &gr, (double)c.weight, (double)gscale, gout, nullptr, c.class_terms, s)) return rc;
    out->extra = b.at<double>(b.l.extra);
    out->gplanes = want_grad ? gout : nullptr;
    return VITSEG_OK;
}

}  // namespace vitseg

extern "C" {

using namespace vitseg;

int vitseg_lovasz_version(void) { return VITSEG_LOVASZ_VERSION; }

size_t vitseg_lovasz_planes_scratch_bytes(int n, int L) { return segments_ok(n, L) ? layout((size_t)n, (size_t)L, 1).total : 0; }

int vitseg_lovasz_planes(const float* prob, const uint8_t* truth_u8, int n, int L, float grad_scale, void* scratch, float* terms,
                         float* grad_prob, int32_t* order, void* stream) {
    VITSEG_CHECK_ARG(prob && truth_u8 && scratch && terms, VITSEG_EINVAL, "lovasz_planes: null pointer");
    VITSEG_CHECK_ARG(((uintptr_t)scratch & 7) == 0, VITSEG_EINVAL, "lovasz_planes: scratch is not 8-byte aligned");
    VITSEG_CHECK_ARG(segments_ok(n, L), VITSEG_EINVAL, "lovasz_planes: %d segments of %d pixels (n * L in 1 .. 2^31 - 1, n <= 2^20)", n, L);
    VITSEG_CHECK_ARG(grad_scale > -INFINITY && grad_scale < INFINITY, VITSEG_EINVAL, "lovasz_planes: grad_scale %f is not finite",
                     (double)grad_scale);
    hipStream_t s = (hipStream_t)stream;
    const size_t total = (size_t)n * L;
    Buffers b{(char*)scratch, layout((size_t)n, (size_t)L, 1)};
    hipLaunchKernelGGL(lov_planes_given_kernel, dim3(blocks256(total)), dim3(256), 0, s, prob, truth_u8, b.at<u32>(b.l.keys[0]),
                       b.at<u32>(b.l.pay[0]), total, (u32)L);
    VITSEG_LAUNCH_CHECK("lovasz planes");
    if (int rc = run_sort(b, (size_t)n, (u32)L, s)) return rc;
    return run_ranks(b, (size_t)n, (u32)L, nullptr, 1.0, (double)grad_scale, grad_prob, order, terms, s);
}

size_t vitseg_lovasz_scratch_bytes(int batch, int K, int S) { return lovasz_scratch_bytes(batch, K, S); }

int vitseg_ce_lovasz_loss(const float* lowres, const void* target, int target_is_u8, float* grad_logits, void* scratch, float* terms,
                          int batch, int C, int g, int S, const vitseg_ce_options* ce_opts, const vitseg_dice_options* dice_opts,
                          const vitseg_lovasz_options* lovasz, float loss_scale, void* stream) {
    VITSEG_CHECK_ARG(batch >= 1 && C >= 1 && g >= 1 && S >= g, VITSEG_EINVAL, "ce_lovasz_loss: bad shape");
    FusedLoss f;
    f.ce = ce_opts;
    f.dice = dice_opts;
    f.lovasz = lovasz;
    f.terms = terms;
    f.terms4 = true;
    return launch_fused_loss(lowres, target, target_is_u8, grad_logits, (double*)scratch, nullptr, batch, C, g, S, f, (hipStream_t)stream,
                             loss_scale);
}

}  // extern "C"
