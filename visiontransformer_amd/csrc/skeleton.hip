// Skeletons of binary masks by parallel thinning, and the crack statistics that follow from them (clDice, length, width).
// The reference wraps skimage.morphology.skeletonize per image on the host (model/PAED/segmentation.py:89-111
// CrackSeg.skeletonize); the contract here is the algorithm that function cites, as published:
//
//   T. Y. Zhang and C. Y. Suen, "A Fast Parallel Algorithm for Thinning Digital Patterns", CACM 27 (3), 1984.
//
// A non-zero byte is a mask pixel, pixels outside the image are background.  Neighbours of P1 clockwise from north:
// P2 = N, P3 = NE, P4 = E, P5 = SE, P6 = S, P7 = SW, P8 = W, P9 = NW.  B = the number of set neighbours, A = the number of
// 0 -> 1 steps in the cyclic sequence P2, P3, ..., P9, P2.  One pass = sub-iteration 1, then sub-iteration 2; each decides
// for ALL pixels from the state before it, then deletes.  A set pixel is deleted when 2 <= B <= 6 and A = 1 and
//   sub-iteration 1: P2 P4 P6 = 0 and P4 P6 P8 = 0;     sub-iteration 2: P2 P4 P8 = 0 and P2 P6 P8 = 0.
// The loop stops after the first pass in which neither sub-iteration deleted a pixel; `passes` counts that pass too.
// The algorithm's known quirks belong to the contract: an isolated 2 x 2 square vanishes, and a full rectangle thins to a
// short segment or a single pixel (a 3 x 36 bar: a 33-pixel line in 2 passes; an 80 x 80 square: 1 pixel in 41 passes).
//
// Planes are packed one bit per pixel: bit i of word j of a row is pixel x = 32 j + i, rows padded to whole words, the
// padding bits 0 (thinning only clears bits, so they stay 0 and never act as neighbours).  thin_word() is one sub-iteration
// of a 32-pixel word from its 3 x 3 surrounding words: the eight neighbour planes are shifts, B a bit-sliced adder over them,
// "A = 1" the planes ~n_i & n_(i+1) folded as "at least one and not at least two": about 70 bitwise operations for 32
// pixels, no per-pixel loop, no table.  A word that is 0 stays 0 and is skipped.
//
// Resident route (one block of 1024 threads per plane; no host synchronisation).  The packed plane lives in LDS with a
// border of zero words: H + 2 rows of stride Ww + 1 words (the word right of a row's last is the word left of the next row's
// first), so a word's neighbours are idx -+ 1, idx -+ stride without a bounds test.  The block packs its plane from HBM with
// wave ballots, loops the passes and unpacks the result.  A sub-iteration must read the whole old state before any word is
// overwritten: each thread keeps the new values of its words (idx = first + k * 1024 + t, k < 40) in registers across a
// barrier and then stores the changed ones; no second LDS buffer, so a 1024 x 1024 plane (135 KB) fits.  "Deleted something"
// is a block-wide OR through one of two alternating LDS flags; every block stops at its own plane's convergence.  The route
// is taken while 4 ((H + 2) (Ww + 1) + 4) bytes fit min(the device's shared memory per block, 160 KiB) -- 40 words per
// thread are what the registers are sized for.
//
// Global route (planes too large for LDS; this route SYNCHRONISES `stream`).  Two packed buffers per plane in the scratch;
// one launch per sub-iteration covers all planes, reading one buffer and writing the other; a one-block launch per pass
// counts the pass, marks the planes that deleted nothing as done and counts the rest.  Done planes are skipped: their last
// pass changed nothing, so both buffers hold the result.  The host reads the count of unfinished planes every 16 passes and
// stops at 0.  No cooperative launch, no grid-wide barrier.
//
// Statistics (vitseg_skeleton_stats), per class c, over the 2 n planes {gt == c} (plane 2 i) and {pred == c} (2 i + 1):
// thin them by either route into byte planes; write the complements and count the sets; launch_sdf_d2 on the complements
// gives d2 = the exact squared distance of every class pixel to the nearest pixel outside the class (vitseg_sdf's "int"
// field before the float conversion, with its virtual feature at (-1, 0) for a plane that is all class); one reduction over
// the skeleton pixels (plane_reduce.hpp, shared with distance.hip) adds sqrt((double) d2) in an order fixed by H * W and
// folds the integers with atomics; a last block per image writes the rows.  The resident route occupies 2 n CUs per class.
#include "kernels.hpp"
#include "plane_reduce.hpp"

namespace vitseg {
namespace {

constexpr int SKEL_MAX_SIDE = 16384, SKEL_MAX_BATCH = 32767;
constexpr int RES_THREADS = 1024, RES_KMAX = 40;      // resident route: words per thread held in registers
constexpr int RES_LDS_CAP = 160 * 1024;               // = 4 * RES_THREADS * RES_KMAX
constexpr int FLAG_PASSES = 16;                       // global route: passes between two reads of the unfinished count
constexpr int NCOUNT = 8;                             // statistics: counter words per plane

// the planes of a call: plane j of `planes` is a[j * P] tested != 0 (cls < 0), or for the statistics (b != NULL) image j / 2
// of a (j even, the ground truth) or b (j odd, the prediction) tested == cls
struct Planes {
    const unsigned char* a;
    const unsigned char* b;
    int cls;
    __device__ __forceinline__ const unsigned char* plane(int j, size_t P) const {
        if (!b) return a + (size_t)j * P;
        return ((j & 1) ? b : a) + (size_t)(j >> 1) * P;
    }
    __device__ __forceinline__ bool set(unsigned char v) const { return cls < 0 ? v != 0 : v == cls; }
};

// One sub-iteration (sub 0 / 1) of the 32 pixels of word c.  u*, m*, d*: the rows above, of and below the word; *l, *r the
// words left and right of it (only bit 31 of a left word and bit 0 of a right word matter).  Returns the word after deletion.
__device__ __forceinline__ unsigned thin_word(unsigned ul, unsigned uc, unsigned ur, unsigned ml, unsigned c, unsigned mr,
                                              unsigned dl, unsigned dc, unsigned dr, int sub) {
    const unsigned p2 = uc, p6 = dc;
    const unsigned p4 = (c >> 1) | (mr << 31), p8 = (c << 1) | (ml >> 31);
    const unsigned p3 = (uc >> 1) | (ur << 31), p9 = (uc << 1) | (ul >> 31);
    const unsigned p5 = (dc >> 1) | (dr << 31), p7 = (dc << 1) | (dl >> 31);
    // B = p2 + ... + p9 per bit: carry-save adders to the bits b0 (ones) .. b3 (eights)
    const unsigned s1 = p2 ^ p3 ^ p4, c1 = (p2 & p3) | (p4 & (p2 ^ p3));
    const unsigned s2 = p5 ^ p6 ^ p7, c2 = (p5 & p6) | (p7 & (p5 ^ p6));
    const unsigned s3 = p8 ^ p9, c3 = p8 & p9;
    const unsigned b0 = s1 ^ s2 ^ s3, c4 = (s1 & s2) | (s3 & (s1 ^ s2));
    const unsigned t1 = c1 ^ c2 ^ c3, d1 = (c1 & c2) | (c3 & (c1 ^ c2));
    const unsigned b1 = t1 ^ c4, d2 = t1 & c4;
    const unsigned b2 = d1 ^ d2, b3 = d1 & d2;
    const unsigned b_ok = (b1 | b2) & ~b3 & ~(b0 & b1 & b2);   // 2 <= B <= 6: not 0, 1, 7 (b0 b1 b2) or 8 (b3)
    // A = 1: exactly one of the eight 0 -> 1 steps
    unsigned one = ~p2 & p3, two = 0, t;
    t = ~p3 & p4; two |= one & t; one |= t;
    t = ~p4 & p5; two |= one & t; one |= t;
    t = ~p5 & p6; two |= one & t; one |= t;
    t = ~p6 & p7; two |= one & t; one |= t;
    t = ~p7 & p8; two |= one & t; one |= t;
    t = ~p8 & p9; two |= one & t; one |= t;
    t = ~p9 & p2; two |= one & t; one |= t;
    const unsigned a_ok = one & ~two;
    const unsigned cond = sub == 0 ? ~(p2 & p4 & p6) & ~(p4 & p6 & p8) : ~(p2 & p4 & p8) & ~(p2 & p6 & p8);
    return c & ~(b_ok & a_ok & cond);
}

// ---- resident route: grid (planes), RES_THREADS threads, dynamic LDS = res_lds_bytes(H, W) ----
__global__ __launch_bounds__(RES_THREADS) void skel_resident_kernel(Planes in, int H, int W,
                                                                    unsigned char* __restrict__ out,
                                                                    int* __restrict__ passes) {
    extern __shared__ __attribute__((aligned(16))) unsigned res_lds[];
    unsigned* flag = res_lds;        // [0], [1]: "deleted something" of the even / odd passes
    unsigned* L = res_lds + 2;       // (H + 2) rows of `stride` words, one word more for the last row's right border
    const int t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
    const int Ww = (W + 31) >> 5, stride = Ww + 1, total = (H + 2) * stride + 1;
    const size_t P = (size_t)H * W;
    const unsigned char* src = in.plane(blockIdx.x, P);
    for (int i = t; i < total; i += RES_THREADS) L[i] = 0;
    if (t < 2) flag[t] = 0;
    __syncthreads();
    // pack: a wave per row, 64 pixels per ballot = words 2 c and 2 c + 1 of the row
    const int C64 = (W + 63) >> 6;
    for (int y = wave; y < H; y += RES_THREADS / WAVE) {
        const unsigned char* row = src + (size_t)y * W;
        unsigned* lrow = L + (y + 1) * stride + 1;
        for (int c = 0; c < C64; ++c) {
            const int x = c * 64 + lane;
            const unsigned long long b = __ballot(x < W && in.set(row[x]));
            if (lane == 0) {
                lrow[2 * c] = (unsigned)b;
                if (2 * c + 1 < Ww) lrow[2 * c + 1] = (unsigned)(b >> 32);
            }
        }
    }
    __syncthreads();
    const int first = stride + 1, end = (H + 1) * stride;   // the words of rows 1 .. H; a border word among them is 0 and stays 0
    unsigned nw[RES_KMAX];
    int pass = 0;
    for (;;) {
        bool deleted = false;
        for (int sub = 0; sub < 2; ++sub) {
            unsigned long long chg = 0;
            int i0 = first + t;
            asm volatile("" : "+v"(i0));   // the 40 x 3 word addresses are recomputed here, not kept in registers across passes
#pragma unroll
            for (int k = 0; k < RES_KMAX; ++k) {
                const int i = i0 + k * RES_THREADS;
                const unsigned c = i < end ? L[i] : 0u;
                if (c != 0) {   // (each k a branch of its own: a break would nest 40 saved exec masks)
                    const unsigned* u = L + i - stride;
                    const unsigned* d = L + i + stride;
                    const unsigned v = thin_word(u[-1], u[0], u[1], L[i - 1], c, L[i + 1], d[-1], d[0], d[1], sub);
                    nw[k] = v;
                    if (v != c) chg |= 1ull << k;
                }
                __builtin_amdgcn_sched_barrier(0);   // one word at a time: hoisting the reads of all 40 would spill
            }
            __syncthreads();   // every word of the old state has been read
            if (chg) {
                deleted = true;
#pragma unroll
                for (int k = 0; k < RES_KMAX; ++k)
                    if ((chg >> k) & 1) L[first + k * RES_THREADS + t] = nw[k];
            }
            if (sub == 1) {
                if (deleted) flag[pass & 1] = 1;
                if (t == 0) flag[(pass + 1) & 1] = 0;   // last read before the barriers of this pass
            }
            __syncthreads();
        }
        const unsigned any = flag[pass & 1];
        ++pass;
        if (!any) break;
    }
    if (passes && t == 0) passes[blockIdx.x] = pass;
    unsigned char* o = out + (size_t)blockIdx.x * P;
    for (int y = wave; y < H; y += RES_THREADS / WAVE) {
        const unsigned* lrow = L + (y + 1) * stride + 1;
        for (int x = lane; x < W; x += WAVE) o[(size_t)y * W + x] = (unsigned char)((lrow[x >> 5] >> (x & 31)) & 1u);
    }
}

// ---- global route ----
struct PlaneState {
    int deleted, done, passes, pad;
};

// grid (ceil(H * C64 / 4), planes), 256 threads: a wave per 64 pixels of a row
__global__ __launch_bounds__(256) void skel_pack_kernel(Planes in, int H, int W, unsigned* __restrict__ buf) {
    const int lane = threadIdx.x & (WAVE - 1), C64 = (W + 63) >> 6, Ww = (W + 31) >> 5;
    const int item = blockIdx.x * 4 + threadIdx.x / WAVE;
    if (item >= H * C64) return;
    const int y = item / C64, c = item - y * C64, x = c * 64 + lane;
    const size_t P = (size_t)H * W;
    const unsigned char* row = in.plane(blockIdx.y, P) + (size_t)y * W;
    const unsigned long long b = __ballot(x < W && in.set(row[x]));
    if (lane == 0) {
        unsigned* o = buf + ((size_t)blockIdx.y * H + y) * Ww;
        o[2 * c] = (unsigned)b;
        if (2 * c + 1 < Ww) o[2 * c + 1] = (unsigned)(b >> 32);
    }
}

// grid (ceil(H * Ww / 256), planes): one sub-iteration src -> dst of every plane that is not done
__global__ __launch_bounds__(256) void skel_step_kernel(const unsigned* __restrict__ src, unsigned* __restrict__ dst,
                                                        PlaneState* __restrict__ state, int H, int Ww, int sub) {
    const int j = blockIdx.y;
    if (state[j].done) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * Ww) return;
    const int y = i / Ww, w = i - y * Ww;
    const unsigned* m = src + (size_t)j * H * Ww + i;
    const unsigned c = m[0];
    unsigned v = 0;
    if (c) {
        const bool up = y > 0, dn = y < H - 1, lf = w > 0, rt = w < Ww - 1;
        const unsigned* u = m - Ww;
        const unsigned* d = m + Ww;
        v = thin_word(up && lf ? u[-1] : 0u, up ? u[0] : 0u, up && rt ? u[1] : 0u, lf ? m[-1] : 0u, c, rt ? m[1] : 0u,
                      dn && lf ? d[-1] : 0u, dn ? d[0] : 0u, dn && rt ? d[1] : 0u, sub);
        if (v != c) atomicOr(&state[j].deleted, 1);
    }
    dst[(size_t)j * H * Ww + i] = v;
}

// one block: end of a pass.  Every plane still running counts the pass; one that deleted nothing is done.
__global__ __launch_bounds__(256) void skel_pass_end_kernel(PlaneState* __restrict__ state, int planes,
                                                            int* __restrict__ remaining) {
    __shared__ int left;
    if (threadIdx.x == 0) left = 0;
    __syncthreads();
    int mine = 0;
    for (int j = threadIdx.x; j < planes; j += 256) {
        PlaneState st = state[j];
        if (st.done) continue;
        st.passes += 1;
        if (st.deleted) ++mine;
        else st.done = 1;
        st.deleted = 0;
        state[j] = st;
    }
    if (mine) atomicAdd(&left, mine);
    __syncthreads();
    if (threadIdx.x == 0) *remaining = left;
}

// grid (ceil(P / 1024), planes): bits -> bytes; block (0, j) also writes the plane's pass count
__global__ __launch_bounds__(256) void skel_unpack_kernel(const unsigned* __restrict__ buf,
                                                          const PlaneState* __restrict__ state, int H, int W,
                                                          unsigned char* __restrict__ out, int* __restrict__ passes) {
    const int Ww = (W + 31) >> 5, j = blockIdx.y;
    const size_t P = (size_t)H * W;
    const unsigned* b = buf + (size_t)j * H * Ww;
    if (passes && blockIdx.x == 0 && threadIdx.x == 0) passes[j] = state[j].passes;
    for (int k = 0; k < 4; ++k) {
        const size_t p = (size_t)blockIdx.x * 1024 + k * 256 + threadIdx.x;
        if (p >= P) return;
        const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
        out[(size_t)j * P + p] = (unsigned char)((b[(size_t)y * Ww + (x >> 5)] >> (x & 31)) & 1u);
    }
}

bool shape_ok(int n, int H, int W) {
    return n >= 1 && n <= SKEL_MAX_BATCH && H >= 1 && H <= SKEL_MAX_SIDE && W >= 1 && W <= SKEL_MAX_SIDE;
}

size_t res_lds_bytes(int H, int W) { return 4 * ((size_t)(H + 2) * (((W + 31) >> 5) + 1) + 4); }

// min(the device's shared memory per block, what the kernel's registers are sized for); 0 when no device answers
int res_lds_limit() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    static int limit[64] = {};
    if (!limit[dev]) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || v <= 0) return 0;
        limit[dev] = v < RES_LDS_CAP ? v : RES_LDS_CAP;
    }
    return limit[dev];
}

// 1 resident, 2 global, 0: route 1 was asked for a plane that does not fit
int pick_route(int H, int W, int route) {
    const bool fits = res_lds_bytes(H, W) <= (size_t)res_lds_limit();
    if (route == 2) return 2;
    if (route == 1) return fits ? 1 : 0;
    return fits ? 1 : 2;
}

struct ThinLayout {
    size_t bufA, bufB, state, remaining, total;
};

ThinLayout thin_layout(int planes, int H, int W, int r) {
    ThinLayout l{};
    if (r == 1) {
        l.total = 256;   // the resident route keeps everything in LDS; a size of 0 means a bad shape
        return l;
    }
    const size_t words = (size_t)H * ((W + 31) >> 5);
    size_t o = 0;
    l.bufA = o;       o += up256((size_t)planes * words * 4);
    l.bufB = o;       o += up256((size_t)planes * words * 4);
    l.state = o;      o += up256((size_t)planes * sizeof(PlaneState));
    l.remaining = o;  o += 256;
    l.total = o;
    return l;
}

// thins `planes` planes into byte planes `out` by route r (1 or 2, from pick_route); scratch as thin_layout
int thin(const Planes& in, int planes, int H, int W, int r, unsigned char* out, int* passes, char* scratch, hipStream_t s) {
    if (r == 1) {
        const size_t lds = res_lds_bytes(H, W);
        int dev = 0;
        static int attr_set[64] = {};   // the attribute is per device: the largest size requested so far
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
        if (lds > 65536 && (int)lds > attr_set[dev]) {
            const hipError_t e = hipFuncSetAttribute((const void*)skel_resident_kernel,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, res_lds_limit());
            if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(skeleton resident)");
            attr_set[dev] = res_lds_limit();
        }
        hipLaunchKernelGGL(skel_resident_kernel, dim3(planes), dim3(RES_THREADS), lds, s, in, H, W, out, passes);
        VITSEG_LAUNCH_CHECK("skeleton resident");
        return VITSEG_OK;
    }
    const ThinLayout l = thin_layout(planes, H, W, 2);
    unsigned* A = (unsigned*)(scratch + l.bufA);
    unsigned* B = (unsigned*)(scratch + l.bufB);
    PlaneState* state = (PlaneState*)(scratch + l.state);
    int* remaining = (int*)(scratch + l.remaining);
    const int Ww = (W + 31) >> 5, C64 = (W + 63) >> 6, words = H * Ww;
    hipError_t e = hipMemsetAsync(state, 0, (size_t)planes * sizeof(PlaneState), s);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(skeleton state)");
    hipLaunchKernelGGL(skel_pack_kernel, dim3((H * C64 + 3) / 4, planes), dim3(256), 0, s, in, H, W, A);
    VITSEG_LAUNCH_CHECK("skeleton pack");
    const dim3 grid((words + 255) / 256, planes);
    for (;;) {   // ends: a pass that deletes nothing ends its plane, and a plane has finitely many pixels to delete
        for (int p = 0; p < FLAG_PASSES; ++p) {
            hipLaunchKernelGGL(skel_step_kernel, grid, dim3(256), 0, s, A, B, state, H, Ww, 0);
            hipLaunchKernelGGL(skel_step_kernel, grid, dim3(256), 0, s, B, A, state, H, Ww, 1);
            hipLaunchKernelGGL(skel_pass_end_kernel, dim3(1), dim3(256), 0, s, state, planes, remaining);
            VITSEG_LAUNCH_CHECK("skeleton pass");
        }
        int left = -1;
        e = hipMemcpyAsync(&left, remaining, sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(e, "skeleton: reading the unfinished count");
        if (left == 0) break;
    }
    hipLaunchKernelGGL(skel_unpack_kernel, dim3((unsigned)(((size_t)H * W + 1023) / 1024), planes), dim3(256), 0, s, A, state,
                       H, W, out, passes);
    VITSEG_LAUNCH_CHECK("skeleton unpack");
    return VITSEG_OK;
}

// ---- statistics ----
enum { C_SET = 0, C_SKEL, C_CROSS, C_ENDS, C_MAXD2 };   // counter words of a plane

// grid (ceil(P / 1024), n): the complements {gt != c} (plane 2 i) and {pred != c} (2 i + 1) as bytes, and |G|, |P|
__global__ __launch_bounds__(256) void skel_planes_kernel(const unsigned char* __restrict__ pred,
                                                          const unsigned char* __restrict__ gt,
                                                          unsigned char* __restrict__ comp, int* __restrict__ counts, int P,
                                                          int c) {
    const int i = blockIdx.y;
    const unsigned char* g = gt + (size_t)i * P;
    const unsigned char* p = pred + (size_t)i * P;
    unsigned char* cg = comp + (size_t)(2 * i) * P;
    unsigned char* cp = cg + P;
    int ng = 0, np = 0;
    for (int k = 0; k < 4; ++k) {
        const int idx = blockIdx.x * 1024 + k * 256 + threadIdx.x;
        if (idx >= P) break;
        const bool a = g[idx] == c, b = p[idx] == c;
        cg[idx] = !a;
        cp[idx] = !b;
        ng += a;
        np += b;
    }
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        ng += __shfl_xor(ng, d);
        np += __shfl_xor(np, d);
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        if (ng) atomicAdd(&counts[(2 * i) * NCOUNT + C_SET], ng);
        if (np) atomicAdd(&counts[(2 * i + 1) * NCOUNT + C_SET], np);
    }
}

// grid (NB, 2 n): over the skeleton pixels of plane j in the chunk: the fp64 partial sum of sqrt(d2) and the integers
__global__ __launch_bounds__(256) void skel_reduce_kernel(const unsigned char* __restrict__ skel, const int* __restrict__ d2,
                                                          const unsigned char* __restrict__ pred,
                                                          const unsigned char* __restrict__ gt, int* __restrict__ counts,
                                                          double* __restrict__ psum, int H, int W, int c) {
    __shared__ double shd[4];
    __shared__ int shi[4];
    const int j = blockIdx.y, P = H * W;
    const unsigned char* sk = skel + (size_t)j * P;
    const int* fld = d2 + (size_t)j * P;
    const unsigned char* other = ((j & 1) ? gt : pred) + (size_t)(j >> 1) * P;   // S_G is met with P, S_P with G
    double s = 0.0;
    int mx = 0, cnt = 0, cross = 0, ends = 0;
    for_source_pixels(sk, P, (P & 3) == 0, [&](int idx) {
        const int v = fld[idx];
        s += sqrt((double)v);
        mx = max(mx, v);
        ++cnt;
        cross += other[idx] == c;
        const int y = idx / W, x = idx - y * W;
        int nb = 0;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx)
                if ((dy || dx) && y + dy >= 0 && y + dy < H && x + dx >= 0 && x + dx < W) nb += sk[idx + dy * W + dx] != 0;
        ends += nb == 1;
    });
    s = block_sum(s, shd);
    mx = block_max(mx, shi);
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        cnt += __shfl_xor(cnt, d);
        cross += __shfl_xor(cross, d);
        ends += __shfl_xor(ends, d);
    }
    int* cj = counts + j * NCOUNT;
    if ((threadIdx.x & (WAVE - 1)) == 0 && cnt) {
        atomicAdd(&cj[C_SKEL], cnt);
        if (cross) atomicAdd(&cj[C_CROSS], cross);
        if (ends) atomicAdd(&cj[C_ENDS], ends);
    }
    if (threadIdx.x == 0) {
        psum[(size_t)j * gridDim.x + blockIdx.x] = s;
        if (mx) atomicMax(&cj[C_MAXD2], mx);
    }
}

// grid (n): the partial sums of planes 2 i, 2 i + 1 in a fixed order, and the rows of image i and class slot k
__global__ __launch_bounds__(256) void skel_finish_kernel(const double* __restrict__ psum, const int* __restrict__ counts,
                                                          long long* __restrict__ stats_i, double* __restrict__ stats_f,
                                                          int NB, int K, int k) {
    __shared__ double shd[4];
    const int i = blockIdx.x;
    double sum[2];
    for (int side = 0; side < 2; ++side) {
        const size_t base = (size_t)(2 * i + side) * NB;
        double s = 0.0;
        for (int b = threadIdx.x; b < NB; b += 256) s += psum[base + b];
        sum[side] = block_sum(s, shd);
    }
    if (threadIdx.x != 0) return;
    const int* g = counts + (2 * i) * NCOUNT;
    const int* p = g + NCOUNT;
    long long* o = stats_i + ((size_t)i * K + k) * 10;
    o[0] = g[C_SET];
    o[1] = p[C_SET];
    o[2] = g[C_SKEL];
    o[3] = p[C_SKEL];
    o[4] = g[C_CROSS];
    o[5] = p[C_CROSS];
    o[6] = g[C_SKEL] ? g[C_MAXD2] : -1;
    o[7] = p[C_SKEL] ? p[C_MAXD2] : -1;
    o[8] = g[C_ENDS];
    o[9] = p[C_ENDS];
    stats_f[((size_t)i * K + k) * 2 + 0] = sum[0];
    stats_f[((size_t)i * K + k) * 2 + 1] = sum[1];
}

struct StatsLayout {
    size_t d2, comp, skel, psum, counts, thin, total;
    int NB;
};

StatsLayout stats_layout(int n, int H, int W, int r) {
    StatsLayout l;
    const size_t P = (size_t)H * W, M = 2 * (size_t)n;
    l.NB = (int)((P + PLANE_CHUNK - 1) / PLANE_CHUNK);
    size_t o = 0;
    l.d2 = o;      o += up256(M * P * sizeof(int));
    l.comp = o;    o += up256(M * P);
    l.skel = o;    o += up256(M * P);
    l.psum = o;    o += up256(M * l.NB * sizeof(double));
    l.counts = o;  o += up256(M * (NCOUNT + 2) * sizeof(int));   // the counters [2 n][NCOUNT], then sdf.hip's maxima [4 n]
    l.thin = o;    o += thin_layout((int)M, H, W, r).total;
    l.total = o;
    return l;
}

bool route_ok(int route) { return route >= 0 && route <= 2; }

}  // namespace

size_t skeleton_scratch_bytes(int n, int H, int W, int route) {
    if (!shape_ok(n, H, W) || !route_ok(route)) return 0;
    const int r = pick_route(H, W, route);
    return r ? thin_layout(n, H, W, r).total : 0;
}

int launch_skeleton(const unsigned char* mask, int n, int H, int W, int route, unsigned char* skeleton, int* passes,
                    void* scratch, size_t scratch_bytes, hipStream_t s) {
    VITSEG_CHECK_ARG(mask && skeleton && scratch, VITSEG_EINVAL, "skeleton: null pointer");
    VITSEG_CHECK_ARG(route_ok(route), VITSEG_EINVAL, "skeleton: route must be 0 (automatic), 1 (resident) or 2 (global), got %d",
                     route);
    VITSEG_CHECK_ARG(shape_ok(n, H, W), VITSEG_ESHAPE, "skeleton: bad shape n=%d H=%d W=%d (1 <= H, W <= %d, 1 <= n <= %d)", n,
                     H, W, SKEL_MAX_SIDE, SKEL_MAX_BATCH);
    const int r = pick_route(H, W, route);
    VITSEG_CHECK_ARG(r != 0, VITSEG_ESHAPE, "skeleton: a %d x %d plane needs %zu bytes of LDS, the resident route has %d", H, W,
                     res_lds_bytes(H, W), res_lds_limit());
    const size_t need = thin_layout(n, H, W, r).total;
    VITSEG_CHECK_ARG(scratch_bytes >= need, VITSEG_EWORKSPACE, "skeleton: scratch of %zu bytes, %zu needed", scratch_bytes, need);
    return thin(Planes{mask, nullptr, -1}, n, H, W, r, skeleton, passes, (char*)scratch, s);
}

size_t skeleton_stats_scratch_bytes(int n, int H, int W, int route) {
    if (!shape_ok(n, H, W) || !route_ok(route)) return 0;
    const int r = pick_route(H, W, route);
    return r ? stats_layout(n, H, W, r).total : 0;
}

int launch_skeleton_stats(const unsigned char* pred, const unsigned char* gt, int n, int H, int W, const int* classes, int K,
                          int route, long long* stats_i, double* stats_f, void* scratch, size_t scratch_bytes, hipStream_t s) {
    VITSEG_CHECK_ARG(pred && gt && classes && stats_i && stats_f && scratch, VITSEG_EINVAL, "skeleton stats: null pointer");
    VITSEG_CHECK_ARG(route_ok(route), VITSEG_EINVAL,
                     "skeleton stats: route must be 0 (automatic), 1 (resident) or 2 (global), got %d", route);
    VITSEG_CHECK_ARG(shape_ok(n, H, W) && K >= 1 && K <= 256, VITSEG_ESHAPE,
                     "skeleton stats: bad shape n=%d H=%d W=%d K=%d (1 <= H, W <= %d, 1 <= n <= %d, 1 <= K <= 256)", n, H, W, K,
                     SKEL_MAX_SIDE, SKEL_MAX_BATCH);
    for (int k = 0; k < K; ++k)
        VITSEG_CHECK_ARG(classes[k] >= 0 && classes[k] <= 255, VITSEG_EINVAL, "skeleton stats: class value %d outside 0..255",
                         classes[k]);
    const int r = pick_route(H, W, route);
    VITSEG_CHECK_ARG(r != 0, VITSEG_ESHAPE, "skeleton stats: a %d x %d plane needs %zu bytes of LDS, the resident route has %d",
                     H, W, res_lds_bytes(H, W), res_lds_limit());
    const StatsLayout l = stats_layout(n, H, W, r);
    VITSEG_CHECK_ARG(scratch_bytes >= l.total, VITSEG_EWORKSPACE, "skeleton stats: scratch of %zu bytes, %zu needed",
                     scratch_bytes, l.total);
    char* base = (char*)scratch;
    int* d2 = (int*)(base + l.d2);
    unsigned char* comp = (unsigned char*)(base + l.comp);
    unsigned char* skel = (unsigned char*)(base + l.skel);
    double* psum = (double*)(base + l.psum);
    int* counts = (int*)(base + l.counts);
    const int P = H * W, M = 2 * n;
    int* maxw = counts + M * NCOUNT;
    for (int k = 0; k < K; ++k) {
        const int c = classes[k];
        const hipError_t e = hipMemsetAsync(counts, 0, (size_t)M * (NCOUNT + 2) * sizeof(int), s);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(skeleton counts)");
        int rc = thin(Planes{gt, pred, c}, M, H, W, r, skel, nullptr, base + l.thin, s);
        if (rc != VITSEG_OK) return rc;
        hipLaunchKernelGGL(skel_planes_kernel, dim3((P + 1023) / 1024, n), dim3(256), 0, s, pred, gt, comp, counts, P, c);
        VITSEG_LAUNCH_CHECK("skeleton planes");
        rc = launch_sdf_d2(comp, M, H, W, d2, maxw, s);
        if (rc != VITSEG_OK) return rc;
        hipLaunchKernelGGL(skel_reduce_kernel, dim3(l.NB, M), dim3(256), 0, s, skel, d2, pred, gt, counts, psum, H, W, c);
        VITSEG_LAUNCH_CHECK("skeleton reduce");
        hipLaunchKernelGGL(skel_finish_kernel, dim3(n), dim3(256), 0, s, psum, counts, stats_i, stats_f, l.NB, K, k);
        VITSEG_LAUNCH_CHECK("skeleton finish");
    }
    return VITSEG_OK;
}

}  // namespace vitseg

extern "C" {

size_t vitseg_skeleton_scratch_bytes(int n, int H, int W, int route) { return vitseg::skeleton_scratch_bytes(n, H, W, route); }

int vitseg_skeleton(const uint8_t* mask, int n, int H, int W, int route, uint8_t* skeleton, int32_t* passes, void* scratch,
                    size_t scratch_bytes, void* stream) {
    return vitseg::launch_skeleton(mask, n, H, W, route, skeleton, passes, scratch, scratch_bytes, (hipStream_t)stream);
}

size_t vitseg_skeleton_stats_scratch_bytes(int n, int H, int W, int route) {
    return vitseg::skeleton_stats_scratch_bytes(n, H, W, route);
}

int vitseg_skeleton_stats(const uint8_t* pred, const uint8_t* gt, int n, int H, int W, const int32_t* classes, int K,
                          int route, int64_t* stats_i, double* stats_f, void* scratch, size_t scratch_bytes, void* stream) {
    return vitseg::launch_skeleton_stats(pred, gt, n, H, W, classes, K, route, (long long*)stats_i, stats_f, scratch,
                                         scratch_bytes, (hipStream_t)stream);
}

}  // extern "C"
