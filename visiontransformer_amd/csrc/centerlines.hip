// Crack centre-lines as a graph (vitseg_centerlines, include/vitseg_centerlines.h): the pixel graph of a skeleton traced into
// nodes, branches and ordered polylines, in integers.  The contract -- the link rule, nodes, branches, closed curves, the
// canonical direction and the numbering -- is stated in the header.
//
// Nothing here thins or measures distances: the skeleton comes from launch_skeleton, d2 from launch_sdf_d2.  The unit of work
// is the half-link (pixel p, direction d to a linked pixel q).  Directions are numbered in the raster order of their targets,
// NW N NE W E SW S SE = 0..7 (the opposite of d is 7 - d), so a half-link's key 8 p + d orders by (raster index of p, raster
// index of q): the order the contract numbers branches by.  The successor of (p -> q) is (q -> r), r the other link of q,
// when q has degree 2; otherwise the half-link is terminal and is its own successor.  A walk from a node therefore ends at
// its first terminal half-link, and a curve without a node is two cycles, one per direction.
//   planes       per pixel: X = {mask selected} and its complement as bytes
//   (skeleton)   thin = 1: launch_skeleton on X; thin = 0: S = X
//   (d2)         launch_sdf_d2 on the complement
//   count        per pixel: its link mask (one byte, from the 3 x 3 pixels of S round it); half-links and nodes per chunk of
//                1024 pixels
//   (scan)       chunk scan of chains.hip, one workgroup per image and field: exclusive scan of the chunk totals; the
//                half-link and node counts
//   build        per pixel: the index of its first half-link, every half-link's key (so half-links are numbered in key order)
//                and the node rows
//   link         per half-link: its successor and its word: its own index, bit 31 set unless it is terminal
//   (jump x R)   chain jumps of chains.hip, R = ceil(log2(4 H W)) rounds: after round j a half-link knows the smallest word among
//                the 2^(j+1) from itself on and the hops to it.  A terminal's word is below every other's on its walk, so a walk
//                ends with (terminal, hops to it) and a cycle with (its smallest half-link, hops to it).  A round that
//                changed nothing leaves a zero in its word of `changed`; the rounds after it return at once (the host never
//                reads that word)
//   leaders      per half-link chunk: the number of leaders and of their branches' points.  With rev(p -> q) = (q -> p), the
//                walk through h starts at rev(terminal(rev(h))); a half-link leaving a node leads its branch when it is
//                below the start of the walk from the other end, rev(terminal(h)); a cycle's smallest half-link leads a closed
//                branch when it is the first half-link of its pixel (the other direction's smallest leaves the same pixel)
//   (scan)       exclusive scan of both over the chunks: branch numbers and point offsets in key order
//   place        per leader: the branch row's first five fields and, in `info`, what its half-links need
//   emit         per half-link of a canonical walk: its head pixel to offset + rank + 1 (the leader also its tail to offset);
//                of a canonical cycle: its tail pixel to offset + rank.  The link's kind, the points' q16 widths and d2
//                go to the branch row with integer atomics, the lanes of a wave that share a row adding once
// Every value is an integer; the only atomics are those sums and maxima (order-independent) and the `changed` flags.
#include "chains.hpp"
#include "kernels.hpp"
#include "../../include/vitseg_centerlines.h"

namespace vitseg {
namespace {

constexpr int CL_MAX_SIDE = 16384, CL_MAX_BATCH = 32767;
constexpr u32 LIVE = 0x80000000u;   // in a half-link's word: it is not terminal

__device__ __forceinline__ int dir_dy(int d) { return (d + (d >= 4)) / 3 - 1; }
__device__ __forceinline__ int dir_dx(int d) { return (d + (d >= 4)) % 3 - 1; }
__device__ __forceinline__ bool dir_diagonal(int d) { return (0xA5 >> d) & 1; }   // NW, NE, SW, SE

// bit d: pixel (y, x) of S is linked to its neighbour in direction d; 0 for a pixel outside S
__device__ __forceinline__ int link_mask(const unsigned char* __restrict__ sk, int y, int x, int H, int W) {
    auto at = [&](int yy, int xx) { return yy >= 0 && yy < H && xx >= 0 && xx < W && sk[yy * W + xx] != 0; };
    if (!at(y, x)) return 0;
    const bool n = at(y - 1, x), w = at(y, x - 1), e = at(y, x + 1), s = at(y + 1, x);
    int m = (n << 1) | (w << 3) | (e << 4) | (s << 6);
    if (!n && !w && at(y - 1, x - 1)) m |= 1;
    if (!n && !e && at(y - 1, x + 1)) m |= 4;
    if (!s && !w && at(y + 1, x - 1)) m |= 32;
    if (!s && !e && at(y + 1, x + 1)) m |= 128;
    return m;
}

// grid (ceil(P / 1024), n): X = {mask != 0} (value < 0) or {mask == value} and its complement, as bytes
__global__ __launch_bounds__(256) void cl_planes_kernel(const unsigned char* __restrict__ mask, unsigned char* __restrict__ X,
                                                        unsigned char* __restrict__ comp, int P, int value) {
    const size_t base = (size_t)blockIdx.y * P;
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long long i = (long long)blockIdx.x * CHUNK + k * 256 + threadIdx.x;
        if (i >= P) return;
        const unsigned char v = mask[base + i];
        const bool in = value < 0 ? v != 0 : v == value;
        X[base + i] = in;
        comp[base + i] = !in;
    }
}

// grid (ceil(P / 1024), n): lmask[pixel]; ptot[image][chunk] = (half-links, nodes) of the chunk
__global__ __launch_bounds__(256) void cl_count_kernel(const unsigned char* __restrict__ skel, unsigned char* __restrict__ lmask,
                                                       int* __restrict__ ptot, int H, int W, int P, int ncp) {
    __shared__ int wsum[4];
    const unsigned char* sk = skel + (size_t)blockIdx.y * P;
    unsigned char* lm = lmask + (size_t)blockIdx.y * P;
    int links = 0, nodes = 0;
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long long i = (long long)blockIdx.x * CHUNK + k * 256 + threadIdx.x;
        if (i < P) {
            const int y = (int)(i / W), x = (int)(i - (long long)y * W);
            const int m = link_mask(sk, y, x, H, W);
            lm[i] = (unsigned char)m;
            links += __popc(m);
            nodes += sk[i] != 0 && __popc(m) != 2;
        }
    }
    int tl, tn;
    block_scan(links, wsum, tl);
    block_scan(nodes, wsum, tn);
    if (threadIdx.x == 0) {
        int* t = ptot + ((size_t)blockIdx.y * ncp + blockIdx.x) * 2;
        t[0] = tl;
        t[1] = tn;
    }
}

// grid (ceil(P / 1024), n): hbase[pixel] = index of the pixel's first half-link; hkey[half-link] = 8 * pixel + direction; the
// node rows (y, x, degree, d2) below max_nodes
__global__ __launch_bounds__(256) void cl_build_kernel(const unsigned char* __restrict__ skel,
                                                       const unsigned char* __restrict__ lmask, const int* __restrict__ d2,
                                                       const int* __restrict__ ptot, int* __restrict__ hbase,
                                                       u32* __restrict__ hkey, int* __restrict__ nodes, int max_nodes, int W,
                                                       int P, int ncp, size_t hcap) {
    __shared__ int wsum[4];
    const size_t pb = (size_t)blockIdx.y * P;
    const unsigned char* sk = skel + pb;
    const unsigned char* lm = lmask + pb;
    int* hb = hbase + pb;
    u32* hk = hkey + (size_t)blockIdx.y * hcap;
    const int* t = ptot + ((size_t)blockIdx.y * ncp + blockIdx.x) * 2;
    int hcarry = t[0], ncarry = t[1];
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long long i = (long long)blockIdx.x * CHUNK + k * 256 + threadIdx.x;
        const int m = i < P ? lm[i] : 0;
        const bool node = i < P && sk[i] != 0 && __popc(m) != 2;
        int total;
        int at = hcarry + block_scan(__popc(m), wsum, total);
        hcarry += total;
        const int nidx = ncarry + block_scan(node, wsum, total);
        ncarry += total;
        if (i < P) {
            hb[i] = at;
            for (int d = 0; d < 8; ++d)
                if (m >> d & 1) hk[at++] = (u32)i * 8u + (u32)d;
            if (node && nidx < max_nodes) {
                int* row = nodes + ((size_t)blockIdx.y * max_nodes + nidx) * 4;
                const int y = (int)(i / W);
                row[0] = y;
                row[1] = (int)(i - (long long)y * W);
                row[2] = __popc(m);
                row[3] = d2[pb + i];
            }
        }
    }
}

struct Graph {   // one image's arrays
    const unsigned char* lmask;
    const int* hbase;
    const u32* hkey;
    int W;
    __device__ __forceinline__ int head(u32 key) const {   // the pixel a half-link points to
        const int d = (int)(key & 7u);
        return (int)(key >> 3) + dir_dy(d) * W + dir_dx(d);
    }
    __device__ __forceinline__ int index(int pixel, int d) const {   // the half-link of `pixel` in direction d (which it has)
        return hbase[pixel] + __popc(lmask[pixel] & ((1 << d) - 1));
    }
    __device__ __forceinline__ int rev(int h) const {   // the half-link back
        const u32 key = hkey[h];
        return index(head(key), 7 - (int)(key & 7u));
    }
};

// grid (JUMP_BLOCKS or fewer, n), half-link-strided: the successor and the word of every half-link
__global__ __launch_bounds__(256) void cl_link_kernel(const unsigned char* __restrict__ lmask, const int* __restrict__ hbase,
                                                      const u32* __restrict__ hkey, const int* __restrict__ hcount,
                                                      int* __restrict__ nxt0, ChainBuf out, int W, int P, size_t hcap) {
    const Graph g{lmask + (size_t)blockIdx.y * P, hbase + (size_t)blockIdx.y * P, hkey + (size_t)blockIdx.y * hcap, W};
    const size_t hb = (size_t)blockIdx.y * hcap;
    const int cnt = hcount[blockIdx.y];
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < cnt; v += (long long)gridDim.x * 256) {
        const u32 key = g.hkey[v];
        const int back = 7 - (int)(key & 7u), q = g.head(key);
        const int lq = g.lmask[q];
        int nx = (int)v;
        u32 word = (u32)v;
        if (__popc(lq) == 2) {
            nx = g.index(q, __ffs(lq & ~(1 << back)) - 1);
            word |= LIVE;
        }
        nxt0[hb + v] = nx;
        out.nxt[hb + v] = nx;
        out.mh[hb + v] = (u64)word << 32;
    }
}

struct Lead {   // what half-link v leads: points == 0: nothing
    int points, kind, end;
};

__device__ __forceinline__ Lead leader_of(const Graph& g, const u64* __restrict__ mh, const int* __restrict__ nxt0, int v) {
    Lead l{0, 0, 0};
    const int p = (int)(g.hkey[v] >> 3);
    const u64 m = mh[v];
    const u32 word = (u32)(m >> 32);
    if (__popc(g.lmask[p]) != 2) {   // leaves a node: the walk ends at the terminal `word`
        const int term = (int)(word & ~LIVE);
        if (v < g.rev(term)) {
            l.points = (int)(m & 0xffffffffull) + 2;
            l.end = g.head(g.hkey[term]);
        }
    } else if (word == ((u32)v | LIVE) && g.hbase[p] == v) {   // the smallest half-link of a curve without a node
        l.points = (int)(mh[nxt0[v]] & 0xffffffffull) + 1;
        l.kind = 1;
        l.end = p;
    }
    return l;
}

// grid (ceil(4 H W / 1024), n): ltot[image][chunk] = (leaders, points of their branches) among the chunk's half-links
__global__ __launch_bounds__(256) void cl_leaders_kernel(const unsigned char* __restrict__ lmask, const int* __restrict__ hbase,
                                                         const u32* __restrict__ hkey, const u64* __restrict__ mh,
                                                         const int* __restrict__ nxt0, const int* __restrict__ hcount,
                                                         int* __restrict__ ltot, int W, int P, size_t hcap, int nhc) {
    __shared__ int wsum[4];
    const Graph g{lmask + (size_t)blockIdx.y * P, hbase + (size_t)blockIdx.y * P, hkey + (size_t)blockIdx.y * hcap, W};
    const size_t hb = (size_t)blockIdx.y * hcap;
    const int cnt = hcount[blockIdx.y];
    int leaders = 0, points = 0;
    for (int k = 0; k < 4; ++k) {
        const long long v = (long long)blockIdx.x * CHUNK + threadIdx.x * 4 + k;
        if (v < cnt) {
            const Lead l = leader_of(g, mh + hb, nxt0 + hb, (int)v);
            leaders += l.points > 0;
            points += l.points;
        }
    }
    int tl, tp;
    block_scan(leaders, wsum, tl);
    block_scan(points, wsum, tp);
    if (threadIdx.x == 0) {
        int* t = ltot + ((size_t)blockIdx.y * nhc + blockIdx.x) * 2;
        t[0] = tl;
        t[1] = tp;
    }
}

// grid as leaders: at every leader its branch's row (the first five fields, below max_branches) and, in `info`, what its
// branch's half-links need: info.nxt[leader] = point offset, info.mh[leader] = branch number << 32 | point count
__global__ __launch_bounds__(256) void cl_place_kernel(const unsigned char* __restrict__ lmask, const int* __restrict__ hbase,
                                                       const u32* __restrict__ hkey, const u64* __restrict__ mh,
                                                       const int* __restrict__ nxt0, const int* __restrict__ hcount,
                                                       const int* __restrict__ ltot, ChainBuf info, long long* __restrict__ branches,
                                                       int max_branches, int W, int P, size_t hcap, int nhc) {
    __shared__ int wsum[4];
    const Graph g{lmask + (size_t)blockIdx.y * P, hbase + (size_t)blockIdx.y * P, hkey + (size_t)blockIdx.y * hcap, W};
    const size_t hb = (size_t)blockIdx.y * hcap;
    const int cnt = hcount[blockIdx.y];
    Lead l[4];
    int leaders = 0, points = 0;
    for (int k = 0; k < 4; ++k) {
        const long long v = (long long)blockIdx.x * CHUNK + threadIdx.x * 4 + k;
        l[k] = v < cnt ? leader_of(g, mh + hb, nxt0 + hb, (int)v) : Lead{0, 0, 0};
        leaders += l[k].points > 0;
        points += l[k].points;
    }
    const int* t = ltot + ((size_t)blockIdx.y * nhc + blockIdx.x) * 2;
    int total;
    int branch = t[0] + block_scan(leaders, wsum, total);
    int off = t[1] + block_scan(points, wsum, total);
    for (int k = 0; k < 4; ++k) {
        if (l[k].points == 0) continue;
        const long long v = (long long)blockIdx.x * CHUNK + threadIdx.x * 4 + k;
        info.nxt[hb + v] = off;
        info.mh[hb + v] = (u64)branch << 32 | (u64)l[k].points;
        if (branch < max_branches) {
            long long* row = branches + ((size_t)blockIdx.y * max_branches + branch) * 9;
            row[0] = (long long)(g.hkey[v] >> 3);
            row[1] = l[k].end;
            row[2] = off;
            row[3] = l[k].points;
            row[4] = l[k].kind;
        }
        ++branch;
        off += l[k].points;
    }
}

// grid as link: every point to its place; the link kinds, the widths and the largest d2 to the branch rows
__global__ __launch_bounds__(256) void cl_emit_kernel(const unsigned char* __restrict__ lmask, const int* __restrict__ hbase,
                                                      const u32* __restrict__ hkey, const u64* __restrict__ mh,
                                                      const int* __restrict__ d2, const int* __restrict__ hcount, ChainBuf info,
                                                      long long* __restrict__ branches, int max_branches, int* __restrict__ points,
                                                      long long max_points, int W, int P, size_t hcap) {
    const Graph g{lmask + (size_t)blockIdx.y * P, hbase + (size_t)blockIdx.y * P, hkey + (size_t)blockIdx.y * hcap, W};
    const int* fld = d2 + (size_t)blockIdx.y * P;
    const size_t hb = (size_t)blockIdx.y * hcap;
    const int cnt = hcount[blockIdx.y];
    auto put = [&](long long pos, int pixel) {
        if ((u64)pos < (u64)max_points) {
            int* out = points + ((size_t)blockIdx.y * max_points + pos) * 3;
            const int y = pixel / W;
            out[0] = y;
            out[1] = pixel - y * W;
            out[2] = fld[pixel];
        }
    };
    const int lane = threadIdx.x & (WAVE - 1);
    for (long long v0 = (long long)blockIdx.x * 256; v0 < cnt; v0 += (long long)gridDim.x * 256) {   // the same trips for a wave
        const long long v = v0 + threadIdx.x;
        int branch = -1, orth = 0, diag = 0, mx = 0;   // what this half-link adds to its branch's row; branch < 0: nothing
        long long w = 0;
        if (v < cnt) {
            const u32 key = g.hkey[v];
            const int p = (int)(key >> 3), q = g.head(key);
            const u64 m = mh[hb + v];
            const u32 word = (u32)(m >> 32);
            const int hops = (int)(m & 0xffffffffull);
            size_t leader = 0;
            long long rank = 0;      // of the point this half-link brings: its head on a walk, its tail on a cycle
            int pixel = -1, first = -1;   // first: the walk's first pixel, brought by the leader as well
            if (!(word & LIVE)) {
                const u64 mr = mh[hb + g.rev((int)v)];   // the walk from the other end, up to here
                const int start = g.rev((int)((u32)(mr >> 32) & ~LIVE));
                if (start < g.rev((int)word)) {   // else the other direction is the reported one
                    leader = hb + start;
                    rank = (long long)(mr & 0xffffffffull) + 1;
                    pixel = q;
                    if (rank == 1) first = p;
                }
            } else {
                const int least = (int)(word & ~LIVE);
                if (g.hbase[g.hkey[least] >> 3] == least) {
                    leader = hb + least;
                    const int len = (int)(info.mh[leader] & 0xffffffffull);
                    rank = hops == 0 ? 0 : len - hops;
                    pixel = p;
                }
            }
            if (pixel >= 0) {
                const long long off = info.nxt[leader];
                const int b = (int)(info.mh[leader] >> 32);
                put(off + rank, pixel);
                if (first >= 0) put(off, first);
                if ((u32)b < (u32)max_branches) {
                    branch = b;
                    diag = dir_diagonal((int)(key & 7u));
                    orth = !diag;
                    mx = fld[pixel];
                    w = llrint(sqrt((double)mx) * 65536.0);
                    if (first >= 0) {
                        w += llrint(sqrt((double)fld[first]) * 65536.0);
                        mx = max(mx, fld[first]);
                    }
                }
            }
        }
        // the lanes of a wave that add to the same row add once: a long branch is thousands of adds to four words otherwise
        u64 pending = __ballot(branch >= 0);
        while (pending) {
            const int src = __ffsll((long long)pending) - 1;
            const bool mine = branch >= 0 && branch == __shfl(branch, src);
            const u64 group = __ballot(mine);
            int o = mine ? orth : 0, d = mine ? diag : 0, x = mine ? mx : 0;
            long long ww = mine ? w : 0;
            if (group & (group - 1)) {   // more than one lane
                for (int sh = WAVE / 2; sh > 0; sh >>= 1) {
                    o += __shfl_xor(o, sh);
                    d += __shfl_xor(d, sh);
                    ww += __shfl_xor(ww, sh);
                    x = max(x, __shfl_xor(x, sh));
                }
            }
            if (lane == src) {
                u64* row = (u64*)(branches + ((size_t)blockIdx.y * max_branches + branch) * 9);
                if (o) atomicAdd(row + 5, (u64)o);
                if (d) atomicAdd(row + 6, (u64)d);
                atomicAdd(row + 7, (u64)ww);
                atomicMax(row + 8, (u64)x);
            }
            pending &= ~group;
        }
    }
}

bool shape_ok(int n, int H, int W) {
    return n >= 1 && n <= CL_MAX_BATCH && H >= 1 && H <= CL_MAX_SIDE && W >= 1 && W <= CL_MAX_SIDE && (long long)H * W < (1ll << 29);
}

struct Layout {   // the thinning's scratch, then the byte planes, the pixel words, the half-link keys and the chain scratch
    size_t X, comp, skel, lmask, d2, maxw, hbase, hcount, ptot, ltot, hkey, chain_at, total;
    ChainLayout chain;   // of the half-links: an image can have four per pixel
    int ncp;
};

// thin_bytes: skeleton_scratch_bytes(n, H, W, route), not 0
Layout layout(int n, int H, int W, size_t thin_bytes) {
    Layout l{};
    const size_t P = (size_t)H * W;
    l.chain = chain_layout(n, 4 * P);
    l.ncp = (int)((P + CHUNK - 1) / CHUNK);
    size_t o = up256(thin_bytes);
    l.X = o;        o += up256((size_t)n * P);
    l.comp = o;     o += up256((size_t)n * P);
    l.skel = o;     o += up256((size_t)n * P);
    l.lmask = o;    o += up256((size_t)n * P);
    l.d2 = o;       o += up256((size_t)n * P * sizeof(int));
    l.maxw = o;     o += up256((size_t)n * 2 * sizeof(int));
    l.hbase = o;    o += up256((size_t)n * P * sizeof(int));
    l.hcount = o;   o += up256((size_t)n * sizeof(int));
    l.ptot = o;     o += up256((size_t)n * l.ncp * 2 * sizeof(int));
    l.ltot = o;     o += up256((size_t)n * l.chain.nchunks * 2 * sizeof(int));
    l.hkey = o;     o += up256((size_t)n * l.chain.cap * sizeof(u32));
    l.chain_at = o; o += l.chain.bytes;
    l.total = o;
    return l;
}

}  // namespace

size_t centerlines_scratch_bytes(int n, int H, int W, int route) {
    if (!shape_ok(n, H, W)) return 0;
    const size_t thin_bytes = skeleton_scratch_bytes(n, H, W, route);   // 0 for a bad route or a plane the route cannot take
    return thin_bytes ? layout(n, H, W, thin_bytes).total : 0;
}

int launch_centerlines(const unsigned char* mask, int n, int H, int W, int value, int thin, int route, int* node_counts,
                       int* branch_counts, long long* point_counts, int* nodes, int max_nodes, long long* branches,
                       int max_branches, int* points, long long max_points, void* scratch, size_t scratch_bytes, hipStream_t s) {
    VITSEG_CHECK_ARG(mask && node_counts && branch_counts && point_counts && scratch, VITSEG_EINVAL,
                     "centerlines: null mask, counts or scratch");
    VITSEG_CHECK_ARG(max_nodes >= 0 && max_branches >= 0 && max_points >= 0, VITSEG_EINVAL,
                     "centerlines: negative max_nodes, max_branches or max_points");
    VITSEG_CHECK_ARG((nodes || max_nodes == 0) && (branches || max_branches == 0) && (points || max_points == 0), VITSEG_EINVAL,
                     "centerlines: null nodes, branches or points with a positive capacity");
    VITSEG_CHECK_ARG(value >= -1 && value <= 255, VITSEG_EINVAL, "centerlines: value must be 0..255 or -1, got %d", value);
    VITSEG_CHECK_ARG(thin == 0 || thin == 1, VITSEG_EINVAL, "centerlines: thin must be 0 or 1, got %d", thin);
    VITSEG_CHECK_ARG(route >= 0 && route <= 2, VITSEG_EINVAL,
                     "centerlines: route must be 0 (automatic), 1 (resident) or 2 (global), got %d", route);
    VITSEG_CHECK_ARG(shape_ok(n, H, W), VITSEG_ESHAPE,
                     "centerlines: bad shape n=%d H=%d W=%d (1 <= H, W <= %d, H*W < 2^29, 1 <= n <= %d)", n, H, W, CL_MAX_SIDE,
                     CL_MAX_BATCH);
    const size_t thin_bytes = skeleton_scratch_bytes(n, H, W, route);
    VITSEG_CHECK_ARG(thin_bytes != 0, VITSEG_ESHAPE, "centerlines: bad shape: a %d x %d plane does not fit the resident route", H,
                     W);
    const Layout l = layout(n, H, W, thin_bytes);
    VITSEG_CHECK_ARG(scratch_bytes >= l.total, VITSEG_EWORKSPACE, "centerlines: scratch of %zu bytes, %zu needed", scratch_bytes,
                     l.total);
    char* base = (char*)scratch;
    unsigned char* X = (unsigned char*)(base + l.X);
    unsigned char* comp = (unsigned char*)(base + l.comp);
    unsigned char* skel = thin ? (unsigned char*)(base + l.skel) : X;
    unsigned char* lmask = (unsigned char*)(base + l.lmask);
    int* d2 = (int*)(base + l.d2);
    int* maxw = (int*)(base + l.maxw);
    int* hbase = (int*)(base + l.hbase);
    int* hcount = (int*)(base + l.hcount);
    int* ptot = (int*)(base + l.ptot);
    int* ltot = (int*)(base + l.ltot);
    u32* hkey = (u32*)(base + l.hkey);
    const ChainScratch c = chain_scratch(base + l.chain_at, l.chain);
    const size_t hcap = l.chain.cap;
    const int P = H * W, nhc = l.chain.nchunks;
    hipError_t e = hipMemsetAsync(maxw, 0, (size_t)n * 2 * sizeof(int), s);
    if (e == hipSuccess && max_nodes > 0) e = hipMemsetAsync(nodes, 0, (size_t)n * max_nodes * 4 * sizeof(int), s);
    if (e == hipSuccess && max_branches > 0) e = hipMemsetAsync(branches, 0, (size_t)n * max_branches * 9 * sizeof(long long), s);
    if (e == hipSuccess && max_points > 0) e = hipMemsetAsync(points, 0, (size_t)n * (size_t)max_points * 3 * sizeof(int), s);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(centerlines)");
    const dim3 pgrid(l.ncp, n), hgrid(nhc, n), sgrid = chain_grid(l.chain);
    hipLaunchKernelGGL(cl_planes_kernel, pgrid, dim3(256), 0, s, mask, X, comp, P, value);
    VITSEG_LAUNCH_CHECK("centerlines planes");
    if (thin)
        if (const int rc = launch_skeleton(X, n, H, W, route, skel, nullptr, scratch, thin_bytes, s)) return rc;
    if (const int rc = launch_sdf_d2(comp, n, H, W, d2, maxw, s)) return rc;
    hipLaunchKernelGGL(cl_count_kernel, pgrid, dim3(256), 0, s, skel, lmask, ptot, H, W, P, l.ncp);
    VITSEG_LAUNCH_CHECK("centerlines count");
    if (const int rc = launch_chunk_scan(ptot, n, l.ncp, 2, ScanOut{{hcount, node_counts}, {nullptr, nullptr}}, s)) return rc;
    hipLaunchKernelGGL(cl_build_kernel, pgrid, dim3(256), 0, s, skel, lmask, d2, ptot, hbase, hkey, nodes, max_nodes, W, P, l.ncp,
                       hcap);
    VITSEG_LAUNCH_CHECK("centerlines build");
    hipLaunchKernelGGL(cl_link_kernel, sgrid, dim3(256), 0, s, lmask, hbase, hkey, hcount, c.nxt0, c.buf[0], W, P, hcap);
    VITSEG_LAUNCH_CHECK("centerlines link");
    ChainBuf fin, info;   // (word, hops) of every half-link; the other side, free for what place tells emit
    if (const int rc = launch_chain_jumps(l.chain, c, hcount, &fin, &info, s)) return rc;
    hipLaunchKernelGGL(cl_leaders_kernel, hgrid, dim3(256), 0, s, lmask, hbase, hkey, fin.mh, c.nxt0, hcount, ltot, W, P, hcap, nhc);
    VITSEG_LAUNCH_CHECK("centerlines leaders");
    if (const int rc = launch_chunk_scan(ltot, n, nhc, 2, ScanOut{{branch_counts, nullptr}, {nullptr, point_counts}}, s)) return rc;
    hipLaunchKernelGGL(cl_place_kernel, hgrid, dim3(256), 0, s, lmask, hbase, hkey, fin.mh, c.nxt0, hcount, ltot, info, branches,
                       max_branches, W, P, hcap, nhc);
    VITSEG_LAUNCH_CHECK("centerlines place");
    hipLaunchKernelGGL(cl_emit_kernel, sgrid, dim3(256), 0, s, lmask, hbase, hkey, fin.mh, d2, hcount, info, branches,
                       max_branches, points, max_points, W, P, hcap);
    VITSEG_LAUNCH_CHECK("centerlines emit");
    return VITSEG_OK;
}

}  // namespace vitseg

extern "C" {

int vitseg_centerlines_version(void) { return VITSEG_CENTERLINES_VERSION; }

size_t vitseg_centerlines_scratch_bytes(int n, int H, int W, int route) {
    return vitseg::centerlines_scratch_bytes(n, H, W, route);
}

int vitseg_centerlines(const uint8_t* mask, int n, int H, int W, int value, int thin, int route, int32_t* node_counts,
                       int32_t* branch_counts, int64_t* point_counts, int32_t* nodes, int max_nodes, int64_t* branches,
                       int max_branches, int32_t* points, int64_t max_points, void* scratch, size_t scratch_bytes, void* stream) {
    return vitseg::launch_centerlines(mask, n, H, W, value, thin, route, node_counts, branch_counts, (long long*)point_counts,
                                      nodes, max_nodes, (long long*)branches, max_branches, points, (long long)max_points, scratch,
                                      scratch_bytes, (hipStream_t)stream);
}

}  // extern "C"
