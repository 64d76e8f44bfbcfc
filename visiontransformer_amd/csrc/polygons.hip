// Region outlines (vitseg_region_polygons, include/vitseg_polygons.h): the boundary of every connected region as polygon
// rings with holes, exact integer geometry on the corner lattice.  The contract -- directed unit edges with the region on
// their right, the successor rule with its saddle case, rings, vertices, areas and the numbering -- is stated in the header.
//
// Nothing here labels: the region index of every pixel comes from the launches of regions.hip.  An edge is named by its key
// 4 * (tail_y * (W + 1) + tail_x) + direction, so that the order of the keys is the order the contract numbers by.  Only the
// edges that are vertices (their predecessor has another direction) become nodes; a straight run is walked once by the node
// it starts at.  Whether an edge leaving a corner exists and whether it is a vertex follow from the 2 x 2 pixels round the
// corner alone (corner_mask), so nothing but the label plane is kept per pixel.
//   (labels)     tile_label, seam_merge, resolve, class_scan, emit, labels of regions.hip
//   count        one thread per corner: the number of vertex edges leaving it; totals per chunk of 1024 corners
//   (scan)       chunk scan of chains.hip, one workgroup per image: exclusive scan of the chunk totals; the image's vertex count
//   build        per corner: the index of its first node (scan within the chunk + the chunk's base); every node's key.
//                Nodes are therefore numbered in key order, and a ring's start edge is its smallest node
//   link         per node: walks the straight run to its end, takes the turn there and looks the next node up
//   (jump x R)   chain jumps of chains.hip over the cyclic lists, R = ceil(log2(4 H W)) rounds: after round j a node knows the
//                smallest node among the 2^(j+1) from itself on and how many hops ahead it lies.  A round that changed nothing
//                leaves a zero in its word of `changed`; the rounds after it return at once (the host never reads that word)
//   rings        per node chunk: the number of leaders (nodes that are their ring's smallest) and of their rings' vertices
//   (scan)       exclusive scan of both over the chunks: ring numbers and vertex offsets in key order; the ring count
//   place        per leader: its ring's row (region, offset, count) and, for its ring's nodes, the ring number and offset
//   emit         per node: rank = hops from the leader; the vertex goes to offset + rank; a node going S or N adds
//                x * (y_next - y) to its ring's area (the shoelace sum, taken over the vertical sides: each term an integer)
// Every value is an integer; the only atomics are the area sums (order-independent) and the `changed` flags.
#include "chains.hpp"
#include "kernels.hpp"
#include "../../include/vitseg_polygons.h"

namespace vitseg {
namespace {

constexpr int POLY_MAX_SIDE = 16384;

__device__ __forceinline__ int label_at(const int* __restrict__ lab, int y, int x, int H, int W) {
    return (y >= 0 && y < H && x >= 0 && x < W) ? lab[y * W + x] : -1;
}

// bit d: the edge leaving corner (y, x) in direction d exists and is a vertex.  a b / c d are the labels of the pixels
// NW NE / SW SE of the corner.  The edge going E is the top side of SE, going S the right side of SW, going W the bottom side
// of NW, going N the left side of NE; it is a vertex unless the straight edge arriving at the corner exists (at a saddle
// neither arriving edge is straight).
__device__ __forceinline__ int corner_mask(const int* __restrict__ lab, int y, int x, int H, int W) {
    const int a = label_at(lab, y - 1, x - 1, H, W), b = label_at(lab, y - 1, x, H, W);
    const int c = label_at(lab, y, x - 1, H, W), d = label_at(lab, y, x, H, W);
    int m = 0;
    if (d >= 0 && b != d && !(c == d && a != d)) m |= 1;
    if (c >= 0 && d != c && !(a == c && b != c)) m |= 2;
    if (a >= 0 && c != a && !(b == a && d != a)) m |= 4;
    if (b >= 0 && a != b && !(d == b && c != b)) m |= 8;
    return m;
}

// grid (ceil(C / 1024), n), C = (H + 1)(W + 1) corners
__global__ __launch_bounds__(256) void poly_count_kernel(const int* __restrict__ labels, int* __restrict__ ctot, int H, int W,
                                                         int C, int ncc) {
    __shared__ int wsum[4];
    const int* lab = labels + (size_t)blockIdx.y * H * W;
    int cnt = 0;
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long long i = (long long)blockIdx.x * CHUNK + k * 256 + threadIdx.x;
        if (i < C) {
            const int y = (int)(i / (W + 1)), x = (int)(i - (long long)y * (W + 1));
            cnt += __popc(corner_mask(lab, y, x, H, W));
        }
    }
    int total;
    block_scan(cnt, wsum, total);
    if (threadIdx.x == 0) ctot[(size_t)blockIdx.y * ncc + blockIdx.x] = total;
}

// grid (ceil(C / 1024), n): cbase[corner] = index of the corner's first node; nkey[node] = 4 * corner + direction
__global__ __launch_bounds__(256) void poly_build_kernel(const int* __restrict__ labels, const int* __restrict__ ctot,
                                                         int* __restrict__ cbase, u32* __restrict__ nkey, int H, int W, int C,
                                                         int ncc, size_t ncap) {
    __shared__ int wsum[4];
    const int* lab = labels + (size_t)blockIdx.y * H * W;
    int* cb = cbase + (size_t)blockIdx.y * C;
    u32* nk = nkey + (size_t)blockIdx.y * ncap;
    int carry = ctot[(size_t)blockIdx.y * ncc + blockIdx.x];
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long long i = (long long)blockIdx.x * CHUNK + k * 256 + threadIdx.x;
        int m = 0;
        if (i < C) {
            const int y = (int)(i / (W + 1)), x = (int)(i - (long long)y * (W + 1));
            m = corner_mask(lab, y, x, H, W);
        }
        int total;
        int at = carry + block_scan(__popc(m), wsum, total);
        carry += total;
        if (i < C) {
            cb[i] = at;
            for (int d = 0; d < 4; ++d)
                if (m >> d & 1) nk[at++] = (u32)i * 4u + (u32)d;
        }
    }
}

__device__ __forceinline__ int dir_y(int d) { return (d == 1) - (d == 3); }   // the step of E, S, W, N
__device__ __forceinline__ int dir_x(int d) { return (d == 0) - (d == 2); }

// grid (JUMP_BLOCKS or fewer, n), node-strided: the node after this one on its ring
__global__ __launch_bounds__(256) void poly_link_kernel(const int* __restrict__ labels, const int* __restrict__ cbase,
                                                        const u32* __restrict__ nkey, const int* __restrict__ ncount,
                                                        int* __restrict__ nxt0, ChainBuf out, int H, int W, int C, size_t ncap,
                                                        int conn8) {
    const int* lab = labels + (size_t)blockIdx.y * H * W;
    const int* cb = cbase + (size_t)blockIdx.y * C;
    const size_t nb = (size_t)blockIdx.y * ncap;
    const int cnt = ncount[blockIdx.y];
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < cnt; v += (long long)gridDim.x * 256) {
        const u32 key = nkey[nb + v];
        const int s = (int)(key & 3u), corner = (int)(key >> 2);
        const int ty = corner / (W + 1), tx = corner - ty * (W + 1);
        // the pixel whose side the edge is: tail (r, c) E, (r, c+1) S, (r+1, c+1) W, (r+1, c) N
        int r = ty - (s == 2 || s == 3), c = tx - (s == 1 || s == 2);
        const int fy = dir_y(s), fx = dir_x(s), oy = dir_y((s + 3) & 3), ox = dir_x((s + 3) & 3);   // ahead; the outside, to the left
        const int R = lab[r * W + c];
        bool A, B;   // the pixel ahead and the one ahead on the outside are in the region
        while (true) {
            A = label_at(lab, r + fy, c + fx, H, W) == R;
            B = label_at(lab, r + fy + oy, c + fx + ox, H, W) == R;
            if (!(A && !B)) break;
            r += fy;
            c += fx;
        }
        int s2;
        if (B && (A || conn8)) {   // left turn: the side of the pixel ahead on the outside
            r += fy + oy;
            c += fx + ox;
            s2 = (s + 3) & 3;
        } else {   // right turn: the next side of the same pixel
            s2 = (s + 1) & 3;
        }
        const int y2 = r + (s2 == 2 || s2 == 3), x2 = c + (s2 == 1 || s2 == 2);
        const int m2 = corner_mask(lab, y2, x2, H, W);
        const int nx = cb[y2 * (W + 1) + x2] + __popc(m2 & ((1 << s2) - 1));
        nxt0[nb + v] = nx;
        out.nxt[nb + v] = nx;
        out.mh[nb + v] = (u64)v << 32;
    }
}

// leader test and ring length of node v (length: hops from the node after the leader back to it, plus one)
__device__ __forceinline__ int ring_len(const u64* __restrict__ mh, const int* __restrict__ nxt0, long long v) {
    if ((long long)(mh[v] >> 32) != v) return 0;
    return (int)(mh[nxt0[v]] & 0xffffffffull) + 1;
}

// grid (ceil(4 H W / 1024), n): ntot[image][chunk] = (leaders, vertices of their rings) among the chunk's nodes
__global__ __launch_bounds__(256) void poly_rings_kernel(const u64* __restrict__ mh, const int* __restrict__ nxt0,
                                                         const int* __restrict__ ncount, int* __restrict__ ntot, size_t ncap,
                                                         int nnc) {
    __shared__ int wsum[4];
    const size_t nb = (size_t)blockIdx.y * ncap;
    const int cnt = ncount[blockIdx.y];
    int leaders = 0, verts = 0;
    for (int k = 0; k < 4; ++k) {
        const long long v = (long long)blockIdx.x * CHUNK + threadIdx.x * 4 + k;
        if (v < cnt) {
            const int len = ring_len(mh + nb, nxt0 + nb, v);
            leaders += len > 0;
            verts += len;
        }
    }
    int tl, tv;
    block_scan(leaders, wsum, tl);
    block_scan(verts, wsum, tv);
    if (threadIdx.x == 0) {
        int* t = ntot + ((size_t)blockIdx.y * nnc + blockIdx.x) * 2;
        t[0] = tl;
        t[1] = tv;
    }
}

// grid as rings: at every leader its ring's row (the first max_rings) and, in `info`, what its ring's nodes need:
// info.nxt[leader] = vertex offset, info.mh[leader] = ring number << 32 | length
__global__ __launch_bounds__(256) void poly_place_kernel(const int* __restrict__ labels, const u32* __restrict__ nkey,
                                                         const u64* __restrict__ mh, const int* __restrict__ nxt0,
                                                         const int* __restrict__ ncount, const int* __restrict__ ntot,
                                                         ChainBuf info, long long* __restrict__ rings, int max_rings, int H, int W,
                                                         size_t ncap, int nnc) {
    __shared__ int wsum[4];
    const size_t nb = (size_t)blockIdx.y * ncap;
    const int* lab = labels + (size_t)blockIdx.y * H * W;
    const int cnt = ncount[blockIdx.y];
    int len[4], leaders = 0, verts = 0;
    for (int k = 0; k < 4; ++k) {
        const long long v = (long long)blockIdx.x * CHUNK + threadIdx.x * 4 + k;
        len[k] = v < cnt ? ring_len(mh + nb, nxt0 + nb, v) : 0;
        leaders += len[k] > 0;
        verts += len[k];
    }
    const int* t = ntot + ((size_t)blockIdx.y * nnc + blockIdx.x) * 2;
    int total;
    int ring = t[0] + block_scan(leaders, wsum, total);
    int off = t[1] + block_scan(verts, wsum, total);
    for (int k = 0; k < 4; ++k) {
        if (len[k] == 0) continue;
        const long long v = (long long)blockIdx.x * CHUNK + threadIdx.x * 4 + k;
        const u32 key = nkey[nb + v];   // a ring starts going E or S: at the top side of pixel (y, x) or the right side of (y, x - 1)
        const int corner = (int)(key >> 2), y = corner / (W + 1), x = corner - y * (W + 1);
        info.nxt[nb + v] = off;
        info.mh[nb + v] = (u64)ring << 32 | (u64)len[k];
        if (ring < max_rings) {
            long long* row = rings + ((size_t)blockIdx.y * max_rings + ring) * 4;
            row[0] = lab[y * W + x - (int)(key & 1u)];
            row[1] = off;
            row[2] = len[k];
        }
        ++ring;
        off += len[k];
    }
}

// grid as link: every node's vertex to its place, the vertical sides' terms to their ring's area
__global__ __launch_bounds__(256) void poly_emit_kernel(const u32* __restrict__ nkey, const u64* __restrict__ mh,
                                                        const int* __restrict__ nxt0, const int* __restrict__ ncount, ChainBuf info,
                                                        long long* __restrict__ rings, int max_rings, int* __restrict__ vertices,
                                                        long long max_vertices, int W, size_t ncap) {
    const size_t nb = (size_t)blockIdx.y * ncap;
    const int cnt = ncount[blockIdx.y];
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < cnt; v += (long long)gridDim.x * 256) {
        const u64 m = mh[nb + v];
        const size_t leader = nb + (size_t)(m >> 32);
        const int hops = (int)(m & 0xffffffffull);
        const u64 rl = info.mh[leader];
        const int ring = (int)(rl >> 32), len = (int)(rl & 0xffffffffull);
        const long long pos = (long long)info.nxt[leader] + (hops == 0 ? 0 : len - hops);
        const u32 key = nkey[nb + v];
        const int corner = (int)(key >> 2), y = corner / (W + 1), x = corner - y * (W + 1);
        if (pos < max_vertices) {
            int* out = vertices + ((size_t)blockIdx.y * max_vertices + pos) * 2;
            out[0] = y;
            out[1] = x;
        }
        if ((key & 1u) && ring < max_rings) {
            const int y2 = (int)(nkey[nb + nxt0[nb + v]] >> 2) / (W + 1);
            atomicAdd((u64*)(rings + ((size_t)blockIdx.y * max_rings + ring) * 4 + 3), (u64)((long long)x * (y2 - y)));
        }
    }
}

bool shape_ok(int n, int H, int W) {
    return n >= 1 && n <= 65535 && H >= 1 && H <= POLY_MAX_SIDE && W >= 1 && W <= POLY_MAX_SIDE && (long long)H * W < (1ll << 29);
}

struct Layout {   // the labelling's scratch, then the label plane, the corner words, the node keys and the chain scratch
    size_t labels, ncount, ctot, ntot, cbase, nkey, chain_at, total;
    ChainLayout chain;   // of the nodes: an image can have 4 H W, every side of every pixel
    int C, ncc;
};

Layout layout(int n, int H, int W) {
    Layout l{};
    const size_t P = (size_t)H * W;
    l.chain = chain_layout(n, 4 * P);
    l.C = (H + 1) * (W + 1);
    l.ncc = (l.C + CHUNK - 1) / CHUNK;
    size_t o = up256(regions_scratch_bytes(n, H, W));
    l.labels = o;    o += up256((size_t)n * P * sizeof(int));
    l.ncount = o;    o += up256((size_t)n * sizeof(int));
    l.ctot = o;      o += up256((size_t)n * l.ncc * sizeof(int));
    l.ntot = o;      o += up256((size_t)n * l.chain.nchunks * 2 * sizeof(int));
    l.cbase = o;     o += up256((size_t)n * l.C * sizeof(int));
    l.nkey = o;      o += up256((size_t)n * l.chain.cap * sizeof(u32));
    l.chain_at = o;  o += l.chain.bytes;
    l.total = o;
    return l;
}

}  // namespace

size_t region_polygons_scratch_bytes(int n, int H, int W) { return shape_ok(n, H, W) ? layout(n, H, W).total : 0; }

int launch_region_polygons(const unsigned char* mask, int n, int H, int W, int connectivity, int background, int* region_counts,
                           int* ring_counts, long long* vertex_counts, long long* rings, int max_rings, int* vertices,
                           long long max_vertices, int* labels, void* scratch, size_t scratch_bytes, hipStream_t s) {
    VITSEG_CHECK_ARG(mask && region_counts && ring_counts && vertex_counts && scratch, VITSEG_EINVAL,
                     "region_polygons: null mask, counts or scratch");
    VITSEG_CHECK_ARG(max_rings >= 0 && max_vertices >= 0, VITSEG_EINVAL, "region_polygons: negative max_rings or max_vertices");
    VITSEG_CHECK_ARG((rings || max_rings == 0) && (vertices || max_vertices == 0), VITSEG_EINVAL,
                     "region_polygons: null rings or vertices with a positive capacity");
    VITSEG_CHECK_ARG(connectivity == 4 || connectivity == 8, VITSEG_EINVAL, "region_polygons: connectivity must be 4 or 8, got %d",
                     connectivity);
    VITSEG_CHECK_ARG(background >= -1 && background <= 255, VITSEG_EINVAL,
                     "region_polygons: background must be 0..255 or -1, got %d", background);
    VITSEG_CHECK_ARG(shape_ok(n, H, W), VITSEG_ESHAPE,
                     "region_polygons: bad shape n=%d H=%d W=%d (1 <= H, W <= %d, H*W < 2^29, 1 <= n <= 65535)", n, H, W,
                     POLY_MAX_SIDE);
    const Layout l = layout(n, H, W);
    VITSEG_CHECK_ARG(scratch_bytes >= l.total, VITSEG_EWORKSPACE, "region_polygons: scratch of %zu bytes, %zu needed",
                     scratch_bytes, l.total);
    char* base = (char*)scratch;
    const RegionWords w = region_words(scratch, n, H, W);
    int* lab = labels ? labels : (int*)(base + l.labels);
    int* ncount = (int*)(base + l.ncount);
    int* ctot = (int*)(base + l.ctot);
    int* ntot = (int*)(base + l.ntot);
    int* cbase = (int*)(base + l.cbase);
    u32* nkey = (u32*)(base + l.nkey);
    const ChainScratch c = chain_scratch(base + l.chain_at, l.chain);
    const size_t ncap = l.chain.cap;
    const int nnc = l.chain.nchunks;
    if (max_rings > 0) {
        const hipError_t e = hipMemsetAsync(rings, 0, (size_t)n * max_rings * 4 * sizeof(long long), s);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(region_polygons rings)");
    }
    if (max_vertices > 0) {
        const hipError_t e = hipMemsetAsync(vertices, 0, (size_t)n * (size_t)max_vertices * 2 * sizeof(int), s);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(region_polygons vertices)");
    }
    if (const int rc = launch_region_labels(mask, n, H, W, connectivity, background, w, s)) return rc;
    if (const int rc = launch_region_index(mask, n, H, W, w, region_counts, nullptr, 0, lab, s)) return rc;
    const dim3 cgrid(l.ncc, n), ngrid(nnc, n), sgrid = chain_grid(l.chain);
    hipLaunchKernelGGL(poly_count_kernel, cgrid, dim3(256), 0, s, lab, ctot, H, W, l.C, l.ncc);
    VITSEG_LAUNCH_CHECK("region_polygons count");
    if (const int rc = launch_chunk_scan(ctot, n, l.ncc, 1, ScanOut{{ncount, nullptr}, {vertex_counts, nullptr}}, s)) return rc;
    hipLaunchKernelGGL(poly_build_kernel, cgrid, dim3(256), 0, s, lab, ctot, cbase, nkey, H, W, l.C, l.ncc, ncap);
    VITSEG_LAUNCH_CHECK("region_polygons build");
    hipLaunchKernelGGL(poly_link_kernel, sgrid, dim3(256), 0, s, lab, cbase, nkey, ncount, c.nxt0, c.buf[0], H, W, l.C, ncap,
                       connectivity == 8);
    VITSEG_LAUNCH_CHECK("region_polygons link");
    ChainBuf fin, info;   // (smallest node, hops) of every node; the other side, free for what place tells emit
    if (const int rc = launch_chain_jumps(l.chain, c, ncount, &fin, &info, s)) return rc;
    hipLaunchKernelGGL(poly_rings_kernel, ngrid, dim3(256), 0, s, fin.mh, c.nxt0, ncount, ntot, ncap, nnc);
    VITSEG_LAUNCH_CHECK("region_polygons rings");
    if (const int rc = launch_chunk_scan(ntot, n, nnc, 2, ScanOut{{ring_counts, nullptr}, {nullptr, nullptr}}, s)) return rc;
    hipLaunchKernelGGL(poly_place_kernel, ngrid, dim3(256), 0, s, lab, nkey, fin.mh, c.nxt0, ncount, ntot, info, rings, max_rings,
                       H, W, ncap, nnc);
    VITSEG_LAUNCH_CHECK("region_polygons place");
    hipLaunchKernelGGL(poly_emit_kernel, sgrid, dim3(256), 0, s, nkey, fin.mh, c.nxt0, ncount, info, rings, max_rings, vertices,
                       max_vertices, W, ncap);
    VITSEG_LAUNCH_CHECK("region_polygons emit");
    return VITSEG_OK;
}

}  // namespace vitseg

extern "C" {

int vitseg_polygons_version(void) { return VITSEG_POLYGONS_VERSION; }

size_t vitseg_region_polygons_scratch_bytes(int n, int H, int W) { return vitseg::region_polygons_scratch_bytes(n, H, W); }

int vitseg_region_polygons(const uint8_t* mask, int n, int H, int W, int connectivity, int background, int32_t* region_counts,
                           int32_t* ring_counts, int64_t* vertex_counts, int64_t* rings, int max_rings, int32_t* vertices,
                           int64_t max_vertices, int32_t* labels, void* scratch, size_t scratch_bytes, void* stream) {
    return vitseg::launch_region_polygons(mask, n, H, W, connectivity, background, region_counts, ring_counts,
                                          (long long*)vertex_counts, (long long*)rings, max_rings, vertices, (long long)max_vertices,
                                          labels, scratch, scratch_bytes, (hipStream_t)stream);
}

}  // extern "C"
