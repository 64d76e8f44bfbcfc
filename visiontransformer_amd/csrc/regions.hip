// Connected regions of class masks and their boxes: the arithmetic of the reference's "Predicted Regions with Boxes"
// panel (model/CE/testViTModel.py:34-42 get_bounding_boxes = scipy.ndimage.label + np.argwhere per label, called per class
// present except 0 at :171-185; the same code in datasetTestViTmodel.py and model/PAED/ViTscriptTest.py).
//
// A region is a maximal 4- or 8-connected set of equal pixels whose value is not `background`.  Its record is
// (class, y_min, x_min, y_max, x_max, area, first, 0), `first` = raster index of its first pixel; the records of an image
// are ordered by (class, first), which is the order of the reference's loop (np.unique classes, then scipy's label
// numbering, which follows the raster order of each component's first pixel).
//
// Every component's representative is its minimum raster index, i.e. `first`, so nothing depends on the order in which
// workgroups run.  Six launches, data passed between them only at kernel boundaries:
//  1. tile_label    one workgroup per 32 x 32 tile: union-find in LDS (link to the smaller index by atomicMin); every
//                   pixel's link = image raster index of its tile-local root, -1 on background; the box / area words of
//                   each tile root are initialised (a component's root is the root of its own tile's part too).
//  2. seam_merge    one thread per pixel on a tile's left or top border: union with its neighbours in the adjacent tiles
//                   by the same rule, in global memory.  Every access to a link word in this launch is an atomic
//                   read-modify-write whose returned value is used (atomics execute at the memory side, so workgroups on
//                   different XCDs see one another's links; no plain load of a word another workgroup writes).
//  3. resolve       follows every pixel's links to its root (links are read-only here) into `root`; box and area by
//                   integer atomicMin / atomicMax / atomicAdd on the root's words, pre-reduced over each wave's runs of
//                   equal roots along a row; per 4096-pixel chunk, the number of roots of each class.
//  4. class_scan    one workgroup per image: exclusive scan of the chunk counts over chunks, then over classes, giving
//                   each (chunk, class) the index of its first record; the region count of the image.
//  5. emit          one wave per chunk walks it in raster order and ranks the roots of each class by wave ballots from
//                   the chunk's offsets: a counting sort, no order-dependent atomics.  Writes the records (the first
//                   max_regions) and stores every root's full index into its link word.
//  6. labels        (optional) labels[x] = index of root[x], -1 on background.
// All results are integers computed by order-independent operations: bitwise reproducible.
#include "kernels.hpp"

namespace vitseg {
namespace {

constexpr int TILE = 32;              // tile side of the LDS labelling
constexpr int TPIX = TILE * TILE;     // 1024 pixels, 4 per thread of a 256-thread block
constexpr int CHUNK = 4096;           // pixels per chunk of the resolve / emit passes
constexpr int NCLS = 256;

__device__ __forceinline__ int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ int lds_find(int* L, int x) {
    int p = lds_load(&L[x]);
    while (p != x) {
        x = p;
        p = lds_load(&L[x]);
    }
    return x;
}

// union of the components of a and b: the larger root is linked to the smaller; if another thread relinked that root
// meanwhile, atomicMin keeps the smaller link and the merge goes on from the root's new parent
__device__ __forceinline__ void lds_merge(int* L, int a, int b) {
    while (true) {
        a = lds_find(L, a);
        b = lds_find(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[b], a);
        if (old == b) return;
        b = old;
    }
}

// global-memory forms for the seam launch.  A link is read as atomicMin(&L[x], x): links never exceed their own index,
// so the operation changes nothing, but it is a read-modify-write at the memory side whose returned value is used (the
// compiler folds an idempotent atomicOr(p, 0) into a plain L2 load, which another XCD's links need not have reached)
__device__ __forceinline__ int g_link(int* L, int x) { return atomicMin(&L[x], x); }

__device__ __forceinline__ int g_find(int* L, int x) {
    int p = g_link(L, x);
    while (p != x) {
        x = p;
        p = g_link(L, x);
    }
    return x;
}

__device__ __forceinline__ void g_merge(int* L, int a, int b) {
    while (true) {
        a = g_find(L, a);
        b = g_find(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[b], a);
        if (old == b) return;
        b = old;
    }
}

struct Stats {   // per-pixel words; only those at tile roots are initialised and used
    int* xmin;
    int* xmax;
    int* ymax;
    int* area;
};

// class of a pixel for labelling: -1 = background (no region), else the 8-bit value
__device__ __forceinline__ int label_class(unsigned char v, int background) { return (int)v == background ? -1 : (int)v; }

__global__ __launch_bounds__(256) void tile_label_kernel(const unsigned char* __restrict__ mask, int* __restrict__ link,
                                                         Stats st, int H, int W, int ntx, int conn8, int background) {
    __shared__ int L[TPIX];
    __shared__ int cls[TPIX];   // -2 outside the image, -1 background
    const size_t P = (size_t)H * W, base = (size_t)blockIdx.y * P;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int y0 = ty * TILE, x0 = tx * TILE;
    for (int k = 0; k < TPIX / 256; ++k) {
        const int li = threadIdx.x + k * 256, y = y0 + li / TILE, x = x0 + li % TILE;
        cls[li] = (y < H && x < W) ? label_class(mask[base + (size_t)y * W + x], background) : -2;
        L[li] = li;
    }
    __syncthreads();
    for (int k = 0; k < TPIX / 256; ++k) {
        const int li = threadIdx.x + k * 256, ly = li / TILE, lx = li % TILE, c = cls[li];
        if (c < 0) continue;
        if (lx > 0 && cls[li - 1] == c) lds_merge(L, li, li - 1);
        if (ly > 0) {
            if (cls[li - TILE] == c) lds_merge(L, li, li - TILE);
            if (conn8) {
                if (lx > 0 && cls[li - TILE - 1] == c) lds_merge(L, li, li - TILE - 1);
                if (lx < TILE - 1 && cls[li - TILE + 1] == c) lds_merge(L, li, li - TILE + 1);
            }
        }
    }
    __syncthreads();
    for (int k = 0; k < TPIX / 256; ++k) {
        const int li = threadIdx.x + k * 256, y = y0 + li / TILE, x = x0 + li % TILE, c = cls[li];
        if (c == -2) continue;
        const size_t gi = base + (size_t)y * W + x;
        if (c < 0) {
            link[gi] = -1;
            continue;
        }
        const int r = lds_find(L, li);
        link[gi] = (y0 + r / TILE) * W + x0 + r % TILE;
        if (r == li) {
            st.xmin[gi] = W;
            st.xmax[gi] = -1;
            st.ymax[gi] = -1;
            st.area[gi] = 0;
        }
    }
}

// seam pixels of one image: the left column of every tile column but the first ((ntx - 1) * H of them), then the top
// row of every tile row but the first ((nty - 1) * W).  A left-column pixel (y, x) joins (y, x - 1) and, for 8-connectivity,
// (y - 1, x - 1) and (y + 1, x - 1); a top-row pixel (y, x) joins (y - 1, x) and (y - 1, x -/+ 1).  That covers every
// adjacent pair whose pixels lie in different tiles.
__global__ __launch_bounds__(256) void seam_merge_kernel(const unsigned char* __restrict__ mask, int* link, int H, int W,
                                                         int ntx, int nty, int conn8, int background) {
    const long long nv = (long long)(ntx - 1) * H, ns = nv + (long long)(nty - 1) * W;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= ns) return;
    const size_t base = (size_t)blockIdx.y * H * W;
    const unsigned char* m = mask + base;
    int* L = link + base;
    int y, x;
    if (i < nv) {
        y = (int)(i % H);
        x = (int)(i / H + 1) * TILE;
    } else {
        x = (int)((i - nv) % W);
        y = (int)((i - nv) / W + 1) * TILE;
    }
    const int p = y * W + x, c = label_class(m[p], background);
    if (c < 0) return;
    auto join = [&](int yy, int xx) {
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) return;
        const int q = yy * W + xx;
        if (label_class(m[q], background) == c) g_merge(L, p, q);
    };
    if (i < nv) {
        join(y, x - 1);
        if (conn8) {
            join(y - 1, x - 1);
            join(y + 1, x - 1);
        }
    } else {
        join(y - 1, x);
        if (conn8) {
            join(y - 1, x - 1);
            join(y - 1, x + 1);
        }
    }
}

__device__ __forceinline__ void flush_run(const Stats& st, size_t base, int r, int y, int xa, int xb, int cnt) {
    atomicMin(&st.xmin[base + r], xa);
    atomicMax(&st.xmax[base + r], xb);
    atomicMax(&st.ymax[base + r], y);
    atomicAdd(&st.area[base + r], cnt);
}

__global__ __launch_bounds__(256) void resolve_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ link,
                                                      int* __restrict__ root, Stats st, int* __restrict__ chunk_counts,
                                                      int H, int W, int nchunks) {
    __shared__ int hist[NCLS];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int P = H * W, lane = threadIdx.x & (WAVE - 1);
    const size_t base = (size_t)blockIdx.y * P;
    const int* Lk = link + base;
    const unsigned long long upto = (2ull << lane) - 1ull;   // this lane and the ones below it
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long long pl = (long long)blockIdx.x * CHUNK + k * 256 + threadIdx.x;   // a wave: 64 consecutive pixels
        const bool in = pl < P;
        const int p = in ? (int)pl : 0;
        int r = in ? Lk[p] : -1;
        if (r >= 0) {
            for (int q = Lk[r]; q != r; q = Lk[r]) r = q;
            if (r == p) atomicAdd(&hist[mask[base + p]], 1);
        }
        if (in) root[base + p] = r;
        // runs of consecutive lanes with the same root in the same row: the run's first lane updates the root's words
        // once for the whole run (a blob costs a few atomics per wave; a checkerboard one per lane, on 64 adjacent words)
        const int y = p / W, x = p - y * W;
        const int r_prev = __shfl_up(r, 1), y_prev = __shfl_up(y, 1);
        const bool head = r >= 0 && (lane == 0 || r_prev != r || y_prev != y);
        const unsigned long long stops = __ballot(head || r < 0) & ~upto;
        if (head) {
            const int end = stops ? __ffsll((long long)stops) - 1 : WAVE;   // first lane past the run
            flush_run(st, base, r, y, x, x + (end - 1 - lane), end - lane);
        }
    }
    __syncthreads();
    chunk_counts[((size_t)blockIdx.y * nchunks + blockIdx.x) * NCLS + threadIdx.x] = hist[threadIdx.x];
}

// one workgroup per image, thread c = class c: offsets[image][chunk][c] = index of the first record of class c in that
// chunk; counts[image] = regions of the image
__global__ __launch_bounds__(256) void class_scan_kernel(const int* __restrict__ chunk_counts, int* __restrict__ offsets,
                                                         int* __restrict__ counts, int nchunks) {
    __shared__ int s[NCLS];
    const int c = threadIdx.x;
    const size_t b0 = (size_t)blockIdx.x * nchunks * NCLS + c;
    int tot = 0;
    for (int b = 0; b < nchunks; ++b) tot += chunk_counts[b0 + (size_t)b * NCLS];
    s[c] = tot;
    __syncthreads();
    for (int d = 1; d < NCLS; d <<= 1) {   // inclusive scan over classes
        const int v = c >= d ? s[c - d] : 0;
        __syncthreads();
        s[c] += v;
        __syncthreads();
    }
    int run = s[c] - tot;
    if (c == NCLS - 1) counts[blockIdx.x] = s[c];
    for (int b = 0; b < nchunks; ++b) {
        const size_t o = b0 + (size_t)b * NCLS;
        const int v = chunk_counts[o];
        offsets[o] = run;
        run += v;
    }
}

// one wave per chunk: the roots of the chunk in raster order, ranked per class from the chunk's offsets
__global__ __launch_bounds__(64) void emit_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ root,
                                                  int* __restrict__ link, Stats st, const int* __restrict__ offsets,
                                                  int* __restrict__ regions, int max_regions, int H, int W, int nchunks) {
    __shared__ int next[NCLS];
    const size_t oc = ((size_t)blockIdx.y * nchunks + blockIdx.x) * NCLS;
    for (int c = threadIdx.x; c < NCLS; c += 64) next[c] = offsets[oc + c];
    __syncthreads();
    const int P = H * W, lane = threadIdx.x;
    const size_t base = (size_t)blockIdx.y * P;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int end = (int)min((long long)P, (long long)(blockIdx.x + 1) * CHUNK);
    for (long long p0 = (long long)blockIdx.x * CHUNK; p0 < end; p0 += 64) {
        const int p = (int)(p0 + lane);
        bool is_root = false;
        int c = -1;
        if (p0 + lane < end && root[base + p] == p) {
            is_root = true;
            c = mask[base + p];
        }
        unsigned long long pending = __ballot(is_root);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const int cl = __shfl(c, leader);
            const unsigned long long same = __ballot(is_root && c == cl);
            const int start = next[cl];
            if (is_root && c == cl) {
                const int idx = start + __popcll(same & below);
                link[base + p] = idx;
                if (idx < max_regions) {
                    const int y = p / W;
                    int4* rec = reinterpret_cast<int4*>(regions + ((size_t)blockIdx.y * max_regions + idx) * 8);
                    rec[0] = make_int4(c, y, st.xmin[base + p], st.ymax[base + p]);
                    rec[1] = make_int4(st.xmax[base + p], st.area[base + p], p, 0);
                }
            }
            __syncthreads();   // every lane has read next[cl] before it moves
            if (lane == leader) next[cl] = start + __popcll(same);
            __syncthreads();
            pending &= ~same;
        }
    }
}

__global__ __launch_bounds__(256) void labels_kernel(const int* __restrict__ root, const int* __restrict__ link,
                                                     int* __restrict__ labels, int P) {
    const long long pl = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pl >= P) return;
    const int p = (int)pl;
    const size_t base = (size_t)blockIdx.y * P;
    const int r = root[base + p];
    labels[base + p] = r < 0 ? -1 : link[base + r];
}

struct Layout {
    size_t link, root, xmin, xmax, ymax, area, counts, offsets, total;
    int nchunks;
};

Layout layout(int n, int H, int W) {
    Layout l{};
    const size_t N = (size_t)n * H * W;
    l.nchunks = (int)(((size_t)H * W + CHUNK - 1) / CHUNK);
    const size_t px = up256(N * sizeof(int)), cc = up256((size_t)n * l.nchunks * NCLS * sizeof(int));
    l.link = 0;
    l.root = l.link + px;
    l.xmin = l.root + px;
    l.xmax = l.xmin + px;
    l.ymax = l.xmax + px;
    l.area = l.ymax + px;
    l.counts = l.area + px;
    l.offsets = l.counts + cc;
    l.total = l.offsets + cc;
    return l;
}

bool shape_ok(int n, int H, int W) { return n > 0 && H > 0 && W > 0 && n <= 65535 && (long long)H * W < (1ll << 31); }

}  // namespace

size_t regions_scratch_bytes(int n, int H, int W) { return shape_ok(n, H, W) ? layout(n, H, W).total : 0; }

bool regions_shape_ok(int n, int H, int W) { return shape_ok(n, H, W); }

RegionWords region_words(void* scratch, int n, int H, int W) {
    const Layout l = layout(n, H, W);
    char* sc = (char*)scratch;
    return RegionWords{(int*)(sc + l.link), (int*)(sc + l.root), (int*)(sc + l.xmin), (int*)(sc + l.xmax), (int*)(sc + l.ymax),
                       (int*)(sc + l.area), (int*)(sc + l.counts), (int*)(sc + l.offsets), l.nchunks};
}

// launches 1 - 3 of the header: the labelling alone.  Arguments are the caller's to check.
int launch_region_labels(const unsigned char* mask, int n, int H, int W, int connectivity, int background,
                         const RegionWords& w, hipStream_t s) {
    const Stats st{w.xmin, w.xmax, w.ymax, w.area};
    const int ntx = (W + TILE - 1) / TILE, nty = (H + TILE - 1) / TILE, conn8 = connectivity == 8;
    hipLaunchKernelGGL(tile_label_kernel, dim3(ntx * nty, n), dim3(256), 0, s, mask, w.link, st, H, W, ntx, conn8, background);
    VITSEG_LAUNCH_CHECK("regions tile_label");
    const long long seams = (long long)(ntx - 1) * H + (long long)(nty - 1) * W;
    if (seams > 0) {
        hipLaunchKernelGGL(seam_merge_kernel, dim3((unsigned)((seams + 255) / 256), n), dim3(256), 0, s, mask, w.link, H, W, ntx,
                           nty, conn8, background);
        VITSEG_LAUNCH_CHECK("regions seam_merge");
    }
    hipLaunchKernelGGL(resolve_kernel, dim3(w.nchunks, n), dim3(256), 0, s, mask, w.link, w.root, st, w.chunk_counts, H, W,
                       w.nchunks);
    VITSEG_LAUNCH_CHECK("regions resolve");
    return VITSEG_OK;
}

int launch_regions(const unsigned char* mask, int n, int H, int W, int connectivity, int background, int* counts,
                   int* regions, int max_regions, int* labels, void* scratch, size_t scratch_bytes, hipStream_t s) {
    VITSEG_CHECK_ARG(mask && counts && scratch && (regions || max_regions == 0) && max_regions >= 0, VITSEG_EINVAL,
                     "regions: null pointer or negative max_regions");
    VITSEG_CHECK_ARG(connectivity == 4 || connectivity == 8, VITSEG_EINVAL, "regions: connectivity must be 4 or 8, got %d",
                     connectivity);
    VITSEG_CHECK_ARG(background >= -1 && background <= 255, VITSEG_EINVAL, "regions: background must be 0..255 or -1, got %d",
                     background);
    VITSEG_CHECK_ARG(!regions || ((uintptr_t)regions & 15) == 0, VITSEG_EINVAL, "regions: records must be 16-byte aligned");
    VITSEG_CHECK_ARG(shape_ok(n, H, W), VITSEG_ESHAPE, "regions: bad shape n=%d H=%d W=%d (positive sizes, H*W < 2^31, n <= 65535)",
                     n, H, W);
    const size_t need = layout(n, H, W).total;
    VITSEG_CHECK_ARG(scratch_bytes >= need, VITSEG_EWORKSPACE, "regions: scratch of %zu bytes, %zu needed", scratch_bytes, need);
    const RegionWords w = region_words(scratch, n, H, W);
    if (max_regions > 0) {
        hipError_t e = hipMemsetAsync(regions, 0, (size_t)n * max_regions * 8 * sizeof(int), s);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(regions)");
    }
    if (const int rc = launch_region_labels(mask, n, H, W, connectivity, background, w, s)) return rc;
    return launch_region_index(mask, n, H, W, w, counts, regions, max_regions, labels, s);
}

// launches 4 - 6 of the header.  Arguments are the caller's to check.
int launch_region_index(const unsigned char* mask, int n, int H, int W, const RegionWords& w, int* counts, int* regions,
                        int max_regions, int* labels, hipStream_t s) {
    const Stats st{w.xmin, w.xmax, w.ymax, w.area};
    const int P = H * W;
    hipLaunchKernelGGL(class_scan_kernel, dim3(n), dim3(256), 0, s, w.chunk_counts, w.offsets, counts, w.nchunks);
    VITSEG_LAUNCH_CHECK("regions class_scan");
    hipLaunchKernelGGL(emit_kernel, dim3(w.nchunks, n), dim3(64), 0, s, mask, w.root, w.link, st, w.offsets, regions, max_regions,
                       H, W, w.nchunks);
    VITSEG_LAUNCH_CHECK("regions emit");
    if (labels) {
        hipLaunchKernelGGL(labels_kernel, dim3((P + 255) / 256, n), dim3(256), 0, s, w.root, w.link, labels, P);
        VITSEG_LAUNCH_CHECK("regions labels");
    }
    return VITSEG_OK;
}

}  // namespace vitseg

extern "C" {

size_t vitseg_regions_scratch_bytes(int n, int H, int W) { return vitseg::regions_scratch_bytes(n, H, W); }

int vitseg_regions(const uint8_t* mask, int n, int H, int W, int connectivity, int background, int32_t* counts,
                   int32_t* regions, int max_regions, int32_t* labels, void* scratch, size_t scratch_bytes, void* stream) {
    return vitseg::launch_regions(mask, n, H, W, connectivity, background, counts, regions, max_regions, labels, scratch,
                                  scratch_bytes, (hipStream_t)stream);
}

}  // extern "C"
