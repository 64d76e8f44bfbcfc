// Per-region measurements (vitseg_region_props): one int64 row of VITSEG_PROPS_FIELDS words per connected region -- the
// record of vitseg_regions, the raw moments, the perimeter in pixel sides, the frame contact and, for the classes asked for,
// the region's share of its class plane's skeleton and distance field (length, end points, widths).  The usual host answer
// is skimage.measure.regionprops plus a skeleton and a distance transform per label, one image at a time.
//
// Nothing here labels, thins or measures distances: those are the launches of regions.hip, skeleton.hip and sdf.hip.  This
// file is the join, a reduction keyed by region.
//   (labels)  tile_label, seam_merge, resolve, class_scan, emit, labels of regions.hip: counts, every root's index, and the
//             index of every pixel's region (into `labels`, or into the scratch when the caller wants none).
//   rows      one thread per pixel: at a root with index < max_regions it writes fields 0..6 from the root's words and
//             starts fields 14..18: -1 for a class that is not measured, else 0 (17: -1, "no skeleton pixel yet").  props was
//             cleared before, so fields 7..13, 19 and the rows past the count are 0.
//   shape     fields 7..13, one launch for all classes: a wave on 64 consecutive pixels (below).
//   per class c in `classes`:
//     planes    {mask == c} and its complement as byte planes;
//     thin      vitseg_skeleton's launches on {mask == c} (launch_skeleton: resident or global route);
//     d2        launch_sdf_d2 on the complement: the exact squared distance of every class pixel to the nearest pixel outside;
//     measure   fields 14..18: a wave on 64 consecutive pixels, keyed by the region index where mask == c.
// The two accumulation kernels are the hot path.  A global atomic per pixel and field would be 10^8 atomics at 32 x 512^2, all
// on one row when one region fills the frame, so they are pre-reduced twice:
//   1. within a wave, the lanes of one image row that form a run of equal region index are reduced at the run's first lane:
//      the coordinate sums are closed forms of the run's ends (an arithmetic series and a difference of square pyramidal
//      numbers), the counts are popcounts of ballots masked to the run, and the maxima and the fixed-point width sum go
//      through a segmented shuffle reduction bounded by the run's end (ballot of "index or row differs from the lane before");
//   2. within a workgroup (a 4096-pixel chunk), the runs of ONE region -- the one found at the chunk's first pixel, else at
//      its middle pixel -- add into LDS and reach the row as one atomic per field and workgroup.  A region large enough to
//      make a hot row covers most of the chunks it touches, so its atomics fall from one per wave and field to one per
//      workgroup and field; small regions have few runs and go to their rows directly.
// All sums are 64-bit integer atomicAdd / atomicMax: order-independent, so the bits do not depend on which region a chunk
// picks, on the schedule, on the route or on the batch.  Products are formed in 64 bits before they are added.
#include "kernels.hpp"
#include "run_reduce.hpp"

namespace vitseg {
namespace {

constexpr int CHUNK = 4096;   // pixels per workgroup of the accumulation passes
constexpr int NF = VITSEG_PROPS_FIELDS;
constexpr int PROPS_MAX_SIDE = 16384, PROPS_MAX_BATCH = 32767;
enum { F_CLASS, F_FIRST, F_AREA, F_YMIN, F_XMIN, F_YMAX, F_XMAX, F_SY, F_SX, F_SYY, F_SXX, F_SXY, F_PERIM, F_FRAME, F_MAXD2,
       F_SKEL, F_ENDS, F_SKELMAX, F_WIDTH };

struct ClassSet {   // bit c of the 256: class c is measured
    unsigned bits[8];
    __host__ __device__ bool has(int c) const { return (bits[c >> 5] >> (c & 31)) & 1u; }
};

// (the runs of equal region index within a wave, find_run / run_reduce: run_reduce.hpp, shared with confidence.hip)

// the region whose runs a workgroup collects in LDS: the one at the chunk's first pixel, else at its middle pixel; -1 when
// neither has one (or its row is not written).  cls >= 0: only a region of that class.
__device__ __forceinline__ int chunk_key(const unsigned char* __restrict__ m, const int* __restrict__ lab, int P, int cls,
                                         int max_regions) {
    const long long p0 = (long long)blockIdx.x * CHUNK;
    const long long p1 = p0 + CHUNK / 2 < P ? p0 + CHUNK / 2 : p0;
    int k = (cls < 0 || m[p0] == cls) ? lab[p0] : -1;
    if (k < 0) k = (cls < 0 || m[p1] == cls) ? lab[p1] : -1;
    return k < max_regions ? k : -1;
}

// grid (ceil(P / 256), n): the rows' record fields and the start values of fields 14..18
__global__ __launch_bounds__(256) void props_rows_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ root,
                                                         const int* __restrict__ link, const int* __restrict__ xmin,
                                                         const int* __restrict__ xmax, const int* __restrict__ ymax,
                                                         const int* __restrict__ area, i64* __restrict__ props,
                                                         int max_regions, int P, int W, ClassSet measured) {
    const long long pl = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pl >= P) return;
    const int p = (int)pl;
    const size_t g = (size_t)blockIdx.y * P + p;
    if (root[g] != p) return;
    const int idx = link[g];
    if (idx >= max_regions) return;
    const int c = mask[g];
    i64* row = props + ((size_t)blockIdx.y * max_regions + idx) * NF;
    row[F_CLASS] = c;
    row[F_FIRST] = p;
    row[F_AREA] = area[g];
    row[F_YMIN] = p / W;
    row[F_XMIN] = xmin[g];
    row[F_YMAX] = ymax[g];
    row[F_XMAX] = xmax[g];
    const bool on = measured.has(c);
    row[F_MAXD2] = on ? 0 : -1;
    row[F_SKEL] = on ? 0 : -1;
    row[F_ENDS] = on ? 0 : -1;
    row[F_SKELMAX] = -1;
    row[F_WIDTH] = on ? 0 : -1;
}

__device__ __forceinline__ i64 pyramid(i64 m) { return m * (m + 1) * (2 * m + 1) / 6; }   // 0^2 + ... + m^2; 0 for m = -1

// grid (ceil(P / CHUNK), n): fields 7..13 of every region
__global__ __launch_bounds__(256) void props_shape_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ labels,
                                                          i64* __restrict__ props, int max_regions, int H, int W) {
    constexpr int NA = 7;   // F_SY .. F_FRAME
    __shared__ u64 acc[NA];
    __shared__ int key_s;
    const int P = H * W, lane = threadIdx.x & (WAVE - 1);
    const unsigned char* m = mask + (size_t)blockIdx.y * P;
    const int* lab = labels + (size_t)blockIdx.y * P;
    i64* rows = props + (size_t)blockIdx.y * max_regions * NF;
    if (threadIdx.x < NA) acc[threadIdx.x] = 0;
    if (threadIdx.x == 0) key_s = chunk_key(m, lab, P, -1, max_regions);
    __syncthreads();
    const int key = key_s;
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long long pl = (long long)blockIdx.x * CHUNK + k * 256 + threadIdx.x;   // a wave: 64 consecutive pixels
        const bool in = pl < P;
        const int p = in ? (int)pl : 0;
        const int idx = in ? lab[p] : -1;
        const int y = p / W, x = p - y * W;
        int sides = 0, frame = 0;
        if (idx >= 0) {
            const unsigned char v = m[p];
            sides = (y == 0 || m[p - W] != v) + (y == H - 1 || m[p + W] != v) + (x == 0 || m[p - 1] != v) +
                    (x == W - 1 || m[p + 1] != v);
            frame = y == 0 || y == H - 1 || x == 0 || x == W - 1;
        }
        const Run r = find_run(idx, y, lane);
        const u64 s1 = __ballot(sides & 1), s2 = __ballot(sides & 2), s4 = __ballot(sides & 4), fr = __ballot(frame);
        if (!r.head || idx >= max_regions) continue;
        const i64 L = r.end - lane, xa = x, xb = x + L - 1;
        const i64 sx = L * (xa + xb) / 2, sxx = pyramid(xb) - pyramid(xa - 1);
        const u64 v[NA] = {(u64)(L * y),
                           (u64)sx,
                           (u64)(L * y * y),
                           (u64)sxx,
                           (u64)(sx * y),
                           (u64)(__popcll(s1 & r.members) + 2 * __popcll(s2 & r.members) + 4 * __popcll(s4 & r.members)),
                           (u64)__popcll(fr & r.members)};
        u64* dst = idx == key ? acc : (u64*)(rows + (size_t)idx * NF + F_SY);
#pragma unroll
        for (int f = 0; f < NA; ++f)
            if (v[f]) atomicAdd(&dst[f], v[f]);
    }
    __syncthreads();
    if (key >= 0 && threadIdx.x < NA && acc[threadIdx.x])
        atomicAdd((u64*)(rows + (size_t)key * NF + F_SY) + threadIdx.x, acc[threadIdx.x]);
}

// grid (ceil(n P / 1024)): {mask == c} and its complement as byte planes
__global__ __launch_bounds__(256) void props_planes_kernel(const unsigned char* __restrict__ mask, unsigned char* __restrict__ ind,
                                                           unsigned char* __restrict__ comp, size_t N, int c) {
    for (int k = 0; k < 4; ++k) {
        const size_t i = (size_t)blockIdx.x * 1024 + k * 256 + threadIdx.x;
        if (i >= N) return;
        const bool a = mask[i] == c;
        ind[i] = a;
        comp[i] = !a;
    }
}

// grid (ceil(P / CHUNK), n): fields 14..18 of the regions of class c
__global__ __launch_bounds__(256) void props_class_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ labels,
                                                          const unsigned char* __restrict__ skel, const int* __restrict__ d2,
                                                          i64* __restrict__ props, int max_regions, int H, int W, int c) {
    __shared__ i64 acc[5];   // F_MAXD2 .. F_WIDTH
    __shared__ int key_s;
    const int P = H * W, lane = threadIdx.x & (WAVE - 1);
    const unsigned char* m = mask + (size_t)blockIdx.y * P;
    const int* lab = labels + (size_t)blockIdx.y * P;
    const unsigned char* sk = skel + (size_t)blockIdx.y * P;
    const int* fld = d2 + (size_t)blockIdx.y * P;
    i64* rows = props + (size_t)blockIdx.y * max_regions * NF;
    if (threadIdx.x < 5) acc[threadIdx.x] = (threadIdx.x == 0 || threadIdx.x == 3) ? -1 : 0;
    if (threadIdx.x == 0) key_s = chunk_key(m, lab, P, c, max_regions);
    __syncthreads();
    const int key = key_s;
    auto imax = [](int a, int b) { return a > b ? a : b; };
    auto ladd = [](i64 a, i64 b) { return a + b; };
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long long pl = (long long)blockIdx.x * CHUNK + k * 256 + threadIdx.x;   // a wave: 64 consecutive pixels
        const bool in = pl < P;
        const int p = in ? (int)pl : 0;
        const int idx = (in && m[p] == c) ? lab[p] : -1;
        const int y = p / W, x = p - y * W;
        int v = -1, sv = -1, is_skel = 0, is_end = 0;
        i64 q = 0;
        if (idx >= 0) {
            v = fld[p];
            if (sk[p]) {
                is_skel = 1;
                sv = v;
                q = llrint(sqrt((double)v) * 65536.0);
                int nb = 0;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx)
                        if ((dy || dx) && y + dy >= 0 && y + dy < H && x + dx >= 0 && x + dx < W) nb += sk[p + dy * W + dx] != 0;
                is_end = nb == 1;
            }
        }
        const Run r = find_run(idx, y, lane);
        const u64 sb = __ballot(is_skel), eb = __ballot(is_end);
        const int vmax = run_reduce(v, lane, r.end, imax);
        int smax = -1;
        i64 qsum = 0;
        if (sb) {   // the same for the whole wave
            smax = run_reduce(sv, lane, r.end, imax);
            qsum = run_reduce(q, lane, r.end, ladd);
        }
        if (!r.head || idx >= max_regions) continue;
        const i64 cnt = __popcll(sb & r.members), ends = __popcll(eb & r.members);
        i64* dst = idx == key ? acc : rows + (size_t)idx * NF + F_MAXD2;
        atomicMax(&dst[0], (i64)vmax);
        if (cnt) {
            atomicAdd((u64*)&dst[1], (u64)cnt);
            if (ends) atomicAdd((u64*)&dst[2], (u64)ends);
            atomicMax(&dst[3], (i64)smax);
            atomicAdd((u64*)&dst[4], (u64)qsum);
        }
    }
    __syncthreads();
    if (key < 0 || threadIdx.x >= 5) return;
    i64* dst = rows + (size_t)key * NF + F_MAXD2;
    const i64 a = acc[threadIdx.x];
    if (threadIdx.x == 0 || threadIdx.x == 3) {
        if (a >= 0) atomicMax(&dst[threadIdx.x], a);
    } else if (a) {
        atomicAdd((u64*)&dst[threadIdx.x], (u64)a);
    }
}

bool shape_ok(int n, int H, int W, int K) {
    return n >= 1 && n <= PROPS_MAX_BATCH && H >= 1 && H <= PROPS_MAX_SIDE && W >= 1 && W <= PROPS_MAX_SIDE && K >= 0 && K <= 256;
}

struct Layout {   // the labelling's scratch, the labels, and with K > 0 the planes of one class and the thinning's scratch
    size_t labels, ind, comp, skel, d2, maxw, thin, thin_bytes, total;
};

// thin_bytes == 0 with K > 0: the plane does not fit the route asked for
Layout layout(int n, int H, int W, int K, int route) {
    Layout l{};
    const size_t N = (size_t)n * H * W;
    size_t o = up256(regions_scratch_bytes(n, H, W));
    l.labels = o;  o += up256(N * sizeof(int));
    if (K > 0) {
        l.ind = o;   o += up256(N);
        l.comp = o;  o += up256(N);
        l.skel = o;  o += up256(N);
        l.d2 = o;    o += up256(N * sizeof(int));
        l.maxw = o;  o += up256((size_t)n * 2 * sizeof(int));
        l.thin = o;
        l.thin_bytes = skeleton_scratch_bytes(n, H, W, route);
        o += up256(l.thin_bytes);
    }
    l.total = o;
    return l;
}

}  // namespace

size_t region_props_scratch_bytes(int n, int H, int W, int K, int route) {
    if (!shape_ok(n, H, W, K) || route < 0 || route > 2) return 0;
    const Layout l = layout(n, H, W, K, route);
    return (K > 0 && l.thin_bytes == 0) ? 0 : l.total;
}

int launch_region_props(const unsigned char* mask, int n, int H, int W, int connectivity, int background, const int* classes,
                        int K, int route, int* counts, long long* props, int max_regions, int* labels, void* scratch,
                        size_t scratch_bytes, hipStream_t s) {
    VITSEG_CHECK_ARG(mask && counts && scratch && (props || max_regions == 0) && max_regions >= 0, VITSEG_EINVAL,
                     "region_props: null pointer or negative max_regions");
    VITSEG_CHECK_ARG(connectivity == 4 || connectivity == 8, VITSEG_EINVAL, "region_props: connectivity must be 4 or 8, got %d",
                     connectivity);
    VITSEG_CHECK_ARG(background >= -1 && background <= 255, VITSEG_EINVAL,
                     "region_props: background must be 0..255 or -1, got %d", background);
    VITSEG_CHECK_ARG(route >= 0 && route <= 2, VITSEG_EINVAL,
                     "region_props: route must be 0 (automatic), 1 (resident) or 2 (global), got %d", route);
    VITSEG_CHECK_ARG(classes || K <= 0, VITSEG_EINVAL, "region_props: null classes with K = %d", K);
    VITSEG_CHECK_ARG(shape_ok(n, H, W, K), VITSEG_ESHAPE,
                     "region_props: bad shape n=%d H=%d W=%d K=%d (1 <= H, W <= %d, 1 <= n <= %d, 0 <= K <= 256)", n, H, W, K,
                     PROPS_MAX_SIDE, PROPS_MAX_BATCH);
    ClassSet measured{};
    for (int k = 0; k < K; ++k) {
        const int c = classes[k];
        VITSEG_CHECK_ARG(c >= 0 && c <= 255 && c != background && !measured.has(c), VITSEG_EINVAL,
                         "region_props: classes[%d] = %d is outside 0..255, the background or repeated", k, c);
        measured.bits[c >> 5] |= 1u << (c & 31);
    }
    const Layout l = layout(n, H, W, K, route);
    VITSEG_CHECK_ARG(K == 0 || l.thin_bytes != 0, VITSEG_ESHAPE,
                     "region_props: a %d x %d plane does not fit the resident route of the skeleton", H, W);
    VITSEG_CHECK_ARG(scratch_bytes >= l.total, VITSEG_EWORKSPACE, "region_props: scratch of %zu bytes, %zu needed", scratch_bytes,
                     l.total);
    char* base = (char*)scratch;
    const RegionWords w = region_words(scratch, n, H, W);
    int* lab = labels ? labels : (int*)(base + l.labels);
    const int P = H * W;
    const size_t N = (size_t)n * P;
    if (max_regions > 0) {
        const hipError_t e = hipMemsetAsync(props, 0, (size_t)n * max_regions * NF * sizeof(long long), s);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(region_props rows)");
    }
    if (const int rc = launch_region_labels(mask, n, H, W, connectivity, background, w, s)) return rc;
    if (const int rc = launch_region_index(mask, n, H, W, w, counts, nullptr, 0, lab, s)) return rc;
    if (max_regions == 0) return VITSEG_OK;
    hipLaunchKernelGGL(props_rows_kernel, dim3((P + 255) / 256, n), dim3(256), 0, s, mask, w.root, w.link, w.xmin, w.xmax, w.ymax,
                       w.area, props, max_regions, P, W, measured);
    VITSEG_LAUNCH_CHECK("region_props rows");
    const dim3 chunks((unsigned)(((long long)P + CHUNK - 1) / CHUNK), n);
    hipLaunchKernelGGL(props_shape_kernel, chunks, dim3(256), 0, s, mask, lab, props, max_regions, H, W);
    VITSEG_LAUNCH_CHECK("region_props shape");
    unsigned char* ind = (unsigned char*)(base + l.ind);
    unsigned char* comp = (unsigned char*)(base + l.comp);
    unsigned char* skel = (unsigned char*)(base + l.skel);
    int* d2 = (int*)(base + l.d2);
    int* maxw = (int*)(base + l.maxw);
    for (int k = 0; k < K; ++k) {
        const int c = classes[k];
        const hipError_t e = hipMemsetAsync(maxw, 0, (size_t)n * 2 * sizeof(int), s);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(region_props maxima)");
        hipLaunchKernelGGL(props_planes_kernel, dim3((unsigned)((N + 1023) / 1024)), dim3(256), 0, s, mask, ind, comp, N, c);
        VITSEG_LAUNCH_CHECK("region_props planes");
        int rc = launch_skeleton(ind, n, H, W, route, skel, nullptr, base + l.thin, l.thin_bytes, s);
        if (rc != VITSEG_OK) return rc;
        rc = launch_sdf_d2(comp, n, H, W, d2, maxw, s);
        if (rc != VITSEG_OK) return rc;
        hipLaunchKernelGGL(props_class_kernel, chunks, dim3(256), 0, s, mask, lab, skel, d2, props, max_regions, H, W, c);
        VITSEG_LAUNCH_CHECK("region_props measure");
    }
    return VITSEG_OK;
}

}  // namespace vitseg

extern "C" {

size_t vitseg_region_props_scratch_bytes(int n, int H, int W, int K, int route) {
    return vitseg::region_props_scratch_bytes(n, H, W, K, route);
}

int vitseg_region_props(const uint8_t* mask, int n, int H, int W, int connectivity, int background, const int32_t* classes,
                        int K, int route, int32_t* counts, int64_t* props, int max_regions, int32_t* labels, void* scratch,
                        size_t scratch_bytes, void* stream) {
    return vitseg::launch_region_props(mask, n, H, W, connectivity, background, classes, K, route, counts, (long long*)props,
                                       max_regions, labels, scratch, scratch_bytes, (hipStream_t)stream);
}

}  // extern "C"
