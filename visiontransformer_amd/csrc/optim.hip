// The fine-tuning optimiser (include/vitseg_optim.h): Adam / AdamW over the parameter arena with parameter groups by 64-float
// chunk, global-norm clipping, a skipped step on a non-finite norm and a weight EMA.  Two or three launches per step on one
// stream: per-block partial sums of the squared gradient (a fixed pairwise tree, plain stores), one block that turns them
// into the step's scalars and the per-group rows, and one pass over the arena with adam_kernel's arithmetic (backward.hip),
// element for element.  No atomics, no block waits for another, the host reads nothing.
#include <math.h>

#include "common.hpp"
#include "../../include/vitseg_optim.h"

namespace vitseg {
namespace {

struct OptimState {   // VITSEG_OPTIM_STATE_BYTES, the words of the header
    int step, skipped;
    float norm, coef, bc1, rbc2;
    int applied, reserved;
};
static_assert(sizeof(OptimState) == VITSEG_OPTIM_STATE_BYTES, "state layout");

constexpr int PART4 = VITSEG_OPTIM_PARTIAL / 4;   // 16-byte pieces per partial: 8 per thread of a 256-thread block
constexpr int PIECES = PART4 / 256;
static_assert(PIECES == 8, "the tree below is written for 8 pieces per thread");

struct Layout {
    size_t n_part, rows, total;   // partials at 0; byte offset of the group rows; bytes in all
};
inline Layout layout(size_t n_floats) {
    Layout l;
    l.n_part = (n_floats + VITSEG_OPTIM_PARTIAL - 1) / VITSEG_OPTIM_PARTIAL;
    l.rows = up256(l.n_part * sizeof(float));
    l.total = l.rows + VITSEG_OPTIM_MAX_GROUPS * sizeof(f32x4);
    return l;
}
inline bool arena_ok(size_t n_floats, int n_groups) {
    return n_floats > 0 && n_floats % VITSEG_OPTIM_CHUNK == 0 && n_groups >= 1 && n_groups <= VITSEG_OPTIM_MAX_GROUPS;
}

// partial[b] = sum of (gs * g)^2 over the floats [b * 8192, (b + 1) * 8192) that lie inside the arena and outside frozen
// chunks.  Pairwise throughout: the 4 squares of a piece, a thread's 8 pieces, the 64 lanes of a wave (wave_sum's DPP tree),
// the 4 waves -- 13 levels of additions for 8192 values, always in the same order.
__global__ __launch_bounds__(256) void optim_norm_kernel(const float* __restrict__ g, size_t n4,
                                                         const uint8_t* __restrict__ map, const float* __restrict__ table,
                                                         int n_groups, float gs, float* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ float wsum[4];
    const size_t base = (size_t)blockIdx.x * PART4 + threadIdx.x;
    // Loads are never conditional per lane (eight stay in flight): a wave with a live piece reads, for a lane's dead piece,
    // the arena's first 16 bytes instead and drops them; a wave with no live piece reads nothing.
    f32x4 x[PIECES];
    int grp[PIECES];
    float lr_mult[PIECES];
    bool live[PIECES], any = false;
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {   // clamped, so that the 8 lookups do not wait for each other
        const size_t i = base + (size_t)j * 256;
        grp[j] = map[i < n4 ? i >> 4 : (size_t)0];
    }
#pragma unroll
    for (int j = 0; j < PIECES; ++j) lr_mult[j] = table[2 * (grp[j] < n_groups ? grp[j] : 0)];
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
        live[j] = lr_mult[j] > 0.f && grp[j] < n_groups && base + (size_t)j * 256 < n4;
        any = any || live[j];
        x[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (__any(any)) {
#pragma unroll
        for (int j = 0; j < PIECES; ++j)
            x[j] = __builtin_nontemporal_load((const f32x4*)g + (live[j] ? base + (size_t)j * 256 : (size_t)0));
#pragma unroll
        for (int j = 0; j < PIECES; ++j)
            if (!live[j]) x[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float s[PIECES];
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
        const f32x4 y = x[j] * gs;
        s[j] = (y[0] * y[0] + y[1] * y[1]) + (y[2] * y[2] + y[3] * y[3]);
    }
    float t = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    t = wave_sum(t);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// One block.  Thread t sums the partials t, t + 256, ... in fp64, thread 0 adds the 256 sums in index order and decides the
// step; then thread r writes the row of group r (all 256 rows are written: a chunk byte can name any of them).
__global__ __launch_bounds__(256) void optim_prepare_kernel(OptimState* __restrict__ st, const float* __restrict__ table,
                                                            int n_groups, const float* __restrict__ partial, size_t n_part,
                                                            int flags, float lr, float b1, float b2, float wd, float max_norm,
                                                            f32x4* __restrict__ rows) {
    __shared__ double acc[256];
    __shared__ double s_bc1;
    __shared__ int s_applied;
    const int tid = threadIdx.x;
    double a = 0.0;
    if (flags & VITSEG_OPTIM_NORM)
        for (size_t i = tid; i < n_part; i += 256) a += (double)partial[i];
    acc[tid] = a;
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int t = 0; t < 256; ++t) total += acc[t];
        const float norm = (flags & VITSEG_OPTIM_NORM) ? (float)sqrt(total) : 0.f;
        float coef = 1.f;
        if (flags & VITSEG_OPTIM_CLIP) {
            const float c = max_norm / (norm + 1e-6f);   // clip_grad_norm_: a NaN norm stays a NaN coefficient
            coef = c > 1.f ? 1.f : c;
        }
        const bool finite = fabsf(norm) <= 3.402823466e38f;   // false for inf and NaN
        st->norm = norm;
        if ((flags & VITSEG_OPTIM_SKIP) && !finite) {
            st->skipped += 1;
            st->coef = 0.f;
            st->applied = 0;
            s_applied = 0;
            s_bc1 = 1.0;
        } else {
            const int step = st->step + 1;
            const double bc1 = 1.0 - pow((double)b1, (double)step), bc2 = 1.0 - pow((double)b2, (double)step);
            st->step = step;
            st->coef = coef;
            st->bc1 = (float)bc1;
            st->rbc2 = (float)(1.0 / sqrt(bc2));
            st->applied = 1;
            s_applied = 1;
            s_bc1 = bc1;
        }
    }
    __syncthreads();
    f32x4 row = {0.f, 0.f, 0.f, 0.f};
    if (tid < n_groups && s_applied) {
        const double lm = (double)table[2 * tid], wm = (double)table[2 * tid + 1];
        if (lm > 0.0) {
            row[0] = (float)((double)lr * lm / s_bc1);
            row[1] = (float)(1.0 - (double)lr * lm * (double)wd * wm);
            row[2] = 1.f;
        }
    }
    rows[tid] = row;
}

// adam_kernel's arithmetic on one 16-byte piece, operation for operation
template <bool EMA>
__device__ __forceinline__ void adam_piece(f32x4& pv, const f32x4& gv, f32x4& mv, f32x4& vv, f32x4& ev, float step_size, float decay,
                                           float b1, float b2, float eps, float gscale, float inv_bc2_sqrt, float d, float omd) {
#pragma clang fp contract(off)   // p.mul_(decay) is rounded before the update is subtracted, as torch does it
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float gr = gv[e] * gscale;
        mv[e] = mv[e] + (gr - mv[e]) * (1.0f - b1);
        vv[e] = vv[e] * b2 + (1.0f - b2) * gr * gr;
        const float denom = sqrtf(vv[e]) * inv_bc2_sqrt + eps;
        pv[e] = pv[e] * decay - step_size * (mv[e] / denom);
        if (EMA) ev[e] = d * ev[e] + omd * pv[e];
    }
}

// adam_kernel (backward.hip) with the step's scalars read from the state and the group's row read through the chunk byte.
// Two 16-byte pieces of each stream per thread and trip, g / m / v (and the EMA) non-temporal.  Whether a piece is loaded at
// all hangs on its row, so the rows of a trip are fetched one trip ahead and its chunk bytes two trips ahead: no load of a
// trip waits for another load of the same trip.
template <bool EMA>
__global__ __launch_bounds__(256) void optim_step_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v, float* __restrict__ ema,
                                                         size_t n4, const uint8_t* __restrict__ map,
                                                         const OptimState* __restrict__ st, const f32x4* __restrict__ rows,
                                                         float b1, float b2, float eps, float grad_scale, float d, float omd) {
    if (!st->applied) return;    // a skipped step stores nothing
    const float gscale = grad_scale * st->coef, inv_bc2_sqrt = st->rbc2;
    const size_t stride = (size_t)gridDim.x * 256, last_chunk = (n4 >> 4) - 1;
    size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    f32x4 row[2];
    unsigned next_grp[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const size_t c0 = (i0 + u * stride) >> 4, c1 = (i0 + (2 + u) * stride) >> 4;
        row[u] = rows[map[c0 < last_chunk ? c0 : last_chunk]];
        next_grp[u] = map[c1 < last_chunk ? c1 : last_chunk];
    }
    for (; i0 < n4; i0 += 2 * stride) {
        f32x4 next_row[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const size_t c2 = (i0 + (4 + u) * stride) >> 4;
            next_row[u] = rows[next_grp[u]];
            next_grp[u] = map[c2 < last_chunk ? c2 : last_chunk];
        }
        const bool live0 = row[0][2] != 0.f, live1 = i0 + stride < n4 && row[1][2] != 0.f;
        if (__all(live0 && live1)) {
            // every lane of the wave updates both pieces: adam_kernel's trip, eight (ten) loads in flight
            f32x4 pv[2], gv[2], mv[2], vv[2], ev[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const size_t i = i0 + u * stride;
                pv[u] = ((f32x4*)p)[i];
                gv[u] = __builtin_nontemporal_load((const f32x4*)g + i);
                mv[u] = __builtin_nontemporal_load((f32x4*)m + i);
                vv[u] = __builtin_nontemporal_load((f32x4*)v + i);
                if (EMA) ev[u] = __builtin_nontemporal_load((f32x4*)ema + i);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const size_t i = i0 + u * stride;
                adam_piece<EMA>(pv[u], gv[u], mv[u], vv[u], ev[u], row[u][0], row[u][1], b1, b2, eps, gscale, inv_bc2_sqrt, d, omd);
                ((f32x4*)p)[i] = pv[u];
                __builtin_nontemporal_store(mv[u], (f32x4*)m + i);
                __builtin_nontemporal_store(vv[u], (f32x4*)v + i);
                if (EMA) __builtin_nontemporal_store(ev[u], (f32x4*)ema + i);
            }
        } else {
            // a wave that meets a frozen chunk or the end of the arena: piece by piece, a frozen one untouched
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const size_t i = i0 + u * stride;
                if (!(u ? live1 : live0)) continue;
                f32x4 pv = ((f32x4*)p)[i], ev = {0.f, 0.f, 0.f, 0.f};
                const f32x4 gv = __builtin_nontemporal_load((const f32x4*)g + i);
                f32x4 mv = __builtin_nontemporal_load((f32x4*)m + i);
                f32x4 vv = __builtin_nontemporal_load((f32x4*)v + i);
                if (EMA) ev = __builtin_nontemporal_load((f32x4*)ema + i);
                adam_piece<EMA>(pv, gv, mv, vv, ev, row[u][0], row[u][1], b1, b2, eps, gscale, inv_bc2_sqrt, d, omd);
                ((f32x4*)p)[i] = pv;
                __builtin_nontemporal_store(mv, (f32x4*)m + i);
                __builtin_nontemporal_store(vv, (f32x4*)v + i);
                if (EMA) __builtin_nontemporal_store(ev, (f32x4*)ema + i);
            }
        }
        row[0] = next_row[0];
        row[1] = next_row[1];
    }
}

inline int step_grid(size_t n4) { return (int)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096); }   // adam_kernel's

}  // namespace
}  // namespace vitseg

extern "C" {

using namespace vitseg;

int vitseg_optim_version(void) { return VITSEG_OPTIM_VERSION; }

size_t vitseg_optim_scratch_bytes(size_t n_floats, int n_groups) {
    return arena_ok(n_floats, n_groups) ? layout(n_floats).total : 0;
}

int vitseg_optim_check_groups(const float* table_host, int n_groups, const uint8_t* chunk_group_host, size_t n_chunks) {
    VITSEG_CHECK_ARG(table_host, VITSEG_EINVAL, "optim_check_groups: null table");
    VITSEG_CHECK_ARG(n_groups >= 1 && n_groups <= VITSEG_OPTIM_MAX_GROUPS, VITSEG_EINVAL,
                     "optim_check_groups: n_groups %d outside 1..256", n_groups);
    for (int r = 0; r < n_groups; ++r)
        for (int c = 0; c < 2; ++c) {
            const float x = table_host[2 * r + c];
            VITSEG_CHECK_ARG(x >= 0.f && x <= 3.402823466e38f, VITSEG_EINVAL,
                             "optim_check_groups: group %d has %s %g (it must be finite and >= 0)", r, c ? "wd_mult" : "lr_mult",
                             (double)x);
        }
    for (size_t i = 0; chunk_group_host && i < n_chunks; ++i)
        VITSEG_CHECK_ARG(chunk_group_host[i] < n_groups, VITSEG_EINVAL, "optim_check_groups: chunk %zu names group %d of %d", i,
                         (int)chunk_group_host[i], n_groups);
    return VITSEG_OK;
}

int vitseg_optim_grad_norm(const float* grads, size_t n_floats, const uint8_t* chunk_group, const float* table, int n_groups,
                           float grad_scale, void* scratch, size_t scratch_bytes, void* stream) {
    VITSEG_CHECK_ARG(grads && chunk_group && table && scratch, VITSEG_EINVAL, "optim_grad_norm: null pointer");
    VITSEG_CHECK_ARG(arena_ok(n_floats, n_groups), VITSEG_EINVAL,
                     "optim_grad_norm: n_floats %zu (a positive multiple of 64) or n_groups %d (1..256)", n_floats, n_groups);
    const Layout l = layout(n_floats);
    VITSEG_CHECK_ARG(scratch_bytes >= l.total, VITSEG_EWORKSPACE, "optim_grad_norm: scratch of %zu bytes, %zu needed", scratch_bytes,
                     l.total);
    VITSEG_CHECK_ARG(l.n_part <= 0x7fffffffu, VITSEG_EINVAL, "optim_grad_norm: n_floats %zu is too large", n_floats);
    hipLaunchKernelGGL(optim_norm_kernel, dim3((unsigned)l.n_part), dim3(256), 0, (hipStream_t)stream, grads, n_floats / 4,
                       chunk_group, table, n_groups, grad_scale, (float*)scratch);
    VITSEG_LAUNCH_CHECK("optim_grad_norm");
    return VITSEG_OK;
}

int vitseg_optim_prepare(void* state, const float* table, int n_groups, size_t n_floats, int flags, float lr, float beta1,
                         float beta2, float weight_decay, float max_norm, void* scratch, size_t scratch_bytes, void* stream) {
    VITSEG_CHECK_ARG(state && table && scratch, VITSEG_EINVAL, "optim_prepare: null pointer");
    VITSEG_CHECK_ARG(arena_ok(n_floats, n_groups), VITSEG_EINVAL,
                     "optim_prepare: n_floats %zu (a positive multiple of 64) or n_groups %d (1..256)", n_floats, n_groups);
    VITSEG_CHECK_ARG(flags >= 0 && flags <= 7 && ((flags & VITSEG_OPTIM_NORM) || flags == 0), VITSEG_EINVAL,
                     "optim_prepare: flags %d (clipping and skipping need the norm)", flags);
    VITSEG_CHECK_ARG(lr >= 0.f && weight_decay >= 0.f, VITSEG_EINVAL, "optim_prepare: lr %g or weight_decay %g is negative",
                     (double)lr, (double)weight_decay);
    VITSEG_CHECK_ARG(!(flags & VITSEG_OPTIM_CLIP) || max_norm > 0.f, VITSEG_EINVAL, "optim_prepare: max_norm %g must be positive",
                     (double)max_norm);
    VITSEG_CHECK_ARG(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, VITSEG_EINVAL,
                     "optim_prepare: betas (%g, %g) outside [0, 1)", (double)beta1, (double)beta2);
    const Layout l = layout(n_floats);
    VITSEG_CHECK_ARG(scratch_bytes >= l.total, VITSEG_EWORKSPACE, "optim_prepare: scratch of %zu bytes, %zu needed", scratch_bytes,
                     l.total);
    hipLaunchKernelGGL(optim_prepare_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (OptimState*)state, table, n_groups,
                       (const float*)scratch, l.n_part, flags, lr, beta1, beta2, weight_decay, max_norm,
                       (f32x4*)((char*)scratch + l.rows));
    VITSEG_LAUNCH_CHECK("optim_prepare");
    return VITSEG_OK;
}

int vitseg_optim_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, size_t n_floats,
                      const uint8_t* chunk_group, const void* state, float beta1, float beta2, float eps, float grad_scale,
                      float ema_decay, const void* scratch, size_t scratch_bytes, void* stream) {
    VITSEG_CHECK_ARG(params && grads && exp_avg && exp_avg_sq && chunk_group && state && scratch, VITSEG_EINVAL,
                     "optim_step: null pointer");
    VITSEG_CHECK_ARG(arena_ok(n_floats, 1), VITSEG_EINVAL, "optim_step: n_floats %zu must be a positive multiple of 64", n_floats);
    VITSEG_CHECK_ARG(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f, VITSEG_EINVAL,
                     "optim_step: betas (%g, %g) outside [0, 1) or eps %g negative", (double)beta1, (double)beta2, (double)eps);
    VITSEG_CHECK_ARG(!ema || (ema_decay >= 0.f && ema_decay < 1.f), VITSEG_EINVAL, "optim_step: ema_decay %g outside [0, 1)",
                     (double)ema_decay);
    const Layout l = layout(n_floats);
    VITSEG_CHECK_ARG(scratch_bytes >= l.total, VITSEG_EWORKSPACE, "optim_step: scratch of %zu bytes, %zu needed", scratch_bytes,
                     l.total);
    const size_t n4 = n_floats / 4;
    const f32x4* rows = (const f32x4*)((const char*)scratch + l.rows);
    const float d = ema ? ema_decay : 0.f, omd = (float)(1.0 - (double)d);
    if (ema)
        hipLaunchKernelGGL(optim_step_kernel<true>, dim3(step_grid(n4)), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg,
                           exp_avg_sq, ema, n4, chunk_group, (const OptimState*)state, rows, beta1, beta2, eps, grad_scale, d, omd);
    else
        hipLaunchKernelGGL(optim_step_kernel<false>, dim3(step_grid(n4)), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg,
                           exp_avg_sq, ema, n4, chunk_group, (const OptimState*)state, rows, beta1, beta2, eps, grad_scale, d, omd);
    VITSEG_LAUNCH_CHECK("optim_step");
    return VITSEG_OK;
}

}  // extern "C"
