// Reduction keyed by runs of equal key within a wave: the first level of the pre-reduction of props.hip and confidence.hip,
// whose accumulation kernels would otherwise issue one atomic per pixel and field, all on one row when one region fills the
// frame.  The second level (one key per workgroup collected in LDS) is each kernel's own.
#pragma once
#include "common.hpp"

namespace vitseg {

typedef unsigned long long u64;
typedef long long i64;

// The lanes of a wave hold consecutive pixels; key >= 0 is the pixel's region index (-1: none) and y its row.  A run is a
// maximal stretch of lanes with one key in one row.  head: this lane starts a run; end: the first lane past the run this lane
// is in (meaningless where key < 0); members: at a head, the lanes of its run.  Whole waves call it.
struct Run {
    bool head;
    int end;
    u64 members;
};

__device__ __forceinline__ Run find_run(int key, int y, int lane) {
    const int key_prev = __shfl_up(key, 1), y_prev = __shfl_up(y, 1);
    Run r;
    r.head = key >= 0 && (lane == 0 || key_prev != key || y_prev != y);
    const u64 upto = (2ull << lane) - 1ull;   // this lane and the ones below it
    const u64 stops = __ballot(r.head || key < 0) & ~upto;
    r.end = stops ? __ffsll((long long)stops) - 1 : WAVE;
    r.members = (r.end == WAVE ? ~0ull : (1ull << r.end) - 1ull) & ~((1ull << lane) - 1ull);
    return r;
}

// at every lane of a run: op over the values from this lane to the run's last; the head gets the run's total.  Whole waves.
template <typename T, typename Op>
__device__ __forceinline__ T run_reduce(T v, int lane, int end, Op op) {
    for (int d = 1; d < WAVE; d <<= 1) {
        const T o = __shfl_down(v, d);
        if (lane + d < end) v = op(v, o);
    }
    return v;
}

}  // namespace vitseg
