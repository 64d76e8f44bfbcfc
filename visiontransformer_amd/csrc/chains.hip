// The two kernels of the chain-ranking core (chains.hpp) and their launchers.
#include "chains.hpp"

namespace vitseg {
namespace {

// grid (n, fields): tot[image][chunk][field] becomes its exclusive scan over the chunks; the sums go to `out`
__global__ __launch_bounds__(256) void chunk_scan_kernel(int* __restrict__ tot, int nchunks, ScanOut out) {
    __shared__ int wsum[4];
    const int f = blockIdx.y, fields = gridDim.y;
    int* t = tot + (size_t)blockIdx.x * nchunks * fields + f;
    int carry = 0;
    for (int b0 = 0; b0 < nchunks; b0 += 256) {
        const int b = b0 + threadIdx.x;
        const int v = b < nchunks ? t[(size_t)b * fields] : 0;
        int total;
        const int ex = block_scan(v, wsum, total);
        if (b < nchunks) t[(size_t)b * fields] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        if (out.t32[f]) out.t32[f][blockIdx.x] = carry;
        if (out.t64[f]) out.t64[f][blockIdx.x] = carry;
    }
}

// grid chain_grid, item-strided: one round of pointer jumping, in -> out.  A round that changed nothing leaves a zero in its
// word of `changed`; the rounds after it return at once (the host never reads that word)
__global__ __launch_bounds__(256) void chain_jump_kernel(ChainBuf in, ChainBuf out, const int* __restrict__ count,
                                                         int* __restrict__ changed, size_t cap, int round, int rounds) {
    int* flags = changed + (size_t)blockIdx.y * rounds;
    if (round > 0 && flags[round - 1] == 0) return;   // the whole launch: the word was written by the launch before
    const size_t nb = (size_t)blockIdx.y * cap;
    const int cnt = count[blockIdx.y];
    bool any = false;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < cnt; v += (long long)gridDim.x * 256) {
        const int j = in.nxt[nb + v];
        u64 mine = in.mh[nb + v];
        const u64 theirs = in.mh[nb + j];
        if ((theirs >> 32) < (mine >> 32)) {
            mine = (theirs & 0xffffffff00000000ull) | ((theirs & 0xffffffffull) + (1ull << round));
            any = true;
        }
        out.nxt[nb + v] = in.nxt[nb + j];
        out.mh[nb + v] = mine;
    }
    if (__syncthreads_or(any) && threadIdx.x == 0) atomicOr(&flags[round], 1);
}

}  // namespace

int launch_chunk_scan(int* tot, int n, int nchunks, int fields, const ScanOut& out, hipStream_t s) {
    hipLaunchKernelGGL(chunk_scan_kernel, dim3(n, fields), dim3(256), 0, s, tot, nchunks, out);
    VITSEG_LAUNCH_CHECK("chunk scan");
    return VITSEG_OK;
}

int launch_chain_jumps(const ChainLayout& l, const ChainScratch& c, const int* count, ChainBuf* fin, ChainBuf* spare,
                       hipStream_t s) {
    const hipError_t e = hipMemsetAsync(c.changed, 0, (size_t)l.n * l.rounds * sizeof(int), s);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(chain flags)");
    for (int r = 0; r < l.rounds; ++r) {
        hipLaunchKernelGGL(chain_jump_kernel, chain_grid(l), dim3(256), 0, s, c.buf[r & 1], c.buf[(r + 1) & 1], count, c.changed,
                           l.cap, r, l.rounds);
        VITSEG_LAUNCH_CHECK("chain jump");
    }
    // after a round that changed nothing both sides hold the same (word, hops)
    *fin = c.buf[l.rounds & 1];
    *spare = c.buf[(l.rounds + 1) & 1];
    return VITSEG_OK;
}

}  // namespace vitseg
