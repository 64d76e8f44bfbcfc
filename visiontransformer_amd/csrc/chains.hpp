// Chain ranking, the core that polygons.hip (rings of vertex edges) and centerlines.hip (walks of half-links) share.  Both
// number their items in key order by a scan over chunks of 1024, link each item to its successor and then jump pointers:
// after round j an item knows the smallest word among the 2^(j+1) items from itself on and how many hops ahead it lies.
// What an item and its word are, and what a leader is, stay with the families; the kernels are in chains.hip.
#pragma once
#include "common.hpp"

namespace vitseg {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int CHUNK = 1024;         // items per workgroup of the chunked launches (count, build, leaders, place): 4 per thread
constexpr int JUMP_BLOCKS = 1024;   // workgroups per image, at most, of the item-strided launches (link, jump, emit)

// exclusive scan of one int per thread over a 256-thread workgroup; total: the sum of all.  Whole workgroups call it.
__device__ __forceinline__ int block_scan(int v, int* wsum /* shared [4] */, int& total) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    int inc = v;
    for (int d = 1; d < WAVE; d <<= 1) {
        const int o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    __syncthreads();   // the words may still be read from the call before
    if (lane == WAVE - 1) wsum[wave] = inc;
    __syncthreads();
    int before = 0, tot = 0;
    for (int w = 0; w < 4; ++w) {
        const int s = wsum[w];
        if (w < wave) before += s;
        tot += s;
    }
    total = tot;
    return before + inc - v;
}

struct ChainBuf {   // one side of the pointer jumping: where the item's window ends, (smallest word in it) << 32 | hops to it
    int* nxt;
    u64* mh;
};

struct ScanOut {   // where the totals of the (up to two) fields of a chunk scan go, [image]; any may be null
    int* t32[2];
    long long* t64[2];
};

// The chain scratch of n images of at most cap items each: byte offsets from its start, every array rounded to 256 bytes.
struct ChainLayout {
    size_t changed, nxt0, nxt[2], mh[2], bytes;   // changed [n][rounds]; nxt0, nxt[i] [n][cap] ints; mh[i] [n][cap] u64
    size_t cap;
    int n, rounds, nchunks;   // rounds = ceil(log2(cap)), at least 1; nchunks = ceil(cap / CHUNK)
};

inline ChainLayout chain_layout(int n, size_t cap) {
    ChainLayout l{};
    l.n = n;
    l.cap = cap;
    l.nchunks = (int)((cap + CHUNK - 1) / CHUNK);
    l.rounds = 1;
    while (((size_t)1 << l.rounds) < cap) ++l.rounds;
    size_t o = 0;
    l.nxt0 = o;     o += up256((size_t)n * cap * sizeof(int));
    for (int i = 0; i < 2; ++i) {
        l.nxt[i] = o;  o += up256((size_t)n * cap * sizeof(int));
        l.mh[i] = o;   o += up256((size_t)n * cap * sizeof(u64));
    }
    l.changed = o;  o += up256((size_t)n * l.rounds * sizeof(int));
    l.bytes = o;
    return l;
}

struct ChainScratch {
    int* changed;   // one word per image and round: the round changed something (only the jump kernel reads them)
    int* nxt0;      // every item's successor, kept through the jumping; the families' link kernels write it
    ChainBuf buf[2];   // the link kernels fill side 0
};

inline ChainScratch chain_scratch(void* base, const ChainLayout& l) {
    char* b = (char*)base;
    return {(int*)(b + l.changed), (int*)(b + l.nxt0),
            {{(int*)(b + l.nxt[0]), (u64*)(b + l.mh[0])}, {(int*)(b + l.nxt[1]), (u64*)(b + l.mh[1])}}};
}

// the grid of the item-strided launches
inline dim3 chain_grid(const ChainLayout& l) { return dim3((unsigned)(l.nchunks < JUMP_BLOCKS ? l.nchunks : JUMP_BLOCKS), l.n); }

// tot[image][chunk][field], fields = 1 or 2, becomes its exclusive scan over the chunks; the sums of the fields go to `out`
int launch_chunk_scan(int* tot, int n, int nchunks, int fields, const ScanOut& out, hipStream_t s);

// Zeroes the flags and runs the rounds of pointer jumping from side 0, count[image] items per image.  *fin: the side that
// holds the result; *spare: the other side, whose words nothing needs any more.
int launch_chain_jumps(const ChainLayout& l, const ChainScratch& c, const int* count, ChainBuf* fin, ChainBuf* spare,
                       hipStream_t s);

}  // namespace vitseg
