// refine_kernels.hip -- the tree refiner of include/rto.h "refiner" for gfx950.
//
// Pass 1 (launch_refine_plan) leaves, for every slot, its rank j among the selected slots (or -1) and, for every j, its slot:
//   ref_links     one thread per slot: bounds check and the claim of the target's parent word by compare-and-swap (a second claim
//                 = a shared child) -- simp_links without the working copies
//   ref_level     one thread per node, pass l = 0 .. 31: a node whose parent slot lies in a node of level l pulls level l + 1
//   ref_hist      pass p = 0 .. 3, one workgroup per tile of kRefineTile slots: the 256-bin histogram of digit p (from the top) of
//                 the candidates' keys that share the prefix picked so far.  A wave first takes the lanes that hold its leader's
//                 digit off in ONE LDS add of their count (all of them when every key is equal), at most kPeel times; what is
//                 left adds lane by lane.  One global add per non-empty bin and workgroup.  Pass 0 also takes the keys' minimum.
//   ref_pick      one workgroup: the suffix sums of the bins from 255 down -> the next digit of the cut and how many keys with
//                 the new prefix are still to be taken.  After pass 0 it knows C: a budget that takes all candidates, or none,
//                 switches the later passes off (they return at once).  No host round trip between passes.
//   ref_count / ref_tile_scan / ref_index   reduce-then-scan over the tiles of slots.  One scan carries two counts packed in 64
//                 bits: the candidates ABOVE the cut (low word) and those EQUAL to it (high word).  The selected slots before a
//                 slot are above + min(equal, rem), so the rank of every selected slot follows from the one scan.
// Pass 2 (launch_refine_write) writes every output byte once:
//   ref_slots     one thread per output slot: child_out (the input's word, the new offset of a selected slot, 0 in a new node)
//                 and slot_src
//   ref_data16    one thread per 16-byte word of data_out: a word of the first cap nodes is the input's word; a word of a new
//                 node is put together from the parent record, which repeats every D halves
//   ref_data2     the half-by-half form for nodes that are no multiple of 16 bytes or buffers not aligned to 16
// Kernel boundaries are the only grid-wide synchronisation; the atomics are integer counts, maxima, one minimum and one
// compare-and-swap per link whose outcome does not depend on order in a well-formed tree; there is no float arithmetic.  The
// arithmetic of the definition is host/tree_refine.h (and host/tree_simplify.h for the links).
#include <hip/hip_runtime.h>

#include "host/tree_refine.h"
#include "rto_refine_launch.h"

namespace rto {
namespace {

constexpr int kItems = kRefineTile / kRefineBlock;
constexpr int kPeel = 4;  // digits a wave takes off as one add each before its lanes add singly

__device__ inline size_t global_thread() { return (size_t)blockIdx.x * kRefineBlock + threadIdx.x; }

__global__ __launch_bounds__(kRefineBlock) void ref_links(const int32_t* __restrict__ child, int64_t cap, int S, int32_t* parent,
                                                          int32_t* __restrict__ level, uint32_t* words) {
    const size_t i = global_thread();
    if (i >= (size_t)cap * S) return;
    if (i == 0) level[0] = 0, words[kRefLevelCount] = 1;
    const int32_t c = child[i];
    if (!c) return;
    const int64_t t = simp_link_target((int64_t)(i / S), c, cap);
    if (t < 0) {
        atomicMax(&words[kRefBadRange], (uint32_t)i + 1u);
        return;
    }
    if (atomicCAS(&parent[t], -1, (int32_t)i) != -1) atomicMax(&words[kRefBadShared], (uint32_t)i + 1u);
}

// one atomic per workgroup and word
__device__ inline void block_add(bool mine, uint32_t* word) {
    const int c = __syncthreads_count(mine ? 1 : 0);
    if (threadIdx.x == 0 && c) atomicAdd(word, (uint32_t)c);
}

__global__ __launch_bounds__(kRefineBlock) void ref_level(int64_t cap, int S, int l, const int32_t* __restrict__ parent, int32_t* level,
                                                          uint32_t* words) {
    if (words[kRefLevelCount + l] == 0) return;  // (the same for every thread of the grid)
    const size_t n = global_thread();
    bool take = false;
    if (n >= 1 && n < (size_t)cap && level[n] == -1) {
        const int32_t ps = parent[n];
        take = ps >= 0 && level[ps / S] == l;
        if (take) level[n] = l + 1;
    }
    block_add(take, &words[kRefLevelCount + l + 1]);
}

// the key of slot i if it is a candidate; i < cap * S
__device__ inline bool candidate_key(size_t i, int S, const int32_t* __restrict__ child, const uint32_t* __restrict__ key,
                                     const int32_t* __restrict__ level, int max_level, uint32_t key_thresh, uint32_t* k) {
    const int32_t c = child[i];
    if (c) return false;
    *k = key ? key[i] : 1u;
    return refine_candidate(c, level[i / S], max_level, *k, key_thresh);
}

__global__ __launch_bounds__(kRefineBlock) void ref_hist(const int32_t* __restrict__ child, const uint32_t* __restrict__ key, int64_t cap,
                                                         int S, const int32_t* __restrict__ level, int max_level, uint32_t key_thresh,
                                                         int pass, uint32_t* __restrict__ hist, uint32_t* words) {
    if (pass && words[kRefMode]) return;  // (the same for every thread of the grid)
    __shared__ uint32_t bins[kRefineBins];
    __shared__ uint32_t lowest;
    bins[threadIdx.x] = 0;  // kRefineBins == kRefineBlock
    if (threadIdx.x == 0) lowest = 0xFFFFFFFFu;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t prefix = pass ? words[kRefPrefix] >> (shift + 8) : 0u;
    const size_t first = (size_t)blockIdx.x * kRefineTile + (size_t)threadIdx.x * kItems;
    uint32_t low = 0xFFFFFFFFu;
    for (int it = 0; it < kItems; ++it) {
        const size_t i = first + it;
        uint32_t k = 0;
        bool mine = i < (size_t)cap * S && candidate_key(i, S, child, key, level, max_level, key_thresh, &k);
        mine = mine && (pass == 0 || (k >> (shift + 8)) == prefix);
        if (mine) low = min(low, k);
        const uint32_t digit = (k >> shift) & 0xFFu;
        // per wave: the lanes that share the leader's digit leave in one add
        for (int round = 0; round < kPeel; ++round) {
            const unsigned long long left = __ballot(mine);
            if (!left) break;
            const int leader = __ffsll((long long)left) - 1;
            const uint32_t d = (uint32_t)__shfl((int)digit, leader);
            const unsigned long long same = __ballot(mine && digit == d);
            if (mine && digit == d) {
                if ((int)(threadIdx.x & 63) == leader) atomicAdd(&bins[d], (uint32_t)__popcll(same));
                mine = false;
            }
        }
        if (mine) atomicAdd(&bins[digit], 1u);
    }
    if (pass == 0 && low != 0xFFFFFFFFu) atomicMin(&lowest, low);
    __syncthreads();
    const uint32_t v = bins[threadIdx.x];
    if (v) atomicAdd(&hist[pass * kRefineBins + threadIdx.x], v);
    if (pass == 0 && threadIdx.x == 0 && lowest != 0xFFFFFFFFu) atomicMin(&words[kRefMinKey], lowest);
}

// exclusive prefix of v over the workgroup's threads (in thread order) and the total; buf: kRefineBlock words of LDS
template <class T>
__device__ inline T block_scan(T v, T* buf, T* total) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int d = 1; d < kRefineBlock; d <<= 1) {
        const T add = t >= d ? buf[t - d] : 0;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    const T incl = buf[t];
    *total = buf[kRefineBlock - 1];
    __syncthreads();
    return incl - v;
}

// one workgroup of kRefineBins threads; thread t looks at bin 255 - t, so the scan runs from the largest digit down
__global__ __launch_bounds__(kRefineBlock) void ref_pick(const uint32_t* __restrict__ hist, int pass, int64_t max_new, uint32_t* words) {
    __shared__ uint32_t buf[kRefineBlock];
    if (pass && words[kRefMode]) return;
    const uint32_t bin = (uint32_t)(kRefineBins - 1 - threadIdx.x);
    const uint32_t v = hist[pass * kRefineBins + bin];
    uint32_t total;
    const uint32_t above = block_scan(v, buf, &total);  // keys of the prefix with a larger digit
    uint32_t remain;
    if (pass == 0) {
        const uint32_t C = total;
        const uint32_t K = max_new < 0 || max_new >= (int64_t)C ? C : (uint32_t)max_new;
        if (K == C || K == 0) {
            if (threadIdx.x == 0) {
                words[kRefCandidates] = C;
                words[kRefMode] = K ? 1u : 2u;  // (no candidate at all: none is taken)
                words[kRefCut] = K ? 0u : 0xFFFFFFFFu;
                words[kRefRem] = K ? 0xFFFFFFFFu : 0u;
            }
            return;
        }
        if (threadIdx.x == 0) words[kRefCandidates] = C;
        remain = K;
    } else {
        remain = words[kRefRemain];
    }
    // 1 <= remain <= total: exactly one bin has above < remain <= above + v.  (Every thread has read words[] before any writes:
    // block_scan ends with a barrier only for `buf`, so the read of kRefRemain is ordered by the barrier below.)
    __syncthreads();
    if (above < remain && remain <= above + v) {
        const int shift = 24 - 8 * pass;
        const uint32_t prefix = (pass ? words[kRefPrefix] : 0u) | (bin << shift);
        words[kRefPrefix] = prefix;
        words[kRefRemain] = remain - above;
        if (pass == kRefinePasses - 1) words[kRefCut] = prefix, words[kRefRem] = remain - above;
    }
}

// (above | equal << 32) of one slot
__device__ inline uint64_t slot_counts(size_t i, int64_t cap, int S, const int32_t* __restrict__ child, const uint32_t* __restrict__ key,
                                       const int32_t* __restrict__ level, int max_level, uint32_t key_thresh, uint32_t cut) {
    uint32_t k = 0;
    if (i >= (size_t)cap * S || !candidate_key(i, S, child, key, level, max_level, key_thresh, &k)) return 0;
    return k > cut ? 1ull : k == cut ? 1ull << 32 : 0ull;
}

__global__ __launch_bounds__(kRefineBlock) void ref_count(const int32_t* __restrict__ child, const uint32_t* __restrict__ key, int64_t cap,
                                                          int S, const int32_t* __restrict__ level, int max_level, uint32_t key_thresh,
                                                          const uint32_t* __restrict__ words, uint64_t* __restrict__ tile) {
    __shared__ uint32_t above, equal;
    if (threadIdx.x == 0) above = 0, equal = 0;
    __syncthreads();
    const uint32_t cut = words[kRefCut];
    const size_t first = (size_t)blockIdx.x * kRefineTile + (size_t)threadIdx.x * kItems;
    uint64_t my = 0;
    for (int it = 0; it < kItems; ++it) my += slot_counts(first + it, cap, S, child, key, level, max_level, key_thresh, cut);
    // per wave first: in mask mode every lane of every wave counts into `equal`
    uint32_t a = (uint32_t)my, e = (uint32_t)(my >> 32);
    for (int d = 32; d >= 1; d >>= 1) a += __shfl_xor((int)a, d), e += __shfl_xor((int)e, d);
    if ((threadIdx.x & 63) == 0) {
        if (a) atomicAdd(&above, a);
        if (e) atomicAdd(&equal, e);
    }
    __syncthreads();
    if (threadIdx.x == 0) tile[blockIdx.x] = (uint64_t)above | (uint64_t)equal << 32;
}

// one workgroup: the tiles' counts -> their exclusive prefix, in chunks of kRefineBlock with a carry (any number of tiles)
__global__ __launch_bounds__(kRefineBlock) void ref_tile_scan(uint64_t* tile, int tiles, uint32_t* words) {
    __shared__ uint64_t buf[kRefineBlock];
    uint64_t carry = 0;
    for (int base = 0; base < tiles; base += kRefineBlock) {
        const int b = base + threadIdx.x;
        const uint64_t v = b < tiles ? tile[b] : 0;
        uint64_t total;
        const uint64_t ex = block_scan(v, buf, &total);
        if (b < tiles) tile[b] = carry + ex;
        carry += total;  // (each half stays below 2^31: no carry from the low word into the high one)
    }
    if (threadIdx.x == 0) {
        const uint64_t rem = words[kRefRem], equal = carry >> 32;
        words[kRefSelected] = (uint32_t)carry + (uint32_t)(equal < rem ? equal : rem);
    }
}

__global__ __launch_bounds__(kRefineBlock) void ref_index(const int32_t* __restrict__ child, const uint32_t* __restrict__ key, int64_t cap,
                                                          int S, const int32_t* __restrict__ level, int max_level, uint32_t key_thresh,
                                                          const uint64_t* __restrict__ tile, int32_t* __restrict__ rank,
                                                          int32_t* __restrict__ picked, uint32_t* words) {
    __shared__ uint64_t buf[kRefineBlock];
    __shared__ uint32_t deepest;
    if (threadIdx.x == 0) deepest = 0;
    const uint32_t cut = words[kRefCut];
    const uint64_t rem = words[kRefRem];
    const size_t first = (size_t)blockIdx.x * kRefineTile + (size_t)threadIdx.x * kItems;
    uint64_t c[kItems], my = 0;
    for (int it = 0; it < kItems; ++it) {
        c[it] = slot_counts(first + it, cap, S, child, key, level, max_level, key_thresh, cut);
        my += c[it];
    }
    uint64_t total;
    uint64_t at = tile[blockIdx.x] + block_scan(my, buf, &total);  // the counts of all slots before this thread's first
    uint32_t deep = 0;
    for (int it = 0; it < kItems; ++it) {
        const size_t i = first + it;
        if (i >= (size_t)cap * S) break;
        const uint64_t above = at & 0xFFFFFFFFull, equal = at >> 32;
        // an `above` slot is refine_selected whatever its rank; an `equal` one when its rank among the equal is below rem
        const bool sel = (c[it] & 0xFFFFFFFFull) != 0 || (c[it] != 0 && refine_selected(cut, cut, equal, rem));
        int32_t j = -1;
        if (sel) {
            j = (int32_t)(above + (equal < rem ? equal : rem));  // j < K <= cap * S: within picked
            picked[j] = (int32_t)i;
            deep = max(deep, (uint32_t)level[i / S] + 1u);
        }
        rank[i] = j;
        at += c[it];
    }
    if (deep) atomicMax(&deepest, deep);
    __syncthreads();
    if (threadIdx.x == 0 && deepest) atomicMax(&words[kRefDeepest], deepest);
}

__global__ __launch_bounds__(kRefineBlock) void ref_slots(const int32_t* __restrict__ child, int64_t cap, int S, int64_t K,
                                                          const int32_t* __restrict__ rank, const int32_t* __restrict__ picked,
                                                          int32_t* __restrict__ child_out, int32_t* __restrict__ slot_src) {
    const size_t g = global_thread();  // the slot of the output
    const size_t old_slots = (size_t)cap * S;
    if (g >= old_slots + (size_t)K * S) return;
    if (g < old_slots) {
        const int32_t j = rank[g];
        child_out[g] = j >= 0 ? (int32_t)(cap + j - (int64_t)(g / S)) : child[g];
        if (slot_src) slot_src[g] = (int32_t)g;
    } else {
        child_out[g] = 0;
        if (slot_src) slot_src[g] = picked[(g - old_slots) / S];
    }
}

union Word16 {
    uint4 v;
    uint16_t h[8];
};

__global__ __launch_bounds__(kRefineBlock) void ref_data16(const uint16_t* __restrict__ data, int64_t cap, int S, int D, int wpn, int64_t K,
                                                           const int32_t* __restrict__ picked, uint16_t* __restrict__ data_out) {
    const size_t g = global_thread();  // the 16-byte word of the output
    const size_t old_words = (size_t)cap * wpn;
    if (g >= old_words + (size_t)K * wpn) return;
    Word16 x;
    if (g < old_words) {
        x.v = reinterpret_cast<const uint4*>(data)[g];
    } else {
        const size_t j = (g - old_words) / wpn;
        const int w = (int)((g - old_words) % wpn);
        const uint16_t* rec = data + (size_t)picked[j] * D;
        int at = (w * 8) % D;  // the node is its parent record over and over
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            x.h[k] = rec[at];
            if (++at == D) at = 0;
        }
    }
    reinterpret_cast<uint4*>(data_out)[g] = x.v;
}

__global__ __launch_bounds__(kRefineBlock) void ref_data2(const uint16_t* __restrict__ data, int64_t cap, int S, int D, int64_t K,
                                                          const int32_t* __restrict__ picked, uint16_t* __restrict__ data_out) {
    const size_t g = global_thread();  // the half of the output
    const size_t per_node = (size_t)S * D, old_halves = (size_t)cap * per_node;
    if (g >= old_halves + (size_t)K * per_node) return;
    if (g < old_halves) {
        data_out[g] = data[g];
    } else {
        const size_t r = g - old_halves;
        data_out[g] = data[(size_t)picked[r / per_node] * D + r % D];  // (r % per_node) % D == r % D: per_node is a multiple of D
    }
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline unsigned blocks_for(size_t threads) { return (unsigned)((threads + kRefineBlock - 1) / kRefineBlock); }

}  // namespace

RefinePlan refine_plan(int64_t cap, int N) {
    static_assert(kRefineBins == kRefineBlock, "ref_hist and ref_pick give every bin a thread");
    RefinePlan p;
    p.cap = cap, p.N = N, p.S = N * N * N;
    const size_t slots = (size_t)cap * p.S;
    p.tiles = (int)((slots + kRefineTile - 1) / kRefineTile);
    size_t at = 0;
    const auto take = [&](size_t bytes) {
        const size_t o = at;
        at = align256(at + bytes);
        return o;
    };
    p.parent = take((size_t)cap * 4);
    p.level = take((size_t)cap * 4);
    p.rank = take(slots * 4);
    p.picked = take(slots * 4);
    p.tile = take((size_t)p.tiles * 8);
    p.hist = take((size_t)kRefinePasses * kRefineBins * 4);
    p.words = take((size_t)kRefWords * 4);
    p.total = at;
    return p;
}

hipError_t launch_refine_plan(const RefinePlan& p, void* scratch, const int32_t* child, const uint32_t* key, uint32_t key_thresh,
                              int64_t max_new, int max_level, hipStream_t stream) {
    char* base = static_cast<char*>(scratch);
    int32_t* parent = reinterpret_cast<int32_t*>(base + p.parent);
    int32_t* level = reinterpret_cast<int32_t*>(base + p.level);
    int32_t* rank = reinterpret_cast<int32_t*>(base + p.rank);
    int32_t* picked = reinterpret_cast<int32_t*>(base + p.picked);
    uint64_t* tile = reinterpret_cast<uint64_t*>(base + p.tile);
    uint32_t* hist = reinterpret_cast<uint32_t*>(base + p.hist);
    uint32_t* words = reinterpret_cast<uint32_t*>(base + p.words);
    hipError_t e = hipMemsetAsync(parent, 0xFF, (size_t)p.cap * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(level, 0xFF, (size_t)p.cap * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(hist, 0, (size_t)kRefinePasses * kRefineBins * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(words, 0, (size_t)kRefWords * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(words + kRefMinKey, 0xFF, 4, stream);
    if (e != hipSuccess) return e;
    const size_t slots = (size_t)p.cap * p.S;
    ref_links<<<blocks_for(slots), kRefineBlock, 0, stream>>>(child, p.cap, p.S, parent, level, words);
    for (int l = 0; l < kSimplifyMaxLevels; ++l)
        ref_level<<<blocks_for((size_t)p.cap), kRefineBlock, 0, stream>>>(p.cap, p.S, l, parent, level, words);
    for (int pass = 0; pass < kRefinePasses; ++pass) {
        ref_hist<<<(unsigned)p.tiles, kRefineBlock, 0, stream>>>(child, key, p.cap, p.S, level, max_level, key_thresh, pass, hist, words);
        ref_pick<<<1, kRefineBlock, 0, stream>>>(hist, pass, max_new, words);
    }
    ref_count<<<(unsigned)p.tiles, kRefineBlock, 0, stream>>>(child, key, p.cap, p.S, level, max_level, key_thresh, words, tile);
    ref_tile_scan<<<1, kRefineBlock, 0, stream>>>(tile, p.tiles, words);
    ref_index<<<(unsigned)p.tiles, kRefineBlock, 0, stream>>>(child, key, p.cap, p.S, level, max_level, key_thresh, tile, rank, picked, words);
    return hipGetLastError();
}

hipError_t launch_refine_write(const RefinePlan& p, const void* scratch, int64_t K, const int32_t* child, const uint16_t* data, int D,
                               int32_t* child_out, uint16_t* data_out, int32_t* slot_src, hipStream_t stream) {
    const char* base = static_cast<const char*>(scratch);
    const int32_t* rank = reinterpret_cast<const int32_t*>(base + p.rank);
    const int32_t* picked = reinterpret_cast<const int32_t*>(base + p.picked);
    const size_t slots = (size_t)(p.cap + K) * p.S;
    ref_slots<<<blocks_for(slots), kRefineBlock, 0, stream>>>(child, p.cap, p.S, K, rank, picked, child_out, slot_src);
    const size_t halves = slots * (size_t)D;
    const bool wide = (size_t)p.S * D % 8 == 0 && (((uintptr_t)data | (uintptr_t)data_out) & 15u) == 0;
    if (wide)
        ref_data16<<<blocks_for(halves / 8), kRefineBlock, 0, stream>>>(data, p.cap, p.S, D, (int)((size_t)p.S * D / 8), K, picked, data_out);
    else
        ref_data2<<<blocks_for(halves), kRefineBlock, 0, stream>>>(data, p.cap, p.S, D, K, picked, data_out);
    return hipGetLastError();
}

}  // namespace rto
