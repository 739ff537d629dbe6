// simplify_kernels.hip -- the tree simplifier of include/rto.h "simplifier" for gfx950.
//
// No pass rewrites a record.  Every slot carries a SOURCE instead: the input slot whose record it holds (itself at first), or
// kSimplifyZero once the kill found it dead.  A merge hands the uniform node's source to the slot that referred to it, so a
// cascade over any number of levels still ends at a slot of the input, and the scatter reads the input once.
//   simp_links    one thread per slot: working copy of the offset, identity source, bounds check, and the claim of the target's
//                 parent word by compare-and-swap (a second claim = a shared child)
//   simp_level    one thread per node, pass l = 0 .. 31: a node whose parent slot lies in a node of level l gets level l + 1 (it
//                 pulls, nothing is pushed: no thread writes another node's word); a pass whose level is empty returns at once
//   simp_kill     one thread per slot
//   simp_merge8   (N = 2) eight lanes per node, one pass per level from the deepest to level 1: all slots leaves, the density
//                 halves equal, then the records as 32-bit words, each lane its slot against a partner slot; rewrites the
//                 parent slot.  simp_merge: any N, one thread per node (simp_node_uniform)
//   simp_count / simp_tile_scan / simp_index   reduce-then-scan of the keep flags over tiles of kSimplifyTile nodes
//   simp_child    one thread per output slot: the rewritten offset, node_map
//   simp_data16   one thread per 16-byte word of the output: a node of N = 2 is 16 D bytes, so it moves as whole words whatever
//                 the parity of D; only a word that touches a slot with a foreign source is put together half by half
//   simp_data2    the half-by-half scatter for nodes that are no multiple of 16 bytes or buffers not aligned to 16
// Kernel boundaries are the only grid-wide synchronisation; the atomics are integer counts, maxima and one compare-and-swap per
// link whose outcome does not depend on order in a well-formed tree.  The arithmetic of the definition is host/tree_simplify.h.
#include <hip/hip_runtime.h>

#include "host/tree_simplify.h"
#include "rto_simplify_launch.h"

namespace rto {
namespace {

constexpr int kItems = kSimplifyTile / kSimplifyBlock;

__device__ inline size_t global_thread() { return (size_t)blockIdx.x * kSimplifyBlock + threadIdx.x; }

__global__ __launch_bounds__(kSimplifyBlock) void simp_links(const int32_t* __restrict__ child, int64_t cap, int S, int32_t* parent,
                                                             int32_t* __restrict__ level, int32_t* __restrict__ wchild,
                                                             int32_t* __restrict__ src, uint32_t* words) {
    const size_t i = global_thread();
    if (i >= (size_t)cap * S) return;
    if (i == 0) level[0] = 0, words[kSimpLevelCount] = 1;
    const int32_t c = child[i];
    wchild[i] = c;
    src[i] = (int32_t)i;
    if (!c) return;
    const int64_t t = simp_link_target((int64_t)(i / S), c, cap);
    if (t < 0) {
        atomicMax(&words[kSimpBadRange], (uint32_t)i + 1u);
        return;
    }
    if (atomicCAS(&parent[t], -1, (int32_t)i) != -1) atomicMax(&words[kSimpBadShared], (uint32_t)i + 1u);
}

// one atomic per workgroup and word: a count per thread (even merged per wave by the compiler) queues tens of thousands of
// atomics on one address
__device__ inline void block_add(bool mine, uint32_t* word) {
    const int c = __syncthreads_count(mine ? 1 : 0);
    if (threadIdx.x == 0 && c) atomicAdd(word, (uint32_t)c);
}

__global__ __launch_bounds__(kSimplifyBlock) void simp_level(int64_t cap, int S, int l, const int32_t* __restrict__ parent,
                                                             int32_t* level, uint32_t* words) {
    if (words[kSimpLevelCount + l] == 0) return;  // (the same for every thread of the grid)
    const size_t n = global_thread();
    bool take = false;
    if (n >= 1 && n < (size_t)cap && level[n] == -1) {
        const int32_t ps = parent[n];
        take = ps >= 0 && level[ps / S] == l;
        if (take) level[n] = l + 1;
    }
    block_add(take, &words[kSimpLevelCount + l + 1]);
}

__global__ __launch_bounds__(kSimplifyBlock) void simp_kill(const uint16_t* __restrict__ data, int64_t cap, int S, int D, uint32_t th,
                                                            const int32_t* __restrict__ level, const int32_t* __restrict__ wchild,
                                                            int32_t* __restrict__ src, uint32_t* words) {
    const size_t i = global_thread();
    const bool dead = i < (size_t)cap * S && level[i / S] >= 0 && wchild[i] == 0 && !simp_half_gt(data[i * D + D - 1], th);
    if (dead) src[i] = kSimplifyZero;
    block_add(dead, &words[kSimpKilled]);
}

// any N: one thread per node
__global__ __launch_bounds__(kSimplifyBlock) void simp_merge(const uint16_t* __restrict__ data, int64_t cap, int S, int D, int l,
                                                             const int32_t* __restrict__ parent, int32_t* level, int32_t* wchild,
                                                             int32_t* src, uint32_t* words) {
    const size_t n = global_thread();
    bool uniform = n < (size_t)cap && level[n] == l;
    if (uniform) {
        const int32_t* wc = wchild + n * S;
        for (int s = 0; s < S && uniform; ++s) uniform = wc[s] == 0;
        uniform = uniform && simp_node_uniform(data, D, src + n * S, S);
    }
    if (uniform) {
        // the parent is a node of level l - 1: no thread of this pass reads its slots
        const int32_t ps = parent[n];
        level[n] = -2;
        wchild[ps] = 0;
        src[ps] = src[n * S];
    }
    block_add(uniform, &words[kSimpMerged]);
}

// N = 2: eight neighbouring lanes per node, one per slot, so the offsets and sources load as whole lines and the eight record
// compares of a node run side by side.  The pairs compared are those of simp_node_uniform (slot 1 with slot 0, slot s with
// slot s - 2): all eight records equal, or not.
__global__ __launch_bounds__(kSimplifyBlock) void simp_merge8(const uint16_t* __restrict__ data, int64_t cap, int D, int l,
                                                              const int32_t* __restrict__ parent, int32_t* level, int32_t* wchild,
                                                              int32_t* src, uint32_t* words) {
    const size_t n = (size_t)blockIdx.x * (kSimplifyBlock / 8) + threadIdx.x / 8;
    const int s = threadIdx.x & 7, lane = threadIdx.x & 63, first = lane & ~7;
    const bool active = n < (size_t)cap && level[n] == l;
    const int32_t wc = active ? wchild[n * 8 + s] : 1;
    const int32_t mine = active ? src[n * 8 + s] : 0;
    const int32_t other = __shfl(mine, s == 0 ? lane : s == 1 ? lane - 1 : lane - 2);  // a lane of the same node
    const bool leaves = ((__ballot(wc != 0) >> first) & 0xFFull) == 0;
    bool differs = false;
    if (active && leaves && s) {
        const uint32_t dm = mine == kSimplifyZero ? 0u : data[(int64_t)mine * D + D - 1];
        const uint32_t dn = other == kSimplifyZero ? 0u : data[(int64_t)other * D + D - 1];
        differs = dm != dn || !simp_src_equal(data, D, mine, other);
    }
    const bool uniform = active && leaves && ((__ballot(differs) >> first) & 0xFFull) == 0;
    if (uniform && s == 0) {
        const int32_t ps = parent[n];
        level[n] = -2;
        wchild[ps] = 0;
        src[ps] = mine;
    }
    block_add(uniform && s == 0, &words[kSimpMerged]);
}

// exclusive prefix of v over the workgroup's threads (in thread order) and the total; buf: kSimplifyBlock words of LDS
__device__ inline uint32_t block_scan(uint32_t v, uint32_t* buf, uint32_t* total) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int d = 1; d < kSimplifyBlock; d <<= 1) {
        const uint32_t add = t >= d ? buf[t - d] : 0;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    const uint32_t incl = buf[t];
    *total = buf[kSimplifyBlock - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(kSimplifyBlock) void simp_count(int64_t cap, const int32_t* __restrict__ level, uint32_t* __restrict__ tile,
                                                             uint32_t* words) {
    __shared__ uint32_t cnt, deepest;
    if (threadIdx.x == 0) cnt = 0, deepest = 0;
    __syncthreads();
    const size_t first = (size_t)blockIdx.x * kSimplifyTile + (size_t)threadIdx.x * kItems;
    uint32_t my = 0, deep = 0;
    for (int k = 0; k < kItems; ++k)
        if (first + k < (size_t)cap) {
            const int32_t lv = level[first + k];
            if (lv >= 0) ++my, deep = max(deep, (uint32_t)lv);
        }
    if (my) atomicAdd(&cnt, my), atomicMax(&deepest, deep);
    __syncthreads();
    if (threadIdx.x == 0) {
        tile[blockIdx.x] = cnt;
        atomicMax(&words[kSimpDeepest], deepest);
    }
}

// one workgroup: the tiles' counts -> their exclusive prefix, in chunks of kSimplifyBlock with a carry
__global__ __launch_bounds__(kSimplifyBlock) void simp_tile_scan(uint32_t* tile, int tiles, uint32_t* words) {
    __shared__ uint32_t buf[kSimplifyBlock];
    uint32_t carry = 0;
    for (int base = 0; base < tiles; base += kSimplifyBlock) {
        const int b = base + threadIdx.x;
        const uint32_t v = b < tiles ? tile[b] : 0;
        uint32_t total;
        const uint32_t ex = block_scan(v, buf, &total);
        if (b < tiles) tile[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) words[kSimpTotal] = carry;
}

__global__ __launch_bounds__(kSimplifyBlock) void simp_index(int64_t cap, const int32_t* __restrict__ level, const uint32_t* __restrict__ tile,
                                                             int32_t* __restrict__ newidx, int32_t* __restrict__ map) {
    __shared__ uint32_t buf[kSimplifyBlock];
    const size_t first = (size_t)blockIdx.x * kSimplifyTile + (size_t)threadIdx.x * kItems;
    bool keep[kItems];
    uint32_t my = 0;
    for (int k = 0; k < kItems; ++k) {
        keep[k] = first + k < (size_t)cap && level[first + k] >= 0;
        my += keep[k] ? 1u : 0u;
    }
    uint32_t total;
    uint32_t at = tile[blockIdx.x] + block_scan(my, buf, &total);
    for (int k = 0; k < kItems; ++k)
        if (keep[k]) {
            newidx[first + k] = (int32_t)at;  // at < survivors <= cap: within map
            map[at] = (int32_t)(first + k);
            ++at;
        }
}

__global__ __launch_bounds__(kSimplifyBlock) void simp_child(int64_t cap, int S, const int32_t* __restrict__ wchild,
                                                             const int32_t* __restrict__ newidx, const int32_t* __restrict__ map,
                                                             const uint32_t* __restrict__ words, int32_t* __restrict__ child_out,
                                                             int64_t* __restrict__ node_map) {
    const size_t g = global_thread();
    const size_t m = g / S;
    if (m >= (size_t)words[kSimpTotal]) return;  // survivors <= cap: g is inside child_out
    const size_t n = (size_t)map[m];
    const int s = (int)(g % S);
    const int32_t wc = wchild[n * S + s];
    // a non-zero working offset passed the bounds check of simp_links and its target was not merged away
    child_out[g] = wc ? newidx[(int64_t)n + wc] - (int32_t)m : 0;
    if (s == 0 && node_map) node_map[m] = (int64_t)n;
}

union Word16 {
    uint4 v;
    uint16_t h[8];
};

__global__ __launch_bounds__(kSimplifyBlock) void simp_data16(const uint16_t* __restrict__ data, int S, int D, int wpn,
                                                              const int32_t* __restrict__ src, const int32_t* __restrict__ map,
                                                              const uint32_t* __restrict__ words, uint16_t* __restrict__ data_out) {
    const size_t g = global_thread();  // the 16-byte word of the output
    const size_t m = g / wpn;
    if (m >= (size_t)words[kSimpTotal]) return;
    const int w = (int)(g % wpn);
    const size_t n = (size_t)map[m];
    const int32_t* sn = src + n * S;
    const int h0 = w * 8, s0 = h0 / D, s1 = (h0 + 7) / D;  // 8 wpn = S D: s1 < S
    Word16 x;
    x.v = reinterpret_cast<const uint4*>(data)[n * wpn + w];
    bool own = true;
    for (int s = s0; s <= s1; ++s) own = own && sn[s] == (int32_t)(n * S + s);
    if (!own) {
        int s = s0, j = h0 - s0 * D;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int32_t from = sn[s];
            if (from == kSimplifyZero)
                x.h[k] = 0;
            else if (from != (int32_t)(n * S + s))
                x.h[k] = data[(size_t)from * D + j];
            if (++j == D) j = 0, ++s;
            if (s >= S) break;  // (only after the node's last half)
        }
    }
    reinterpret_cast<uint4*>(data_out)[g] = x.v;
}

__global__ __launch_bounds__(kSimplifyBlock) void simp_data2(const uint16_t* __restrict__ data, int S, int D, const int32_t* __restrict__ src,
                                                             const int32_t* __restrict__ map, const uint32_t* __restrict__ words,
                                                             uint16_t* __restrict__ data_out) {
    const size_t g = global_thread();  // the half of the output
    const size_t per_node = (size_t)S * D;
    const size_t m = g / per_node;
    if (m >= (size_t)words[kSimpTotal]) return;
    const size_t r = g % per_node, n = (size_t)map[m];
    const int32_t from = src[n * S + r / D];
    data_out[g] = from == kSimplifyZero ? (uint16_t)0 : data[(size_t)from * D + r % D];
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline unsigned blocks_for(size_t threads) { return (unsigned)((threads + kSimplifyBlock - 1) / kSimplifyBlock); }

}  // namespace

SimplifyPlan simplify_plan(int64_t cap, int N, int D) {
    SimplifyPlan p;
    p.cap = cap, p.N = N, p.S = N * N * N, p.D = D;
    p.tiles = (int)((cap + kSimplifyTile - 1) / kSimplifyTile);
    size_t at = 0;
    const auto take = [&](size_t bytes) {
        const size_t o = at;
        at = align256(at + bytes);
        return o;
    };
    p.parent = take((size_t)cap * 4);
    p.level = take((size_t)cap * 4);
    p.wchild = take((size_t)cap * p.S * 4);
    p.src = take((size_t)cap * p.S * 4);
    p.newidx = take((size_t)cap * 4);
    p.map = take((size_t)cap * 4);
    p.tile = take((size_t)p.tiles * 4);
    p.words = take((size_t)kSimpWords * 4);
    p.total = at;
    return p;
}

hipError_t launch_simplify_links(const SimplifyPlan& p, void* scratch, const int32_t* child, hipStream_t stream) {
    char* base = static_cast<char*>(scratch);
    int32_t* parent = reinterpret_cast<int32_t*>(base + p.parent);
    int32_t* level = reinterpret_cast<int32_t*>(base + p.level);
    int32_t* wchild = reinterpret_cast<int32_t*>(base + p.wchild);
    int32_t* src = reinterpret_cast<int32_t*>(base + p.src);
    uint32_t* words = reinterpret_cast<uint32_t*>(base + p.words);
    hipError_t e = hipMemsetAsync(parent, 0xFF, (size_t)p.cap * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(level, 0xFF, (size_t)p.cap * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(words, 0, (size_t)kSimpWords * 4, stream);
    if (e != hipSuccess) return e;
    simp_links<<<blocks_for((size_t)p.cap * p.S), kSimplifyBlock, 0, stream>>>(child, p.cap, p.S, parent, level, wchild, src, words);
    for (int l = 0; l < kSimplifyMaxLevels; ++l)
        simp_level<<<blocks_for((size_t)p.cap), kSimplifyBlock, 0, stream>>>(p.cap, p.S, l, parent, level, words);
    return hipGetLastError();
}

hipError_t launch_simplify_rest(const SimplifyPlan& p, void* scratch, const uint16_t* data, int kill, uint32_t th, int n_levels,
                                int32_t* child_out, uint16_t* data_out, int64_t* node_map, hipStream_t stream) {
    char* base = static_cast<char*>(scratch);
    int32_t* parent = reinterpret_cast<int32_t*>(base + p.parent);
    int32_t* level = reinterpret_cast<int32_t*>(base + p.level);
    int32_t* wchild = reinterpret_cast<int32_t*>(base + p.wchild);
    int32_t* src = reinterpret_cast<int32_t*>(base + p.src);
    int32_t* newidx = reinterpret_cast<int32_t*>(base + p.newidx);
    int32_t* map = reinterpret_cast<int32_t*>(base + p.map);
    uint32_t* tile = reinterpret_cast<uint32_t*>(base + p.tile);
    uint32_t* words = reinterpret_cast<uint32_t*>(base + p.words);
    const size_t slots = (size_t)p.cap * p.S;
    if (kill) simp_kill<<<blocks_for(slots), kSimplifyBlock, 0, stream>>>(data, p.cap, p.S, p.D, th, level, wchild, src, words);
    for (int l = n_levels - 1; l >= 1; --l) {
        if (p.S == 8)
            simp_merge8<<<blocks_for((size_t)p.cap * 8), kSimplifyBlock, 0, stream>>>(data, p.cap, p.D, l, parent, level, wchild, src, words);
        else
            simp_merge<<<blocks_for((size_t)p.cap), kSimplifyBlock, 0, stream>>>(data, p.cap, p.S, p.D, l, parent, level, wchild, src, words);
    }
    simp_count<<<(unsigned)p.tiles, kSimplifyBlock, 0, stream>>>(p.cap, level, tile, words);
    simp_tile_scan<<<1, kSimplifyBlock, 0, stream>>>(tile, p.tiles, words);
    simp_index<<<(unsigned)p.tiles, kSimplifyBlock, 0, stream>>>(p.cap, level, tile, newidx, map);
    simp_child<<<blocks_for(slots), kSimplifyBlock, 0, stream>>>(p.cap, p.S, wchild, newidx, map, words, child_out, node_map);
    const size_t halves = slots * (size_t)p.D;
    const bool wide = (size_t)p.S * p.D % 8 == 0 && (((uintptr_t)data | (uintptr_t)data_out) & 15u) == 0;
    if (wide)
        simp_data16<<<blocks_for(halves / 8), kSimplifyBlock, 0, stream>>>(data, p.S, p.D, (int)((size_t)p.S * p.D / 8), src, map, words, data_out);
    else
        simp_data2<<<blocks_for(halves), kSimplifyBlock, 0, stream>>>(data, p.S, p.D, src, map, words, data_out);
    return hipGetLastError();
}

}  // namespace rto
