// build_kernels.hip -- the grid builder of include/rto.h "grid builder" for gfx950: a dense grid of records -> child[] / data[].
//
// Pass 1 (plan) leaves in the handle's scratch one flag per cell and level (mixed / uniform / uniform and dead, in Morton order,
// so the eight children of cell m are the bytes 8 m .. 8 m + 7 of the next level: one 64-bit load) and per level the Morton codes
// of its nodes, ascending.  Pass 2 (write) derives every output slot from those two and reads the grid for the records.
//   bld_flags_lines  the finest level, the pass that reads the whole grid: a workgroup copies four neighbouring lines of voxels
//                  to LDS in 16-byte words, lanes along z, and compares the eight records of every cell there, half by half
//                  (a grid aligned to 16 bytes, R >= 8, D <= 512; anything else takes bld_flags)
//   bld_flags      one thread per cell of level l, the coarser levels bottom-up: the eight children's flags, then their records
//                  (gb_cell_flag: the density halves first, then the records as 32-bit words, an even number of voxels apart).
//                  Threads are numbered in raster order with z fastest; the flag goes to the cell's Morton code.  At the
//                  finest level it counts the dead voxels.
//   bld_count / bld_tile_scan / bld_index   per level l = 0 .. L - 2, reduce-then-scan over tiles of 256 nodes, one node per
//                  thread: the mixed children of the level's nodes become the next level's list.  The level's count lives on
//                  the device, so the grid is fixed and the workgroups stride over the tiles there are: work proportional to
//                  nodes, and the host reads the counts back once.
//   bld_child      per level, one thread per node: the same scan within a tile plus the tile's prefix gives the rank of the
//                  node's first child; eight offsets per thread
//   bld_data16     one thread per 16-byte word of data_out (a node is 16 D bytes: whole words whatever the parity of D); the
//                  halves are gathered one by one, a record of the grid being 2-byte aligned only
//   bld_data2      one thread per half, for a data_out that is not aligned to 16 bytes
// Kernel boundaries are the only grid-wide synchronisation; the only atomics are integer counts.  The arithmetic of the
// definition is host/grid_build.h.
#include <hip/hip_runtime.h>

#include "host/grid_build.h"
#include "rto_build_launch.h"

namespace rto {
namespace {

__device__ inline size_t global_thread() { return (size_t)blockIdx.x * kBuildBlock + threadIdx.x; }

__global__ __launch_bounds__(kBuildBlock) void bld_init(uint32_t* list0, uint32_t* words) {
    if (threadIdx.x == 0 && blockIdx.x == 0) list0[0] = 0u, words[kBuildLevelCount] = 1u;
}

__global__ __launch_bounds__(kBuildBlock) void bld_flags(GridView g, int l, const uint8_t* __restrict__ next, uint8_t* __restrict__ flags,
                                                         uint32_t* words) {
    __shared__ uint32_t dead_sum;
    if (threadIdx.x == 0) dead_sum = 0;
    __syncthreads();
    const size_t t = global_thread();
    int dead = 0;
    if (t < ((size_t)1 << (3 * l))) {
        const uint32_t side = (1u << l) - 1u;
        const uint32_t z = (uint32_t)t & side, y = (uint32_t)(t >> l) & side, x = (uint32_t)(t >> (2 * l));
        const uint32_t m = gb_encode(x, y, z, l);  // below 8^l: inside flags
        flags[m] = gb_cell_flag(g, l, x, y, z, m, next, &dead);
    }
    if (dead) atomicAdd(&dead_sum, (uint32_t)dead);
    __syncthreads();
    if (threadIdx.x == 0 && dead_sum) atomicAdd(reinterpret_cast<unsigned long long*>(words + kBuildKilled), (unsigned long long)dead_sum);
}

// The finest level (l = L - 1, the pass that reads the whole grid) for a grid aligned to 16 bytes with R >= 8: a workgroup takes
// C consecutive cells along z of one cell row (x, y): four lines of voxels, (2x, 2y), (2x, 2y+1), (2x+1, 2y), (2x+1, 2y+1), each
// 2 C D halves that start at a multiple of 16 bytes (C is a multiple of 4).  It copies them to LDS in 16-byte words, lanes along
// the line, so a wave reads 1 KiB of one line per instruction whatever D is; the kill reads the density halves there; then one
// work item per (cell, half j) holds the eight halves j of the cell's records against the first, dead records counting as +0.
// The flags are those of gb_cell_flag: the same comparison, half by half instead of word by word.
// LDS: lines[4][2 C D] halves, dead[4][2 C] bytes, mixed[C] bytes (the launcher sizes it and C).
__global__ __launch_bounds__(kBuildBlock) void bld_flags_lines(GridView g, int C, uint8_t* __restrict__ flags, uint32_t* words) {
    extern __shared__ uint4 lds16[];
    const int D = g.D, L = g.L;
    const int line = 2 * C * D;  // halves of one line's segment: a multiple of 8
    uint16_t* lines = reinterpret_cast<uint16_t*>(lds16);
    uint8_t* dead = reinterpret_cast<uint8_t*>(lines + 4 * (size_t)line);
    uint8_t* mixed = dead + 8 * C;
    __shared__ uint32_t dead_sum;
    const int segs = (1 << (L - 1)) / C;  // segments per cell row
    const uint32_t seg = blockIdx.x % (uint32_t)segs, row = blockIdx.x / (uint32_t)segs;
    const uint32_t cy = row & ((1u << (L - 1)) - 1u), cx = row >> (L - 1);  // below 2^(L-1) by the grid's size
    const int c0 = (int)seg * C;
    if (threadIdx.x == 0) dead_sum = 0;
    for (int c = threadIdx.x; c < C; c += kBuildBlock) mixed[c] = 0;
    const int words_per_line = line / 8;
    for (int w = threadIdx.x; w < 4 * words_per_line; w += kBuildBlock) {
        const int r = w / words_per_line, i = w - r * words_per_line;
        // the first half of the segment of line r: 64-bit, a multiple of 8 halves from a base aligned to 16 bytes
        const int64_t first = ((int64_t)gb_voxel(g, 2 * cx + (uint32_t)(r >> 1), 2 * cy + (uint32_t)(r & 1), 0) + 2 * c0) * D;
        lds16[(size_t)r * words_per_line + i] = *reinterpret_cast<const uint4*>(g.grid + first + 8 * (int64_t)i);
    }
    __syncthreads();
    int my_dead = 0;
    for (int v = threadIdx.x; v < 8 * C; v += kBuildBlock) {  // v = line * 2 C + voxel of the segment
        const int r = v / (2 * C), k = v - r * 2 * C;
        const bool d = g.kill && !simp_half_gt(lines[(size_t)r * line + (size_t)k * D + D - 1], g.th);
        dead[v] = d ? 1 : 0;
        my_dead += d ? 1 : 0;
    }
    if (my_dead) atomicAdd(&dead_sum, (uint32_t)my_dead);
    __syncthreads();
    for (int i = threadIdx.x; i < C * D; i += kBuildBlock) {
        const int c = i / D, j = i - c * D;
        const uint32_t ref = dead[2 * c] ? 0u : lines[(size_t)(2 * c) * D + j];
        bool differs = false;
#pragma unroll
        for (int s = 1; s < 8; ++s) {  // s = 4 dx + 2 dy + dz: line 2 dx + dy, voxel 2 c + dz
            const int r = s >> 1, k = 2 * c + (s & 1);
            const uint32_t h = dead[r * 2 * C + k] ? 0u : lines[(size_t)r * line + (size_t)k * D + j];
            differs = differs || h != ref;
        }
        if (differs) mixed[c] = 1;  // (every writer stores the same value)
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += kBuildBlock) {
        int n_dead = 0;
        for (int s = 0; s < 8; ++s) n_dead += dead[(s >> 1) * 2 * C + 2 * c + (s & 1)];
        // below 8^(L-1): inside flags
        flags[gb_encode(cx, cy, (uint32_t)(c0 + c), L - 1)] = n_dead == 8 ? kCellDead : mixed[c] ? kCellMixed : kCellUniform;
    }
    if (threadIdx.x == 0 && dead_sum) atomicAdd(reinterpret_cast<unsigned long long*>(words + kBuildKilled), (unsigned long long)dead_sum);
}

// the mixed children of the node of cell m, one bit per slot; next: the flags of the next level
__device__ inline uint32_t mixed_mask(const uint8_t* __restrict__ next, uint32_t m) {
    const uint64_t f = *reinterpret_cast<const uint64_t*>(next + (size_t)m * 8);  // (every level's flags start 256-aligned)
    uint32_t mask = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s) mask |= ((f >> (8 * s)) & 0xFFu) == kCellMixed ? 1u << s : 0u;
    return mask;
}

// exclusive prefix of v over the workgroup's threads (in thread order) and the total; buf: kBuildBlock words of LDS
__device__ inline uint32_t block_scan(uint32_t v, uint32_t* buf, uint32_t* total) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int d = 1; d < kBuildBlock; d <<= 1) {
        const uint32_t add = t >= d ? buf[t - d] : 0;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    const uint32_t incl = buf[t];
    *total = buf[kBuildBlock - 1];
    __syncthreads();
    return incl - v;
}

// (the trip counts of the loops over tiles depend on blockIdx and the level's count only: a workgroup's threads stay together)
__global__ __launch_bounds__(kBuildBlock) void bld_count(int l, const uint32_t* __restrict__ list, const uint8_t* __restrict__ next,
                                                         uint32_t* __restrict__ tile, const uint32_t* __restrict__ words) {
    __shared__ uint32_t buf[kBuildBlock];
    const uint32_t count = words[kBuildLevelCount + l];
    const uint32_t tiles = (count + kBuildBlock - 1) / kBuildBlock;  // at most ceil(8^l / 256): inside tile
    for (uint32_t b = blockIdx.x; b < tiles; b += gridDim.x) {
        const uint32_t i = b * kBuildBlock + threadIdx.x;
        const uint32_t c = i < count ? (uint32_t)__popc(mixed_mask(next, list[i])) : 0u;
        uint32_t total;
        (void)block_scan(c, buf, &total);
        if (threadIdx.x == 0) tile[b] = total;
    }
}

// one workgroup: the tiles' counts -> their exclusive prefix, in chunks of kBuildBlock with a carry; the total is the next
// level's count
__global__ __launch_bounds__(kBuildBlock) void bld_tile_scan(int l, uint32_t* tile, uint32_t* words) {
    __shared__ uint32_t buf[kBuildBlock];
    const uint32_t count = words[kBuildLevelCount + l];
    const uint32_t tiles = (count + kBuildBlock - 1) / kBuildBlock;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < tiles; base += kBuildBlock) {
        const uint32_t b = base + threadIdx.x;
        const uint32_t v = b < tiles ? tile[b] : 0;
        uint32_t total;
        const uint32_t ex = block_scan(v, buf, &total);
        if (b < tiles) tile[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) words[kBuildLevelCount + l + 1] = carry;
}

__global__ __launch_bounds__(kBuildBlock) void bld_index(int l, const uint32_t* __restrict__ list, const uint8_t* __restrict__ next,
                                                         const uint32_t* __restrict__ tile, const uint32_t* __restrict__ words,
                                                         uint32_t* __restrict__ list_next) {
    __shared__ uint32_t buf[kBuildBlock];
    const uint32_t count = words[kBuildLevelCount + l];
    const uint32_t tiles = (count + kBuildBlock - 1) / kBuildBlock;
    for (uint32_t b = blockIdx.x; b < tiles; b += gridDim.x) {
        const uint32_t i = b * kBuildBlock + threadIdx.x;
        const uint32_t m = i < count ? list[i] : 0u;
        const uint32_t mask = i < count ? mixed_mask(next, m) : 0u;
        uint32_t total;
        uint32_t at = tile[b] + block_scan((uint32_t)__popc(mask), buf, &total);
        for (uint32_t s = 0; s < 8; ++s)
            if ((mask >> s) & 1u) list_next[at++] = m * 8u + s;  // at < the next level's count <= 8^(l + 1): inside list_next
    }
}

// next == nullptr: the level's nodes have no child nodes (the deepest level that holds nodes)
__global__ __launch_bounds__(kBuildBlock) void bld_child(uint32_t count, uint32_t start, uint32_t start_next, const uint32_t* __restrict__ list,
                                                         const uint8_t* __restrict__ next, const uint32_t* __restrict__ tile,
                                                         int32_t* __restrict__ child_out) {
    __shared__ uint32_t buf[kBuildBlock];
    const uint32_t i = blockIdx.x * kBuildBlock + threadIdx.x;
    const uint32_t mask = i < count && next ? mixed_mask(next, list[i]) : 0u;
    uint32_t total;
    const uint32_t ex = block_scan((uint32_t)__popc(mask), buf, &total);
    if (i >= count) return;
    const uint32_t n = start + i;  // below nodes: inside child_out
    uint32_t to = start_next + (next ? tile[blockIdx.x] : 0u) + ex;
    int32_t out[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) out[s] = (mask >> s) & 1u ? (int32_t)(to++ - n) : 0;
    int4* dst = reinterpret_cast<int4*>(child_out + (size_t)n * 8);  // (child_out is 4-byte aligned only)
    if (((uintptr_t)dst & 15u) == 0) {
        dst[0] = make_int4(out[0], out[1], out[2], out[3]);
        dst[1] = make_int4(out[4], out[5], out[6], out[7]);
    } else {
#pragma unroll
        for (int s = 0; s < 8; ++s) child_out[(size_t)n * 8 + s] = out[s];
    }
}

// what the record kernels need of a finished plan
struct BuildTree {
    GridView g;
    uint32_t start[kGridBuildMaxL + 1];
    const uint32_t* list[kGridBuildMaxL];
    const uint8_t* flags[kGridBuildMaxL + 1];  // flags[l + 1] = the children of level l, nullptr behind the finest level
    int levels;
};

__device__ inline int level_of(const BuildTree& t, uint32_t n) {
    int l = 0;
    while (l + 1 < t.levels && n >= t.start[l + 1]) ++l;
    return l;
}

union Word16 {
    uint4 v;
    uint16_t h[8];
};

__global__ __launch_bounds__(kBuildBlock) void bld_data16(BuildTree t, size_t n_words, uint16_t* __restrict__ data_out) {
    const size_t w = global_thread();  // the 16-byte word of the output; a node holds D of them
    if (w >= n_words) return;
    const int D = t.g.D;
    const uint32_t n = (uint32_t)(w / (size_t)D);
    const int l = level_of(t, n);
    const uint32_t m = t.list[l][n - t.start[l]];
    int h = (int)(w % (size_t)D) * 8;
    int s = h / D, j = h - s * D;
    int32_t from = gb_slot_src(t.g, l, m, s, t.flags[l + 1]);
    Word16 x;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        x.h[k] = from == kSimplifyZero ? (uint16_t)0 : t.g.grid[(int64_t)from * D + j];
        if (++j == D && k < 7) {
            j = 0, ++s;  // 8 (w % D) + 7 < 8 D: s stays below 8
            from = gb_slot_src(t.g, l, m, s, t.flags[l + 1]);
        }
    }
    reinterpret_cast<uint4*>(data_out)[w] = x.v;
}

__global__ __launch_bounds__(kBuildBlock) void bld_data2(BuildTree t, size_t n_halves, uint16_t* __restrict__ data_out) {
    const size_t i = global_thread();  // the half of the output
    if (i >= n_halves) return;
    const int D = t.g.D;
    const size_t per_node = (size_t)8 * D;
    const uint32_t n = (uint32_t)(i / per_node);
    const int r = (int)(i % per_node), s = r / D, j = r - s * D;
    const int l = level_of(t, n);
    const int32_t from = gb_slot_src(t.g, l, t.list[l][n - t.start[l]], s, t.flags[l + 1]);
    data_out[i] = from == kSimplifyZero ? (uint16_t)0 : t.g.grid[(int64_t)from * D + j];
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline unsigned blocks_for(size_t threads) { return (unsigned)((threads + kBuildBlock - 1) / kBuildBlock); }
inline size_t tiles_of_level(int l) { return (((size_t)1 << (3 * l)) + kBuildBlock - 1) / kBuildBlock; }

constexpr unsigned kMaxStrideBlocks = 2048;  // the fixed grid of the kernels whose work the device counts

}  // namespace

BuildPlan build_plan(int L, int D) {
    BuildPlan p;
    p.L = L, p.D = D;
    size_t at = 0;
    const auto take = [&](size_t bytes) {
        const size_t o = at;
        at = align256(at + bytes);
        return o;
    };
    for (int l = 0; l < L; ++l) p.flags[l] = take((size_t)1 << (3 * l));
    for (int l = 0; l < L; ++l) p.list[l] = take(((size_t)1 << (3 * l)) * 4);
    for (int l = 0; l + 1 < L; ++l) p.tile[l] = take(tiles_of_level(l) * 4);
    p.words = take((size_t)kBuildWords * 4);
    p.total = at;
    return p;
}

hipError_t launch_build_plan(const BuildPlan& p, void* scratch, const GridView& g, hipStream_t stream) {
    char* base = static_cast<char*>(scratch);
    const auto flags = [&](int l) { return reinterpret_cast<uint8_t*>(base + p.flags[l]); };
    const auto list = [&](int l) { return reinterpret_cast<uint32_t*>(base + p.list[l]); };
    const auto tile = [&](int l) { return reinterpret_cast<uint32_t*>(base + p.tile[l]); };
    uint32_t* words = reinterpret_cast<uint32_t*>(base + p.words);
    const hipError_t e = hipMemsetAsync(words, 0, (size_t)kBuildWords * 4, stream);
    if (e != hipSuccess) return e;
    bld_init<<<1, kBuildBlock, 0, stream>>>(list(0), words);
    // (level 0 only at L = 1, for its count of dead voxels: the root is a node whatever its flag)
    // the finest level by lines where they can be read in 16-byte words: C cells per workgroup, a power of two from 4 up to the
    // cells of a row, four lines of 2 C D halves within 32 KiB of LDS
    int C = 0;
    if (p.L >= 3 && ((uintptr_t)g.grid & 15u) == 0 && p.D <= 512) {
        C = 4;
        while (2 * C <= (1 << (p.L - 1)) && 2 * C * p.D <= 2048) C *= 2;
    }
    for (int l = p.L - 1; l >= (p.L == 1 ? 0 : 1); --l) {
        if (l == p.L - 1 && C) {
            const size_t lds = (size_t)16 * C * p.D + (size_t)9 * C;
            const unsigned blocks = (unsigned)((((size_t)1 << (2 * l)) << l) / (size_t)C);
            bld_flags_lines<<<blocks, kBuildBlock, lds, stream>>>(g, C, flags(l), words);
        } else {
            bld_flags<<<blocks_for((size_t)1 << (3 * l)), kBuildBlock, 0, stream>>>(g, l, l + 1 < p.L ? flags(l + 1) : nullptr, flags(l), words);
        }
    }
    for (int l = 0; l + 1 < p.L; ++l) {
        const unsigned blocks = (unsigned)(tiles_of_level(l) < kMaxStrideBlocks ? tiles_of_level(l) : kMaxStrideBlocks);
        bld_count<<<blocks, kBuildBlock, 0, stream>>>(l, list(l), flags(l + 1), tile(l), words);
        bld_tile_scan<<<1, kBuildBlock, 0, stream>>>(l, tile(l), words);
        bld_index<<<blocks, kBuildBlock, 0, stream>>>(l, list(l), flags(l + 1), tile(l), words, list(l + 1));
    }
    return hipGetLastError();
}

hipError_t launch_build_write(const BuildPlan& p, const void* scratch, const GridView& g, const BuildCounts& c, int32_t* child_out,
                              uint16_t* data_out, hipStream_t stream) {
    const char* base = static_cast<const char*>(scratch);
    BuildTree t;
    t.g = g;
    t.levels = c.levels;
    for (int l = 0; l <= kGridBuildMaxL; ++l) t.start[l] = c.start[l], t.flags[l] = nullptr;
    for (int l = 0; l < kGridBuildMaxL; ++l) t.list[l] = nullptr;
    for (int l = 0; l < p.L; ++l) {
        t.list[l] = reinterpret_cast<const uint32_t*>(base + p.list[l]);
        t.flags[l] = reinterpret_cast<const uint8_t*>(base + p.flags[l]);
    }
    const uint32_t nodes = c.start[c.levels];
    for (int l = 0; l < c.levels; ++l) {
        const uint32_t count = c.start[l + 1] - c.start[l];
        const bool has_children = l + 1 < c.levels;
        bld_child<<<blocks_for(count), kBuildBlock, 0, stream>>>(count, c.start[l], c.start[l + 1], t.list[l], has_children ? t.flags[l + 1] : nullptr,
                                                                  has_children ? reinterpret_cast<const uint32_t*>(base + p.tile[l]) : nullptr,
                                                                  child_out);
    }
    if (((uintptr_t)data_out & 15u) == 0) {
        const size_t n_words = (size_t)nodes * (size_t)p.D;
        bld_data16<<<blocks_for(n_words), kBuildBlock, 0, stream>>>(t, n_words, data_out);
    } else {
        const size_t n_halves = (size_t)nodes * 8 * (size_t)p.D;
        bld_data2<<<blocks_for(n_halves), kBuildBlock, 0, stream>>>(t, n_halves, data_out);
    }
    return hipGetLastError();
}

}  // namespace rto
