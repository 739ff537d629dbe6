// quantize_kernels.hip -- the deterministic median cut of include/rto.h "quantiser" for gfx950.
//
// Boxes are contiguous segments of a row permutation, box b of level l at [start_l[b], start_l[b + 1]): a box of cnt rows always
// splits into (cnt + 1) / 2 and cnt / 2, so every boundary of every level follows from m alone (mc_starts).  All boxes of a level
// hold floor or ceil of m / 2^l rows, so a level is either "big" or "small" as a whole:
//   big (some box above kQuantSmall rows): grid-wide passes over tiles of one box each, kernel boundaries the only grid-wide
//     synchronisation -- min / max of the three keys (mc_minmax), radix select of the median key on the widest axis in two 8-bit
//     histogram passes (mc_hist<1>, mc_select<1>, mc_hist<2>, mc_select<2>), rows below / equal to it per tile (mc_count) and
//     their prefix over the box's tiles (mc_tile_scan), then a stable partition (mc_scatter).  The partition keeps the original
//     row order inside a box, so the rank of a tie by row index is its rank by position.  Across workgroups only integer
//     atomics on per-box words, each after a reduction in LDS (one atomic per workgroup and word).
//   small: one workgroup per box loads it into LDS and runs ALL remaining rounds there (mc_small): rows carry their index, a
//     round ranks every row among its sub-box by (key, row) and moves it to that rank; then ids and the palette are written.
// When the rounds end while boxes are still big, mc_final_big / mc_palette_big write ids and palette instead.
// The arithmetic of the definition (keys, widest axis, palette rounding) is host/median_cut.h, shared with the host twin.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "host/median_cut.h"
#include "rto_quantize_launch.h"

namespace rto {
namespace {

constexpr int kItems = kQuantTile / kQuantBlock;  // consecutive rows per thread in the order-preserving passes
constexpr int kSmallItems = kQuantSmall / kQuantBlock;
// words of a box's record (kQuantSegWords each)
constexpr int kSegMinInv = 0, kSegMax = 3, kSegBucket = 6, kSegBelowBucket = 7, kSegKey = 8, kSegTiesDown = 9, kSegHist = 16;

__host__ __device__ inline size_t starts_offset(int level) { return ((size_t)1 << level) - 1 + (size_t)level; }
__device__ inline uint32_t key_of(uint64_t k, int axis) { return (uint32_t)(k >> (16 * axis)) & 0xFFFFu; }

__device__ inline int seg_axis(const uint32_t* seg) {
    uint32_t lo[3], hi[3];
    for (int c = 0; c < 3; ++c) lo[c] = 0xFFFFu - seg[kSegMinInv + c], hi[c] = seg[kSegMax + c];
    return mc_widest_axis(lo, hi);
}

// exclusive prefix of v over the workgroup's 256 threads (in thread order) and the total; buf: 256 words of LDS
__device__ inline uint64_t block_scan(uint64_t v, uint64_t* buf, uint64_t* total) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int d = 1; d < kQuantBlock; d <<= 1) {
        const uint64_t add = t >= d ? buf[t - d] : 0;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    const uint64_t incl = buf[t];
    *total = buf[kQuantBlock - 1];
    __syncthreads();
    return incl - v;
}

// the tile of this workgroup: box `seg` of the level and the positions [s, e) of it (empty for the spare tile of a short box)
struct Tile {
    uint32_t seg, seg_start, seg_end, s, e;
};
__device__ inline Tile tile_of(const uint32_t* start, uint32_t tiles_per_seg) {
    Tile t;
    t.seg = blockIdx.x / tiles_per_seg;
    t.seg_start = start[t.seg], t.seg_end = start[t.seg + 1];
    const uint64_t s = (uint64_t)t.seg_start + (uint64_t)(blockIdx.x % tiles_per_seg) * kQuantTile;
    t.s = (uint32_t)(s < t.seg_end ? s : t.seg_end);
    t.e = (uint32_t)(s + kQuantTile < t.seg_end ? s + kQuantTile : t.seg_end);
    return t;
}

__global__ __launch_bounds__(kQuantBlock) void mc_prepare(const uint16_t* __restrict__ rows, uint32_t m, uint64_t* __restrict__ keys,
                                                          uint32_t* __restrict__ row_of, uint32_t* __restrict__ flags) {
    __shared__ uint32_t bad, max_abs;
    if (threadIdx.x == 0) bad = 0, max_abs = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * kQuantBlock + threadIdx.x;
    if (i < m) {
        uint64_t k = 0;
        uint32_t my_bad = 0, my_max = 0;
        for (int c = 0; c < 3; ++c) {
            const uint32_t h = rows[(size_t)i * 3 + c];
            my_bad |= mc_finite(h) ? 0u : 1u;
            my_max = max(my_max, h & 0x7FFFu);
            k |= (uint64_t)mc_key(h) << (16 * c);
        }
        keys[i] = k;
        row_of[i] = i;
        if (my_bad) atomicOr(&bad, 1u);
        atomicMax(&max_abs, my_max);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (bad) atomicOr(&flags[0], 1u);
        atomicMax(&flags[1], max_abs);
    }
}

// every level's box boundaries, one workgroup
__global__ __launch_bounds__(kQuantBlock) void mc_starts(uint32_t* __restrict__ st, uint32_t m, int levels) {
    if (threadIdx.x == 0) st[0] = 0, st[1] = m;
    __syncthreads();
    for (int l = 0; l < levels; ++l) {
        const uint32_t* cur = st + starts_offset(l);
        uint32_t* nxt = st + starts_offset(l + 1);
        const uint32_t nb = 1u << l;
        for (uint32_t b = threadIdx.x; b < nb; b += kQuantBlock) {
            const uint32_t s = cur[b], e = cur[b + 1];
            nxt[2 * b] = s;
            nxt[2 * b + 1] = s + (e - s + 1) / 2;
        }
        if (threadIdx.x == 0) nxt[2 * nb] = m;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kQuantBlock) void mc_minmax(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ start,
                                                         uint32_t tiles_per_seg, uint32_t* __restrict__ segs) {
    __shared__ uint32_t red[6];
    const Tile t = tile_of(start, tiles_per_seg);
    if (t.s >= t.e) return;
    if (threadIdx.x < 6) red[threadIdx.x] = 0;
    __syncthreads();
    uint32_t inv_lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (uint32_t p = t.s + threadIdx.x; p < t.e; p += kQuantBlock) {
        const uint64_t k = keys[p];
        for (int c = 0; c < 3; ++c) {
            const uint32_t kc = key_of(k, c);
            inv_lo[c] = max(inv_lo[c], 0xFFFFu - kc), hi[c] = max(hi[c], kc);
        }
    }
    for (int c = 0; c < 3; ++c) {
        atomicMax(&red[kSegMinInv + c], inv_lo[c]);
        atomicMax(&red[kSegMax + c], hi[c]);
    }
    __syncthreads();
    if (threadIdx.x < 6) atomicMax(&segs[(size_t)t.seg * kQuantSegWords + threadIdx.x], red[threadIdx.x]);
}

// PASS 1: histogram of the high byte of the key on the widest axis; PASS 2: of the low byte, among the rows of the selected bucket
template <int PASS>
__global__ __launch_bounds__(kQuantBlock) void mc_hist(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ start,
                                                       uint32_t tiles_per_seg, uint32_t* __restrict__ segs) {
    __shared__ uint32_t hist[256];
    const Tile t = tile_of(start, tiles_per_seg);
    if (t.s >= t.e) return;
    uint32_t* seg = segs + (size_t)t.seg * kQuantSegWords;
    hist[threadIdx.x] = 0;
    const int axis = seg_axis(seg);
    const uint32_t bucket = PASS == 2 ? seg[kSegBucket] : 0;
    __syncthreads();
    for (uint32_t p = t.s + threadIdx.x; p < t.e; p += kQuantBlock) {
        const uint32_t k = key_of(keys[p], axis);
        if (PASS == 1)
            atomicAdd(&hist[k >> 8], 1u);
        else if ((k >> 8) == bucket)
            atomicAdd(&hist[k & 255u], 1u);
    }
    __syncthreads();
    const uint32_t n = hist[threadIdx.x];
    if (n) atomicAdd(&seg[kSegHist + (PASS - 1) * 256 + threadIdx.x], n);
}

// one wave per box: the bin that holds the row of rank (cnt + 1) / 2 - 1
template <int PASS>
__global__ __launch_bounds__(64) void mc_select(const uint32_t* __restrict__ start, uint32_t* __restrict__ segs) {
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    uint32_t* seg = segs + (size_t)b * kQuantSegWords;
    const uint32_t cnt = start[b + 1] - start[b], half = (cnt + 1) / 2;
    if (cnt == 0) return;
    const uint32_t below = PASS == 2 ? seg[kSegBelowBucket] : 0;
    const uint32_t rank = half - 1 - below;  // among the rows this pass counted
    const uint32_t* hist = seg + kSegHist + (PASS - 1) * 256 + lane * 4;
    const uint32_t h[4] = {hist[0], hist[1], hist[2], hist[3]};
    const uint32_t mine = h[0] + h[1] + h[2] + h[3];
    uint32_t incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if ((int)lane >= d) incl += up;
    }
    uint32_t before = incl - mine;
    if (before <= rank && rank < incl) {  // exactly one lane
        int bin = 0;
        while (bin < 3 && before + h[bin] <= rank) before += h[bin], ++bin;
        if (PASS == 1) {
            seg[kSegBucket] = lane * 4 + bin;
            seg[kSegBelowBucket] = before;
        } else {
            seg[kSegKey] = seg[kSegBucket] << 8 | (lane * 4 + bin);
            seg[kSegTiesDown] = half - (below + before);  // of the rows equal to the median key, the first so many go down
        }
    }
}

__global__ __launch_bounds__(kQuantBlock) void mc_count(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ start,
                                                        uint32_t tiles_per_seg, const uint32_t* __restrict__ segs,
                                                        uint64_t* __restrict__ tiles) {
    __shared__ uint32_t red[2];
    const Tile t = tile_of(start, tiles_per_seg);
    const uint32_t* seg = segs + (size_t)t.seg * kQuantSegWords;
    if (threadIdx.x < 2) red[threadIdx.x] = 0;
    __syncthreads();
    if (t.s < t.e) {
        const int axis = seg_axis(seg);
        const uint32_t key = seg[kSegKey];
        uint32_t less = 0, eq = 0;
        for (uint32_t p = t.s + threadIdx.x; p < t.e; p += kQuantBlock) {
            const uint32_t k = key_of(keys[p], axis);
            less += k < key, eq += k == key;
        }
        if (less) atomicAdd(&red[0], less);
        if (eq) atomicAdd(&red[1], eq);
    }
    __syncthreads();
    if (threadIdx.x == 0) tiles[blockIdx.x] = (uint64_t)red[0] | (uint64_t)red[1] << 32;
}

// one workgroup per box: exclusive prefix of the tile counts over the box's tiles, in place
__global__ __launch_bounds__(kQuantBlock) void mc_tile_scan(uint32_t tiles_per_seg, uint64_t* __restrict__ tiles) {
    __shared__ uint64_t buf[kQuantBlock];
    uint64_t* mine = tiles + (size_t)blockIdx.x * tiles_per_seg;
    uint64_t carry = 0;
    for (uint32_t c0 = 0; c0 < tiles_per_seg; c0 += kQuantBlock) {
        const uint32_t i = c0 + threadIdx.x;
        const uint64_t v = i < tiles_per_seg ? mine[i] : 0;
        uint64_t total;
        const uint64_t excl = block_scan(v, buf, &total);
        if (i < tiles_per_seg) mine[i] = carry + excl;
        carry += total;
    }
}

// stable partition of every box at its median: rows below the key and the first ties_down rows equal to it go to the lower
// child, in their order; the others to the upper child, in their order
__global__ __launch_bounds__(kQuantBlock) void mc_scatter(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ row_of,
                                                          const uint32_t* __restrict__ start, uint32_t tiles_per_seg,
                                                          const uint32_t* __restrict__ segs, const uint64_t* __restrict__ tiles,
                                                          uint64_t* __restrict__ keys_out, uint32_t* __restrict__ row_out) {
    __shared__ uint64_t buf[kQuantBlock];
    const Tile t = tile_of(start, tiles_per_seg);
    if (t.s >= t.e) return;
    const uint32_t* seg = segs + (size_t)t.seg * kQuantSegWords;
    const int axis = seg_axis(seg);
    const uint32_t key = seg[kSegKey], ties_down = seg[kSegTiesDown];
    const uint32_t half = (t.seg_end - t.seg_start + 1) / 2;
    uint64_t k[kItems];
    uint32_t less = 0, eq = 0;
    const uint32_t p0 = t.s + threadIdx.x * kItems;
    for (int i = 0; i < kItems; ++i) {
        k[i] = p0 + i < t.e ? keys[p0 + i] : 0;
        if (p0 + i < t.e) {
            const uint32_t ka = key_of(k[i], axis);
            less += ka < key, eq += ka == key;
        }
    }
    uint64_t total;
    const uint64_t before = tiles[blockIdx.x] + block_scan((uint64_t)less | (uint64_t)eq << 32, buf, &total);
    uint32_t n_less = (uint32_t)before, n_eq = (uint32_t)(before >> 32);  // among the box's rows ahead of this one
    for (int i = 0; i < kItems; ++i) {
        const uint32_t p = p0 + i;
        if (p >= t.e) break;
        const uint32_t ka = key_of(k[i], axis);
        const uint32_t lower_before = n_less + min(n_eq, ties_down);
        const bool down = ka < key || (ka == key && n_eq < ties_down);
        const uint32_t dest = down ? t.seg_start + lower_before : t.seg_start + half + ((p - t.seg_start) - lower_before);
        if (dest >= t.seg_start && dest < t.seg_end) {  // (always, when the counts are the histogram's)
            keys_out[dest] = k[i];
            row_out[dest] = row_of[p];
        }
        n_less += ka < key, n_eq += ka == key;
    }
}

// ids and integer sums of the final boxes while they are still big
__global__ __launch_bounds__(kQuantBlock) void mc_final_big(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ row_of,
                                                            const uint32_t* __restrict__ start, uint32_t tiles_per_seg, uint32_t m,
                                                            unsigned long long* __restrict__ sums, uint16_t* __restrict__ ids) {
    __shared__ unsigned long long red[3];
    const Tile t = tile_of(start, tiles_per_seg);
    if (t.s >= t.e) return;
    if (threadIdx.x < 3) red[threadIdx.x] = 0;
    __syncthreads();
    int64_t sum[3] = {0, 0, 0};
    for (uint32_t p = t.s + threadIdx.x; p < t.e; p += kQuantBlock) {
        const uint64_t k = keys[p];
        for (int c = 0; c < 3; ++c) sum[c] += mc_fixed(mc_unkey(key_of(k, c)));
        const uint32_t r = row_of[p];
        if (r < m) ids[r] = (uint16_t)t.seg;
    }
    for (int c = 0; c < 3; ++c) atomicAdd(&red[c], (unsigned long long)sum[c]);
    __syncthreads();
    if (threadIdx.x < 3) atomicAdd(&sums[(size_t)t.seg * 3 + threadIdx.x], red[threadIdx.x]);
}

__global__ __launch_bounds__(kQuantBlock) void mc_palette_big(const unsigned long long* __restrict__ sums, const uint32_t* __restrict__ start,
                                                              uint32_t boxes, uint16_t* __restrict__ palette) {
    const uint32_t b = blockIdx.x * kQuantBlock + threadIdx.x;
    if (b >= boxes) return;
    const int64_t cnt = (int64_t)start[b + 1] - (int64_t)start[b];
    for (int c = 0; c < 3; ++c) palette[(size_t)b * 3 + c] = mc_palette_entry((int64_t)sums[(size_t)b * 3 + c], cnt);
}

// One workgroup per box of level `level`, at most kQuantSmall rows: `rounds` further rounds in LDS, then ids and palette.
// A position p of the LDS image belongs to the sub-box [s, e) that the halvings of the box's count give it; a round moves
// every row to s + its rank by (key on the sub-box's widest axis, row index) among the sub-box's rows.
__global__ __launch_bounds__(kQuantBlock) void mc_small(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ row_of,
                                                        const uint32_t* __restrict__ start, int rounds, uint32_t m,
                                                        uint16_t* __restrict__ palette, uint16_t* __restrict__ ids) {
    __shared__ uint64_t kk[kQuantSmall], sw[kQuantSmall];
    __shared__ uint32_t rr[kQuantSmall], mm[kQuantSmall * 6];
    const uint32_t box = blockIdx.x, base = start[box];
    const uint32_t n = start[box + 1] - base;
    if (n == 0 || n > (uint32_t)kQuantSmall) return;
    uint32_t s[kSmallItems], e[kSmallItems], rel[kSmallItems];
    for (int i = 0; i < kSmallItems; ++i) {
        const uint32_t p = threadIdx.x + i * kQuantBlock;
        s[i] = 0, e[i] = n, rel[i] = 0;
        if (p < n) kk[p] = keys[base + p], rr[p] = row_of[base + p];
    }
    __syncthreads();
    for (int r = 0; r < rounds; ++r) {
        for (int i = 0; i < kSmallItems; ++i) {
            const uint32_t p = threadIdx.x + i * kQuantBlock;
            if (p < n)
                for (int c = 0; c < 6; ++c) mm[p * 6 + c] = 0;
        }
        __syncthreads();
        for (int i = 0; i < kSmallItems; ++i) {
            const uint32_t p = threadIdx.x + i * kQuantBlock;
            if (p < n && e[i] - s[i] > 1) {
                const uint64_t k = kk[p];
                for (int c = 0; c < 3; ++c) {
                    atomicMax(&mm[s[i] * 6 + kSegMinInv + c], 0xFFFFu - key_of(k, c));
                    atomicMax(&mm[s[i] * 6 + kSegMax + c], key_of(k, c));
                }
            }
        }
        __syncthreads();
        for (int i = 0; i < kSmallItems; ++i) {
            const uint32_t p = threadIdx.x + i * kQuantBlock;
            if (p < n && e[i] - s[i] > 1) sw[p] = (uint64_t)key_of(kk[p], seg_axis(&mm[s[i] * 6])) << 32 | rr[p];
        }
        __syncthreads();
        uint64_t k_new[kSmallItems];
        uint32_t r_new[kSmallItems], dest[kSmallItems];
        for (int i = 0; i < kSmallItems; ++i) {
            const uint32_t p = threadIdx.x + i * kQuantBlock;
            dest[i] = p;
            if (p < n) {
                k_new[i] = kk[p], r_new[i] = rr[p];
                if (e[i] - s[i] > 1) {
                    const uint64_t w = sw[p];
                    uint32_t rank = 0;
                    for (uint32_t j = s[i]; j < e[i]; ++j) rank += sw[j] < w;
                    dest[i] = s[i] + rank;
                }
            }
        }
        __syncthreads();
        for (int i = 0; i < kSmallItems; ++i) {
            const uint32_t p = threadIdx.x + i * kQuantBlock;
            if (p < n) {
                if (dest[i] < n) kk[dest[i]] = k_new[i], rr[dest[i]] = r_new[i];
                const uint32_t half = (e[i] - s[i] + 1) / 2, up = p - s[i] >= half;
                if (up) s[i] += half; else e[i] = s[i] + half;
                rel[i] = rel[i] * 2 + up;
            }
        }
        __syncthreads();
    }
    for (int i = 0; i < kSmallItems; ++i) {
        const uint32_t p = threadIdx.x + i * kQuantBlock;
        if (p >= n) continue;
        const uint32_t id = (box << rounds) + rel[i];
        if (rr[p] < m) ids[rr[p]] = (uint16_t)id;
        if (p == s[i]) {  // the first row of a final box adds the box up
            int64_t sum[3] = {0, 0, 0};
            for (uint32_t j = s[i]; j < e[i]; ++j)
                for (int c = 0; c < 3; ++c) sum[c] += mc_fixed(mc_unkey(key_of(kk[j], c)));
            for (int c = 0; c < 3; ++c) palette[(size_t)id * 3 + c] = mc_palette_entry(sum[c], (int64_t)(e[i] - s[i]));
        }
    }
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline uint32_t tiles_per_seg(int64_t m, int level) {
    const int64_t max_seg = (m + ((int64_t)1 << level) - 1) >> level;  // ceil(m / 2^level)
    return (uint32_t)((max_seg + kQuantTile - 1) / kQuantTile);
}

}  // namespace

QuantPlan quantize_plan(int64_t m, int bits) {
    QuantPlan p;
    p.m = m, p.bits = bits;
    while (p.big_levels < bits && ((m + ((int64_t)1 << p.big_levels) - 1) >> p.big_levels) > kQuantSmall) ++p.big_levels;
    size_t tiles = 1;
    for (int l = 0; l <= p.big_levels; ++l) tiles = std::max(tiles, ((size_t)1 << l) * tiles_per_seg(m, l));
    size_t off = 0;
    const auto take = [&](size_t bytes) {
        const size_t at = off;
        off = align256(off + bytes);
        return at;
    };
    for (int i = 0; i < 2; ++i) p.keys[i] = take((size_t)m * 8), p.rows[i] = take((size_t)m * 4);
    p.starts = take((starts_offset(p.big_levels) + ((size_t)1 << p.big_levels) + 1) * 4);
    p.seg = take(((size_t)1 << (p.big_levels > 0 ? p.big_levels - 1 : 0)) * kQuantSegWords * 4);
    p.tiles = take(tiles * 8);
    p.sums = take(p.big_levels == bits ? ((size_t)3 << bits) * 8 : 8);
    p.flags = take(8);
    p.total = off;
    return p;
}

hipError_t launch_quantize(const QuantPlan& plan, void* scratch, const uint16_t* rows, uint16_t* palette, uint16_t* ids, hipStream_t stream) {
    char* base = static_cast<char*>(scratch);
    uint64_t* keys[2] = {(uint64_t*)(base + plan.keys[0]), (uint64_t*)(base + plan.keys[1])};
    uint32_t* row_of[2] = {(uint32_t*)(base + plan.rows[0]), (uint32_t*)(base + plan.rows[1])};
    uint32_t* starts = (uint32_t*)(base + plan.starts);
    uint32_t* segs = (uint32_t*)(base + plan.seg);
    uint64_t* tiles = (uint64_t*)(base + plan.tiles);
    unsigned long long* sums = (unsigned long long*)(base + plan.sums);
    uint32_t* flags = (uint32_t*)(base + plan.flags);
    const uint32_t m = (uint32_t)plan.m;
    const int L = plan.big_levels;
    hipError_t e;
    if ((e = hipMemsetAsync(flags, 0, 8, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(palette, 0, ((size_t)3 << plan.bits) * sizeof(uint16_t), stream)) != hipSuccess) return e;
    mc_prepare<<<(m + kQuantBlock - 1) / kQuantBlock, kQuantBlock, 0, stream>>>(rows, m, keys[0], row_of[0], flags);
    mc_starts<<<1, kQuantBlock, 0, stream>>>(starts, m, L);
    int cur = 0;
    for (int l = 0; l < L; ++l) {
        const uint32_t nb = 1u << l, tps = tiles_per_seg(plan.m, l), grid = nb * tps;
        const uint32_t* st = starts + starts_offset(l);
        if ((e = hipMemsetAsync(segs, 0, (size_t)nb * kQuantSegWords * 4, stream)) != hipSuccess) return e;
        mc_minmax<<<grid, kQuantBlock, 0, stream>>>(keys[cur], st, tps, segs);
        mc_hist<1><<<grid, kQuantBlock, 0, stream>>>(keys[cur], st, tps, segs);
        mc_select<1><<<nb, 64, 0, stream>>>(st, segs);
        mc_hist<2><<<grid, kQuantBlock, 0, stream>>>(keys[cur], st, tps, segs);
        mc_select<2><<<nb, 64, 0, stream>>>(st, segs);
        mc_count<<<grid, kQuantBlock, 0, stream>>>(keys[cur], st, tps, segs, tiles);
        mc_tile_scan<<<nb, kQuantBlock, 0, stream>>>(tps, tiles);
        mc_scatter<<<grid, kQuantBlock, 0, stream>>>(keys[cur], row_of[cur], st, tps, segs, tiles, keys[cur ^ 1], row_of[cur ^ 1]);
        cur ^= 1;
    }
    const uint32_t* st = starts + starts_offset(L);
    if (L == plan.bits) {
        const uint32_t nb = 1u << L, tps = tiles_per_seg(plan.m, L);
        if ((e = hipMemsetAsync(sums, 0, (size_t)nb * 3 * 8, stream)) != hipSuccess) return e;
        mc_final_big<<<nb * tps, kQuantBlock, 0, stream>>>(keys[cur], row_of[cur], st, tps, m, sums, ids);
        mc_palette_big<<<(nb + kQuantBlock - 1) / kQuantBlock, kQuantBlock, 0, stream>>>(sums, st, nb, palette);
    } else {
        mc_small<<<1u << L, kQuantBlock, 0, stream>>>(keys[cur], row_of[cur], st, plan.bits - L, m, palette, ids);
    }
    return hipGetLastError();
}

}  // namespace rto
