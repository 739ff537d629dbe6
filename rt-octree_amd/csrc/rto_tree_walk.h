// rto_tree_walk.h -- the walk from a point to the leaf that holds it, over whatever the tree has resident (the two-level image,
// the one-level image or child[]).  query_kernels.hip (rto_tree_query, the probe) and grid_kernels.hip (rto_draw_grid_layers)
// include it; the functions are force-inlined.  Include it behind the translation unit's `#pragma clang fp contract(off)`.
//
// The integer walk names the leaf the float descent reaches: after the clamp to [0, 1 - 1e-6] every operation of the descent
// (x *= 2; floor; x -= floor) is exact in fp32, so the child digit at level l is bit 23 - l of floor(x * 2^24) -- for the 24
// levels those bits last, which is the depth the upload builds a traversal image for.
#pragma once
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"
#include "rto_tree_device.h"
#include "rto_launch.h"

#pragma clang fp contract(off)

namespace rto {

constexpr float kPos24f = 16777216.f;  // a clamped coordinate times 2^24 is its 24-bit fixed point, exactly

// what one point's walk ends in
struct Leaf {
    uint32_t index;   // kWalkWide: entry of the two-level image; else the leaf's slot in child[] / data[]
    uint32_t sigma;   // fp16 bits
    int level;        // levels of child[] visited (root's children: 1); -1: not answered
    float cube[4];    // min corner in tree coordinates, side
};

// xyz = offset + scale * p (volrend.cu:220-222), the reference's clamp, then the walk.  TREE_SPACE: p is in tree coordinates
// already (xyz = p)
template <bool TREE_SPACE = false>
RTO_DEV Leaf walk_point(const TreeDev& tree, int walk, const float* p) {
    Leaf r;
    r.index = 0u;
    r.sigma = 0u;
    r.level = -1;
    r.cube[0] = r.cube[1] = r.cube[2] = r.cube[3] = 0.f;
    if (!(__builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]))) return r;
    float xyz[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) xyz[i] = TREE_SPACE ? p[i] : tree.offset[i] + tree.scale[i] * p[i];
    if (walk == kWalkChild) {
        float cube_sz;
        float local[3] = {xyz[0], xyz[1], xyz[2]};
#pragma unroll
        for (int i = 0; i < 3; ++i) xyz[i] = f_max(f_min(xyz[i], 1.f - 1e-6f), 0.f);  // (what query_from_root does to `local`)
        const int64_t slot = query_from_root(tree, local, cube_sz);
        r.index = (uint32_t)slot;
        r.sigma = tree.data[slot * tree.data_dim + tree.data_dim - 1];
        // cube_sz = N^level: count the multiplications back (exact while N^level is a float, far beyond any tree's depth)
        int level = 1;
        for (float c = (float)tree.N; c < cube_sz; c *= (float)tree.N) ++level;
        r.level = level;
#pragma unroll
        for (int i = 0; i < 3; ++i) r.cube[i] = xyz[i] - local[i] / cube_sz;
        r.cube[3] = 1.f / cube_sz;
        return r;
    }
    uint32_t q[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = (uint32_t)(f_max(f_min(xyz[i], 1.f - 1e-6f), 0.f) * kPos24f);  // (exact product, < 2^24)
    int level0 = -1;  // the leaf's node level, root = 0
    if (walk == kWalkWide) {
        // wide_entry_of's walk, keeping the leaf word: G bits per axis at the grid, two per wide node below
        const int G = tree.top_levels;
        uint32_t node = 0u, u = 0u, w = 0u;
        for (int pr = -1; pr < 12; ++pr) {
            const uint32_t b = node ? 2u : (uint32_t)G, msk = (1u << b) - 1u;
            const uint32_t off = node ? (uint32_t)(22 - G - 2 * pr) : 24u - (uint32_t)G;
            u = (((node << b | ((q[0] >> off) & msk)) << b | ((q[1] >> off) & msk)) << b) | ((q[2] >> off) & msk);
            w = tree.widew[u];
            if (nodew_is_leaf(w)) break;
            node = w;
        }
        if (!nodew_is_leaf(w)) return r;  // (cannot happen: the image covers at most 24 levels)
        r.index = u;
        r.sigma = w & 0xffffu;
        level0 = (int)((w & kWideLevelMask) >> kWideLevelShift);
    } else {  // kWalkNodew: the top grid's cell, then one word per level
        const int G = tree.topgrid ? tree.top_levels : 0;
        uint32_t node = 0u, slot = 0u, w = 0u;
        int l = 0;
        bool leaf = false;
        if (G > 0) {
            const uint32_t sh = 24u - (uint32_t)G;
            const uint2 e = tree.topgrid[((q[0] >> sh) << (2 * G)) | ((q[1] >> sh) << G) | (q[2] >> sh)];
            slot = e.x & kGridSlotMask;
            w = e.y;
            l = (int)(e.x >> kGridSlotBits);
            leaf = nodew_is_leaf(w);
            if (!leaf) {  // internal at level G - 1
                node = (slot >> 3) + w;
                l = G;
            }
        }
        for (; !leaf && l < 24; ++l) {
            const int b = 23 - l;
            slot = node * 8u + ((((q[0] >> b) & 1u) << 2) | (((q[1] >> b) & 1u) << 1) | ((q[2] >> b) & 1u));
            w = tree.nodew[slot];
            if (nodew_is_leaf(w)) {
                leaf = true;
                break;
            }
            node += w;
        }
        if (!leaf) return r;  // (cannot happen: the upload builds the image for trees of depth <= 24 only)
        r.index = slot;
        r.sigma = w & 0xffffu;
        level0 = l;
    }
    r.level = level0 + 1;
    const uint32_t sh = 23u - (uint32_t)level0;  // bits of q below the leaf's cell
#pragma unroll
    for (int i = 0; i < 3; ++i) r.cube[i] = (float)((q[i] >> sh) << sh) * (1.f / kPos24f);
    r.cube[3] = __uint_as_float((uint32_t)(127 - r.level) << 23);  // 2^-level = 1 / cube_sz
    return r;
}

}  // namespace rto
