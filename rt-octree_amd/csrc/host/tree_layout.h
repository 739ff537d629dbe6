// tree_layout.h -- host-side preparation of a tree for the kernels: breadth-first relayout, culling cells and the two-level
// traversal image.  Pure host code (no HIP): tests/test_wide_image.py runs it without a device.
// Where a function takes (sigma, stride), the fp16 density of slot sl is sigma[sl * stride]: (q_sigma, 1) for a quantised
// tree, (data + data_dim - 1, data_dim) for a dense one.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rto {
struct HostTree;  // host/n3tree_host.h
}

#pragma GCC visibility push(hidden)
namespace rto {

// IEEE binary16 -> binary32 (exact), for the host-side look at a leaf's density
float half_to_float(uint16_t h);

// The culling cells of a tree (TreeDev::occ_cells): boxes that together contain every leaf of positive density.  A dense leaf
// no finer than kOccLevel is its own cell, the cube; every node of level kOccLevel whose subtree holds a dense leaf is one cell,
// the axis-aligned bounds of those leaves inside its cube.  Eight floats each: {centre in WORLD coordinates, 0} {half-extents
// per axis, margin included, in TREE units, 0} (the box is axis-aligned in both; its world half-widths are half-extent / |scale|).
// cubes, if not null: the same cells in the same order and format with every node's whole cube for its bounds (the cells before
// the bounds: tuning "cull_cubes").  Returns false when the node order does not allow the single top-down pass (a child stored
// before its parent: cannot happen after the breadth-first relayout).
bool culling_cells(const int32_t* child, int64_t capacity, const float scale[3], const float offset[3], const uint16_t* sigma,
                   size_t stride, std::vector<float>& out, std::vector<float>* cubes = nullptr);

// Breadth-first node order of a tree: order[new] = old.  Children are visited in slot order, so after the
// renumbering the internal children of every node are consecutive, in slot order, and every level is stored
// in Morton order of its cells -- whatever order the file used (svox appends the children of
// whichever leaves a refinement step selected).  Nodes the root does not reach (spare capacity) keep their
// relative order behind the reachable ones.
std::vector<int64_t> bfs_order(const int32_t* child, int64_t capacity, int64_t N3);

// The same tree with its nodes stored in `order`: child offsets recomputed, per-slot arrays gathered.
struct Relaid {
    std::vector<int32_t> child;
    std::vector<uint16_t> data, q_map, q_sigma, q_retained;
};
void relay_tree(const std::vector<int64_t>& order, const int32_t* child, const uint16_t* data, int64_t capacity, int64_t N3,
                int data_dim, const HostTree* quant, Relaid& out);

// ---- two-level ("wide") traversal image for the batched traversal kernel (round 4) ----
// The persistent kernel visits one node per loop iteration; 0.65 of its 1.65 visits per march step are descents through
// internal nodes.  A wide node merges an octree node at level L = G + 2p (G = top-grid levels) with its eight children:
// 64 words, indexed by TWO bits per axis of the sample point, each holding what the two-level walk below that node ends in --
//   a leaf at level L (replicated into its 8 entries) or L + 1:  kLeafTag | level << 23 (kWideLevelShift) | sigma fp16   (the level rides in the
//                                                                 word because the entry no longer says which it was)
//   an internal node at level L + 2:                              the absolute index of ITS wide node
// so a walk costs one load per TWO levels.  Entry layout inside a wide node: (x2 << 4) | (y2 << 2) | z2 with x2 = the two
// bits (level L, level L + 1) of x: the eight entries below one child of the node share a 128-byte half.  Derived data:
// every (point -> leaf level, sigma, original leaf slot) answer equals the walk over child[] (tests/test_wide_image.py).
// worig[wide node] = its octree node, for translating a hit entry back to the leaf's slot in data[] / shrec[].
// ONE array holds the top grid and the wide nodes: entries [0, 8^G) are the grid cells (the "root node": G bits per axis),
// padded to whole nodes of 64; wide node k is node number grid_nodes + k of that array.  A walk is then uniform -- entry index
// = ((node << b | x bits) << b | y bits) << b | z bits with (node, b) = (0, G) at the grid and (node number, 2) below -- and an
// entry's index doubles as the hit index of its leaf.  gslot[grid cell] = the slot of a leaf cell above the grid levels.
struct WideImage {
    std::vector<uint32_t> widew, worig, gslot;
    uint32_t n_wide = 0, grid_nodes = 0;
};
// child[]: breadth-first node order, N == 2.  false: the tree has no such image (not breadth-first, too deep or too large)
bool build_wide_image(const int32_t* child, int64_t capacity, int G, const uint16_t* sigma, size_t stride,
                      WideImage& out);

// The walk of the image for n points given as 24-bit fixed-point coordinates, exactly as render_persist does it (top grid of the
// wide image, two bits per axis per wide node, hit index -> leaf slot as flush_hits translates it): the leaf each point lies in
void wide_image_lookup(const WideImage& wi, const int32_t* child, int G, const uint32_t* points, int64_t n, int32_t* out_level,
                       int64_t* out_slot, uint16_t* out_sigma);

}  // namespace rto
#pragma GCC visibility pop
