// grid_build.h -- the grid builder of include/rto.h "grid builder": the arithmetic both implementations share (Morton codes of
// cells, the kill, the uniform flag of a cell, the source of a slot's record) and the host twin.
// Plain C++17, no HIP include: g++ compiles host/grid_build.cpp alone (tools/sanitize/run_grid_build.sh); the kernels
// (build_kernels.hip) include this header for the RTO_MC_HD functions, so both sides run the same statements.  The threshold,
// its comparison and the bit compare of two records are the simplifier's (host/tree_simplify.h).
#pragma once
#include <cstdint>
#include <string>

#include "host/tree_simplify.h"
#include "rto.h"

namespace rto {

constexpr int kGridBuildMaxL = 10;  // R = 2^L <= 1024: a voxel index stays below 2^30, a Morton code of a cell as well

// the flag of a cell (one byte per cell and level, in Morton order)
constexpr uint8_t kCellMixed = 0;    // not uniform: the cell becomes a node
constexpr uint8_t kCellUniform = 1;  // uniform
constexpr uint8_t kCellDead = 2;     // uniform, and every voxel of it is dead: its record is D halves +0 without reading one

struct GridView {
    const uint16_t* grid = nullptr;  // [R][R][R][D]
    int L = 0, D = 0;
    int kill = 0;     // 0: kill_thresh was a NaN
    uint32_t th = 0;  // the threshold as an fp16 pattern
};

// the coordinates of the cell with Morton code m at level l: three bits per level, x the most significant of each triple
RTO_MC_HD void gb_decode(uint32_t m, int l, uint32_t* x, uint32_t* y, uint32_t* z) {
    uint32_t cx = 0, cy = 0, cz = 0;
    for (int b = 0; b < l; ++b) {
        cz |= ((m >> (3 * b)) & 1u) << b;
        cy |= ((m >> (3 * b + 1)) & 1u) << b;
        cx |= ((m >> (3 * b + 2)) & 1u) << b;
    }
    *x = cx, *y = cy, *z = cz;
}

RTO_MC_HD uint32_t gb_encode(uint32_t x, uint32_t y, uint32_t z, int l) {
    uint32_t m = 0;
    for (int b = 0; b < l; ++b)
        m |= (((x >> b) & 1u) << (3 * b + 2)) | (((y >> b) & 1u) << (3 * b + 1)) | (((z >> b) & 1u) << (3 * b));
    return m;
}

// the index of voxel (x, y, z), below 2^30; the index of one of its halves is 64-bit: index * D + j
RTO_MC_HD int32_t gb_voxel(const GridView& g, uint32_t x, uint32_t y, uint32_t z) {
    return (int32_t)((((int64_t)x << g.L) + (int64_t)y) << g.L) + (int32_t)z;
}

RTO_MC_HD bool gb_dead(const GridView& g, int32_t v) {
    return g.kill && !simp_half_gt(g.grid[(int64_t)v * g.D + g.D - 1], g.th);
}

// The flag of cell (x, y, z) of level l < L.  next: the flags of level l + 1 (unused at l = L - 1, where the children are
// voxels); m: the cell's Morton code.  *dead_voxels: the dead ones among the eight voxels of a cell of level L - 1, else 0.
RTO_MC_HD uint8_t gb_cell_flag(const GridView& g, int l, uint32_t x, uint32_t y, uint32_t z, uint32_t m, const uint8_t* next,
                               int* dead_voxels) {
    const bool finest = l == g.L - 1;
    const int shift = g.L - l - 1;  // a child covers 2^shift voxels per side
    int32_t src[8];
    int dead = 0;
    for (int s = 0; s < 8; ++s) {
        uint8_t f = kCellUniform;
        if (!finest) {
            f = next[(size_t)m * 8 + s];
            if (f == kCellMixed) {
                *dead_voxels = 0;
                return kCellMixed;
            }
        }
        const int32_t v = gb_voxel(g, (2 * x + (uint32_t)(s >> 2)) << shift, (2 * y + (uint32_t)((s >> 1) & 1)) << shift,
                                   (2 * z + (uint32_t)(s & 1)) << shift);
        const bool d = f == kCellDead || gb_dead(g, v);
        src[s] = d ? kSimplifyZero : v;
        dead += d ? 1 : 0;
    }
    *dead_voxels = finest ? dead : 0;
    if (dead == 8) return kCellDead;
    return simp_node_uniform(g.grid, g.D, src, 8) ? kCellUniform : kCellMixed;
}

// The voxel whose record slot s of the node of cell m at level l holds, or kSimplifyZero: a slot that refers to a node, or a
// dead record.  next: the flags of level l + 1 (unused at l = L - 1).
RTO_MC_HD int32_t gb_slot_src(const GridView& g, int l, uint32_t m, int s, const uint8_t* next) {
    if (l < g.L - 1) {
        const uint8_t f = next[(size_t)m * 8 + s];
        if (f != kCellUniform) return kSimplifyZero;
    }
    uint32_t x, y, z;
    gb_decode(m * 8u + (uint32_t)s, l + 1, &x, &y, &z);
    const int shift = g.L - l - 1;
    const int32_t v = gb_voxel(g, x << shift, y << shift, z << shift);
    return gb_dead(g, v) ? kSimplifyZero : v;
}

// The argument refusals both entries share (everything but the device checks); nodes: the room of the outputs (0 with null
// outputs).  An empty string = accepted.
std::string grid_build_check_args(const uint16_t* grid, int L, int D, const int32_t* child_out, const uint16_t* data_out, int64_t nodes);

// "nodes * 8 must stay below 2^31": the simplifier's bound on a tree
inline bool grid_build_too_large(int64_t nodes) { return nodes >= ((int64_t)1 << 28); }

// The host twin: the definition followed literally, level by level.  Host memory.  child_out == nullptr counts only.
// RTO_OK, or RTO_E_INVALID with *err set (room too small: *out_capacity is set all the same).
int grid_build_host(const uint16_t* grid, int L, int D, float kill_thresh, int32_t* child_out, uint16_t* data_out, int64_t room,
                    int64_t* out_capacity, rto_grid_build_stats* stats, std::string* err);

}  // namespace rto
