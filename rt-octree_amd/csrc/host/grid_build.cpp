// grid_build.cpp -- the host twin of the grid builder (include/rto.h "grid builder"): the uniform flags bottom-up, one level at a
// time, then the nodes breadth-first.  No HIP: compiled alone by tools/sanitize/run_grid_build.sh.
#include "host/grid_build.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace rto {

namespace {

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

}  // namespace

std::string grid_build_check_args(const uint16_t* grid, int L, int D, const int32_t* child_out, const uint16_t* data_out, int64_t nodes) {
    if (!grid) return "null argument";
    if (L < 1 || L > kGridBuildMaxL) return "L must lie in 1 .. " + std::to_string(kGridBuildMaxL) + ", not " + std::to_string(L);
    if (D < 1) return "D must be at least 1, not " + std::to_string(D);
    if ((uintptr_t)grid & 1u) return "grid is not aligned to 2 bytes";
    if (!child_out && !data_out) return std::string();
    if (!child_out || !data_out) return "null argument";
    if ((uintptr_t)child_out & 3u) return "child_out is not aligned to 4 bytes";
    if ((uintptr_t)data_out & 1u) return "data_out is not aligned to 2 bytes";
    if (nodes < 0) return "room must not be negative";
    if (grid_build_too_large(nodes)) nodes = ((int64_t)1 << 28) - 1;  // (no result is larger: room beyond it is never written)
    // (D is not bounded: the products below stay within size_t for every buffer that exists)
    const size_t gb = ((size_t)1 << (3 * L)) * (size_t)D * 2, cb = (size_t)nodes * 8 * 4, db = (size_t)nodes * 8 * (size_t)D * 2;
    if (cb && (ranges_overlap(child_out, cb, grid, gb) || ranges_overlap(data_out, db, grid, gb))) return "an output overlaps an input";
    if (cb && ranges_overlap(child_out, cb, data_out, db)) return "two outputs overlap";
    return std::string();
}

int grid_build_host(const uint16_t* grid, int L, int D, float kill_thresh, int32_t* child_out, uint16_t* data_out, int64_t room,
                    int64_t* out_capacity, rto_grid_build_stats* stats, std::string* err) {
    if (!out_capacity) {
        *err = "null argument";
        return RTO_E_INVALID;
    }
    const std::string bad = grid_build_check_args(grid, L, D, child_out, data_out, child_out || data_out ? room : 0);
    if (!bad.empty()) {
        *err = bad;
        return RTO_E_INVALID;
    }
    GridView g;
    g.grid = grid, g.L = L, g.D = D;
    g.kill = std::isnan(kill_thresh) ? 0 : 1;
    g.th = g.kill ? simp_thresh_half(kill_thresh) : 0u;
    // 1. the flags of the cells of levels L - 1 .. 0, in Morton order (level 0 is computed for its count of dead voxels at
    //    L = 1 only: the root is a node whatever its flag)
    std::vector<std::vector<uint8_t>> flags((size_t)L);
    int64_t killed = 0;
    for (int l = L - 1; l >= 0; --l) {
        const uint32_t cells = 1u << (3 * l);
        flags[(size_t)l].resize(cells);
        const uint8_t* next = l < L - 1 ? flags[(size_t)l + 1].data() : nullptr;
        for (uint32_t m = 0; m < cells; ++m) {
            uint32_t x, y, z;
            gb_decode(m, l, &x, &y, &z);
            int dead = 0;
            flags[(size_t)l][m] = gb_cell_flag(g, l, x, y, z, m, next, &dead);
            killed += dead;
        }
    }
    // 2. the nodes, level by level, by Morton code within a level
    std::vector<std::vector<uint32_t>> list((size_t)L);
    list[0].push_back(0u);
    int64_t nodes = 1;
    int levels = 1;
    for (int l = 0; l + 1 < L; ++l) {
        for (const uint32_t m : list[(size_t)l])
            for (uint32_t s = 0; s < 8; ++s)
                if (flags[(size_t)l + 1][(size_t)m * 8 + s] == kCellMixed) list[(size_t)l + 1].push_back(m * 8u + s);
        if (list[(size_t)l + 1].empty()) break;
        nodes += (int64_t)list[(size_t)l + 1].size();
        levels = l + 2;
    }
    *out_capacity = nodes;
    if (stats) *stats = rto_grid_build_stats{nodes, killed, (int64_t)levels};
    if (grid_build_too_large(nodes)) {
        *err = "nodes * 8 must stay below 2^31, nodes = " + std::to_string(nodes);
        return RTO_E_INVALID;
    }
    if (!child_out) return RTO_OK;
    if (room < nodes) {
        *err = "room for " + std::to_string(room) + " nodes, the tree has " + std::to_string(nodes);
        return RTO_E_INVALID;
    }
    // 3. the slots
    int64_t start = 0;
    for (int l = 0; l < levels; ++l) {
        const std::vector<uint32_t>& here = list[(size_t)l];
        const int64_t next_start = start + (int64_t)here.size();
        const uint8_t* next = l < L - 1 ? flags[(size_t)l + 1].data() : nullptr;
        int64_t rank = 0;  // of the next child node within its level
        for (size_t i = 0; i < here.size(); ++i) {
            const int64_t n = start + (int64_t)i;
            const uint32_t m = here[i];
            for (int s = 0; s < 8; ++s) {
                const bool node = next && next[(size_t)m * 8 + s] == kCellMixed;
                child_out[n * 8 + s] = node ? (int32_t)(next_start + rank++ - n) : 0;
                uint16_t* dst = data_out + (n * 8 + s) * D;
                const int32_t from = gb_slot_src(g, l, m, s, next);
                if (from == kSimplifyZero)
                    std::memset(dst, 0, (size_t)D * 2);
                else
                    std::memcpy(dst, grid + (int64_t)from * D, (size_t)D * 2);
            }
        }
        start = next_start;
    }
    return RTO_OK;
}

}  // namespace rto
