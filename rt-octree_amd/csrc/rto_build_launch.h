// rto_build_launch.h -- host-callable launchers of the grid builder's kernels (build_kernels.hip) and the layout of their
// scratch.  Apart from rto_launch.h for the reason rto_quantize_launch.h is.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "host/grid_build.h"

namespace rto {

constexpr int kBuildBlock = 256;  // threads of every workgroup, and the nodes of one tile of the scans (one node per thread)

// the words the host reads back (uint32 each, at plan.words)
enum BuildWord {
    kBuildKilled = 0,      // [2]: one 64-bit count
    kBuildLevelCount = 2,  // [kGridBuildMaxL]: nodes per level 0 .. L - 1
    kBuildWords = 16,
};

// Offsets are bytes into the handle's scratch, each aligned to 256.  A level holds at most 8^l nodes and 8^l cells.
struct BuildPlan {
    int L = 0, D = 0;
    size_t flags[kGridBuildMaxL] = {};  // uint8 [8^l], levels 0 .. L - 1: the flag of every cell, in Morton order
    size_t list[kGridBuildMaxL] = {};   // uint32 [8^l], levels 0 .. L - 1: the Morton codes of the level's nodes, ascending
    size_t tile[kGridBuildMaxL] = {};   // uint32 [ceil(8^l / 256)], levels 0 .. L - 2: child nodes per tile, then their exclusive prefix
    size_t words = 0;                   // uint32 [kBuildWords]
    size_t total = 0;
};
BuildPlan build_plan(int L, int D);

// the node counts of a finished plan: start[l] = the index of the first node of level l, start[levels .. ] = nodes
struct BuildCounts {
    uint32_t start[kGridBuildMaxL + 1] = {};
    int levels = 0;
};

// Everything is enqueued on `stream`.  Pass 1: the flags of every level from the finest up, then the node lists from the root
// down; the caller reads the words back.
hipError_t launch_build_plan(const BuildPlan& plan, void* scratch, const GridView& g, hipStream_t stream);
// Pass 2: the offsets level by level, then the records.
hipError_t launch_build_write(const BuildPlan& plan, const void* scratch, const GridView& g, const BuildCounts& counts,
                              int32_t* child_out, uint16_t* data_out, hipStream_t stream);

}  // namespace rto
