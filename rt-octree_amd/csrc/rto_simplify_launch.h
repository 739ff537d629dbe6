// rto_simplify_launch.h -- host-callable launchers of the tree simplifier's kernels (simplify_kernels.hip) and the layout of
// their scratch.  Apart from rto_launch.h for the reason rto_quantize_launch.h is.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rto {

constexpr int kSimplifyBlock = 256;   // threads of every workgroup
constexpr int kSimplifyTile = 1024;   // nodes of one workgroup in the scan of the keep flags, 4 consecutive nodes per thread

// the words the host reads back (uint32 each, at plan.words)
enum SimplifyWord {
    kSimpBadRange = 0,   // 1 + the slot of a link outside [1, cap) (the largest such slot), 0 = none
    kSimpBadShared = 1,  // 1 + the largest slot that found its target already taken, 0 = none
    kSimpKilled = 2,
    kSimpMerged = 3,
    kSimpTotal = 4,      // survivors = out_capacity
    kSimpDeepest = 5,    // the deepest level of a survivor
    kSimpLevelCount = 8, // [33]: nodes per level 0 .. 32
    kSimpWords = 48,
};

// Offsets are bytes into the handle's scratch, each aligned to 256.
struct SimplifyPlan {
    int64_t cap = 0;
    int N = 0, S = 0, D = 0, tiles = 0;
    size_t parent = 0;   // int32 [cap]: the slot that refers to the node, -1 = none
    size_t level = 0;    // int32 [cap]: -1 = not reached, -2 = merged away
    size_t wchild = 0;   // int32 [cap][S]: the offsets as the merges rewrite them
    size_t src = 0;      // int32 [cap][S]: the input slot whose record the slot holds, kSimplifyZero = a dead record
    size_t newidx = 0;   // int32 [cap]: the rank of a survivor
    size_t map = 0;      // int32 [cap]: the old index of a new node
    size_t tile = 0;     // uint32 [tiles]: survivors per tile, then their exclusive prefix
    size_t words = 0;    // uint32 [kSimpWords]
    size_t total = 0;
};
SimplifyPlan simplify_plan(int64_t cap, int N, int D);

// Everything is enqueued on `stream`.  Phase 1: links and levels; the caller reads the words back and refuses a malformed tree.
hipError_t launch_simplify_links(const SimplifyPlan& plan, void* scratch, const int32_t* child, hipStream_t stream);
// Phase 2: kill (kill != 0, th the fp16 threshold), one merge pass per level n_levels - 1 .. 1, scan, scatter.
hipError_t launch_simplify_rest(const SimplifyPlan& plan, void* scratch, const uint16_t* data, int kill, uint32_t th, int n_levels,
                                int32_t* child_out, uint16_t* data_out, int64_t* node_map, hipStream_t stream);

}  // namespace rto
