// rto_refine_launch.h -- host-callable launchers of the tree refiner's kernels (refine_kernels.hip) and the layout of their
// scratch.  Apart from rto_launch.h for the reason rto_quantize_launch.h is.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rto {

constexpr int kRefineBlock = 256;   // threads of every workgroup
constexpr int kRefineTile = 1024;   // slots of one workgroup in the histograms and the scans, 4 consecutive slots per thread
constexpr int kRefineBins = 256;    // one 8-bit digit of the key per pass of the select
constexpr int kRefinePasses = 4;

// the words the host reads back (uint32 each, at plan.words)
enum RefineWord {
    kRefBadRange = 0,    // 1 + the slot of a link outside [1, cap) (the largest such slot), 0 = none
    kRefBadShared = 1,   // 1 + the largest slot that found its target already taken, 0 = none
    kRefCandidates = 2,  // C
    kRefMode = 3,        // 0: the select runs, 1: every candidate is taken, 2: none is
    kRefPrefix = 4,      // the digits of the cut picked so far
    kRefRemain = 5,      // how many keys with that prefix are still to be taken
    kRefCut = 6,         // cut_key as the flag kernels use it (mode 1: 0, mode 2: 0xFFFFFFFF)
    kRefRem = 7,         // rem as the flag kernels use it (mode 1: 0xFFFFFFFF, mode 2: 0)
    kRefLevelCount = 8,  // [33]: nodes per level 0 .. 32
    kRefMinKey = 41,     // the smallest key of a candidate (0xFFFFFFFF without one)
    kRefSelected = 42,   // K
    kRefDeepest = 43,    // the deepest level of a new node
    kRefWords = 48,
};

// Offsets are bytes into the handle's scratch, each aligned to 256.
struct RefinePlan {
    int64_t cap = 0;
    int N = 0, S = 0, tiles = 0;
    size_t parent = 0;  // int32 [cap]: the slot that refers to the node, -1 = none
    size_t level = 0;   // int32 [cap]: -1 = not reached
    size_t rank = 0;    // int32 [cap * S]: j of a selected slot, -1 otherwise
    size_t picked = 0;  // int32 [cap * S]: the slot with rank j (K <= cap * S of them)
    size_t tile = 0;    // uint64 [tiles]: (equal << 32 | above) per tile, then their exclusive prefix
    size_t hist = 0;    // uint32 [kRefinePasses][kRefineBins]
    size_t words = 0;   // uint32 [kRefWords]
    size_t total = 0;
};
RefinePlan refine_plan(int64_t cap, int N);

// Everything is enqueued on `stream`.  Pass 1: links, levels, the select, the flags and the ranks; the caller reads the words back.
hipError_t launch_refine_plan(const RefinePlan& plan, void* scratch, const int32_t* child, const uint32_t* key, uint32_t key_thresh,
                              int64_t max_new, int max_level, hipStream_t stream);
// Pass 2: the outputs of cap + K nodes (slot_src may be null).
hipError_t launch_refine_write(const RefinePlan& plan, const void* scratch, int64_t K, const int32_t* child, const uint16_t* data, int D,
                               int32_t* child_out, uint16_t* data_out, int32_t* slot_src, hipStream_t stream);

}  // namespace rto
