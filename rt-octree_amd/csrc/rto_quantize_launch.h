// rto_quantize_launch.h -- host-callable launcher of the median-cut kernels (quantize_kernels.hip) and the layout of their
// scratch.  Apart from rto_launch.h for the reason rto_metrics_launch.h is: the render kernels' code id changes with the render
// kernels only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rto {

constexpr int kQuantBlock = 256;      // threads of every workgroup but the bucket selection's (one wave)
constexpr int kQuantTile = 2048;      // rows of one workgroup in the grid-wide passes, 8 consecutive rows per thread
constexpr int kQuantSmall = 1024;     // a box of at most this many rows finishes all its remaining rounds in one workgroup's LDS
constexpr int kQuantSegWords = 528;   // per box and round: 6 min / max words, 4 selection words, 6 spare, 2 x 256 histogram bins

// Levels 0 .. big_levels - 1 run as grid-wide passes; at level big_levels every box holds at most kQuantSmall rows (or the
// rounds are over: big_levels == bits).  Offsets are bytes into the handle's scratch, each aligned to 256.
struct QuantPlan {
    int64_t m = 0;
    int bits = 0, big_levels = 0;
    size_t keys[2] = {0, 0};  // uint64 [m]: the three keys of a row, 16 bits each, in box order; ping and pong
    size_t rows[2] = {0, 0};  // uint32 [m]: the row's index
    size_t starts = 0;        // uint32: per level l <= big_levels the 2^l + 1 box boundaries, level l at word 2^l - 1 + l
    size_t seg = 0;           // uint32 [2^(big_levels - 1)][kQuantSegWords]
    size_t tiles = 0;         // uint64 per tile: rows below the median key | rows equal to it << 32, then their prefix
    size_t sums = 0;          // int64 [2^bits][3], only when big_levels == bits
    size_t flags = 0;         // uint32 [2]: a non-finite value was seen; the largest |value| pattern
    size_t total = 0;
};
QuantPlan quantize_plan(int64_t m, int bits);

// rows [m][3] fp16 patterns, palette [2^bits][3], ids [m]: device memory; scratch: plan.total bytes.  Everything is enqueued on
// `stream`; the caller reads the two flag words afterwards.
hipError_t launch_quantize(const QuantPlan& plan, void* scratch, const uint16_t* rows, uint16_t* palette, uint16_t* ids, hipStream_t stream);

}  // namespace rto
