// rto_fit_launch.h -- launchers of fit_kernels.hip and fit_rays_kernels.hip (rto_tree_fit_grad / rto_tree_fit_grad_rays /
// rto_fit_sgd_step, include/rto.h "tree fit").
#pragma once
#include <hip/hip_runtime.h>

#include "rto.h"
#include "rto_fit_march.h"
#include "rto_kernel_types.h"
#include "rto_layer_pass.h"

namespace rto {

// the per-camera planes of one launch, by value beside the cameras: [H][W][3] float32 each, or nullptr
struct FitPlanes {
    const float* target[kLayerCamChunk];
    float* image[kLayerCamChunk];
};

// `frames` (1 .. kLayerCamChunk) consecutive cameras of ONE size; one lane per pixel's ray, a wave per 8x8 tile, blockIdx.z =
// camera.  walk: kWalkChild / kWalkNodew / kWalkWide of rto_launch.h.  basis: the tree's basis_dim (1, 4, 9, 16, 25), 0 for RGBA.
// params: float32 in the numbering node_old translates to (nullptr: the resident numbering); grad: nullptr = forward only;
// stats: two words or nullptr.
hipError_t launch_fit_grad(const TreeDev& tree, int walk, int basis, const fm::Opt& opt, const LayerCams& cams, const FitPlanes& planes,
                           int frames, const uint32_t* node_old, const float* params, int64_t* grad, uint64_t* stats, hipStream_t stream);

// fit_rays_kernels.hip: n (<= kFitRaysPerLaunch) rays of the caller's, one lane per ray, workgroups of `block` threads (64, 128
// or 256; kFitRaysBlock is the library's choice).  origins / dirs [n][3]; targets / out [n][3] or nullptr; the rest as above.
constexpr int64_t kFitRaysPerLaunch = (int64_t)1 << 30;
constexpr int kFitRaysBlock = 64;
hipError_t launch_fit_grad_rays(const TreeDev& tree, int walk, int basis, const fm::Opt& opt, const uint32_t* node_old, const float* params,
                                const float* origins, const float* dirs, const float* targets, float* out, int64_t n, int block,
                                int64_t* grad, uint64_t* stats, hipStream_t stream);

// params[i] -= lr * g(grad[i]); grad[i] = 0 for i < count
hipError_t launch_fit_sgd_step(float* params, int64_t* grad, int64_t count, float lr, hipStream_t stream);

// fit_sparse_kernels.hip: launch_fit_grad_rays with the touched bitmap (rto_tree_fit_grad_rays_touched): grad and touched are
// required.  mark_read: a lane reads the bitmap word and issues its atomicOr only when the bit is clear (the library's choice;
// false is the measuring hook of tools/fit_sparse_bench.py -- the bytes do not depend on it).
hipError_t launch_fit_grad_rays_touched(const TreeDev& tree, int walk, int basis, const fm::Opt& opt, const uint32_t* node_old,
                                        const float* params, const float* origins, const float* dirs, const float* targets, float* out,
                                        int64_t n, int block, int64_t* grad, uint64_t* stats, uint32_t* touched, bool mark_read,
                                        hipStream_t stream);

// the list of a touched bitmap (rto_fit_touched_list): three launches on the stream -- a popcount sum per block of
// kFitTouchedBlockWords words (256 threads x 8 consecutive words), ONE workgroup that turns the block sums into offsets and writes
// count, and the scatter, which clears under `clear`.  scratch: one uint32 per block.  slots < 2^31, so at most 2^15 blocks.
constexpr int kFitTouchedBlockWords = 2048;
constexpr int kFitTouchedThreadWords = 8;
inline int64_t fit_touched_blocks(int64_t slots) { return (((slots + 31) >> 5) + kFitTouchedBlockWords - 1) / kFitTouchedBlockWords; }
hipError_t launch_fit_touched_list(uint32_t* touched, int64_t slots, bool clear, uint32_t* list, int64_t list_capacity, uint64_t* count,
                                   uint32_t* scratch, hipStream_t stream);

// the sparse step (rto_fit_step_sparse): a grid of kFitStepSparseBlocks x 256 threads strides over (list position, k) flattened
constexpr int kFitStepSparseBlocks = 2048;
hipError_t launch_fit_step_sparse(float* params, int64_t* grad, float* m, float* v, int64_t slots, int row, const uint32_t* list,
                                  const uint64_t* count, int64_t list_capacity, const rto_fit_optim& o, hipStream_t stream);

}  // namespace rto
