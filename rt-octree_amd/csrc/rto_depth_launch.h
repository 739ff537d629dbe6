// rto_depth_launch.h -- host launchers of the depth-carrying kernels, shared by render_kernels.hip (caller) and depth_kernels.hip
// (definitions and explicit instantiations).
#pragma once
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"

namespace rto {

// Launchers of the depth-carrying instantiations (render_rays_depth, render_rays_generic_depth,
// render_fast_layers_depth, render_generic_layers_depth), defined and explicitly instantiated in depth_kernels.hip for every supported SPP (and
// LOBES = 0, kFmtSG, kFmtASG); render_kernels.hip's launch_render / launch_rays call them when depth outputs are asked for.
// The fast forms choose the traversal image as launch_fast does.
template <int SPP, int LOBES>
void launch_fast_depth(const TreeDev& tree, const CamDev& cam, const OptDev& opt, const Pcg32& rng, const PcgJumpEntry* jump,
                       const FrameOut& fo, int strip_rows, const LayerDev& layers, const DepthOut& depth, hipStream_t stream);
template <int SPP>
void launch_generic_depth(const TreeDev& tree, const CamDev& cam, const OptDev& opt, const Pcg32& rng, const FrameOut& fo,
                          const LayerDev& layers, const DepthOut& depth, hipStream_t stream);
template <int SPP, int LOBES>
void launch_rays_depth_fast(const TreeDev& tree, const OptDev& opt, const Pcg32& rng, const PcgJumpEntry* jump, const RayBatch& rb,
                            const DepthOut& depth, dim3 grid, hipStream_t stream);
template <int SPP>
void launch_rays_depth_generic(const TreeDev& tree, const OptDev& opt, const Pcg32& rng, const RayBatch& rb, const DepthOut& depth,
                               dim3 grid, hipStream_t stream);

// render_persist_depth<SPP, 32, RTO_WPS_DEFAULT, WIDE, STACK> (the batched traversal with depth outputs, default tuning only), for
// launch_batch_impl: the kernel a launch takes -- regstack: STACK = 1, the two-level image's register-stack form -- as the identity
// its OccupancyCache, occupancy query and dynamic-LDS request go by, and its launch.  lds: launch_batch_impl's size, which counts
// the kernel's two more rows.  layers: both pointers null = offscreen.  depth: plane f = batch frame f, both pointers set.
template <int SPP, bool WIDE>
const void* persist_depth_kernel(bool regstack);
template <int SPP, bool WIDE>
void launch_persist_depth(bool regstack, int grid, size_t lds, hipStream_t stream, const TreeDev& tree, const OptDev& opt,
                          const FrameBatch& fb, unsigned long long* queue, uint32_t* hits, uint32_t chunk, const LayerDev& layers,
                          const DepthOut& depth);

}  // namespace rto
