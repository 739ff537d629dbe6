// rto_render_internal.h -- the host launchers the render stage's units call in each other (the unit map: render_kernels.hip).  The
// interface of the ABI units is rto_launch.h; nothing outside the units below includes this.
//   shade_kernels.hip  defines launch_shade, called by render_kernels.hip (launch_batch_impl)
//   depth_kernels.hip  defines the depth launchers, called by frame_kernels.hip (launch_render), ray_kernels.hip (launch_rays) and
//                      render_kernels.hip (launch_batch_impl)
#pragma once
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"

namespace rto {

// The shading stage of a batched launch, behind its traversal on `stream`: shade_kernel<spp, P, MODE, LOBES>, or shade_kernel_layers
// over the colour layer where layers && layers->color.  The grid, pixels per lane and the quantised / record-mode / lobes dispatch
// are shade_kernels.hip's own.  hits: the traversal's hand-off buffer.  An spp outside {1,2,3,4,6,8,16,32} is hipErrorInvalidValue
// (nothing launched), else hipGetLastError().
hipError_t launch_shade(int spp, const TreeDev& tree, const OptDev& opt, const FrameBatch& fb, const uint32_t* hits, const LayerDev* layers,
                        hipStream_t stream);

// Launchers of the depth-carrying instantiations (render_rays_depth, render_rays_generic_depth, render_fast_layers_depth,
// render_generic_layers_depth); launch_render (frame_kernels.hip) and launch_rays (ray_kernels.hip) call them when depth outputs are asked for.
// Plain functions: spp, the tree's lobe form and its traversal image become template arguments inside depth_kernels.hip, by the rules
// of rto_dispatch.h.  An spp outside {1,2,3,4,6,8,16,32} is hipErrorInvalidValue (nothing launched), else hipGetLastError().
hipError_t launch_fast_depth(int spp, const TreeDev& tree, const CamDev& cam, const OptDev& opt, const Pcg32& rng, const PcgJumpEntry* jump,
                             const FrameOut& fo, int strip_rows, const LayerDev& layers, const DepthOut& depth, hipStream_t stream);
hipError_t launch_generic_depth(int spp, const TreeDev& tree, const CamDev& cam, const OptDev& opt, const Pcg32& rng, const FrameOut& fo,
                                const LayerDev& layers, const DepthOut& depth, hipStream_t stream);
hipError_t launch_rays_depth_fast(int spp, const TreeDev& tree, const OptDev& opt, const Pcg32& rng, const PcgJumpEntry* jump,
                                  const RayBatch& rb, const DepthOut& depth, dim3 grid, hipStream_t stream);
hipError_t launch_rays_depth_generic(int spp, const TreeDev& tree, const OptDev& opt, const Pcg32& rng, const RayBatch& rb,
                                     const DepthOut& depth, dim3 grid, hipStream_t stream);

// render_persist_depth<SPP, 32, RTO_WPS_DEFAULT, WIDE, STACK> (the batched traversal with depth outputs, default tuning only), for
// launch_batch_impl: the kernel a launch on `tree` takes, as the identity its OccupancyCache, occupancy query and dynamic-LDS
// request go by (nullptr for an unsupported spp), and its launch.  lds: launch_batch_impl's size, which counts the kernel's two
// more rows.  layers: both pointers null = offscreen.  depth: plane f = batch frame f, both pointers set.
const void* persist_depth_kernel(int spp, const TreeDev& tree);
hipError_t launch_persist_depth(int spp, const TreeDev& tree, int grid, size_t lds, hipStream_t stream, const OptDev& opt,
                                const FrameBatch& fb, unsigned long long* queue, uint32_t* hits, uint32_t chunk, const LayerDev& layers,
                                const DepthOut& depth);

}  // namespace rto
