// depth_kernels.hip -- the depth-carrying instantiations of the single-frame and ray kernels (include/rto.h "depth outputs";
// DESIGN.md section 7e): the bodies of frame_kernels.hip and render_kernels.hip (rto_render_fast.inc, rto_render_generic.inc,
// rto_render_persist.inc) with RTO_DEPTH defined, which also keep the distance of a ray's hits and store depth and t_near through a
// DepthOut argument.  A translation unit of its own: those units keep their kernels, their text and their compile time, and all
// compile side by side (the unit map: render_kernels.hip).
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"
#include "rto_launch.h"
#include "rto_tree_device.h"

#pragma clang fp contract(off)

#include "rto_render_internal.h"
#include "rto_dispatch.h"
#include "rto_render_shared.h"

namespace rto {

// ---- the depth-carrying forms (rto_launch_rays_ex with depth / t_near; a context with rto_ctx_enable_depth): the same bodies
// with RTO_DEPTH -- instantiations of their own, so that the kernels above keep their text, their arguments and their code
template <int SPP>
__global__ void __launch_bounds__(256) render_rays_generic_depth(const TreeDev tree, const OptDev opt, const Pcg32 rng_base,
                                                                  const RayBatch rays, const DepthOut dout) {
#define RTO_GENERIC_RAYS 1
#define RTO_DEPTH 1
#include "rto_render_generic.inc"
#undef RTO_DEPTH
#undef RTO_GENERIC_RAYS
}

// (the frame form is the layered body: both layer pointers null is the offscreen frame)
template <int SPP>
__global__ void __launch_bounds__(256) render_generic_layers_depth(const TreeDev tree, const CamDev cam, const OptDev opt, const Pcg32 rng_base,
                                                                    const FrameOut fo, const LayerDev layers, const DepthOut dout) {
#define RTO_GENERIC_LAYERS 1
#define RTO_DEPTH 1
#include "rto_render_generic.inc"
#undef RTO_DEPTH
#undef RTO_GENERIC_LAYERS
}

// The depth-carrying forms of render_rays and render_fast_layers (RTO_DEPTH; DepthOut behind their siblings' arguments).  One frame family
// serves offscreen and layered contexts: both layer pointers null is the offscreen frame.  (render_persist's depth form is
// render_persist_depth below: its hit hand-off has no room for t, so the traversal kernel itself accumulates.)
// Waves per SIMD the two kernels are built for: their siblings' (RTO_FAST_WPS up to SPP 8, 4 above), one less where the two more
// live registers would otherwise go to the private segment -- render_rays at SPP 8 on the two-level image already keeps 8 bytes
// per lane at 5 waves, and the SPP-32 forms 132-136 at 4; with one wave less the depth forms hold no more than their siblings
// (tests/test_depth.py::test_depth_kernels_codegen).
constexpr int depth_rays_wps(int spp) { return spp < 8 ? RTO_FAST_WPS : spp == 8 ? RTO_FAST_WPS - 1 : spp < 32 ? 4 : 3; }
constexpr int depth_frame_wps(int spp) { return spp <= 8 ? RTO_FAST_WPS : spp < 32 ? 4 : 3; }

template <int SPP, bool WIDE, int STACK, int LOBES>
__global__ void __launch_bounds__(256, depth_rays_wps(SPP)) render_rays_depth(const TreeDev tree, const OptDev opt, const Pcg32 rng_base,
                                                          const PcgJumpEntry* __restrict__ jump, const RayBatch rays,
                                                          const DepthOut dout) {
    constexpr bool STATS = false;
#define RTO_FAST_RAYS 1
#define RTO_DEPTH 1
#include "rto_render_fast.inc"
#undef RTO_DEPTH
#undef RTO_FAST_RAYS
}

template <int SPP, bool WIDE, int STACK, int LOBES>
__global__ void __launch_bounds__(256, depth_frame_wps(SPP)) render_fast_layers_depth(const TreeDev tree, const CamDev cam, const OptDev opt,
                                                                 const Pcg32 rng_base, const PcgJumpEntry* __restrict__ jump,
                                                                 const TileMap tm, const FrameOut fo, const LayerDev layers,
                                                                 const DepthOut dout) {
    constexpr bool STATS = false;
#define RTO_FAST_LAYERS 1
#define RTO_DEPTH 1
#include "rto_render_fast.inc"
#undef RTO_DEPTH
#undef RTO_FAST_LAYERS
}

// The depth-carrying form of render_persist_layers (rto_ctx_enable_depth(RTO_DEPTH_BATCHED)): the layered body of
// the batched traversal with RTO_DEPTH -- at a hit the ray adds (float)cnt * (t * delta_scale) to a sum and keeps its first hit's
// distance, both in two LDS rows of their own, and stores its pixel's depth and t_near when its hit list leaves (DepthOut: plane f
// = batch frame f).  Both layer pointers null is the offscreen batch.  The shading kernels take no part in it.  Instantiated for the
// default tuning only (REFILL 32, RTO_WPS_DEFAULT waves per SIMD), as render_persist_layers is.
// Waves per SIMD: the sibling's WPS, one less for the SPP-32 forms on the two-level image -- their 32-entry flush already keeps
// 56-64 bytes per lane at 8 waves, and the depth store beside it 4-12 more; with 72 registers they hold less than the sibling
// (tests/test_depth_batch.py::test_depth_batch_codegen).
constexpr int persist_depth_wps(int spp, int wps, bool wide) { return spp == 32 && wide ? wps - 1 : wps; }
template <int SPP, int REFILL, int WPS, bool WIDE, int STACK>
__global__ void __launch_bounds__(256, persist_depth_wps(SPP, WPS, WIDE)) render_persist_depth(const TreeDev tree, const OptDev opt, const FrameBatch fb,
                                                             unsigned long long* __restrict__ queue,
                                                             uint32_t* __restrict__ hits, const uint32_t chunk, const LayerDev layers,
                                                             const DepthOut dout) {
#define RTO_PERSIST_LAYERS 1
#define RTO_DEPTH 1
#include "rto_render_persist.inc"
#undef RTO_DEPTH
#undef RTO_PERSIST_LAYERS
}

// ------------------------------------------------------------------ launchers (declared in rto_render_internal.h)
// spp, lobe form and traversal image are dispatched here, by the helpers the other render units' launchers use (rto_dispatch.h)

const void* persist_depth_kernel(int spp, const TreeDev& tree) {
    const void* fn = nullptr;
    (void)with_spp(spp, [&](auto SPP) {
        with_image(tree, [&](auto wide, auto stack) { fn = reinterpret_cast<const void*>(&render_persist_depth<SPP, 32, RTO_WPS_DEFAULT, wide, stack>); });
        return hipSuccess;
    });
    return fn;
}

hipError_t launch_persist_depth(int spp, const TreeDev& tree, int grid, size_t lds, hipStream_t stream, const OptDev& opt, const FrameBatch& fb,
                                unsigned long long* queue, uint32_t* hits, uint32_t chunk, const LayerDev& layers, const DepthOut& depth) {
    return with_spp(spp, [&](auto SPP) {
        with_image(tree, [&](auto wide, auto stack) {
            hipLaunchKernelGGL((render_persist_depth<SPP, 32, RTO_WPS_DEFAULT, wide, stack>), dim3(grid), dim3(256), lds, stream, tree, opt, fb, queue,
                               hits, chunk, layers, depth);
        });
        return hipGetLastError();
    });
}

hipError_t launch_fast_depth(int spp, const TreeDev& tree, const CamDev& cam, const OptDev& opt, const Pcg32& rng, const PcgJumpEntry* jump,
                             const FrameOut& fo, int strip_rows, const LayerDev& layers, const DepthOut& depth, hipStream_t stream) {
    const TileMap tm = make_tile_map(cam.width, cam.height, strip_rows);
    const dim3 grid(8 * tm.per_xcd), block(256);
    return with_spp(spp, [&](auto SPP) {
        with_lobes(tree, [&](auto LOBES) {
            with_image(tree, [&](auto wide, auto stack) {
                hipLaunchKernelGGL((render_fast_layers_depth<SPP, wide, stack, LOBES>), grid, block, fast_lds_bytes(tree), stream, tree, cam, opt, rng,
                                   jump, tm, fo, layers, depth);
            });
        });
        return hipGetLastError();
    });
}

hipError_t launch_generic_depth(int spp, const TreeDev& tree, const CamDev& cam, const OptDev& opt, const Pcg32& rng, const FrameOut& fo,
                                const LayerDev& layers, const DepthOut& depth, hipStream_t stream) {
    const int64_t size = (int64_t)cam.width * cam.height;
    return with_spp(spp, [&](auto SPP) {
        hipLaunchKernelGGL(render_generic_layers_depth<SPP>, dim3((unsigned)((size + 255) / 256)), dim3(256), 0, stream, tree, cam, opt, rng, fo,
                           layers, depth);
        return hipGetLastError();
    });
}

hipError_t launch_rays_depth_fast(int spp, const TreeDev& tree, const OptDev& opt, const Pcg32& rng, const PcgJumpEntry* jump,
                                  const RayBatch& rb, const DepthOut& depth, dim3 grid, hipStream_t stream) {
    return with_spp(spp, [&](auto SPP) {
        with_lobes(tree, [&](auto LOBES) {
            with_image(tree, [&](auto wide, auto stack) {
                hipLaunchKernelGGL((render_rays_depth<SPP, wide, stack, LOBES>), grid, dim3(256), fast_lds_bytes(tree), stream, tree, opt, rng, jump,
                                   rb, depth);
            });
        });
        return hipGetLastError();
    });
}

hipError_t launch_rays_depth_generic(int spp, const TreeDev& tree, const OptDev& opt, const Pcg32& rng, const RayBatch& rb,
                                     const DepthOut& depth, dim3 grid, hipStream_t stream) {
    return with_spp(spp, [&](auto SPP) {
        hipLaunchKernelGGL(render_rays_generic_depth<SPP>, grid, dim3(256), 0, stream, tree, opt, rng, rb, depth);
        return hipGetLastError();
    });
}

}  // namespace rto
