// ray_kernels.hip -- the ray kernels (rto_launch_rays): render_rays_generic and render_rays, the bodies of the single-frame kernels
// (frame_kernels.hip) over the rays of a batch instead of a camera's pixels, and their launcher launch_rays (rto_launch.h).  One of
// the render stage's units: see the map in render_kernels.hip.  Their depth-carrying forms are depth_kernels.hip.
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"
#include "rto_tree_device.h"

#pragma clang fp contract(off)

// ray set-up, pixel / ray outputs, tiles, hit entries, packed shading, RTO_FAST_WPS: shared with the other render units
#include "rto_render_shared.h"
#include "rto_render_internal.h"  // the launchers of depth_kernels.hip, which launch_rays forwards to

namespace rto {

// rto_launch_rays on any tree the fast kernel does not take (N != 2, hit entries too wide) and RTO_KERNEL_GENERIC
template <int SPP>
__global__ void __launch_bounds__(256) render_rays_generic(const TreeDev tree, const OptDev opt, const Pcg32 rng_base,
                                                            const RayBatch rays) {
#define RTO_GENERIC_RAYS 1
#include "rto_render_generic.inc"
#undef RTO_GENERIC_RAYS
}

// rto_launch_rays on an N == 2 tree: the same body with the rays of the batch for the camera's pixels -- one thread per ray, no
// tile map and no culling marks (both are per camera tile), each ray's own depth limit and backdrop, a float4 per ray
template <int SPP, bool WIDE, int STACK, int LOBES>
__global__ void __launch_bounds__(256, SPP <= 8 ? RTO_FAST_WPS : 4) render_rays(const TreeDev tree, const OptDev opt, const Pcg32 rng_base,
                                                    const PcgJumpEntry* __restrict__ jump, const RayBatch rays) {
    constexpr bool STATS = false;
#define RTO_FAST_RAYS 1
#include "rto_render_fast.inc"
#undef RTO_FAST_RAYS
}

}  // namespace rto

// ------------------------------------------------------------------ host launcher (C++ linkage,
// declared in rto_launch.h)
#include "rto_dispatch.h"
#include "rto_launch.h"

namespace rto {

hipError_t launch_rays(int kernel, int spp, const TreeDev& tree, const OptDev& opt, const Pcg32& rng, const PcgJumpEntry* jump,
                       const RayBatch& rb_in, const DepthOut* depth, bool xcd_order, hipStream_t stream) {
    if (rb_in.n == 0) return hipSuccess;
    if ((uint64_t)rb_in.n * (uint64_t)spp >= (uint64_t(1) << 32)) return hipErrorInvalidValue;  // (the RNG offset of a ray is 32-bit)
    RayBatch rb = rb_in;
    const uint32_t blocks = (uint32_t)(((uint64_t)rb.n + 255) / 256);
    rb.per_xcd = xcd_order ? (blocks + 7) / 8 : 0u;
    const dim3 grid(xcd_order ? 8 * rb.per_xcd : blocks);
    if (depth)  // the depth-carrying kernels (depth_kernels.hip)
        return kernel == 2 ? launch_rays_depth_fast(spp, tree, opt, rng, jump, rb, *depth, grid, stream)
                           : launch_rays_depth_generic(spp, tree, opt, rng, rb, *depth, grid, stream);
    return with_spp(spp, [&](auto SPP) {
        if (kernel == 2)
            with_lobes(tree, [&](auto LOBES) {
                with_image(tree, [&](auto wide, auto stack) {
                    hipLaunchKernelGGL((render_rays<SPP, wide, stack, LOBES>), grid, dim3(256), fast_lds_bytes(tree), stream, tree, opt, rng, jump, rb);
                });
            });
        else
            hipLaunchKernelGGL(render_rays_generic<SPP>, grid, dim3(256), 0, stream, tree, opt, rng, rb);
        return hipGetLastError();
    });
}

}  // namespace rto
