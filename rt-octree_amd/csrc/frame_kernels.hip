// frame_kernels.hip -- the single-frame kernels (rto_launch_renderer): render_generic and render_fast in their offscreen and
// layered forms, and their launcher launch_render (rto_launch.h).  One of the render stage's units: see the map in
// render_kernels.hip, whose overview describes the kernels.  The same bodies over a batch of rays are ray_kernels.hip, their
// depth-carrying forms depth_kernels.hip.
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"
#include "rto_tree_device.h"

#pragma clang fp contract(off)

// ray set-up, pixel / ray outputs, tiles, hit entries, packed shading, RTO_FAST_WPS: shared with the other render units
#include "rto_render_shared.h"
#include "rto_render_internal.h"  // the launchers of depth_kernels.hip, which launch_render forwards to

namespace rto {

// ------------------------------------------------------------------ generic kernel (any N)

template <int SPP>
__global__ void __launch_bounds__(256) render_generic(const TreeDev tree, const CamDev cam, const OptDev opt,
                                                       const Pcg32 rng_base, const FrameOut fo) {
#include "rto_render_generic.inc"
}

// rto_launch_renderer over the context's layers (rto_ctx_set_layers) on any tree the fast kernel does not take and RTO_KERNEL_GENERIC
template <int SPP>
__global__ void __launch_bounds__(256) render_generic_layers(const TreeDev tree, const CamDev cam, const OptDev opt, const Pcg32 rng_base,
                                                              const FrameOut fo, const LayerDev layers) {
#define RTO_GENERIC_LAYERS 1
#include "rto_render_generic.inc"
#undef RTO_GENERIC_LAYERS
}

// ------------------------------------------------------------------ fast kernel (N == 2)

// STATS: also count the units of SURVEY 8(d)'s algorithmic-byte formula (march steps, descent
// levels a root-restart walk would visit, distinct hit leaves, ...) into fo.stats.  Separate
// instantiation; the timed kernel carries none of it.
// STACK == 1 (two-level image, at most two pairs of levels below the grid; the launcher decides): the restart of render_persist's
// register-stack form -- the node a step starts from is chosen by where the ray is and which coordinate bits changed
// (rto_march_leaf.inc), positions are kept scaled by 2^24 (kPos24), the step's power-of-two factors come from the level bits of
// the leaf word -- seven dependent instructions fewer on the chain a lone frame's longest rays wait for
// The body (rto_render_fast.inc) serves two kernels: render_fast for SH and RGBA trees and render_fast_lobes for SG / ASG trees
// (LOBES = kFmtSG / kFmtASG, see ray_basis), so that the SH kernels keep their names and their code.
template <int SPP, bool STATS, bool WIDE, int STACK = 0>
__global__ void __launch_bounds__(256, SPP <= 8 ? RTO_FAST_WPS : 4) render_fast(const TreeDev tree, const CamDev cam, const OptDev opt,
                                                    const Pcg32 rng_base, const PcgJumpEntry* __restrict__ jump,
                                                    const TileMap tm, const FrameOut fo) {
    constexpr int LOBES = 0;
#include "rto_render_fast.inc"
}

// the single-frame kernel of an SG / ASG tree (LOBES = kFmtSG / kFmtASG): the same body under its own name
template <int SPP, bool STATS, bool WIDE, int STACK, int LOBES>
__global__ void __launch_bounds__(256, SPP <= 8 ? RTO_FAST_WPS : 4) render_fast_lobes(const TreeDev tree, const CamDev cam, const OptDev opt,
                                                          const Pcg32 rng_base, const PcgJumpEntry* __restrict__ jump,
                                                          const TileMap tm, const FrameOut fo) {
#include "rto_render_fast.inc"
}

// rto_launch_renderer over the context's layers (rto_ctx_set_layers) on an N == 2 tree: the same body, each pixel's ray stopped at
// its depth and composited over its colour; the tiles culled by fo.cull_marks get their backdrop.  No counting instantiation
// (layers and rto_ctx_enable_stats are refused together).
template <int SPP, bool WIDE, int STACK, int LOBES>
__global__ void __launch_bounds__(256, SPP <= 8 ? RTO_FAST_WPS : 4) render_fast_layers(const TreeDev tree, const CamDev cam, const OptDev opt,
                                                           const Pcg32 rng_base, const PcgJumpEntry* __restrict__ jump,
                                                           const TileMap tm, const FrameOut fo, const LayerDev layers) {
    constexpr bool STATS = false;
#define RTO_FAST_LAYERS 1
#include "rto_render_fast.inc"
#undef RTO_FAST_LAYERS
}

}  // namespace rto

// ------------------------------------------------------------------ host launchers (C++ linkage,
// declared in rto_launch.h)
#include "rto_dispatch.h"
#include "rto_launch.h"

namespace rto {

TileMap make_tile_map(int width, int height, int strip_rows) {
    TileMap tm;
    tm.tiles_x = (width + kTileW - 1) / kTileW;
    tm.tiles_y = (height + kTileH - 1) / kTileH;
    tm.strip_rows = strip_rows < 1 ? 1 : strip_rows;
    const int strips = (tm.tiles_y + tm.strip_rows - 1) / tm.strip_rows;
    const int strips_per_xcd = (strips + 7) / 8;
    tm.per_xcd = strips_per_xcd * tm.strip_rows * tm.tiles_x;
    return tm;
}

template <int SPP, int LOBES>
static void launch_fast(const TreeDev& tree, const CamDev& cam, const OptDev& opt, const Pcg32& rng, const PcgJumpEntry* jump,
                        const FrameOut& fo, int strip_rows, const LayerDev* layers, hipStream_t stream) {
    const TileMap tm = make_tile_map(cam.width, cam.height, strip_rows);
    const size_t lds = fast_lds_bytes(tree);
    const dim3 grid(8 * tm.per_xcd), block(256);
    const auto offscreen = [&](auto stats, auto wide, auto stack) {
        if constexpr (LOBES == 0)
            hipLaunchKernelGGL((render_fast<SPP, stats, wide, stack>), grid, block, lds, stream, tree, cam, opt, rng, jump, tm, fo);
        else
            hipLaunchKernelGGL((render_fast_lobes<SPP, stats, wide, stack, LOBES>), grid, block, lds, stream, tree, cam, opt, rng, jump, tm, fo);
    };
    if (fo.stats && !layers) {  // (the counting instantiation walks the one-level image: its units are defined on that walk)
        offscreen(std::true_type{}, std::false_type{}, int_c<0>{});
        return;
    }
    with_image(tree, [&](auto wide, auto stack) {
        if (layers)  // (the host refuses layers with work counters)
            hipLaunchKernelGGL((render_fast_layers<SPP, wide, stack, LOBES>), grid, block, lds, stream, tree, cam, opt, rng, jump, tm, fo, *layers);
        else
            offscreen(std::false_type{}, wide, stack);
    });
}

hipError_t launch_render(int kernel, int spp, const TreeDev& tree, const CamDev& cam, const OptDev& opt,
                         const Pcg32& rng, const PcgJumpEntry* jump, const FrameOut& fo, int strip_rows,
                         const LayerDev* layers, const DepthOut* depth, hipStream_t stream) {
    if (depth) {  // the depth-carrying layered kernels (depth_kernels.hip), over the context's layers or none
        const LayerDev ld = layers ? *layers : LayerDev{nullptr, nullptr};
        return kernel == 2 ? launch_fast_depth(spp, tree, cam, opt, rng, jump, fo, strip_rows, ld, *depth, stream)
                           : launch_generic_depth(spp, tree, cam, opt, rng, fo, ld, *depth, stream);
    }
    return with_spp(spp, [&](auto SPP) {
        const dim3 ggrid((unsigned)(((int64_t)cam.width * cam.height + 255) / 256));
        if (kernel == 2)
            with_lobes(tree, [&](auto LOBES) { launch_fast<SPP, LOBES>(tree, cam, opt, rng, jump, fo, strip_rows, layers, stream); });
        else if (layers)
            hipLaunchKernelGGL(render_generic_layers<SPP>, ggrid, dim3(256), 0, stream, tree, cam, opt, rng, fo, *layers);
        else
            hipLaunchKernelGGL(render_generic<SPP>, ggrid, dim3(256), 0, stream, tree, cam, opt, rng, fo);
        return hipGetLastError();
    });
}

}  // namespace rto
