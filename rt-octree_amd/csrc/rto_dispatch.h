// rto_dispatch.h -- host only: the run-time values a launcher turns into template arguments, each rule stated once.  A helper calls
// a generic lambda with std::integral_constant arguments, which convert to the kernels' template arguments:
//     with_spp(spp, [&](auto SPP) { hipLaunchKernelGGL(render_rays_generic<SPP>, ...); return hipGetLastError(); });
// Used by the launchers of the render units (render_kernels.hip, frame_kernels.hip, shade_kernels.hip) and depth_kernels.hip ("Where dispatch lives").
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rto_kernel_types.h"

namespace rto {

template <int V>
using int_c = std::integral_constant<int, V>;

// f(int_c<spp>) for a supported spp, hipErrorInvalidValue otherwise; f returns hipError_t
template <class F>
hipError_t with_spp(int spp, F&& f) {
    switch (spp) {  // volrend.cu:266-278
#ifndef RTO_DEV_SPP6_ONLY  // (development builds: compile the benchmark's instantiation only)
        case 1: return f(int_c<1>{});
        case 2: return f(int_c<2>{});
        case 3: return f(int_c<3>{});
        case 4: return f(int_c<4>{});
        case 8: return f(int_c<8>{});
        case 16: return f(int_c<16>{});
        case 32: return f(int_c<32>{});
#endif
        case 6: return f(int_c<6>{});
        default: return hipErrorInvalidValue;
    }
}

// LOBES: kFmtSG / kFmtASG for a tree of that format, 0 for SH and RGBA trees
template <class F>
auto with_lobes(const TreeDev& tree, F&& f) {
    if (tree.format == kFmtSG) return f(int_c<kFmtSG>{});
    if (tree.format == kFmtASG) return f(int_c<kFmtASG>{});
    return f(int_c<0>{});
}

// The traversal image a launch walks, (WIDE, STACK): the two-level image when the tree has one (always, unless it would not fit
// its index space or the device's memory: host/tree_layout.cpp build_wide_image), else the one-level image <false, 0>: the same
// pixels either way.  On the two-level image, two pairs of levels below the grid at most take STACK = 1: the ancestor stack is two
// registers (in the batched kernel its LDS rows only park a ray's two hand-off offsets); deeper trees keep the stack in LDS, STACK = 0.
inline bool register_stack(const TreeDev& tree) { return tree.widew && (tree.max_depth - tree.top_levels + 1) / 2 <= 2; }
// (a caller that already knows tree.widew != nullptr: the A/B tuning instantiations, built for the two-level image only)
template <class F>
auto with_wide_image(const TreeDev& tree, F&& f) {
    return register_stack(tree) ? f(std::true_type{}, int_c<1>{}) : f(std::true_type{}, int_c<0>{});
}
template <class F>
auto with_image(const TreeDev& tree, F&& f) {
    return tree.widew ? with_wide_image(tree, f) : f(std::false_type{}, int_c<0>{});
}

// dynamic LDS of the single-frame and ray kernels on any image: one row of ancestors per level, per lane
inline size_t fast_lds_bytes(const TreeDev& tree) { return (size_t)(tree.max_depth + 1) * 256 * sizeof(uint32_t); }

// MODE of the shading kernel for an expanded tree: 28 / 49 / 76 for a tree whose leaves are records of that data_dim (`records`:
// SH, SG and ASG trees; the layout does not depend on the basis), 0 for any other
template <class F>
auto with_record_mode(const TreeDev& tree, bool records, F&& f) {
    if (records && tree.data_dim == 28) return f(int_c<28>{});
    if (records && tree.data_dim == 49) return f(int_c<49>{});
    if (records && tree.data_dim == 76) return f(int_c<76>{});
    return f(int_c<0>{});
}

}  // namespace rto
