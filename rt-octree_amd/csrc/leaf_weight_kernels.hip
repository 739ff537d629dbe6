// leaf_weight_kernels.hip -- per-leaf peak compositing weights over a set of cameras (rto_tree_leaf_weights, include/rto.h
// "leaf weights"): what the pruning step of PlenOctree extraction records before it drops the leaves no training view sees.
//
// One lane per pixel's ray; a wave covers an 8x8 pixel tile (its lanes stay in the same cells), a workgroup 16x16, blockIdx.z
// is the camera of the launch -- the cameras travel by value, kLayerCamChunk per launch (rto_layer_pass.h).  The march itself is
// rto_leaf_march.h, the text the host twin compiles too; here it is given
//   locate: the walk over what the tree has resident, exactly rto_tree_walk.h's -- the two-level image, the one-level image, or
//           child[] with the reference's float descent.  The leaf-local point of the image walks is fract(pos * 2^level), exact.
//   exp:    det_expf_mid for an argument in [-87, 0] (every dense step of a sane tree), det_expf elsewhere: the same float.
//   update: an unsigned atomic max on the weight's bit pattern (weights are never NaN nor negative, so the integer order is
//           the float order), skipped when the word already holds as much: it only ever grows, so a stale read costs at most a
//           redundant atomic.  After the first cameras almost every update is skipped.  An entry of the two-level image is
//           translated to its slot (wide_to_slot) only here, for the dense leaves -- and, where the upload re-laid the nodes
//           breadth-first, the slot to the numbering of the caller's arrays (node_old).
// No LDS, no scratch; the result does not depend on the order the rays run in.
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"
#include "rto_tree_device.h"
#include "rto_launch.h"

#pragma clang fp contract(off)

#include "rto_leaf_march.h"
#include "rto_leaf_weights_launch.h"
#include "rto_tree_walk.h"

namespace rto {

template <int WALK>
__global__ void __launch_bounds__(256) leaf_weights_kernel(const TreeDev tree, const lm::Opt opt, const LayerCams cams,
                                                           const uint32_t* __restrict__ node_old, uint32_t* weights) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const CamDev& cd = cams.c[blockIdx.z];
    const int x = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    const int y = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (x >= cd.width || y >= cd.height) return;
    lm::Cam cam;
    cam.width = cd.width;
    cam.height = cd.height;
    cam.fx = cd.fx;
    cam.fy = cd.fy;
#pragma unroll
    for (int i = 0; i < 12; ++i) cam.transform[i] = cd.transform[i];
    lm::Frame fr;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        fr.offset[i] = tree.offset[i];
        fr.scale[i] = tree.scale[i];
    }
    fr.ndc_width = tree.ndc_width;
    fr.ndc_height = tree.ndc_height;
    fr.ndc_focal = tree.ndc_focal;

    const auto locate = [&](const float* pos, lm::Leaf& leaf) -> bool {
        if constexpr (WALK == kWalkChild) {
#pragma unroll
            for (int i = 0; i < 3; ++i) leaf.local[i] = pos[i];
            const int64_t slot = lm::descend_child(tree.child, tree.N, leaf.local, leaf.cube_sz);
            leaf.index = (uint32_t)slot;
            leaf.sigma_bits = tree.data[slot * tree.data_dim + tree.data_dim - 1];
            return true;
        } else {
            float p[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) p[i] = f_max(f_min(pos[i], 1.f - 1e-6f), 0.f);
            const Leaf r = walk_point<true>(tree, WALK, p);
            if (r.level < 1) return false;  // (cannot happen, see walk_point)
            leaf.index = r.index;
            leaf.sigma_bits = r.sigma;
            leaf.cube_sz = __uint_as_float((uint32_t)(127 + r.level) << 23);  // 2^level
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float u = p[i] * leaf.cube_sz;  // (exact, as is the subtraction: the cell is p's fixed point masked at level)
                leaf.local[i] = u - floorf(u);
            }
            return true;
        }
    };
    const auto exp_ = [](float v) -> float { return (v >= -87.f && v <= 0.f) ? det_expf_mid(v) : det_expf(v); };
    const auto update = [&](uint32_t index, float w) {
        const uint32_t b = __float_as_uint(w);
        if (b == 0u) return;
        uint32_t slot = WALK == kWalkWide ? wide_to_slot(tree, index) : index;
        if (node_old) {  // (uniform) the upload re-laid the nodes: back to the caller's numbering
            const uint32_t N3 = (uint32_t)tree.N3, node = slot / N3;
            slot = node_old[node] * N3 + (slot - node * N3);
        }
        if (b > __atomic_load_n(weights + slot, __ATOMIC_RELAXED)) atomicMax(weights + slot, b);
    };
    lm::march_pixel(fr, opt, cam, x, y, locate, exp_, update);
}

hipError_t launch_leaf_weights(const TreeDev& tree, int walk, const lm::Opt& opt, const LayerCams& cams, int frames, const uint32_t* node_old,
                               uint32_t* weights, hipStream_t stream) {
    if (frames <= 0) return hipSuccess;
    if (frames > kLayerCamChunk || cams.c[0].width <= 0 || cams.c[0].height <= 0) return hipErrorInvalidValue;
    if (walk == kWalkChild && !(tree.child && tree.data)) return hipErrorInvalidValue;
    if (walk == kWalkNodew && !tree.nodew) return hipErrorInvalidValue;
    if (walk == kWalkWide && !(tree.widew && tree.nodew && tree.wgslot && tree.worig)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((cams.c[0].width + 15) / 16), (unsigned)((cams.c[0].height + 15) / 16), (unsigned)frames);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    if (walk == kWalkWide)
        hipLaunchKernelGGL(leaf_weights_kernel<kWalkWide>, grid, dim3(256), 0, stream, tree, opt, cams, node_old, weights);
    else if (walk == kWalkNodew)
        hipLaunchKernelGGL(leaf_weights_kernel<kWalkNodew>, grid, dim3(256), 0, stream, tree, opt, cams, node_old, weights);
    else if (walk == kWalkChild)
        hipLaunchKernelGGL(leaf_weights_kernel<kWalkChild>, grid, dim3(256), 0, stream, tree, opt, cams, node_old, weights);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace rto
