// rto_leaf_weights_launch.h -- launcher of leaf_weight_kernels.hip (rto_tree_leaf_weights, include/rto.h "leaf weights").
#pragma once
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"
#include "rto_layer_pass.h"
#include "rto_leaf_march.h"

namespace rto {

// `frames` (1 .. kLayerCamChunk) consecutive cameras of ONE size, by value in cams.c[0 .. frames - 1]; one lane per pixel's ray,
// blockIdx.z = camera.  walk: kWalkChild / kWalkNodew / kWalkWide of rto_launch.h (kWalkChild needs tree.child and tree.data).
// weights: capacity * N^3 words in device memory, raised by an unsigned atomic max.  node_old: nullptr, or per node of the
// resident tree its index in the numbering `weights` goes by (an upload that re-laid the nodes: rto_tree::d_node_old).
hipError_t launch_leaf_weights(const TreeDev& tree, int walk, const lm::Opt& opt, const LayerCams& cams, int frames, const uint32_t* node_old,
                               uint32_t* weights, hipStream_t stream);

}  // namespace rto
