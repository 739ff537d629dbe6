// rto_leaf_weights_abi.cpp -- C ABI of the per-leaf peak weights (include/rto.h "leaf weights"): the device entry
// (leaf_weight_kernels.hip) and the host twin (host/leaf_weights.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "host/leaf_weights.h"
#include "rto_internal.h"
#include "rto_leaf_weights_launch.h"

extern "C" {

int rto_tree_leaf_weights(const rto_tree* tree, const rto_camera* cams, int n, const rto_options* opt, uint32_t* weights, void* stream) {
    const std::string w = "rto_tree_leaf_weights: ";
    if (!tree || !opt) return set_err(RTO_E_INVALID, w + "null tree or options");
    const std::string bad = rto::leaf_weights_check_cams(cams, n, weights);
    if (!bad.empty()) return set_err(RTO_E_INVALID, w + bad);
    if (pointer_device(weights) != tree->device) return set_err(RTO_E_INVALID, w + "weights is not memory of the tree's device");
    int walk;
    rto::ValuesSrc vs;
    (void)query_plan(tree, false, &walk, &vs);
    if (walk == rto::kWalkChild && !(tree->dev.child && tree->dev.data))
        return set_err(RTO_E_UNSUPPORTED, w + "the tree has neither a traversal image nor child[] / data[] resident");
    if (n == 0) return RTO_OK;
    DeviceGuard guard(tree->device);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    rto::lm::Opt o;
    o.step_size = opt->step_size;
    o.sigma_thresh = opt->sigma_thresh;
    o.stop_thresh = opt->stop_thresh;
    for (int i = 0; i < 6; ++i) o.render_bbox[i] = opt->render_bbox[i];
    // a launch takes a run of consecutive cameras of one size, at most kLayerCamChunk of them (the unused slots hold the first)
    for (int f0 = 0; f0 < n;) {
        int k = 1;
        while (k < rto::kLayerCamChunk && f0 + k < n && cams[f0 + k].width == cams[f0].width && cams[f0 + k].height == cams[f0].height) ++k;
        rto::LayerCams lc;
        for (int f = 0; f < rto::kLayerCamChunk; ++f) lc.c[f] = cam_dev(cams[f0 + (f < k ? f : 0)]);
        const hipError_t e = rto::launch_leaf_weights(tree->dev, walk, o, lc, k, (const uint32_t*)tree->d_node_old, weights, (hipStream_t)stream);
        if (e != hipSuccess) return set_err(RTO_E_HIP, w + "launch failed: " + hipGetErrorString(e));
        f0 += k;
    }
    return RTO_OK;
}

int rto_leaf_weights_host(const int32_t* child, const uint16_t* data, int64_t capacity, int N, int data_dim, const float scale[3],
                          const float offset[3], const float* ndc, const rto_camera* cams, int n, const rto_options* opt, int threads,
                          uint32_t* weights) {
    std::string err;
    const int rc = rto::leaf_weights_host(child, data, capacity, N, data_dim, scale, offset, ndc, cams, n, opt, threads, weights, &err);
    if (rc != RTO_OK) return set_err(rc, "rto_leaf_weights_host: " + err);
    return RTO_OK;
}

}  // extern "C"
