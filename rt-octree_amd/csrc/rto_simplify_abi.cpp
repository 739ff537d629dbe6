// rto_simplify_abi.cpp -- C ABI of the tree simplifier (include/rto.h "simplifier"): the device entry (simplify_kernels.hip) and
// the host twin (host/tree_simplify.cpp).  Errors, the device scope, the shared checks and the scratch buffer come from
// rto_abi_common.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "host/tree_simplify.h"
#include "rto.h"
#include "rto_abi_common.h"
#include "rto_simplify_launch.h"

struct rto_simplifier {
    int device = 0;
    DeviceBuf scratch;  // rto::SimplifyPlan lays it out
};

extern "C" {

int rto_simplifier_create(int device, rto_simplifier** out) {
    if (!out) return set_err(RTO_E_INVALID, "rto_simplifier_create: null argument");
    *out = nullptr;
    if (const int rc = check_device_index(device, "no HIP device available")) return rc;
    rto_simplifier* s = new rto_simplifier();
    s->device = device;
    *out = s;
    return RTO_OK;
}

void rto_simplifier_free(rto_simplifier* s) {
    if (!s) return;
    {
        DeviceGuard guard(s->device);
        if (s->scratch.p) (void)hipDeviceSynchronize();
        s->scratch.release();
    }
    delete s;
}

int rto_tree_simplify(rto_simplifier* s, void* stream, const int32_t* child, const uint16_t* data, int64_t cap, int N, int D,
                      float kill_thresh, int32_t* child_out, uint16_t* data_out, int64_t* out_capacity, int64_t* node_map,
                      rto_simplify_stats* stats) {
    const std::string w = "rto_tree_simplify";
    if (!s) return set_err(RTO_E_INVALID, w + ": null argument");
    const std::string bad = rto::simplify_check_args(child, data, cap, N, D, child_out, data_out, out_capacity, node_map);
    if (!bad.empty()) return set_err(RTO_E_INVALID, w + ": " + bad);
    const int64_t S = (int64_t)N * N * N;
    if (cap * S > (((int64_t)1 << 39) - 1) / D) return set_err(RTO_E_INVALID, w + ": cap * N^3 * D must stay below 2^39");
    if (pointer_device(child) != s->device) return set_err(RTO_E_INVALID, w + ": child is not memory of the handle's device");
    if (pointer_device(data) != s->device) return set_err(RTO_E_INVALID, w + ": data is not memory of the handle's device");
    if (pointer_device(child_out) != s->device) return set_err(RTO_E_INVALID, w + ": child_out is not memory of the handle's device");
    if (pointer_device(data_out) != s->device) return set_err(RTO_E_INVALID, w + ": data_out is not memory of the handle's device");
    if (node_map && pointer_device(node_map) != s->device) return set_err(RTO_E_INVALID, w + ": node_map is not memory of the handle's device");
    DeviceGuard guard(s->device);
    const rto::SimplifyPlan plan = rto::simplify_plan(cap, N, D);
    if (const int rc = s->scratch.reserve(plan.total, "simplifier scratch")) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint32_t words[rto::kSimpWords];
    const auto read_words = [&]() {
        hipError_t e = hipMemcpyAsync(words, s->scratch.as<char>() + plan.words, sizeof(words), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        return e;
    };
    hipError_t e = rto::launch_simplify_links(plan, s->scratch.p, child, st);
    if (e != hipSuccess) return set_err(RTO_E_HIP, w + ": launch failed: " + hipGetErrorString(e));
    if ((e = read_words()) != hipSuccess) return set_err(RTO_E_HIP, w + ": " + hipGetErrorString(e));
    if (const uint32_t at = words[rto::kSimpBadRange])
        return set_err(RTO_E_FORMAT, w + ": node " + std::to_string((at - 1) / S) + " slot " + std::to_string((at - 1) % S) +
                                         ": the offset refers outside [1, " + std::to_string(cap) + ")");
    if (const uint32_t at = words[rto::kSimpBadShared])
        return set_err(RTO_E_FORMAT, w + ": node " + std::to_string((at - 1) / S) + " slot " + std::to_string((at - 1) % S) +
                                         ": its target is referred to by more than one slot");
    if (words[rto::kSimpLevelCount + rto::kSimplifyMaxLevels])
        return set_err(RTO_E_FORMAT, w + ": the walk from the root does not end within " + std::to_string(rto::kSimplifyMaxLevels) + " levels");
    int n_levels = 0;
    int64_t reachable = 0;
    while (n_levels < rto::kSimplifyMaxLevels && words[rto::kSimpLevelCount + n_levels]) reachable += words[rto::kSimpLevelCount + n_levels++];
    const bool kill = !std::isnan(kill_thresh);
    e = rto::launch_simplify_rest(plan, s->scratch.p, data, kill ? 1 : 0, kill ? rto::simp_thresh_half(kill_thresh) : 0u, n_levels,
                                  child_out, data_out, node_map, st);
    if (e != hipSuccess) return set_err(RTO_E_HIP, w + ": launch failed: " + hipGetErrorString(e));
    if ((e = read_words()) != hipSuccess) return set_err(RTO_E_HIP, w + ": " + hipGetErrorString(e));
    *out_capacity = (int64_t)words[rto::kSimpTotal];
    if (stats)
        *stats = rto_simplify_stats{reachable, cap - reachable, (int64_t)words[rto::kSimpKilled], (int64_t)words[rto::kSimpMerged],
                                    (int64_t)words[rto::kSimpDeepest] + 1};
    return RTO_OK;
}

int rto_tree_simplify_host(const int32_t* child, const uint16_t* data, int64_t cap, int N, int D, float kill_thresh,
                           int32_t* child_out, uint16_t* data_out, int64_t* out_capacity, int64_t* node_map,
                           rto_simplify_stats* stats) {
    std::string err;
    const int rc = rto::tree_simplify_host(child, data, cap, N, D, kill_thresh, child_out, data_out, out_capacity, node_map, stats, &err);
    if (rc != RTO_OK) return set_err(rc, "rto_tree_simplify_host: " + err);
    return RTO_OK;
}

}  // extern "C"
