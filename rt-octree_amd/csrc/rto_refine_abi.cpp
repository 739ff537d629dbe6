// rto_refine_abi.cpp -- C ABI of the tree refiner (include/rto.h "refiner"): the device entries (refine_kernels.hip) and the host
// twin (host/tree_refine.cpp).  Errors, the device scope, the shared checks and the scratch buffer come from rto_abi_common.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "host/tree_refine.h"
#include "rto.h"
#include "rto_abi_common.h"
#include "rto_refine_launch.h"

struct rto_refiner {
    int device = 0;
    DeviceBuf scratch;  // rto::RefinePlan lays it out
    bool planned = false;
    rto::RefinePlan plan;
    int64_t selected = 0;
};

extern "C" {

int rto_refiner_create(int device, rto_refiner** out) {
    if (!out) return set_err(RTO_E_INVALID, "rto_refiner_create: null argument");
    *out = nullptr;
    if (const int rc = check_device_index(device, "no HIP device available")) return rc;
    rto_refiner* r = new rto_refiner();
    r->device = device;
    *out = r;
    return RTO_OK;
}

void rto_refiner_free(rto_refiner* r) {
    if (!r) return;
    {
        DeviceGuard guard(r->device);
        if (r->scratch.p) (void)hipDeviceSynchronize();
        r->scratch.release();
    }
    delete r;
}

int rto_tree_refine_plan(rto_refiner* r, void* stream, const int32_t* child, const uint32_t* key, int64_t cap, int N, uint32_t key_thresh,
                         int64_t max_new, int max_level, int64_t* out_capacity, rto_refine_stats* stats) {
    const std::string w = "rto_tree_refine_plan";
    if (!r || !out_capacity) return set_err(RTO_E_INVALID, w + ": null argument");
    r->planned = false;
    const std::string bad = rto::refine_check_inputs(child, key, cap, N, max_level);
    if (!bad.empty()) return set_err(RTO_E_INVALID, w + ": " + bad);
    if (pointer_device(child) != r->device) return set_err(RTO_E_INVALID, w + ": child is not memory of the handle's device");
    if (key && pointer_device(key) != r->device) return set_err(RTO_E_INVALID, w + ": key is not memory of the handle's device");
    DeviceGuard guard(r->device);
    const rto::RefinePlan plan = rto::refine_plan(cap, N);
    if (const int rc = r->scratch.reserve(plan.total, "refiner scratch")) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = rto::launch_refine_plan(plan, r->scratch.p, child, key, key_thresh, max_new, max_level, st);
    if (e != hipSuccess) return set_err(RTO_E_HIP, w + ": launch failed: " + hipGetErrorString(e));
    uint32_t words[rto::kRefWords];
    e = hipMemcpyAsync(words, r->scratch.as<char>() + plan.words, sizeof(words), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return set_err(RTO_E_HIP, w + ": " + hipGetErrorString(e));
    const int64_t S = plan.S;
    if (const uint32_t at = words[rto::kRefBadRange])
        return set_err(RTO_E_FORMAT, w + ": node " + std::to_string((at - 1) / S) + " slot " + std::to_string((at - 1) % S) +
                                         ": the offset refers outside [1, " + std::to_string(cap) + ")");
    if (const uint32_t at = words[rto::kRefBadShared])
        return set_err(RTO_E_FORMAT, w + ": node " + std::to_string((at - 1) / S) + " slot " + std::to_string((at - 1) % S) +
                                         ": its target is referred to by more than one slot");
    if (words[rto::kRefLevelCount + rto::kSimplifyMaxLevels])
        return set_err(RTO_E_FORMAT, w + ": the walk from the root does not end within " + std::to_string(rto::kSimplifyMaxLevels) + " levels");
    int n_levels = 0;
    int64_t reachable = 0;
    while (n_levels < rto::kSimplifyMaxLevels && words[rto::kRefLevelCount + n_levels]) reachable += words[rto::kRefLevelCount + n_levels++];
    const int64_t K = (int64_t)words[rto::kRefSelected];
    const int64_t cut = K == 0 ? 0 : words[rto::kRefMode] == 1 ? (int64_t)words[rto::kRefMinKey] : (int64_t)words[rto::kRefCut];
    const int64_t cap_out = cap + K;
    *out_capacity = cap_out;
    if (stats)
        *stats = rto_refine_stats{reachable, (int64_t)words[rto::kRefCandidates], K,
                                  std::max<int64_t>(n_levels - 1, (int64_t)words[rto::kRefDeepest]) + 1, cut};
    if (rto::refine_too_large(cap_out, S))
        return set_err(RTO_E_INVALID, w + ": the result's cap * N^3 must stay below 2^31, cap = " + std::to_string(cap_out));
    r->plan = plan, r->selected = K;
    r->planned = true;
    return RTO_OK;
}

int rto_tree_refine_write(rto_refiner* r, void* stream, const int32_t* child, const uint16_t* data, int D, int32_t* child_out,
                          uint16_t* data_out, int32_t* slot_src) {
    const std::string w = "rto_tree_refine_write";
    if (!r || !child) return set_err(RTO_E_INVALID, w + ": null argument");
    if (!r->planned) return set_err(RTO_E_INVALID, w + ": no successful rto_tree_refine_plan precedes the call");
    if ((uintptr_t)child & 3u) return set_err(RTO_E_INVALID, w + ": child is not aligned to 4 bytes");
    const int64_t cap = r->plan.cap, nodes = cap + r->selected, S = r->plan.S;
    // (the keys were read by the plan only: no output can disturb them)
    const std::string bad = rto::refine_check_outputs(child, data, nullptr, cap, r->plan.N, D, child_out, data_out, slot_src, nodes);
    if (!bad.empty()) return set_err(RTO_E_INVALID, w + ": " + bad);
    if (nodes * S > (((int64_t)1 << 39) - 1) / D) return set_err(RTO_E_INVALID, w + ": cap * N^3 * D must stay below 2^39");
    if (pointer_device(child) != r->device) return set_err(RTO_E_INVALID, w + ": child is not memory of the handle's device");
    if (pointer_device(data) != r->device) return set_err(RTO_E_INVALID, w + ": data is not memory of the handle's device");
    if (pointer_device(child_out) != r->device) return set_err(RTO_E_INVALID, w + ": child_out is not memory of the handle's device");
    if (pointer_device(data_out) != r->device) return set_err(RTO_E_INVALID, w + ": data_out is not memory of the handle's device");
    if (slot_src && pointer_device(slot_src) != r->device) return set_err(RTO_E_INVALID, w + ": slot_src is not memory of the handle's device");
    DeviceGuard guard(r->device);
    const hipError_t e = rto::launch_refine_write(r->plan, r->scratch.p, r->selected, child, data, D, child_out, data_out, slot_src,
                                                  (hipStream_t)stream);
    if (e != hipSuccess) return set_err(RTO_E_HIP, w + ": launch failed: " + hipGetErrorString(e));
    return RTO_OK;
}

int rto_tree_refine_host(const int32_t* child, const uint16_t* data, const uint32_t* key, int64_t cap, int N, int D, uint32_t key_thresh,
                         int64_t max_new, int max_level, int32_t* child_out, uint16_t* data_out, int64_t room, int64_t* out_capacity,
                         int32_t* slot_src, rto_refine_stats* stats) {
    std::string err;
    const int rc = rto::tree_refine_host(child, data, key, cap, N, D, key_thresh, max_new, max_level, child_out, data_out, room,
                                         out_capacity, slot_src, stats, &err);
    if (rc != RTO_OK) return set_err(rc, "rto_tree_refine_host: " + err);
    return RTO_OK;
}

}  // extern "C"
