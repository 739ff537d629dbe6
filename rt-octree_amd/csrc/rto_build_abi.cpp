// rto_build_abi.cpp -- C ABI of the grid builder (include/rto.h "grid builder"): the device entries (build_kernels.hip) and the
// host twin (host/grid_build.cpp).  Errors, the device scope, the shared checks and the scratch buffer come from
// rto_abi_common.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "host/grid_build.h"
#include "rto.h"
#include "rto_abi_common.h"
#include "rto_build_launch.h"

struct rto_tree_builder {
    int device = 0;
    DeviceBuf scratch;  // rto::BuildPlan lays it out
    bool planned = false;
    rto::BuildPlan plan;
    rto::GridView grid;
    rto::BuildCounts counts;
};

extern "C" {

int rto_tree_builder_create(int device, rto_tree_builder** out) {
    if (!out) return set_err(RTO_E_INVALID, "rto_tree_builder_create: null argument");
    *out = nullptr;
    if (const int rc = check_device_index(device, "no HIP device available")) return rc;
    rto_tree_builder* b = new rto_tree_builder();
    b->device = device;
    *out = b;
    return RTO_OK;
}

void rto_tree_builder_free(rto_tree_builder* b) {
    if (!b) return;
    {
        DeviceGuard guard(b->device);
        if (b->scratch.p) (void)hipDeviceSynchronize();
        b->scratch.release();
    }
    delete b;
}

int rto_tree_build_plan(rto_tree_builder* b, void* stream, const uint16_t* grid, int L, int D, float kill_thresh, int64_t* out_capacity,
                        rto_grid_build_stats* stats) {
    const std::string w = "rto_tree_build_plan";
    if (!b || !out_capacity) return set_err(RTO_E_INVALID, w + ": null argument");
    b->planned = false;
    const std::string bad = rto::grid_build_check_args(grid, L, D, nullptr, nullptr, 0);
    if (!bad.empty()) return set_err(RTO_E_INVALID, w + ": " + bad);
    if (pointer_device(grid) != b->device) return set_err(RTO_E_INVALID, w + ": grid is not memory of the handle's device");
    DeviceGuard guard(b->device);
    const rto::BuildPlan plan = rto::build_plan(L, D);
    if (const int rc = b->scratch.reserve(plan.total, "grid builder scratch")) return rc;
    rto::GridView g;
    g.grid = grid, g.L = L, g.D = D;
    g.kill = std::isnan(kill_thresh) ? 0 : 1;
    g.th = g.kill ? rto::simp_thresh_half(kill_thresh) : 0u;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = rto::launch_build_plan(plan, b->scratch.p, g, st);
    if (e != hipSuccess) return set_err(RTO_E_HIP, w + ": launch failed: " + hipGetErrorString(e));
    uint32_t words[rto::kBuildWords];
    e = hipMemcpyAsync(words, b->scratch.as<char>() + plan.words, sizeof(words), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return set_err(RTO_E_HIP, w + ": " + hipGetErrorString(e));
    rto::BuildCounts counts;
    int64_t nodes = 0;
    int levels = 0;
    while (levels < L && words[rto::kBuildLevelCount + levels]) nodes += words[rto::kBuildLevelCount + levels++];
    uint64_t killed;
    std::memcpy(&killed, words + rto::kBuildKilled, sizeof(killed));
    *out_capacity = nodes;
    if (stats) *stats = rto_grid_build_stats{nodes, (int64_t)killed, (int64_t)levels};
    if (rto::grid_build_too_large(nodes)) return set_err(RTO_E_INVALID, w + ": nodes * 8 must stay below 2^31, nodes = " + std::to_string(nodes));
    counts.levels = levels;
    uint32_t at = 0;
    for (int l = 0; l <= rto::kGridBuildMaxL; ++l) {
        counts.start[l] = at;
        if (l < levels) at += words[rto::kBuildLevelCount + l];
    }
    b->plan = plan, b->grid = g, b->counts = counts;
    b->planned = true;
    return RTO_OK;
}

int rto_tree_build_write(rto_tree_builder* b, void* stream, int32_t* child_out, uint16_t* data_out) {
    const std::string w = "rto_tree_build_write";
    if (!b || !child_out || !data_out) return set_err(RTO_E_INVALID, w + ": null argument");
    if (!b->planned) return set_err(RTO_E_INVALID, w + ": no successful rto_tree_build_plan precedes the call");
    const int64_t nodes = b->counts.start[b->counts.levels];
    const std::string bad = rto::grid_build_check_args(b->grid.grid, b->grid.L, b->grid.D, child_out, data_out, nodes);
    if (!bad.empty()) return set_err(RTO_E_INVALID, w + ": " + bad);
    if (pointer_device(child_out) != b->device) return set_err(RTO_E_INVALID, w + ": child_out is not memory of the handle's device");
    if (pointer_device(data_out) != b->device) return set_err(RTO_E_INVALID, w + ": data_out is not memory of the handle's device");
    DeviceGuard guard(b->device);
    const hipError_t e = rto::launch_build_write(b->plan, b->scratch.p, b->grid, b->counts, child_out, data_out, (hipStream_t)stream);
    if (e != hipSuccess) return set_err(RTO_E_HIP, w + ": launch failed: " + hipGetErrorString(e));
    return RTO_OK;
}

int rto_tree_build_host(const uint16_t* grid, int L, int D, float kill_thresh, int32_t* child_out, uint16_t* data_out, int64_t room,
                        int64_t* out_capacity, rto_grid_build_stats* stats) {
    std::string err;
    if (!out_capacity) return set_err(RTO_E_INVALID, "rto_tree_build_host: null argument");
    const int rc = rto::grid_build_host(grid, L, D, kill_thresh, child_out, data_out, room, out_capacity, stats, &err);
    if (rc != RTO_OK) return set_err(rc, "rto_tree_build_host: " + err);
    return RTO_OK;
}

}  // extern "C"
