// rto_quantize_abi.cpp -- C ABI of the median-cut quantiser (include/rto.h "quantiser"): the device entry (quantize_kernels.hip)
// and the host twin (host/median_cut.cpp).  Errors, the device scope, the shared checks and the scratch buffer come from
// rto_abi_common.h.
#include <hip/hip_runtime.h>

#include <string>

#include "host/median_cut.h"
#include "rto.h"
#include "rto_abi_common.h"
#include "rto_quantize_launch.h"

struct rto_quantizer {
    int device = 0;
    DeviceBuf scratch;  // rto::QuantPlan lays it out
};

extern "C" {

int rto_quantizer_create(int device, rto_quantizer** out) {
    if (!out) return set_err(RTO_E_INVALID, "rto_quantizer_create: null argument");
    *out = nullptr;
    if (const int rc = check_device_index(device, "no HIP device available")) return rc;
    rto_quantizer* q = new rto_quantizer();
    q->device = device;
    *out = q;
    return RTO_OK;
}

void rto_quantizer_free(rto_quantizer* q) {
    if (!q) return;
    {
        DeviceGuard guard(q->device);
        if (q->scratch.p) (void)hipDeviceSynchronize();
        q->scratch.release();
    }
    delete q;
}

int rto_quantize_median_cut(rto_quantizer* q, void* stream, const uint16_t* rows, int64_t m, int bits, uint16_t* palette, uint16_t* ids) {
    const std::string w = "rto_quantize_median_cut";
    if (!q || !rows || !palette || !ids) return set_err(RTO_E_INVALID, w + ": null argument");
    if (m < 1 || m > (int64_t)INT32_MAX) return set_err(RTO_E_INVALID, w + ": m must be in 1 .. 2^31 - 1, not " + std::to_string(m));
    if (bits < 1 || bits > rto::kMedianCutMaxBits) return set_err(RTO_E_INVALID, w + ": bits must be in 1 .. 16, not " + std::to_string(bits));
    if (((uintptr_t)rows | (uintptr_t)palette | (uintptr_t)ids) & 1u) return set_err(RTO_E_INVALID, w + ": a pointer is not aligned to 2 bytes");
    if (pointer_device(rows) != q->device) return set_err(RTO_E_INVALID, w + ": rows is not memory of the handle's device");
    if (pointer_device(palette) != q->device) return set_err(RTO_E_INVALID, w + ": palette is not memory of the handle's device");
    if (pointer_device(ids) != q->device) return set_err(RTO_E_INVALID, w + ": ids is not memory of the handle's device");
    DeviceGuard guard(q->device);
    const rto::QuantPlan plan = rto::quantize_plan(m, bits);
    if (const int rc = q->scratch.reserve(plan.total, "quantiser scratch")) return rc;
    hipError_t e = rto::launch_quantize(plan, q->scratch.p, rows, palette, ids, (hipStream_t)stream);
    if (e != hipSuccess) return set_err(RTO_E_HIP, w + ": launch failed: " + hipGetErrorString(e));
    uint32_t flags[2] = {0, 0};
    e = hipMemcpyAsync(flags, q->scratch.as<char>() + plan.flags, sizeof(flags), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return set_err(RTO_E_HIP, w + ": " + hipGetErrorString(e));
    if (flags[0]) return set_err(RTO_E_INVALID, w + ": a row holds a NaN or an infinity");
    if (rto::mc_sum_overflows(m, flags[1])) return set_err(RTO_E_INVALID, w + ": m * max|value| * 2^24 reaches 2^63: a box sum could overflow");
    return RTO_OK;
}

int rto_quantize_median_cut_host(const uint16_t* rows, int64_t m, int bits, uint16_t* palette, uint16_t* ids) {
    std::string err;
    if (!rto::median_cut_host(rows, m, bits, palette, ids, &err)) return set_err(RTO_E_INVALID, "rto_quantize_median_cut_host: " + err);
    return RTO_OK;
}

}  // extern "C"
