// rto_abi_common.h -- what every translation unit behind the C ABI needs, whether it knows the render handles (rto_internal.h
// includes this) or not (rto_guidance_abi.cpp, rto_metrics_abi.cpp, rto_guidance_train_abi.cpp): the error plumbing, the device
// scope of a call, the checks the *_create and frame-taking entries share, and the scratch buffer of a handle.
// Depends on the HIP runtime, <string> and rto.h only.  Not installed; nothing here is an exported symbol.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "rto.h"

#pragma GCC visibility push(hidden)

// records msg as the calling thread's last error (rto_last_error; the string lives in rto_abi.cpp) and returns code
int set_err(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                                        \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return set_err(RTO_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" + \
                                          std::to_string(__LINE__) + ")");                                   \
    } while (0)

// set the device for the scope of one ABI call, restore the caller's device afterwards: a handle's buffers live on its own
// device, so the call launches (and frees) there, whatever device is current
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) {
            ok = false;
            return;
        }
        if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// the device that owns p, or -1: the query failed, or p is a plain host pointer
inline int pointer_device(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    if (a.type == hipMemoryTypeUnregistered) return -1;
    return a.device;
}

// the device argument of a *_create; no_device_msg: what a machine without a device is told
inline int check_device_index(int device, const char* no_device_msg) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();  // (the failed query is not the next call's error)
        return set_err(RTO_E_HIP, no_device_msg);
    }
    if (device < 0 || device >= ndev) return set_err(RTO_E_INVALID, "device index out of range");
    return RTO_OK;
}

// n frames of H x W pixels as the kernels index them: all at least 1, and n * H * W within an int
inline int check_frames(const std::string& who, int n, int H, int W) {
    const auto dims = [&](const char* sep) { return std::to_string(n) + sep + std::to_string(H) + sep + std::to_string(W); };
    if (n < 1 || H < 1 || W < 1) return set_err(RTO_E_INVALID, who + ": n, H and W must be at least 1, not " + dims(", "));
    if ((int64_t)n * H * W > (int64_t)INT32_MAX)
        return set_err(RTO_E_INVALID, who + ": " + dims(" x ") + " pixels exceed the 2^31 - 1 the index arithmetic takes");
    return RTO_OK;
}

// A scratch buffer of a handle, on the handle's device (the caller holds a DeviceGuard).  It only ever grows.  Growing frees the
// old buffer, which work enqueued earlier may still use: that is the one place the ABI synchronises the device on behalf of a
// scratch -- callers that must stay asynchronous reserve up front (rto_guidance_net_reserve).
struct DeviceBuf {
    void* p = nullptr;
    size_t bytes = 0;

    // at least need_bytes; what: the buffer's name in the message of a failed allocation.  *regrown = true when the buffer was
    // replaced (its contents are gone); after a failed allocation the buffer is empty
    int reserve(size_t need_bytes, const char* what, bool* regrown = nullptr) {
        if (need_bytes <= bytes) return RTO_OK;
        if (p) {
            if (hipDeviceSynchronize() != hipSuccess || hipFree(p) != hipSuccess) return set_err(RTO_E_HIP, "hipFree failed");
            p = nullptr;
            bytes = 0;
        }
        if (regrown) *regrown = true;
        if (hipMalloc(&p, need_bytes) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            return set_err(RTO_E_HIP, std::string("hipMalloc(") + what + ") failed");
        }
        bytes = need_bytes;
        return RTO_OK;
    }
    // (a *_free synchronises once before it releases its buffers)
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

#pragma GCC visibility pop
