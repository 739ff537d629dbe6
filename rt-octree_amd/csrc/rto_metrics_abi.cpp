// rto_metrics_abi.cpp -- C ABI of the image metrics (include/rto.h, metrics_kernels.hip) and of the PNG reader (host/png_read.cpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>

#include "host/png_read.h"
#include "rto.h"
#include "rto_metrics_launch.h"

struct rto_metrics {
    int device = 0;
    rto::MetricsWindow window{};
    double* partials = nullptr;  // [frame][workgroup][4]
    size_t partials_doubles = 0;
    double* results = nullptr;   // rto_metrics_compute: [n][4]
    size_t results_doubles = 0;
};

namespace {
// rto_abi.cpp owns the thread-local error string; this translation unit reports through it
extern "C" int rto_set_error_(int code, const char* msg);
int fail(int code, const std::string& m) { return rto_set_error_(code, m.c_str()); }

struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

int pointer_device(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    if (a.type == hipMemoryTypeUnregistered) return -1;  // (a plain host pointer)
    return a.device;
}

// grows a scratch of the handle to `need` doubles.  Growing frees the old buffer, which earlier work may still use: the one
// place this file synchronises (the rule of reserve_packed, rto_guidance_abi.cpp)
int reserve(double** buf, size_t* have, size_t need, const char* what) {
    if (need <= *have) return RTO_OK;
    if (*buf) {
        if (hipDeviceSynchronize() != hipSuccess || hipFree(*buf) != hipSuccess) return fail(RTO_E_HIP, "hipFree failed");
        *buf = nullptr;
        *have = 0;
    }
    if (hipMalloc((void**)buf, need * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        *buf = nullptr;
        return fail(RTO_E_HIP, std::string("hipMalloc(") + what + ") failed");
    }
    *have = need;
    return RTO_OK;
}

bool known_format(int f) { return f == RTO_IMAGE_RGBA32F || f == RTO_IMAGE_RGBA8; }

// everything that is refused, decided before anything is enqueued; `out` may be the handle's own result buffer (checked = false)
int validate(const char* who, const rto_metrics* m, const void* pred, int pred_format, const void* truth, int truth_format, int n,
             int H, int W, int flags, float background, const void* out, bool out_is_device) {
    const std::string w(who);
    if (!m || !pred || !truth || !out) return fail(RTO_E_INVALID, w + ": null argument");
    if (n < 1 || H < 1 || W < 1)
        return fail(RTO_E_INVALID, w + ": n, H and W must be at least 1, not " + std::to_string(n) + ", " + std::to_string(H) + ", " + std::to_string(W));
    if (!known_format(pred_format) || !known_format(truth_format))
        return fail(RTO_E_INVALID, w + ": unknown image format " + std::to_string(known_format(pred_format) ? truth_format : pred_format) +
                                       " (RTO_IMAGE_RGBA32F or RTO_IMAGE_RGBA8)");
    if (flags & ~RTO_METRICS_TRUTH_OVER_BACKGROUND) return fail(RTO_E_INVALID, w + ": unknown flag bits " + std::to_string(flags & ~RTO_METRICS_TRUTH_OVER_BACKGROUND));
    if ((flags & RTO_METRICS_TRUTH_OVER_BACKGROUND) && !std::isfinite(background))
        return fail(RTO_E_INVALID, w + ": the background is not finite");
    if ((int64_t)n * H * W > (int64_t)INT32_MAX)
        return fail(RTO_E_INVALID, w + ": " + std::to_string(n) + " x " + std::to_string(H) + " x " + std::to_string(W) + " pixels exceed the 2^31 - 1 the index arithmetic takes");
    const auto misaligned = [](const void* p, int format) { return ((uintptr_t)p & (format == RTO_IMAGE_RGBA32F ? 15u : 3u)) != 0; };
    if (misaligned(pred, pred_format) || misaligned(truth, truth_format))
        return fail(RTO_E_INVALID, w + ": an image is not aligned to its pixel size (16 bytes RGBA32F, 4 bytes RGBA8)");
    if (pointer_device(pred) != m->device) return fail(RTO_E_INVALID, w + ": pred is not memory of the handle's device");
    if (pointer_device(truth) != m->device) return fail(RTO_E_INVALID, w + ": truth is not memory of the handle's device");
    if (out_is_device) {
        if ((uintptr_t)out & 7u) return fail(RTO_E_INVALID, w + ": device_out is not aligned to 8 bytes");
        if (pointer_device(out) != m->device) return fail(RTO_E_INVALID, w + ": device_out is not memory of the handle's device");
    }
    return RTO_OK;
}

int enqueue(rto_metrics* m, hipStream_t stream, const void* pred, int pred_format, const void* truth, int truth_format, int n, int H,
            int W, int flags, float background, double* device_out) {
    if (const int rc = reserve(&m->partials, &m->partials_doubles, rto::metrics_scratch_doubles(n, H, W), "metric partial sums")) return rc;
    const hipError_t e = rto::launch_metrics(pred, pred_format == RTO_IMAGE_RGBA8, truth, truth_format == RTO_IMAGE_RGBA8, n, H, W,
                                             (flags & RTO_METRICS_TRUTH_OVER_BACKGROUND) != 0, background, m->window, m->partials,
                                             device_out, stream);
    if (e != hipSuccess) return fail(RTO_E_HIP, std::string("metrics launch failed: ") + hipGetErrorString(e));
    return RTO_OK;
}
}  // namespace

extern "C" {

int rto_metrics_create(int device, rto_metrics** out) {
    if (!out) return fail(RTO_E_INVALID, "rto_metrics_create: null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(RTO_E_HIP, "no HIP device available");
    }
    if (device < 0 || device >= ndev) return fail(RTO_E_INVALID, "device index out of range");
    rto_metrics* m = new rto_metrics();
    m->device = device;
    double sum = 0.0;  // pytorch_msssim _fspecial_gauss_1d(11, 1.5)
    for (int i = 0; i < rto::kMetricsTaps; ++i) sum += (m->window.g[i] = std::exp(-(double)((i - 5) * (i - 5)) / 4.5));
    for (int i = 0; i < rto::kMetricsTaps; ++i) m->window.g[i] /= sum;
    *out = m;
    return RTO_OK;
}

void rto_metrics_free(rto_metrics* m) {
    if (!m) return;
    {
        DeviceScope scope(m->device);
        if (m->partials || m->results) (void)hipDeviceSynchronize();
        if (m->partials) (void)hipFree(m->partials);
        if (m->results) (void)hipFree(m->results);
    }
    delete m;
}

int rto_metrics_compute_async(rto_metrics* m, void* stream, const void* pred, int pred_format, const void* truth, int truth_format,
                              int n, int H, int W, int flags, float background, double* device_out) {
    if (const int rc = validate("rto_metrics_compute_async", m, pred, pred_format, truth, truth_format, n, H, W, flags, background, device_out, true))
        return rc;
    DeviceScope scope(m->device);
    return enqueue(m, (hipStream_t)stream, pred, pred_format, truth, truth_format, n, H, W, flags, background, device_out);
}

int rto_metrics_compute(rto_metrics* m, void* stream, const void* pred, int pred_format, const void* truth, int truth_format, int n,
                        int H, int W, int flags, float background, rto_frame_metrics* host_out) {
    if (const int rc = validate("rto_metrics_compute", m, pred, pred_format, truth, truth_format, n, H, W, flags, background, host_out, false))
        return rc;
    static_assert(sizeof(rto_frame_metrics) == 4 * sizeof(double), "rto_frame_metrics is the device row");
    DeviceScope scope(m->device);
    if (const int rc = reserve(&m->results, &m->results_doubles, (size_t)n * 4, "metric results")) return rc;
    if (const int rc = enqueue(m, (hipStream_t)stream, pred, pred_format, truth, truth_format, n, H, W, flags, background, m->results)) return rc;
    hipError_t e = hipMemcpyAsync(host_out, m->results, (size_t)n * sizeof(rto_frame_metrics), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return fail(RTO_E_HIP, std::string("metrics download failed: ") + hipGetErrorString(e));
    return RTO_OK;
}

int rto_image_read_png(const char* path, int* width, int* height, uint8_t* rgba, size_t cap) {
    if (!path || !width || !height) return fail(RTO_E_INVALID, "rto_image_read_png: null argument");
    try {
        int w = 0, h = 0;
        rto::png_read_size(path, &w, &h);
        *width = w, *height = h;
        if (!rgba || cap < (size_t)w * (size_t)h * 4) return RTO_OK;
        const rto::PngImage img = rto::png_read(path);
        std::memcpy(rgba, img.rgba.data(), img.rgba.size());
    } catch (const std::exception& e) {
        return fail(RTO_E_IO, e.what());
    }
    return RTO_OK;
}

}  // extern "C"
