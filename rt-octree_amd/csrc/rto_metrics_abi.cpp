// rto_metrics_abi.cpp -- C ABI of the image metrics (include/rto.h, metrics_kernels.hip) and of the PNG reader (host/png_read.cpp).
// Errors, the device scope, the shared checks and the two scratch buffers come from rto_abi_common.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>

#include "host/png_read.h"
#include "rto.h"
#include "rto_abi_common.h"
#include "rto_metrics_launch.h"

struct rto_metrics {
    int device = 0;
    rto::MetricsWindow window{};
    DeviceBuf partials;  // doubles [frame][workgroup][4]
    DeviceBuf results;   // rto_metrics_compute: doubles [n][4]
};

namespace {
bool known_format(int f) { return f == RTO_IMAGE_RGBA32F || f == RTO_IMAGE_RGBA8; }

// everything that is refused, decided before anything is enqueued; `out` may be the handle's own result buffer (checked = false)
int validate(const char* who, const rto_metrics* m, const void* pred, int pred_format, const void* truth, int truth_format, int n,
             int H, int W, int flags, float background, const void* out, bool out_is_device) {
    const std::string w(who);
    if (!m || !pred || !truth || !out) return set_err(RTO_E_INVALID, w + ": null argument");
    if (const int rc = check_frames(w, n, H, W)) return rc;
    if (!known_format(pred_format) || !known_format(truth_format))
        return set_err(RTO_E_INVALID, w + ": unknown image format " + std::to_string(known_format(pred_format) ? truth_format : pred_format) +
                                       " (RTO_IMAGE_RGBA32F or RTO_IMAGE_RGBA8)");
    if (flags & ~RTO_METRICS_TRUTH_OVER_BACKGROUND) return set_err(RTO_E_INVALID, w + ": unknown flag bits " + std::to_string(flags & ~RTO_METRICS_TRUTH_OVER_BACKGROUND));
    if ((flags & RTO_METRICS_TRUTH_OVER_BACKGROUND) && !std::isfinite(background))
        return set_err(RTO_E_INVALID, w + ": the background is not finite");
    const auto misaligned = [](const void* p, int format) { return ((uintptr_t)p & (format == RTO_IMAGE_RGBA32F ? 15u : 3u)) != 0; };
    if (misaligned(pred, pred_format) || misaligned(truth, truth_format))
        return set_err(RTO_E_INVALID, w + ": an image is not aligned to its pixel size (16 bytes RGBA32F, 4 bytes RGBA8)");
    if (pointer_device(pred) != m->device) return set_err(RTO_E_INVALID, w + ": pred is not memory of the handle's device");
    if (pointer_device(truth) != m->device) return set_err(RTO_E_INVALID, w + ": truth is not memory of the handle's device");
    if (out_is_device) {
        if ((uintptr_t)out & 7u) return set_err(RTO_E_INVALID, w + ": device_out is not aligned to 8 bytes");
        if (pointer_device(out) != m->device) return set_err(RTO_E_INVALID, w + ": device_out is not memory of the handle's device");
    }
    return RTO_OK;
}

int enqueue(rto_metrics* m, hipStream_t stream, const void* pred, int pred_format, const void* truth, int truth_format, int n, int H,
            int W, int flags, float background, double* device_out) {
    if (const int rc = m->partials.reserve(rto::metrics_scratch_doubles(n, H, W) * sizeof(double), "metric partial sums")) return rc;
    const hipError_t e = rto::launch_metrics(pred, pred_format == RTO_IMAGE_RGBA8, truth, truth_format == RTO_IMAGE_RGBA8, n, H, W,
                                             (flags & RTO_METRICS_TRUTH_OVER_BACKGROUND) != 0, background, m->window, m->partials.as<double>(),
                                             device_out, stream);
    if (e != hipSuccess) return set_err(RTO_E_HIP, std::string("metrics launch failed: ") + hipGetErrorString(e));
    return RTO_OK;
}
}  // namespace

extern "C" {

int rto_metrics_create(int device, rto_metrics** out) {
    if (!out) return set_err(RTO_E_INVALID, "rto_metrics_create: null argument");
    *out = nullptr;
    if (const int rc = check_device_index(device, "no HIP device available")) return rc;
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
        DeviceGuard guard(m->device);
        if (m->partials.p || m->results.p) (void)hipDeviceSynchronize();
        m->partials.release();
        m->results.release();
    }
    delete m;
}

int rto_metrics_compute_async(rto_metrics* m, void* stream, const void* pred, int pred_format, const void* truth, int truth_format,
                              int n, int H, int W, int flags, float background, double* device_out) {
    if (const int rc = validate("rto_metrics_compute_async", m, pred, pred_format, truth, truth_format, n, H, W, flags, background, device_out, true))
        return rc;
    DeviceGuard guard(m->device);
    return enqueue(m, (hipStream_t)stream, pred, pred_format, truth, truth_format, n, H, W, flags, background, device_out);
}

int rto_metrics_compute(rto_metrics* m, void* stream, const void* pred, int pred_format, const void* truth, int truth_format, int n,
                        int H, int W, int flags, float background, rto_frame_metrics* host_out) {
    if (const int rc = validate("rto_metrics_compute", m, pred, pred_format, truth, truth_format, n, H, W, flags, background, host_out, false))
        return rc;
    static_assert(sizeof(rto_frame_metrics) == 4 * sizeof(double), "rto_frame_metrics is the device row");
    DeviceGuard guard(m->device);
    if (const int rc = m->results.reserve((size_t)n * sizeof(rto_frame_metrics), "metric results")) return rc;
    if (const int rc = enqueue(m, (hipStream_t)stream, pred, pred_format, truth, truth_format, n, H, W, flags, background, m->results.as<double>()))
        return rc;
    hipError_t e = hipMemcpyAsync(host_out, m->results.p, (size_t)n * sizeof(rto_frame_metrics), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return set_err(RTO_E_HIP, std::string("metrics download failed: ") + hipGetErrorString(e));
    return RTO_OK;
}

int rto_image_read_png(const char* path, int* width, int* height, uint8_t* rgba, size_t cap) {
    if (!path || !width || !height) return set_err(RTO_E_INVALID, "rto_image_read_png: null argument");
    try {
        int w = 0, h = 0;
        rto::png_read_size(path, &w, &h);
        *width = w, *height = h;
        if (!rgba || cap < (size_t)w * (size_t)h * 4) return RTO_OK;
        const rto::PngImage img = rto::png_read(path);
        std::memcpy(rgba, img.rgba.data(), img.rgba.size());
    } catch (const std::exception& e) {
        return set_err(RTO_E_IO, e.what());
    }
    return RTO_OK;
}

}  // extern "C"
