// rto_metrics_launch.h -- host-callable launchers of the image-metric kernels (metrics_kernels.hip): per-frame squared error,
// SMAPE and SSIM of a predicted against a true image, in float64.  Apart from rto_launch.h for the reason rto_denoise_launch.h
// is: the render kernels' code id changes with the render kernels only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rto {

// one workgroup = one tile of kMetricsTileW x kMetricsTileH pixels of one frame: the error sums over those pixels, the SSIM
// map over the output positions of the same coordinates (which read kMetricsHalo more pixels to the right and below)
constexpr int kMetricsTileW = 32, kMetricsTileH = 16;
constexpr int kMetricsTaps = 11, kMetricsHalo = kMetricsTaps - 1;
constexpr int kMetricsPartials = 4;  // per workgroup: sum (p - t)^2, sum smape terms, sum of the SSIM map, non-finite pixels

struct MetricsWindow {
    double g[kMetricsTaps];  // exp(-(i - 5)^2 / 4.5) / sum, computed in double on the host
};

inline int metrics_tiles_x(int W) { return (W + kMetricsTileW - 1) / kMetricsTileW; }
inline int metrics_tiles_y(int H) { return (H + kMetricsTileH - 1) / kMetricsTileH; }
// doubles of partial-sum scratch a call of n frames of H x W needs
inline size_t metrics_scratch_doubles(int n, int H, int W) {
    return (size_t)n * metrics_tiles_x(W) * metrics_tiles_y(H) * kMetricsPartials;
}

// pred / truth: [n][H][W][4], float32 (u8 = false) or 8-bit (u8 = true, value / 255.0f); composite: truth rgb becomes
// rgb * a + background * (1 - a) in float32.  partials: metrics_scratch_doubles(n, H, W) doubles; out: [n][4] doubles =
// mse, psnr, smape, ssim.  Two kernels on `stream`; no atomics, every frame's sums are taken in a fixed order.
hipError_t launch_metrics(const void* pred, bool pred_u8, const void* truth, bool truth_u8, int n, int H, int W, bool composite,
                          float background, const MetricsWindow& window, double* partials, double* out, hipStream_t stream);

}  // namespace rto
