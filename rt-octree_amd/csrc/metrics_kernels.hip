// metrics_kernels.hip -- image metrics of a predicted against a true image, per frame and in float64: mean squared error
// (PSNR), SMAPE (denoiser/metrics.py:7-9, 61-62) and SSIM as pytorch_msssim.ssim(X, Y, data_range = 1) defines it (11-tap
// Gaussian, sigma 1.5, no padding; denoiser/metrics.py:78-79).  DESIGN.md 7h.
//
// metrics_tiles: one workgroup per 32 x 16 tile of one frame.  It converts the tile's pixels and a halo of 10 to the right and
// below of both images to float32 (8-bit values / 255.0f, the true image composited over the background if asked) into LDS,
// adds up the error terms of the tile's OWN pixels, and -- where the tile holds positions of the (H - 10) x (W - 10) SSIM map
// -- filters the five moment planes x, y, xx, yy, xy of one channel at a time, along H then along W, evaluates the map and adds
// it up.  Every sum is a double, taken in an order fixed by the thread and tile indices; the workgroup's four sums go to
// partials[frame][tile].  metrics_finish adds each frame's partials in tile order: no atomics, so a frame's result depends on
// neither the batch around it nor the run.
// The file is compiled with -ffp-contract=off (the Makefile's CXXFLAGS): with x == y the map is then 1.0 exactly.
#include <hip/hip_runtime.h>

#include "rto_metrics_launch.h"

namespace rto {
namespace {

constexpr int kTW = kMetricsTileW, kTH = kMetricsTileH;
constexpr int kSW = kTW + kMetricsHalo, kSH = kTH + kMetricsHalo;  // staged region 42 x 26
constexpr int kThreads = 256;
constexpr int kStaged = kSW * kSH;  // 1092 pixels
constexpr int kRows = kTH * kSW;    // 672 values per moment plane after the pass along H
static_assert(5 * kRows >= kMetricsPartials * kThreads, "the reduction reuses the moment planes");

template <bool U8>
__device__ inline float4 load_pixel(const void* __restrict__ base, size_t idx) {
    if (U8) {
        const uchar4 v = reinterpret_cast<const uchar4*>(base)[idx];
        return make_float4((float)v.x / 255.0f, (float)v.y / 255.0f, (float)v.z / 255.0f, (float)v.w / 255.0f);
    }
    return reinterpret_cast<const float4*>(base)[idx];
}

__device__ inline bool finite3(float4 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

__device__ inline void error_terms(float p, float t, double& se, double& sm) {
    const double pd = (double)p, td = (double)t;
    const double d = pd - td;
    se += d * d;
    sm += fabs(d) / (fabs(pd) + fabs(td) + 1e-5);
}

template <bool PU8, bool TU8>
__global__ __launch_bounds__(kThreads) void metrics_tiles(const void* __restrict__ pred, const void* __restrict__ truth, int H, int W,
                                                          int tiles_x, int tiles_per_frame, int composite, float bg,
                                                          MetricsWindow win, double* __restrict__ partials) {
    __shared__ float sx[3][kStaged];
    __shared__ float sy[3][kStaged];
    __shared__ double mom[5][kRows];

    const int tid = threadIdx.x;
    const int frame = blockIdx.x / tiles_per_frame;
    const int tile = blockIdx.x - frame * tiles_per_frame;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int x0 = tx * kTW, y0 = ty * kTH;
    const size_t fbase = (size_t)frame * (size_t)H * (size_t)W;

    double se = 0.0, sm = 0.0, ss = 0.0, bad = 0.0;
    for (int i = tid; i < kStaged; i += kThreads) {
        const int ly = i / kSW, lx = i - ly * kSW;
        const int gx = x0 + lx, gy = y0 + ly;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f), t = p;
        if (gx < W && gy < H) {
            const size_t idx = fbase + (size_t)gy * W + gx;
            p = load_pixel<PU8>(pred, idx);
            t = load_pixel<TU8>(truth, idx);
            if (composite) {  // denoiser/dataset.py:82-84, float32, products and sum rounded one by one
                const float rest = bg * (1.0f - t.w);
                t.x = t.x * t.w + rest;
                t.y = t.y * t.w + rest;
                t.z = t.z * t.w + rest;
            }
            if (lx < kTW && ly < kTH) {  // the tile's own pixels: each pixel of the frame belongs to exactly one tile
                error_terms(p.x, t.x, se, sm);
                error_terms(p.y, t.y, se, sm);
                error_terms(p.z, t.z, se, sm);
                if (!finite3(p) || !finite3(t)) bad += 1.0;
            }
        }
        sx[0][i] = p.x, sx[1][i] = p.y, sx[2][i] = p.z;
        sy[0][i] = t.x, sy[1][i] = t.y, sy[2][i] = t.z;
    }
    __syncthreads();

    const int map_w = W - kMetricsHalo, map_h = H - kMetricsHalo;
    if (x0 < map_w && y0 < map_h) {  // (uniform over the workgroup)
        for (int c = 0; c < 3; ++c) {
            // along H: moment planes at the tile's 16 rows, all 42 columns
            for (int i = tid; i < kRows; i += kThreads) {
                double ax = 0.0, ay = 0.0, axx = 0.0, ayy = 0.0, axy = 0.0;
#pragma unroll
                for (int k = 0; k < kMetricsTaps; ++k) {
                    const double x = (double)sx[c][i + k * kSW], y = (double)sy[c][i + k * kSW];
                    const double g = win.g[k];
                    ax += g * x;
                    ay += g * y;
                    axx += g * (x * x);
                    ayy += g * (y * y);
                    axy += g * (x * y);
                }
                mom[0][i] = ax, mom[1][i] = ay, mom[2][i] = axx, mom[3][i] = ayy, mom[4][i] = axy;
            }
            __syncthreads();
            // along W, then the map (pytorch_msssim _ssim: C1 = 0.01^2, C2 = 0.03^2 at data_range 1)
            for (int o = tid; o < kTW * kTH; o += kThreads) {
                const int oy = o / kTW, ox = o - oy * kTW;
                if (x0 + ox < map_w && y0 + oy < map_h) {
                    const int b = oy * kSW + ox;
                    double mx = 0.0, my = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
#pragma unroll
                    for (int k = 0; k < kMetricsTaps; ++k) {
                        const double g = win.g[k];
                        mx += g * mom[0][b + k];
                        my += g * mom[1][b + k];
                        exx += g * mom[2][b + k];
                        eyy += g * mom[3][b + k];
                        exy += g * mom[4][b + k];
                    }
                    const double C1 = 1e-4, C2 = 9e-4;
                    const double mxx = mx * mx, myy = my * my, mxy = mx * my;
                    const double vxx = exx - mxx, vyy = eyy - myy, vxy = exy - mxy;
                    const double cs = (2.0 * vxy + C2) / (vxx + vyy + C2);
                    const double lum = (2.0 * mxy + C1) / (mxx + myy + C1);
                    ss += lum * cs;
                }
            }
            __syncthreads();
        }
    }

    // the workgroup's sums: a tree over the thread index, the same additions every time
    double* red = &mom[0][0];
    red[0 * kThreads + tid] = se;
    red[1 * kThreads + tid] = sm;
    red[2 * kThreads + tid] = ss;
    red[3 * kThreads + tid] = bad;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < kMetricsPartials; ++q) red[q * kThreads + tid] += red[q * kThreads + tid + s];
        }
        __syncthreads();
    }
    if (tid < kMetricsPartials) partials[(size_t)blockIdx.x * kMetricsPartials + tid] = red[tid * kThreads];
}

// one workgroup per frame; lane q < 4 adds partial q of the frame's tiles in tile order, lane 0 writes the four results
__global__ __launch_bounds__(64) void metrics_finish(const double* __restrict__ partials, int tiles_per_frame, int H, int W,
                                                     double* __restrict__ out) {
    __shared__ double sums[kMetricsPartials];
    const int frame = blockIdx.x, q = threadIdx.x;
    if (q < kMetricsPartials) {
        const double* p = partials + (size_t)frame * tiles_per_frame * kMetricsPartials + q;
        double s = 0.0;
        for (int w = 0; w < tiles_per_frame; ++w) s += p[(size_t)w * kMetricsPartials];
        sums[q] = s;
    }
    __syncthreads();
    if (q == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        const double count = 3.0 * (double)H * (double)W;
        const int map_w = W - kMetricsHalo, map_h = H - kMetricsHalo;
        double mse = sums[0] / count;
        double psnr = -10.0 * log10(mse);
        double smape = sums[1] / count;
        double ssim = (map_w > 0 && map_h > 0) ? sums[2] / (3.0 * (double)map_w * (double)map_h) : nan;
        if (sums[3] != 0.0) mse = psnr = smape = ssim = nan;  // a non-finite pixel: the frame has no measure
        double* o = out + (size_t)frame * 4;
        o[0] = mse, o[1] = psnr, o[2] = smape, o[3] = ssim;
    }
}

}  // namespace

hipError_t launch_metrics(const void* pred, bool pred_u8, const void* truth, bool truth_u8, int n, int H, int W, bool composite,
                          float background, const MetricsWindow& window, double* partials, double* out, hipStream_t stream) {
    const int tiles_x = metrics_tiles_x(W), tiles = tiles_x * metrics_tiles_y(H);
    const dim3 grid((unsigned)((size_t)tiles * n)), block(kThreads);
    const int comp = composite ? 1 : 0;
    if (pred_u8 && truth_u8)
        metrics_tiles<true, true><<<grid, block, 0, stream>>>(pred, truth, H, W, tiles_x, tiles, comp, background, window, partials);
    else if (pred_u8)
        metrics_tiles<true, false><<<grid, block, 0, stream>>>(pred, truth, H, W, tiles_x, tiles, comp, background, window, partials);
    else if (truth_u8)
        metrics_tiles<false, true><<<grid, block, 0, stream>>>(pred, truth, H, W, tiles_x, tiles, comp, background, window, partials);
    else
        metrics_tiles<false, false><<<grid, block, 0, stream>>>(pred, truth, H, W, tiles_x, tiles, comp, background, window, partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    metrics_finish<<<dim3((unsigned)n), dim3(64), 0, stream>>>(partials, tiles, H, W, out);
    return hipGetLastError();
}

}  // namespace rto
