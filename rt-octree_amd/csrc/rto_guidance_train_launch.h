// rto_guidance_train_launch.h -- host-callable launchers of the GuidanceNet training kernels (guidance_train_kernels.hip): the
// network's forward with saved activations, its backward (dW, db per layer) and the image loss with its gradient.  Apart from
// rto_launch.h for the reason rto_denoise_launch.h is: the render kernels' code id changes with the render kernels only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rto {

constexpr int kTrainMaxLayers = 3;
constexpr int kTrainMaxChannels = 64;  // c1 in 1..64 (the fused inference network's domain)
constexpr int kTrainMaxLevels = 6;

// one layer's effective 3x3 convolution, device pointers: w [cout][cin][3][3], b [cout]; dw / db: the backward's outputs
struct TrainLayer {
    const float* w;
    const float* b;
    float* dw;
    float* db;
    int cin, cout;
};

// floats of `acts`: every layer's post-activation planes [n][cout_l][H][W], in layer order
size_t train_acts_floats(const TrainLayer* layers, int num_layers, int n, int H, int W);
// floats of ONE of the backward's two dz buffers (n * widest layer * H * W) and of its partial-sum scratch
size_t train_dz_floats(const TrainLayer* layers, int num_layers, int n, int H, int W);
size_t train_partial_floats(const TrainLayer* layers, int num_layers, int n, int H, int W);

// aux [n][8][H][W] -> acts, weight_map / guidance_map [n][levels][H][W].  One kernel per layer on `stream`.
hipError_t launch_train_forward(const float* aux, const TrainLayer* layers, int num_layers, int levels, int n, int H, int W,
                                float* acts, float* weight_map, float* guidance_map, hipStream_t stream);
// grad_weight_map / grad_guidance_map [n][levels][H][W] -> layers[l].dw / .db, overwritten.  dz0 / dz1: train_dz_floats each;
// partials: train_partial_floats.  No atomics: per-workgroup partial sums, added by a finishing kernel in workgroup order.
hipError_t launch_train_backward(const float* grad_weight_map, const float* grad_guidance_map, const float* aux, const float* acts,
                                 const TrainLayer* layers, int num_layers, int levels, int n, int H, int W, float* dz0, float* dz1,
                                 float* partials, hipStream_t stream);

constexpr int kLossSmape = 0, kLossMse = 1;
constexpr int kLossPixelsPerGroup = 1024;
inline size_t loss_partial_doubles(int n, int H, int W) {
    return ((size_t)n * H * W + kLossPixelsPerGroup - 1) / kLossPixelsPerGroup;
}
// pred / truth [n][H][W][4] float32 -> *loss_out (device double) = mean over r, g, b of the term; grad [n][H][W][4] = d loss / d pred
hipError_t launch_loss(const float* pred, const float* truth, int n, int H, int W, int kind, double* partials, double* loss_out,
                       float* grad, hipStream_t stream);

}  // namespace rto
