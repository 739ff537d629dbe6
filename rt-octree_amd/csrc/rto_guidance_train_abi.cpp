// rto_guidance_train_abi.cpp -- C ABI of the GuidanceNet training kernels and the image loss (include/rto.h "GuidanceNet under
// training", guidance_train_kernels.hip).  Thin argument checking: everything that is refused is refused before any device use.
// Errors, the device scope, the shared checks and the scratch buffers come from rto_abi_common.h.
#include <hip/hip_runtime.h>

#include <string>

#include "cli/imwrite.h"
#include "rto.h"
#include "rto_abi_common.h"
#include "rto_guidance_train_launch.h"

struct rto_guidance_train {
    int device = 0;
    DeviceBuf dz[2];          // the backward's two dz buffers (floats)
    DeviceBuf partials;       // floats [workgroup][cout * cin * 9 + cout]
    DeviceBuf loss_partials;  // doubles
};

namespace {
// the shape checks shared by the size query, the forward and the backward; fills `out` with the layers as the launchers take them
int check_shape(const std::string& w, const rto_guidance_train_layer* layers, int num_layers, int levels, int n, int H, int W,
                bool need_grads, rto::TrainLayer* out) {
    if (!layers) return set_err(RTO_E_INVALID, w + ": null argument");
    if (const int rc = check_frames(w, n, H, W)) return rc;
    if (num_layers < 2 || num_layers > rto::kTrainMaxLayers)
        return set_err(RTO_E_INVALID, w + ": num_layers must be 2 or 3, not " + std::to_string(num_layers));
    for (int l = 0; l < num_layers; ++l) {
        const rto_guidance_train_layer& y = layers[l];
        if (!y.weight || !y.bias || (need_grads && (!y.grad_weight || !y.grad_bias)))
            return set_err(RTO_E_INVALID, w + ": null pointer in layer " + std::to_string(l));
        if (y.cin < 1 || y.cout < 1) return set_err(RTO_E_INVALID, w + ": layer " + std::to_string(l) + " has no channels");
        if (y.cin != (l == 0 ? RTO_AUX_CHANNELS : layers[l - 1].cout))
            return set_err(RTO_E_INVALID, w + ": layer " + std::to_string(l) + " takes " + std::to_string(y.cin) + " channels but is given " +
                                           std::to_string(l == 0 ? RTO_AUX_CHANNELS : layers[l - 1].cout));
    }
    if (layers[num_layers - 1].cout != 2 * levels)
        return set_err(RTO_E_INVALID, w + ": the last layer writes " + std::to_string(layers[num_layers - 1].cout) + " channels, not 2 * levels = " + std::to_string(2 * levels));
    const int c1 = layers[0].cout;
    if (c1 > rto::kTrainMaxChannels || levels < 1 || levels > rto::kTrainMaxLevels || (num_layers == 3 && layers[1].cout != c1))
        return set_err(RTO_E_UNSUPPORTED, w + ": 8 -> c1 [-> c1] -> 2 * levels with c1 in 1..64 and levels in 1..6 only (c1 " + std::to_string(c1) +
                                           ", levels " + std::to_string(levels) + ")");
    for (int l = 0; l < num_layers; ++l)
        out[l] = rto::TrainLayer{layers[l].weight, layers[l].bias, layers[l].grad_weight, layers[l].grad_bias, layers[l].cin, layers[l].cout};
    return RTO_OK;
}
}  // namespace

extern "C" {

int rto_guidance_train_create(int device, rto_guidance_train** out) {
    if (!out) return set_err(RTO_E_INVALID, "rto_guidance_train_create: null argument");
    *out = nullptr;
    if (const int rc = check_device_index(device, "no HIP device available")) return rc;
    rto_guidance_train* t = new rto_guidance_train();
    t->device = device;
    *out = t;
    return RTO_OK;
}

void rto_guidance_train_free(rto_guidance_train* t) {
    if (!t) return;
    {
        DeviceGuard guard(t->device);
        DeviceBuf* const bufs[4] = {&t->dz[0], &t->dz[1], &t->partials, &t->loss_partials};
        if (t->dz[0].p || t->dz[1].p || t->partials.p || t->loss_partials.p) (void)hipDeviceSynchronize();
        for (DeviceBuf* b : bufs) b->release();
    }
    delete t;
}

int rto_guidance_train_acts_bytes(const rto_guidance_train_layer* layers, int num_layers, int levels, int n, int H, int W, size_t* bytes) {
    if (!bytes) return set_err(RTO_E_INVALID, "rto_guidance_train_acts_bytes: null argument");
    rto::TrainLayer tl[rto::kTrainMaxLayers];
    if (const int rc = check_shape("rto_guidance_train_acts_bytes", layers, num_layers, levels, n, H, W, false, tl)) return rc;
    *bytes = rto::train_acts_floats(tl, num_layers, n, H, W) * sizeof(float);
    return RTO_OK;
}

int rto_guidance_train_forward(rto_guidance_train* t, void* stream, const float* aux, const rto_guidance_train_layer* layers, int num_layers,
                               int levels, int n, int H, int W, float* acts, float* weight_map, float* guidance_map) {
    const char* who = "rto_guidance_train_forward";
    if (!t || !aux || !acts || !weight_map || !guidance_map) return set_err(RTO_E_INVALID, std::string(who) + ": null argument");
    rto::TrainLayer tl[rto::kTrainMaxLayers];
    if (const int rc = check_shape(who, layers, num_layers, levels, n, H, W, false, tl)) return rc;
    DeviceGuard guard(t->device);
    const hipError_t e = rto::launch_train_forward(aux, tl, num_layers, levels, n, H, W, acts, weight_map, guidance_map, (hipStream_t)stream);
    if (e != hipSuccess) return set_err(RTO_E_HIP, std::string("training forward launch failed: ") + hipGetErrorString(e));
    return RTO_OK;
}

int rto_guidance_train_backward(rto_guidance_train* t, void* stream, const float* grad_weight_map, const float* grad_guidance_map,
                                const float* aux, const float* acts, const rto_guidance_train_layer* layers, int num_layers, int levels, int n,
                                int H, int W) {
    const char* who = "rto_guidance_train_backward";
    if (!t || !grad_weight_map || !grad_guidance_map || !aux || !acts) return set_err(RTO_E_INVALID, std::string(who) + ": null argument");
    rto::TrainLayer tl[rto::kTrainMaxLayers];
    if (const int rc = check_shape(who, layers, num_layers, levels, n, H, W, true, tl)) return rc;
    DeviceGuard guard(t->device);
    const size_t dz_bytes = rto::train_dz_floats(tl, num_layers, n, H, W) * sizeof(float);
    for (DeviceBuf& dz : t->dz)
        if (const int rc = dz.reserve(dz_bytes, "dz")) return rc;
    if (const int rc = t->partials.reserve(rto::train_partial_floats(tl, num_layers, n, H, W) * sizeof(float), "gradient partial sums")) return rc;
    const hipError_t e = rto::launch_train_backward(grad_weight_map, grad_guidance_map, aux, acts, tl, num_layers, levels, n, H, W,
                                                    t->dz[0].as<float>(), t->dz[1].as<float>(), t->partials.as<float>(), (hipStream_t)stream);
    if (e != hipSuccess) return set_err(RTO_E_HIP, std::string("training backward launch failed: ") + hipGetErrorString(e));
    return RTO_OK;
}

int rto_loss_forward_backward(rto_guidance_train* t, void* stream, const float* pred, const float* truth, int n, int H, int W, int kind,
                              double* device_loss, float* grad_pred) {
    const std::string w("rto_loss_forward_backward");
    if (!t || !pred || !truth || !device_loss || !grad_pred) return set_err(RTO_E_INVALID, w + ": null argument");
    if (const int rc = check_frames(w, n, H, W)) return rc;
    if (kind != RTO_LOSS_SMAPE && kind != RTO_LOSS_MSE) return set_err(RTO_E_INVALID, w + ": unknown loss " + std::to_string(kind) + " (RTO_LOSS_SMAPE or RTO_LOSS_MSE)");
    if ((((uintptr_t)pred | (uintptr_t)truth | (uintptr_t)grad_pred) & 15u) || ((uintptr_t)device_loss & 7u))
        return set_err(RTO_E_INVALID, w + ": an image is not aligned to 16 bytes, or device_loss not to 8");
    DeviceGuard guard(t->device);
    if (const int rc = t->loss_partials.reserve(rto::loss_partial_doubles(n, H, W) * sizeof(double), "loss partial sums")) return rc;
    static_assert(RTO_LOSS_SMAPE == rto::kLossSmape && RTO_LOSS_MSE == rto::kLossMse, "the header's loss kinds are the kernels'");
    const hipError_t e = rto::launch_loss(pred, truth, n, H, W, kind, t->loss_partials.as<double>(), device_loss, grad_pred, (hipStream_t)stream);
    if (e != hipSuccess) return set_err(RTO_E_HIP, std::string("loss launch failed: ") + hipGetErrorString(e));
    return RTO_OK;
}

int rto_image_write_png(const char* path, const uint8_t* rgba, int width, int height) {
    if (!path || !rgba || width < 1 || height < 1) return set_err(RTO_E_INVALID, "rto_image_write_png: a null argument or an empty image");
    if (!rto::write_png_rgba8(path, rgba, width, height)) return set_err(RTO_E_IO, std::string("cannot write ") + path);
    return RTO_OK;
}

}  // extern "C"
