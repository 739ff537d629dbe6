// The host-decided refusals of the C ABI, called from a program of its own whose host code -- the units behind the ABI and
// rto_abi_common.h -- is built with AddressSanitizer + UBSan (tools/sanitize/run_abi.sh).  Needs no device: every call here is
// refused before the device is used, or because there is none.  Each call must return its code and leave a message.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rto.h"

static int g_calls = 0, g_bad = 0;
static void expect(const char* what, int rc, int code, const char* part) {
    ++g_calls;
    const char* msg = rto_last_error();
    if (rc != code || !msg || !std::strstr(msg, part)) {
        ++g_bad;
        std::printf("FAIL %s: %d '%s' (expected %d, '...%s...')\n", what, rc, msg ? msg : "(null)", code, part);
    }
}

int main() {
    float* const P = reinterpret_cast<float*>(0x1000);  // non-null; no refused call reads through it
    const bool no_device = rto_device_count() <= 0;

    // check_frames and check_shape, through the size query
    rto_guidance_train_layer tl[4];
    for (auto& l : tl) l = rto_guidance_train_layer{P, P, P, P, 8, 8};
    size_t bytes = 0;
    expect("acts n 0", rto_guidance_train_acts_bytes(tl, 2, 4, 0, 8, 8, &bytes), RTO_E_INVALID, "at least 1, not 0, 8, 8");
    expect("acts 2^31", rto_guidance_train_acts_bytes(tl, 2, 4, 2, 32768, 32768, &bytes), RTO_E_INVALID, "2 x 32768 x 32768 pixels exceed");
    expect("acts layers", rto_guidance_train_acts_bytes(tl, 4, 4, 1, 8, 8, &bytes), RTO_E_INVALID, "num_layers must be 2 or 3, not 4");
    expect("acts levels", rto_guidance_train_acts_bytes(tl, 2, 3, 1, 8, 8, &bytes), RTO_E_INVALID, "not 2 * levels = 6");
    expect("acts null", rto_guidance_train_acts_bytes(nullptr, 2, 4, 1, 8, 8, &bytes), RTO_E_INVALID, "null argument");
    tl[0].cout = tl[1].cin = 65;
    expect("acts c1", rto_guidance_train_acts_bytes(tl, 2, 4, 1, 8, 8, &bytes), RTO_E_UNSUPPORTED, "c1 65");
    expect("loss null", rto_loss_forward_backward(nullptr, nullptr, P, P, 1, 8, 8, 0, nullptr, P), RTO_E_INVALID, "null argument");

    // rto_guidance_net_create_layers: the host validation reads the weights
    std::vector<float> w0(8 * 8 * 9, 0.125f), w1(8 * 8 * 9, 0.125f), b(8, 0.f);
    rto_guidance_layer gl[2] = {{w0.data(), b.data(), 8, 8}, {w1.data(), b.data(), 8, 8}};
    rto_guidance_net* net = nullptr;
    expect("net levels", rto_guidance_net_create_layers(gl, 2, 3, 0, &net), RTO_E_INVALID, "kernel_levels = 3");
    w1.back() = NAN;
    expect("net nan", rto_guidance_net_create_layers(gl, 2, 4, 0, &net), RTO_E_INVALID, "layer 1 has a non-finite weight");
    w1.back() = 0.125f;
    rto_metrics* m = nullptr;
    rto_guidance_train* t = nullptr;
    rto_ctx* ctx = nullptr;
    if (no_device) {  // check_device_index
        expect("net create", rto_guidance_net_create_layers(gl, 2, 4, 0, &net), RTO_E_HIP, "no HIP device available");
        expect("metrics create", rto_metrics_create(0, &m), RTO_E_HIP, "no HIP device available");
        expect("train create", rto_guidance_train_create(0, &t), RTO_E_HIP, "no HIP device available");
        expect("ctx create", rto_ctx_create_batch(8, 8, 1, 0, &ctx), RTO_E_HIP, "(librto has no CPU fallback)");
    }

    // the plain filter entries
    expect("batch null", rto_filtering_batch(nullptr, nullptr, P, 4, 8, 8, 1, P, P + 4), RTO_E_INVALID, "rto_filtering: null pointer or bad size");
    expect("batch L", rto_filtering_batch(nullptr, P, P, 7, 8, 8, 1, P, P + 4), RTO_E_INVALID, "Kernel size == 15 not supported.");
    expect("batch alias", rto_filtering_batch(nullptr, P, P, 4, 8, 8, 1, P, P), RTO_E_INVALID, "rto_filtering: img_in and img_out must differ");
    expect("mode", rto_filtering_batch_mode(nullptr, nullptr, P, 4, 8, 8, 1, P, P + 4, 7), RTO_E_INVALID, "rto_filtering_batch_mode: unknown mode");
    expect("mode fast H", rto_filtering_batch_mode(nullptr, P, P, 4, 0, 8, 1, P, P + 4, RTO_FILTER_FACTORISED), RTO_E_INVALID, "rto_filtering: null pointer");
    expect("train null", rto_filtering_train_forward(nullptr, P, P, 4, 8, 8, 1, P, P + 4, P, P, nullptr), RTO_E_INVALID, "rto_filtering_train_forward: null pointer");
    expect("train alias", rto_filtering_train_forward(nullptr, P, P, 4, 8, 8, 1, P, P, P, P, P), RTO_E_INVALID, "rto_filtering_train_forward: img_in and img_out");
    expect("backward n", rto_filtering_backward(nullptr, P, P, P, P, P, P, P, 4, 8, 8, 0, P, P), RTO_E_INVALID, "rto_filtering_backward: null pointer or bad size");
    expect("backward L", rto_filtering_backward(nullptr, P, P, P, P, P, P, P, 0, 8, 8, 1, P, P), RTO_E_INVALID, "Kernel size == 1 not supported.");

    // null handles of the folded entries: the message names the entry that was called
    expect("forward_ex", rto_guidance_net_forward_ex(nullptr, nullptr, P, 1, 8, 8, P, P, 0), RTO_E_INVALID, "rto_guidance_net_forward: bad argument");
    expect("forward_culled", rto_guidance_net_forward_culled(nullptr, nullptr, P, 1, 8, 8, P, P, 0, reinterpret_cast<uint32_t*>(P), 2, 0.f),
           RTO_E_INVALID, "rto_guidance_net_forward_culled: bad argument");
    expect("packed", rto_filtering_packed(nullptr, nullptr, P, P + 4, 1, 8, 8), RTO_E_INVALID, "rto_filtering_packed: bad argument");
    expect("packed_culled", rto_filtering_packed_culled(nullptr, nullptr, P, P + 4, 1, 8, 8, reinterpret_cast<uint32_t*>(P), 2, 0.f), RTO_E_INVALID,
           "rto_filtering_packed_culled: bad argument");
    expect("metrics null", rto_metrics_compute(nullptr, nullptr, P, 0, P, 0, 1, 8, 8, 0, 0.f, nullptr), RTO_E_INVALID, "rto_metrics_compute: null argument");
    int fs = 0;
    expect("strips", rto_denoise_launch_strips(1, 8, 8, &fs, nullptr), RTO_E_INVALID, "rto_denoise_launch_strips: bad argument");
    rto_guidance_net_free(nullptr);
    rto_metrics_free(nullptr);
    rto_guidance_train_free(nullptr);

    std::printf("abi refusals: %d calls, %d wrong%s\n", g_calls, g_bad, no_device ? " (no device)" : "");
    return g_bad ? 1 : 0;
}
