// rto_guidance_abi.cpp -- C ABI of the fused GuidanceNet forward (include/rto.h, guidance_kernels.hip).  Errors, the device
// scope and the two scratch buffers (packed maps, map planes) come from rto_abi_common.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "rto.h"
#include "rto_abi_common.h"
#include "rto_launch.h"
#include "rto_denoise_launch.h"

struct rto_guidance_net {
    int device = 0, c1 = 0, levels = 0, num_layers = 2;
    void* w1 = nullptr;   // fp16 [c1][96]
    void* w2 = nullptr;   // fp16 [16][9*c1]
    float* b2 = nullptr;  // [16]
    // every shape but c1 = 32, levels = 4, two layers is a "general" net (guidance_general.inc): c1 padded to c1p in {16, 32, 64},
    // w1 fp16 [c1p][96], w2 fp16 [16][KS*32] and b2 [16] = the LAST layer, wm fp16 [c1p][KS*32] and bm [c1p] = the middle layer of
    // three; fp32 planes only -- no packed maps, no sparse frames
    bool general = false;
    int c1p = 0;
    void* wm = nullptr;
    float* bm = nullptr;
    DeviceBuf packed;            // scratch of the packed route: fp16 [n][H][W][8]
    int packed_n = 0, packed_h = 0, packed_w = 0;  // what the scratch currently holds
    // rto_filtering_packed_culled: the filter's output tile over pure background of brightness fill_bg (see ensure_fill_tile)
    std::mutex fill_mu;
    float* fill_tile = nullptr;  // device [32][32][4] (factorised filter) then [8][32][4] (exact filter)
    float fill_planes[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // the background maps as fp32 planes hold them: `levels` softmax weights, `levels` guidance values
    bool packed_sparse = false;  // the packed maps hold nothing for the tiles the network skipped (RTO_NET_INPUT_SPARSE)
    uint32_t fill_k[4] = {0, 0, 0, 0};  // ... and the network's 8 fp16 outputs for a pixel whose neighbourhood is background
    float fill_bg = 0.f;
    bool fill_valid = false;
    DeviceBuf planes;  // rto_denoise(EXACT): weight + guidance planes, 2 x [n][levels][H][W] floats
};

extern "C" {

int rto_guidance_net_create_layers(const rto_guidance_layer* layers, int num_layers, int levels, int device, rto_guidance_net** out) {
    // ---- validation, before any device use
    if (!layers || !out || num_layers < 1) return set_err(RTO_E_INVALID, "rto_guidance_net_create_layers: null argument");
    for (int i = 0; i < num_layers; ++i)
        if (!layers[i].weight || !layers[i].bias || layers[i].cin < 1 || layers[i].cout < 1)
            return set_err(RTO_E_INVALID, "rto_guidance_net_create_layers: layer " + std::to_string(i) + " has a null pointer or no channels");
    if (layers[0].cin != 8) return set_err(RTO_E_INVALID, "rto_guidance_net_create_layers: the first layer reads the 8 aux channels, not " + std::to_string(layers[0].cin));
    for (int i = 1; i < num_layers; ++i)
        if (layers[i].cin != layers[i - 1].cout)
            return set_err(RTO_E_INVALID, "rto_guidance_net_create_layers: layer " + std::to_string(i) + " reads " + std::to_string(layers[i].cin) +
                                           " channels, the layer before it writes " + std::to_string(layers[i - 1].cout));
    if (levels < 1 || layers[num_layers - 1].cout != 2 * levels)
        return set_err(RTO_E_INVALID, "rto_guidance_net_create_layers: the last layer writes " + std::to_string(layers[num_layers - 1].cout) +
                                       " channels, kernel_levels = " + std::to_string(levels) + " needs twice that number");
    const int c1 = layers[0].cout;
    const std::string shape = "8 -> " + std::to_string(c1) + " x " + std::to_string(num_layers - 1) + " -> 2 x " + std::to_string(levels);
    if (num_layers < 2 || num_layers > 3) return set_err(RTO_E_UNSUPPORTED, "fused GuidanceNet: two or three layers, not " + std::to_string(num_layers));
    if (c1 > 64) return set_err(RTO_E_UNSUPPORTED, "fused GuidanceNet: mid_channels 1..64 (" + shape + ")");
    if (num_layers == 3 && layers[1].cout != c1) return set_err(RTO_E_UNSUPPORTED, "fused GuidanceNet: the middle layer keeps mid_channels (" + shape + ")");
    if (levels > 6) return set_err(RTO_E_UNSUPPORTED, "fused GuidanceNet: kernel_levels 1..6 (" + shape + ")");
    for (int i = 0; i < num_layers; ++i) {
        const size_t nw = (size_t)layers[i].cout * layers[i].cin * 9;
        for (size_t k = 0; k < nw; ++k)
            if (!std::isfinite(layers[i].weight[k])) return set_err(RTO_E_INVALID, "rto_guidance_net_create_layers: layer " + std::to_string(i) + " has a non-finite weight");
        for (int k = 0; k < layers[i].cout; ++k)
            if (!std::isfinite(layers[i].bias[k])) return set_err(RTO_E_INVALID, "rto_guidance_net_create_layers: layer " + std::to_string(i) + " has a non-finite bias");
    }
    if (const int rc = check_device_index(device, "no HIP device available")) return rc;

    const bool general = !(c1 == 32 && levels == 4 && num_layers == 2);
    const int cout = 2 * levels;
    const int c1p = !general ? c1 : c1 <= 16 ? 16 : c1 <= 32 ? 32 : 64;  // zero channels: relu6(0) = +0 adds exact zeros downstream
    // rows of a c1p-input layer: k = tap*c1p + ci, tap = ky*3 + kx; the reference shape keeps its 9*c1, a general net has
    // KS k-steps of 32 (c1p = 16: 5, the tenth half-step -- "tap 9" -- zero)
    const size_t row = !general ? (size_t)9 * c1 : (size_t)(c1p == 16 ? 5 : 9 * c1p / 32) * 32;
    const rto_guidance_layer &first = layers[0], &last = layers[num_layers - 1];
    // layer 1: rows padded to 96 (12 taps).  The reference runs the module after `.half()` (network.py:194-201): its biases are
    // fp16 values too.  Layer 1's occupies the first padding slot of its weight row (k = 72; the kernel multiplies it by a constant 1).
    std::vector<_Float16> p1((size_t)c1p * 96, (_Float16)0.f), p2((size_t)16 * row, (_Float16)0.f), pm;
    for (int co = 0; co < c1; ++co) {
        for (int ci = 0; ci < 8; ++ci)
            for (int t = 0; t < 9; ++t) p1[(size_t)co * 96 + t * 8 + ci] = (_Float16)first.weight[((size_t)co * 8 + ci) * 9 + t];
        p1[(size_t)co * 96 + 72] = (_Float16)first.bias[co];
    }
    auto pack_rows = [&](std::vector<_Float16>& dst, const rto_guidance_layer& l) {  // (l.cin == c1)
        for (int co = 0; co < l.cout; ++co)
            for (int ci = 0; ci < c1; ++ci)
                for (int t = 0; t < 9; ++t) dst[(size_t)co * row + (size_t)t * c1p + ci] = (_Float16)l.weight[((size_t)co * c1 + ci) * 9 + t];
    };
    pack_rows(p2, last);
    std::vector<float> pb2(16, 0.f), pbm;
    for (int co = 0; co < cout; ++co) pb2[co] = (float)(_Float16)last.bias[co];
    if (num_layers == 3) {
        pm.assign((size_t)c1p * row, (_Float16)0.f);
        pack_rows(pm, layers[1]);
        pbm.assign((size_t)c1p, 0.f);
        for (int co = 0; co < c1; ++co) pbm[co] = (float)(_Float16)layers[1].bias[co];
    }

    DeviceGuard guard(device);
    auto n = new rto_guidance_net();
    n->device = device;
    n->c1 = c1;
    n->levels = levels;
    n->num_layers = num_layers;
    n->general = general;
    n->c1p = c1p;
    bool ok = hipMalloc(&n->w1, p1.size() * 2) == hipSuccess && hipMalloc(&n->w2, p2.size() * 2) == hipSuccess &&
              hipMalloc((void**)&n->b2, 16 * sizeof(float)) == hipSuccess;
    ok = ok && hipMemcpy(n->w1, p1.data(), p1.size() * 2, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(n->w2, p2.data(), p2.size() * 2, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(n->b2, pb2.data(), 16 * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    if (ok && num_layers == 3)
        ok = hipMalloc(&n->wm, pm.size() * 2) == hipSuccess && hipMalloc((void**)&n->bm, pbm.size() * sizeof(float)) == hipSuccess &&
             hipMemcpy(n->wm, pm.data(), pm.size() * 2, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(n->bm, pbm.data(), pbm.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        rto_guidance_net_free(n);
        return set_err(RTO_E_HIP, "uploading the GuidanceNet weights failed");
    }
    *out = n;
    return RTO_OK;
}

int rto_guidance_net_create(const float* w1, const float* b1, const float* w2, const float* b2, int c1, int levels,
                            int device, rto_guidance_net** out) {
    if (!w1 || !b1 || !w2 || !b2 || !out) return set_err(RTO_E_INVALID, "rto_guidance_net_create: null argument");
    if (c1 < 1 || c1 > 64 || levels < 1 || levels > 6)
        return set_err(RTO_E_UNSUPPORTED, "fused GuidanceNet supports mid_channels 1..64, kernel_levels 1..6");
    const rto_guidance_layer layers[2] = {{w1, b1, 8, c1}, {w2, b2, c1, 2 * levels}};
    return rto_guidance_net_create_layers(layers, 2, levels, device, out);
}

int rto_guidance_net_get_info(const rto_guidance_net* net, rto_guidance_net_info* info) {
    if (!net || !info) return set_err(RTO_E_INVALID, "rto_guidance_net_get_info: null argument");
    info->c1 = net->c1;
    info->levels = net->levels;
    info->num_layers = net->num_layers;
    info->halo = net->num_layers;
    info->packed_route = net->general ? 0 : 1;
    return RTO_OK;
}

// the network on fp32 planes, by the kernel of its shape.  fill_planes != nullptr (with marks): tile skipping
static hipError_t launch_planes(const rto_guidance_net* net, const float* aux, int n, int H, int W, float* weight_map, float* guidance_map,
                                int in_mode, const uint32_t* marks, int words, const float* fill_planes, hipStream_t stream) {
    if (net->general)
        return rto::launch_guidance_general(aux, net->w1, net->wm, net->w2, net->bm, net->b2, net->c1p, net->num_layers, net->levels, n, H, W,
                                            weight_map, guidance_map, in_mode, marks, words, fill_planes, stream);
    return rto::launch_guidance_net(aux, net->w1, net->w2, net->b2, net->c1, net->levels, n, H, W, weight_map, guidance_map, in_mode, marks,
                                    words, nullptr, fill_planes, 0, 0.f, stream);
}

// the packed fp16 maps and sparse frames exist for the reference shape only (filter_fast<4, true>)
static int refuse_general(const char* who, const rto_guidance_net* net) {
    if (!net->general) return RTO_OK;
    return set_err(RTO_E_UNSUPPORTED, std::string(who) + ": the packed / sparse route serves mid_channels = 32, kernel_levels = 4, two layers only; this net is 8 -> " +
                                       std::to_string(net->c1) + (net->num_layers == 3 ? " -> " + std::to_string(net->c1) : std::string()) + " -> 2 x " +
                                       std::to_string(net->levels) + " (" + std::to_string(net->num_layers) + " layers): use the fp32 planes (rto_guidance_net_forward*, rto_filtering_culled, rto_denoise)");
}

// flags of the forward calls -> launch_guidance_net's in_mode
static int net_in_mode(int flags) { return (flags & RTO_NET_INPUT_RGBA) ? 2 : (flags & RTO_NET_AUX_SQUARES_IMPLIED) ? 1 : 0; }

int rto_guidance_net_forward(const rto_guidance_net* net, void* stream, const float* aux, int n, int H, int W,
                             float* weight_map, float* guidance_map) {
    return rto_guidance_net_forward_ex(net, stream, aux, n, H, W, weight_map, guidance_map, 0);
}

int rto_guidance_net_forward_ex(const rto_guidance_net* net, void* stream, const float* aux, int n, int H, int W,
                                float* weight_map, float* guidance_map, int flags) {
    // (without marks the culled body touches nothing of the handle)
    return rto_guidance_net_forward_culled(const_cast<rto_guidance_net*>(net), stream, aux, n, H, W, weight_map, guidance_map, flags, nullptr, 0, 0.f);
}

// grows the scratch of the packed route to n x H x W pixels; maps of a buffer that was replaced are gone
static int reserve_packed(rto_guidance_net* net, int n, int H, int W) {
    bool regrown = false;
    const int rc = net->packed.reserve((size_t)n * H * W * 16, "packed maps", &regrown);
    if (regrown) net->packed_n = 0;
    return rc;
}

int rto_guidance_net_reserve(rto_guidance_net* net, int n, int H, int W) {
    if (!net || n < 1 || H < 1 || W < 1) return set_err(RTO_E_INVALID, "rto_guidance_net_reserve: bad argument");
    if (const int rc = refuse_general("rto_guidance_net_reserve", net)) return rc;
    DeviceGuard guard(net->device);
    return reserve_packed(net, n, H, W);
}

static int ensure_fill_tile(rto_guidance_net* net, float bg, hipStream_t stream);
static int check_marks(const char* who, const rto_guidance_net* net, const uint32_t* tile_marks, int words_per_frame, int H, int W) {
    const int tiles = ((W + 7) / 8) * ((H + 7) / 8);
    if (words_per_frame != (tiles + 31) / 32 + 1)
        return set_err(RTO_E_INVALID, std::string(who) + ": the tile marks are not those of a " + std::to_string(H) + " x " + std::to_string(W) +
                                       " frame (rto_ctx_tile_marks)");
    if (pointer_device(tile_marks) != net->device)
        return set_err(RTO_E_INVALID, std::string(who) + ": the tile marks are not memory of the network's device");
    return RTO_OK;
}

int rto_guidance_net_forward_packed_culled(rto_guidance_net* net, void* stream, const float* aux, int n, int H, int W, int flags,
                                           const uint32_t* tile_marks, int words_per_frame, float background) {
    if (!net || !aux || n < 1 || H < 1 || W < 1) return set_err(RTO_E_INVALID, "rto_guidance_net_forward_packed: bad argument");
    if (const int rc = refuse_general("rto_guidance_net_forward_packed", net)) return rc;
    if (pointer_device(aux) != net->device)
        return set_err(RTO_E_INVALID, "rto_guidance_net_forward_packed: aux is not memory of the network's device");
    DeviceGuard guard(net->device);
    if (const int rc = reserve_packed(net, n, H, W)) return rc;
    if (tile_marks) {
        if (const int rc = check_marks("rto_guidance_net_forward_packed_culled", net, tile_marks, words_per_frame, H, W)) return rc;
        if (const int rc = ensure_fill_tile(net, background, (hipStream_t)stream)) return rc;
    }
    const bool sparse = (flags & RTO_NET_INPUT_SPARSE) != 0;
    if (sparse && (!tile_marks || !(flags & RTO_NET_INPUT_RGBA)))
        return set_err(RTO_E_INVALID, "rto_guidance_net_forward_packed_culled: RTO_NET_INPUT_SPARSE needs the tile marks of the launch and RTO_NET_INPUT_RGBA");
    const hipError_t e = rto::launch_guidance_net(aux, net->w1, net->w2, net->b2, net->c1, net->levels, n, H, W,
                                                  (float*)net->packed.p, nullptr, net_in_mode(flags),
                                                  tile_marks, words_per_frame, tile_marks ? net->fill_k : nullptr, nullptr, sparse ? 1 : 0, background,
                                                  (hipStream_t)stream);
    if (e != hipSuccess) return set_err(RTO_E_HIP, std::string("GuidanceNet launch failed: ") + hipGetErrorString(e));
    net->packed_sparse = sparse;
    net->packed_n = n;
    net->packed_h = H;
    net->packed_w = W;
    return RTO_OK;
}

int rto_guidance_net_forward_packed(rto_guidance_net* net, void* stream, const float* aux, int n, int H, int W, int flags) {
    return rto_guidance_net_forward_packed_culled(net, stream, aux, n, H, W, flags, nullptr, 0, 0.f);
}

int rto_filtering_packed(const rto_guidance_net* net, void* stream, const float* img_in, float* img_out, int n, int H, int W) {
    // (without marks the culled body touches nothing of the handle)
    return rto_filtering_packed_culled(const_cast<rto_guidance_net*>(net), stream, img_in, img_out, n, H, W, nullptr, 0, 0.f);
}

// The output tile of a filter workgroup that sees nothing but background: run the two real kernels once on a synthetic
// 96 x 96 background frame (aux = what write_pixel stores for a ray that meets nothing: colour = bg, alpha = 0) and keep
// the tile of the centre workgroup, whose staged region + the network's receptive field lie inside the frame.  Any other
// such workgroup executes the same instructions on the same values, thread for thread.
static int ensure_fill_tile(rto_guidance_net* net, float bg, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(net->fill_mu);
    if (net->fill_valid && std::memcmp(&net->fill_bg, &bg, sizeof(float)) == 0) return RTO_OK;
    constexpr int S = 3 * rto::kFilterFillSide, T = rto::kFilterFillSide;
    const size_t px = (size_t)S * S;
    std::vector<float> aux(8 * px, 0.f), img(4 * px);
    for (size_t i = 0; i < px; ++i) {
        for (int c = 0; c < 3; ++c) {
            aux[c * px + i] = bg;
            aux[(4 + c) * px + i] = bg * bg;
            img[4 * i + c] = bg;
        }
        img[4 * i + 3] = 1.f;
    }
    float *d_aux = nullptr, *d_img = nullptr, *d_out = nullptr, *d_w = nullptr, *d_g = nullptr;
    void* d_maps = nullptr;
    auto cleanup = [&] {
        for (void* p : {(void*)d_aux, (void*)d_img, (void*)d_out, d_maps, (void*)d_w, (void*)d_g})
            if (p) (void)hipFree(p);
    };
    hipError_t e = hipSuccess;
    auto ok = [&](hipError_t r) { return (e = r) == hipSuccess; };
    constexpr int TE = rto::kFilterExactFillH, YE = (S / 2 / TE) * TE;  // the exact filter's tile: 32 x 8; its row in the frame
    if (!net->fill_tile && !ok(hipMalloc((void**)&net->fill_tile, (size_t)(T + TE) * T * 4 * sizeof(float))))
        return set_err(RTO_E_HIP, std::string("fill tile: ") + hipGetErrorString(e));
    const int L = net->levels;
    bool good = ok(hipMalloc((void**)&d_aux, aux.size() * sizeof(float))) && ok(hipMalloc((void**)&d_img, img.size() * sizeof(float))) &&
                ok(hipMalloc((void**)&d_out, img.size() * sizeof(float))) && ok(hipMalloc((void**)&d_w, L * px * sizeof(float))) &&
                ok(hipMalloc((void**)&d_g, L * px * sizeof(float))) &&
                ok(hipMemcpyAsync(d_aux, aux.data(), aux.size() * sizeof(float), hipMemcpyHostToDevice, stream)) &&
                ok(hipMemcpyAsync(d_img, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    if (good && !net->general)  // the factorised filter's tile and the packed background maps, by the packed route
        good = ok(hipMalloc(&d_maps, px * 8 * sizeof(uint16_t))) &&
               ok(rto::launch_guidance_net(d_aux, net->w1, net->w2, net->b2, net->c1, net->levels, 1, S, S, (float*)d_maps, nullptr, false, nullptr, 0, nullptr, nullptr, 0, 0.f, stream)) &&
               ok(rto::launch_filter_fast_packed(d_maps, S, S, 1, d_img, d_out, nullptr, 0, nullptr, 0, 0.f, nullptr, stream)) &&
               ok(hipMemcpy2DAsync(net->fill_tile, (size_t)T * 4 * sizeof(float), d_out + ((size_t)T * S + T) * 4, (size_t)S * 4 * sizeof(float),
                                   (size_t)T * 4 * sizeof(float), T, hipMemcpyDeviceToDevice, stream)) &&
               ok(hipMemcpyAsync(net->fill_k, (const char*)d_maps + ((size_t)(S / 2) * S + S / 2) * 16, 16, hipMemcpyDeviceToHost, stream));
    // the same through fp32 planes and the exact filter (rto_guidance_net_forward_culled / rto_filtering_culled), by the net's own
    // kernel and levels; a general net has no packed route: its factorised tile comes from the planes too
    good = good && ok(launch_planes(net, d_aux, 1, S, S, d_w, d_g, 0, nullptr, 0, nullptr, stream));
    if (good && net->general)
        good = ok(rto::launch_filter_fast(d_w, d_g, L, S, S, 1, d_img, d_out, stream)) &&
               ok(hipMemcpy2DAsync(net->fill_tile, (size_t)T * 4 * sizeof(float), d_out + ((size_t)T * S + T) * 4, (size_t)S * 4 * sizeof(float),
                                   (size_t)T * 4 * sizeof(float), T, hipMemcpyDeviceToDevice, stream));
    if (!good ||
        !ok(rto::launch_filter(d_w, d_g, L, S, S, 1, d_img, d_out, stream)) ||
        !ok(hipMemcpy2DAsync(net->fill_tile + (size_t)T * T * 4, (size_t)T * 4 * sizeof(float), d_out + ((size_t)YE * S + T) * 4,
                             (size_t)S * 4 * sizeof(float), (size_t)T * 4 * sizeof(float), TE, hipMemcpyDeviceToDevice, stream)) ||
        !ok(hipMemcpy2DAsync(net->fill_planes, sizeof(float), d_w + (size_t)(S / 2) * S + S / 2, px * sizeof(float), sizeof(float), L,
                             hipMemcpyDeviceToHost, stream)) ||
        !ok(hipMemcpy2DAsync(net->fill_planes + L, sizeof(float), d_g + (size_t)(S / 2) * S + S / 2, px * sizeof(float), sizeof(float), L,
                             hipMemcpyDeviceToHost, stream)) ||
        !ok(hipStreamSynchronize(stream))) {
        cleanup();
        net->fill_valid = false;
        return set_err(RTO_E_HIP, std::string("fill tile: ") + hipGetErrorString(e));
    }
    cleanup();
    net->fill_bg = bg;
    net->fill_valid = true;
    return RTO_OK;
}

int rto_filtering_packed_culled(rto_guidance_net* net, void* stream, const float* img_in, float* img_out, int n, int H, int W,
                                const uint32_t* tile_marks, int words_per_frame, float background) {
    // without marks this is rto_filtering_packed, which names itself in its messages
    const std::string who = tile_marks ? "rto_filtering_packed_culled" : "rto_filtering_packed";
    if (!net || !img_in || !img_out || img_in == img_out) return set_err(RTO_E_INVALID, who + ": bad argument");
    if (const int rc = refuse_general(who.c_str(), net)) return rc;
    if (!net->packed.p || net->packed_n < 1) return set_err(RTO_E_INVALID, who + ": no packed maps (call rto_guidance_net_forward_packed first)");
    // the images are the caller's: their extent must be the one the maps were computed for, or the kernel would read and
    // write past a smaller buffer
    if (n != net->packed_n || H != net->packed_h || W != net->packed_w)
        return set_err(RTO_E_INVALID, who + ": " + std::to_string(n) + " x " + std::to_string(H) + " x " + std::to_string(W) +
                                          " images, but the packed maps hold " + std::to_string(net->packed_n) + " x " +
                                          std::to_string(net->packed_h) + " x " + std::to_string(net->packed_w));
    if (tile_marks)
        if (const int rc = check_marks(who.c_str(), net, tile_marks, words_per_frame, H, W)) return rc;
    if (pointer_device(img_out) != net->device || pointer_device(img_in) != net->device)
        return set_err(RTO_E_INVALID, who + ": the images are not memory of the network's device");
    if (!tile_marks && net->packed_sparse)
        return set_err(RTO_E_INVALID, who + ": the packed maps are sparse (RTO_NET_INPUT_SPARSE): the filter needs the same tile marks "
                                            "(rto_filtering_packed_culled)");
    DeviceGuard guard(net->device);
    if (tile_marks)
        if (const int rc = ensure_fill_tile(net, background, (hipStream_t)stream)) return rc;
    // (without marks: no fill tile, no background; the maps are not sparse)
    const hipError_t e = rto::launch_filter_fast_packed(net->packed.p, net->packed_h, net->packed_w, net->packed_n, img_in, img_out, tile_marks,
                                                        tile_marks ? words_per_frame : 0, tile_marks ? net->fill_tile : nullptr,
                                                        net->packed_sparse ? 1 : 0, tile_marks ? background : 0.f,
                                                        tile_marks ? net->fill_k : nullptr, (hipStream_t)stream);
    if (e != hipSuccess) return set_err(RTO_E_HIP, std::string("filter launch failed: ") + hipGetErrorString(e));
    return RTO_OK;
}

int rto_guidance_net_forward_culled(rto_guidance_net* net, void* stream, const float* aux, int n, int H, int W, float* weight_map,
                                    float* guidance_map, int flags, const uint32_t* tile_marks, int words_per_frame, float background) {
    // without marks this is rto_guidance_net_forward_ex, which names itself in its messages
    const bool culled = tile_marks != nullptr;
    if (!net || !aux || !weight_map || !guidance_map || n < 1 || H < 1 || W < 1)
        return set_err(RTO_E_INVALID, culled ? "rto_guidance_net_forward_culled: bad argument" : "rto_guidance_net_forward: bad argument");
    if ((flags & RTO_NET_INPUT_SPARSE) && net->general)
        if (const int rc = refuse_general(culled ? "rto_guidance_net_forward_culled(RTO_NET_INPUT_SPARSE)" : "rto_guidance_net_forward_ex(RTO_NET_INPUT_SPARSE)", net))
            return rc;
    if (culled)
        if (const int rc = check_marks("rto_guidance_net_forward_culled", net, tile_marks, words_per_frame, H, W)) return rc;
    DeviceGuard guard(net->device);
    if (culled)
        if (const int rc = ensure_fill_tile(net, background, (hipStream_t)stream)) return rc;
    const hipError_t e = launch_planes(net, aux, n, H, W, weight_map, guidance_map, net_in_mode(flags), tile_marks, culled ? words_per_frame : 0,
                                       culled ? net->fill_planes : nullptr, (hipStream_t)stream);
    if (e != hipSuccess) return set_err(RTO_E_HIP, std::string("GuidanceNet launch failed: ") + hipGetErrorString(e));
    return RTO_OK;
}

int rto_filtering_culled(rto_guidance_net* net, void* stream, const float* weight_map, const float* guidance_map, int H, int W, int n,
                         const float* img_in, float* img_out, int mode, const uint32_t* tile_marks, int words_per_frame, float background) {
    if (!net) return set_err(RTO_E_INVALID, "rto_filtering_culled: null network handle");
    if (!tile_marks) return rto_filtering_batch_mode(stream, weight_map, guidance_map, net->levels, H, W, n, img_in, img_out, mode);
    if (!weight_map || !guidance_map || !img_in || !img_out || img_in == img_out || H < 1 || W < 1 || n < 1)
        return set_err(RTO_E_INVALID, "rto_filtering_culled: bad argument");
    if (mode != RTO_FILTER_EXACT && mode != RTO_FILTER_FACTORISED) return set_err(RTO_E_INVALID, "rto_filtering_culled: unknown mode");
    if (const int rc = check_marks("rto_filtering_culled", net, tile_marks, words_per_frame, H, W)) return rc;
    // The filter kernels skip a tile whose staged region grown by TWO pixels (the receptive field of two 3x3 layers) is background.
    // A map value of a three-layer net depends on the aux pixels three away: those nets run the plain kernels here (only their
    // network is culled) -- the same bits either way, since the skipped tiles are copies of what the plain kernels compute.
    if (net->num_layers > 2) return rto_filtering_batch_mode(stream, weight_map, guidance_map, net->levels, H, W, n, img_in, img_out, mode);
    if (pointer_device(img_out) != net->device || pointer_device(img_in) != net->device)
        return set_err(RTO_E_INVALID, "rto_filtering_culled: the images are not memory of the network's device");
    DeviceGuard guard(net->device);
    if (const int rc = ensure_fill_tile(net, background, (hipStream_t)stream)) return rc;
    constexpr size_t kExactTile = (size_t)rto::kFilterFillSide * rto::kFilterFillSide * 4;
    const hipError_t e = mode == RTO_FILTER_EXACT
                             ? rto::launch_filter_culled(weight_map, guidance_map, net->levels, H, W, n, img_in, img_out, tile_marks,
                                                         words_per_frame, net->fill_tile + kExactTile, (hipStream_t)stream)
                             : rto::launch_filter_fast_culled(weight_map, guidance_map, net->levels, H, W, n, img_in, img_out, tile_marks,
                                                              words_per_frame, net->fill_tile, (hipStream_t)stream);
    if (e != hipSuccess) return set_err(RTO_E_HIP, std::string("filter launch failed: ") + hipGetErrorString(e));
    return RTO_OK;
}

int rto_denoise(rto_guidance_net* net, rto_ctx* ctx, int n, int mode, void* stream) {
    if (!net || !ctx || n < 1) return set_err(RTO_E_INVALID, "rto_denoise: bad argument");
    if (mode != RTO_FILTER_EXACT && mode != RTO_FILTER_FACTORISED) return set_err(RTO_E_INVALID, "rto_denoise: unknown mode");
    const int W = rto_ctx_width(ctx), H = rto_ctx_height(ctx), sel = rto_ctx_selected_frame(ctx);
    if (sel + n > rto_ctx_frames(ctx))
        return set_err(RTO_E_INVALID, "rto_denoise: " + std::to_string(n) + " frames from slot " + std::to_string(sel) + " of a context of " +
                                       std::to_string(rto_ctx_frames(ctx)));
    const float* aux = rto_ctx_aux(ctx);
    const float* noisy = rto_ctx_noisy(ctx);
    float* image = rto_ctx_image(ctx);
    // the tile marks of the launch that rendered these frames, if it was a batched one over exactly these slots
    const uint32_t* marks = nullptr;
    int words = 0, first = 0, frames = 0;
    float bg = 0.f;
    if (rto_ctx_tile_marks(ctx, &marks, &words, &first, &frames, &bg) != RTO_OK || first != sel || frames < n) marks = nullptr;
    // frames of a lean batched launch (rto_ctx_set_lean_outputs): their aux planes were not written, the noisy image
    // carries r, g, b, alpha -- the network reads that
    int net_flags = RTO_NET_AUX_SQUARES_IMPLIED;
    const int lean = rto_ctx_frames_lean_level(ctx, sel, n);  // 0 full, 1 lean, 2 sparse; -1: the slots disagree
    if (lean < 0)
        return set_err(RTO_E_INVALID, "rto_denoise: slots " + std::to_string(sel) + ".." + std::to_string(sel + n - 1) +
                                       " mix full, lean and sparse outputs (a later launch rewrote some of them): denoise each run of slots by itself");
    if (lean) {
        aux = noisy;
        net_flags = RTO_NET_INPUT_RGBA;
        if (lean == 2) {  // sparse: nothing was stored for the pixels of culled tiles
            if (!marks)
                return set_err(RTO_E_INVALID, "rto_denoise: sparse lean frames need the tile marks of the launch that rendered them (another launch "
                                           "into this context replaced them)");
            if (mode != RTO_FILTER_FACTORISED)
                return set_err(RTO_E_UNSUPPORTED, "rto_denoise: sparse lean frames (rto_ctx_set_lean_outputs level 2) take the factorised route only");
            net_flags |= RTO_NET_INPUT_SPARSE;
        }
    }
    if (lean == 2)
        if (const int rc = refuse_general("rto_denoise on sparse lean frames (rto_ctx_set_lean_outputs level 2)", net)) return rc;
    if (mode == RTO_FILTER_FACTORISED && !net->general) {
        if (const int rc = rto_guidance_net_forward_packed_culled(net, stream, aux, n, H, W, net_flags, marks, words, bg)) return rc;
        return rto_filtering_packed_culled(net, stream, noisy, image, n, H, W, marks, words, bg);
    }
    // fp32 planes: the exact route, and both routes of a general net (no packed maps for it)
    const size_t plane_floats = (size_t)n * net->levels * H * W;
    {
        DeviceGuard guard(net->device);
        if (const int rc = net->planes.reserve(2 * plane_floats * sizeof(float), "map planes")) return rc;
    }
    float *wm = net->planes.as<float>(), *gm = wm + plane_floats;
    if (const int rc = rto_guidance_net_forward_culled(net, stream, aux, n, H, W, wm, gm, net_flags, marks, words, bg)) return rc;
    return rto_filtering_culled(net, stream, wm, gm, H, W, n, noisy, image, mode, marks, words, bg);
}

int rto_denoise_launch_strips(int n, int H, int W, int* filter_strip, int* net_strip) {
    if (n < 1 || H < 1 || W < 1 || !filter_strip || !net_strip) return set_err(RTO_E_INVALID, "rto_denoise_launch_strips: bad argument");
    *filter_strip = rto::filter_fast_strip(n, H, W);
    *net_strip = rto::guidance_net_strip(n, H, W);
    return RTO_OK;
}

void rto_guidance_net_free(rto_guidance_net* net) {
    if (!net) return;
    DeviceGuard guard(net->device);
    if (net->packed.p || net->planes.p) (void)hipDeviceSynchronize();
    net->packed.release();
    net->planes.release();
    if (net->fill_tile) (void)hipFree(net->fill_tile);
    if (net->w1) (void)hipFree(net->w1);
    if (net->w2) (void)hipFree(net->w2);
    if (net->wm) (void)hipFree(net->wm);
    if (net->bm) (void)hipFree(net->bm);
    if (net->b2) (void)hipFree(net->b2);
    delete net;
}

}  // extern "C"
