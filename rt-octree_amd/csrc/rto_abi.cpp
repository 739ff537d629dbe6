// rto_abi.cpp -- the C ABI declared in include/rto.h: version, errors, options, the rto_ctx_* surface, the filtering entry
// points, downloads and timers.  Trees: rto_tree.cpp; the launch entries: rto_render_abi.cpp.  Owns the error string that
// set_err (rto_abi_common.h) records for every unit of the library.  Host logic only; every computation on frame data
// happens in the gfx950 kernels (the render units mapped in render_kernels.hip, filter_kernels.hip).  There is no CPU fallback.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

#include "host/mini_json.h"
#include "rto_denoise_launch.h"
#include "rto_internal.h"

namespace {
thread_local std::string g_err;
}

int set_err(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

namespace {

void pcg_seed(rto::Pcg32& r, uint64_t initstate, uint64_t initseq) {  // pcg32.h:53-59
    auto next = [&]() { r.state = r.state * rto::kPcgMult + r.inc; };
    r.state = 0U;
    r.inc = (initseq << 1u) | 1u;
    next();
    r.state += initstate;
    next();
}

int options_from_value(const rto::json::Value& j, rto_options* o) {
    rto_options r;
    rto_options_default(&r);
    try {
        // NLOHMANN_DEFINE_TYPE_INTRUSIVE (render_options.hpp:61-77): every listed key is required
        r.step_size = (float)j.at("step_size").as_number();
        r.sigma_thresh = (float)j.at("sigma_thresh").as_number();
        r.stop_thresh = (float)j.at("stop_thresh").as_number();
        r.background_brightness = (float)j.at("background_brightness").as_number();
        r.show_grid = j.at("show_grid").as_bool();
        r.grid_max_depth = (int)j.at("grid_max_depth").as_number();
        r.enable_probe = j.at("enable_probe").as_bool();
        const auto& p = j.at("probe");
        if (p.size() != 3) throw std::runtime_error("json: 'probe' must have 3 elements");
        for (int i = 0; i < 3; ++i) r.probe[i] = (float)p.at(i).as_number();
        r.probe_disp_size = (int)j.at("probe_disp_size").as_number();
        r.denoise = j.at("denoise").as_bool();
        r.spp = (int)j.at("spp").as_number();
    } catch (const std::exception& e) {
        return set_err(RTO_E_FORMAT, std::string("render options: ") + e.what());
    }
    *o = r;
    return RTO_OK;
}

}  // namespace

// RenderOptions -> the fields the kernels read.  rodrigues (volrend.cu:58-73): angle, axis, cos and sin
// depend on the options only, so they are evaluated here once per launch (float arithmetic, libm cosf /
// sinf: the same calls the CPU oracle makes) instead of once per pixel.
rto::OptDev make_opt_dev(const rto_options* o) {
    rto::OptDev od;
    od.step_size = o->step_size;
    od.sigma_thresh = o->sigma_thresh;
    od.background_brightness = o->background_brightness;
    std::memcpy(od.render_bbox, o->render_bbox, sizeof(od.render_bbox));
    od.basis_minmax[0] = o->basis_minmax[0];
    od.basis_minmax[1] = o->basis_minmax[1];
    const float* a = o->rot_dirs;
    const float angle = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);  // _norm common.cuh:16-20
    od.rot_on = !(angle < 1e-6);
    od.rot_k[0] = od.rot_k[1] = od.rot_k[2] = 0.f;
    od.rot_cos = 1.f;
    od.rot_sin = 0.f;
    od.rot_omc = 0.0;
    if (od.rot_on) {
        for (int i = 0; i < 3; ++i) od.rot_k[i] = a[i] / angle;
        od.rot_cos = cosf(angle);
        od.rot_sin = sinf(angle);
        od.rot_omc = 1.0 - od.rot_cos;
    }
    return od;
}

// The four plain filter entries take device pointers only, and differ in one line: the launch.  Their checks, in one order:
// `ptrs` are non-null and the sizes positive (who: the prefix of the entry's own messages), the window is one the reference has
// (filtering.cu:362-366), `in` and `out` differ (both null: the entry has no such pair); then launch() -> hipError_t runs on the
// device that owns dev_ptr, the entry's output (a process that drives several GPUs may have another one current).
template <class Launch>
static int filter_call(const char* who, std::initializer_list<const void*> ptrs, int L, int H, int W, int n, const void* in,
                       const void* out, const void* dev_ptr, const char* launch_name, Launch launch) {
    bool null = false;
    for (const void* p : ptrs) null = null || !p;
    if (null || H <= 0 || W <= 0 || n < 1) return set_err(RTO_E_INVALID, std::string(who) + ": null pointer or bad size");
    if (L < 1 || L > 6) return set_err(RTO_E_INVALID, "Kernel size == " + std::to_string(L * 2 + 1) + " not supported.");
    if (in && in == out) return set_err(RTO_E_INVALID, std::string(who) + ": img_in and img_out must differ");
    const int dev = pointer_device(dev_ptr);
    if (dev < 0) return set_err(RTO_E_INVALID, "filtering: the output pointer is not device memory");
    DeviceGuard guard(dev);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    const hipError_t e = launch();
    if (e != hipSuccess) return set_err(RTO_E_HIP, std::string(launch_name) + " launch failed: " + hipGetErrorString(e));
    return RTO_OK;
}

extern "C" {

const char* rto_version(void) { return "rt-octree_amd 0.1 (gfx950)"; }
const char* rto_last_error(void) { return g_err.c_str(); }

int rto_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return set_err(RTO_E_HIP, "hipGetDeviceCount failed");
    return n;
}

void rto_options_default(rto_options* o) {  // render_options.hpp:15-58
    if (!o) return;
    o->step_size = 1e-4f;
    o->sigma_thresh = 1e-2f;
    o->stop_thresh = 1e-2f;
    o->background_brightness = 1.f;
    const float bb[6] = {0.f, 0.f, 0.f, 1.f, 1.f, 1.f};
    std::memcpy(o->render_bbox, bb, sizeof(bb));
    o->basis_minmax[0] = 0;
    o->basis_minmax[1] = RTO_BASIS_MAX - 1;
    o->rot_dirs[0] = o->rot_dirs[1] = o->rot_dirs[2] = 0.f;
    o->show_grid = 0;
    o->grid_max_depth = 4;
    o->render_depth = 0;
    o->enable_probe = 0;
    o->probe[0] = 0.f;
    o->probe[1] = 0.f;
    o->probe[2] = 1.f;
    o->probe_disp_size = 100;
    o->denoise = 1;
    o->spp = 1;
}

int rto_options_from_json(const char* text, rto_options* o) {
    if (!text || !o) return set_err(RTO_E_INVALID, "rto_options_from_json: null argument");
    rto::json::ValuePtr v;
    try {
        v = rto::json::parse(text);
    } catch (const std::exception& e) {
        return set_err(RTO_E_FORMAT, e.what());
    }
    return options_from_value(*v, o);
}

int rto_options_from_json_file(const char* path, rto_options* o) {
    if (!path || !o) return set_err(RTO_E_INVALID, "rto_options_from_json_file: null argument");
    std::ifstream f(path);
    if (!f) return set_err(RTO_E_IO, std::string("cannot open options file '") + path + "'");
    std::stringstream ss;
    ss << f.rdbuf();
    return rto_options_from_json(ss.str().c_str(), o);
}

int rto_ctx_create(int width, int height, int device, rto_ctx** out) {
    return rto_ctx_create_batch(width, height, 1, device, out);
}


// Queue orders of the 8x8 ray tiles (persistent kernel).
//  * tile_order: rings around the image centre, innermost first, each ring walked by angle -- the
//    frame's long rays (the object) start early, the queue ends on cheap border tiles, consecutive
//    tiles stay neighbours;
//  * wedge_order: the tiles of the 8 XCD ray queues.  Rounds 3-5: the image cut into 8 angular wedges around the centre, blocks of
//    tile_block x tile_block tiles centre-out, Morton order inside a block.  Round 6 (queue_bands > 0, the default): BANDS of
//    queue_bands tile rows, band j -> queue j % 8, centre bands first, a band's tiles centre-out.  Every queue still gets its share
//    of the expensive centre and of the cheap border (the bands interleave), but what its XCD's L2 has to hold is a few horizontal
//    slabs of the tree: a camera that orbits the scene's vertical axis keeps a leaf in its rows from frame to frame, while an
//    angular wedge of the image sees the whole scene turn past it over the batch.
static int build_tile_tables(rto_ctx* c) {
    const int tx8 = (c->width + 7) / 8, ty8 = (c->height + 7) / 8;
    const int B = c->tile_block < 1 ? 1 : c->tile_block;
    struct Keyed { int wedge; double ring, ang; uint32_t morton; uint32_t code; };
    std::vector<Keyed> keyed;
    keyed.reserve((size_t)tx8 * ty8);
    const double cx = 0.5 * (tx8 - 1), cy = 0.5 * (ty8 - 1);
    const double pi = 3.14159265358979323846;
    auto polar = [&](double x, double y, double& ring, double& ang) {
        const double dx = x - cx, dy = y - cy;
        ring = std::floor(std::fmax(std::fabs(dx), std::fabs(dy)) + 0.5);
        ang = std::atan2(dy, dx) + pi;  // [0, 2pi]
    };
    auto spread = [](uint32_t v) {  // interleave helper for up to 8 bits
        uint32_t r = 0;
        for (int i = 0; i < 8; ++i) r |= ((v >> i) & 1u) << (2 * i);
        return r;
    };
    std::vector<std::pair<double, uint32_t>> plain;
    plain.reserve((size_t)tx8 * ty8);
    for (int ty = 0; ty < ty8; ++ty)
        for (int tx = 0; tx < tx8; ++tx) {
            const uint32_t code = ((uint32_t)ty << 16) | (uint32_t)tx;
            double ring, ang;
            polar(tx, ty, ring, ang);
            plain.emplace_back(ring * 16.0 + ang, code);
            // wedge / order key of the block the tile belongs to (block centre, in tile units)
            const int bx = tx / B, by = ty / B;
            double bring, bang;
            polar(bx * B + 0.5 * (B - 1), by * B + 0.5 * (B - 1), bring, bang);
            int wedge = (int)(bang / (2.0 * pi) * rto::kMaxQueues);
            if (wedge >= rto::kMaxQueues) wedge = rto::kMaxQueues - 1;
            if (c->queue_bands > 0) {
                // BANDS (round 6): band j of queue_bands tile rows -> queue j % 8.  A camera that orbits the scene's vertical axis keeps
                // a leaf in its rows from frame to frame, so a queue's rays -- the same tiles of all frames of the batch in turn --
                // stay inside a few horizontal slabs of the tree, which is what that XCD's L2 then has to hold; an angular wedge of
                // the image sees the whole scene turn past it.  Centre bands first, a band's tiles centre-out.
                const int band = ty / c->queue_bands;
                wedge = band % rto::kMaxQueues;
                bring = std::fabs((band + 0.5) * c->queue_bands - 0.5 - cy);
                bang = std::fabs(tx - cx) / (tx8 + 1.0);  // (< 1: orders inside a band; ring * 16 + ang stays monotone in the band)
                keyed.push_back({wedge, bring, bang, (uint32_t)(ty % c->queue_bands), code});
                continue;
            }
            keyed.push_back({wedge, bring, bang, spread((uint32_t)(tx % B)) | (spread((uint32_t)(ty % B)) << 1), code});
        }
    std::stable_sort(plain.begin(), plain.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    std::vector<uint32_t> order(plain.size());
    for (size_t i = 0; i < plain.size(); ++i) order[i] = plain[i].second;
    std::stable_sort(keyed.begin(), keyed.end(), [](const Keyed& a, const Keyed& b) {
        if (a.wedge != b.wedge) return a.wedge < b.wedge;
        const double ka = a.ring * 16.0 + a.ang, kb = b.ring * 16.0 + b.ang;
        if (ka != kb) return ka < kb;
        return a.morton < b.morton;
    });
    std::vector<uint32_t> worder(keyed.size());
    for (int k = 0; k <= rto::kMaxQueues; ++k) c->wedge_start[k] = 0;
    for (size_t i = 0; i < keyed.size(); ++i) {
        worder[i] = keyed[i].code;
        c->wedge_start[keyed[i].wedge + 1] = (int)i + 1;
    }
    for (int k = 1; k <= rto::kMaxQueues; ++k)  // empty wedges (tiny images) inherit the previous end
        if (c->wedge_start[k] < c->wedge_start[k - 1]) c->wedge_start[k] = c->wedge_start[k - 1];
    if (!c->tile_order && hipMalloc((void**)&c->tile_order, order.size() * 4) != hipSuccess)
        return set_err(RTO_E_HIP, "hipMalloc(tile_order) failed");
    if (!c->wedge_order && hipMalloc((void**)&c->wedge_order, worder.size() * 4) != hipSuccess)
        return set_err(RTO_E_HIP, "hipMalloc(tile_order) failed");
    if (hipMemcpy(c->tile_order, order.data(), order.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->wedge_order, worder.data(), worder.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return set_err(RTO_E_HIP, "tile table upload failed");
    return RTO_OK;
}

int rto_ctx_create_batch(int width, int height, int frames, int device, rto_ctx** out) {
    if (width <= 0 || height <= 0 || !out) return set_err(RTO_E_INVALID, "rto_ctx_create: bad size");
    if (frames < 1 || frames > rto::kMaxBatch)
        return set_err(RTO_E_INVALID, "rto_ctx_create_batch: frames must be in 1.." + std::to_string(rto::kMaxBatch));
    if ((int64_t)width * height * 32 > 0x7fffffffLL)
        return set_err(RTO_E_INVALID, "rto_ctx_create: width*height*32 exceeds the int range of idx*SPP (volrend.cu:157)");
    if (const int rc = check_device_index(device, kNoDeviceMsg)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    auto c = new rto_ctx();
    c->device = device;
    c->width = width;
    c->height = height;
    c->frames = frames;
    c->lean_slot.assign((size_t)frames, 0);
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
            c->num_cus = prop.multiProcessorCount;
    }
    const size_t px = (size_t)width * height * frames;
    if (hipMalloc((void**)&c->aux, px * RTO_AUX_CHANNELS * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&c->noisy, px * 4 * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&c->image, px * 4 * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&c->rgba8, px * 4) != hipSuccess ||
        hipMalloc((void**)&c->queue, rto::kQueueWords * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc((void**)&c->d_frames, rto::kMaxBatch * sizeof(rto::FrameDesc)) != hipSuccess ||
        hipMalloc((void**)&c->probe_coeffs, kProbeFloats * sizeof(float)) != hipSuccess ||
        hipMemset(c->queue, 0, rto::kQueueWords * sizeof(unsigned long long)) != hipSuccess) {
        rto_ctx_free(c);
        return set_err(RTO_E_HIP, "hipMalloc(ctx buffers) failed");
    }
    (void)hipMemset(c->aux, 0, px * RTO_AUX_CHANNELS * sizeof(float));
    (void)hipMemset(c->noisy, 0, px * 4 * sizeof(float));
    (void)hipMemset(c->image, 0, px * 4 * sizeof(float));
    {
        int rc = build_tile_tables(c);
        if (rc != RTO_OK) {
            rto_ctx_free(c);
            return rc;
        }
    }
    pcg_seed(c->rng, 20230418ULL, 1);  // render_context.hpp:16
    for (int i = 0; i < 3; ++i) {
        if (hipEventCreate(&c->t_start[i]) != hipSuccess || hipEventCreate(&c->t_stop[i]) != hipSuccess) {
            rto_ctx_free(c);
            return set_err(RTO_E_HIP, "hipEventCreate failed");
        }
    }
    *out = c;
    return RTO_OK;
}

void rto_ctx_free(rto_ctx* c) {
    if (!c) return;
    DeviceGuard guard(c->device);
    for (void* p : {(void*)c->aux, (void*)c->noisy, (void*)c->image, (void*)c->rgba8, (void*)c->jump, (void*)c->queue, (void*)c->tile_mask,
                    (void*)c->qlist, (void*)c->qscratch, (void*)c->d_frames, (void*)c->probe_coeffs, (void*)c->hits, (void*)c->tile_order,
                    (void*)c->wedge_order, (void*)c->stats, (void*)c->depth, (void*)c->t_near})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : c->kt_ev) (void)hipEventDestroy(e);
    for (int i = 0; i < 3; ++i) {
        if (c->t_start[i]) (void)hipEventDestroy(c->t_start[i]);
        if (c->t_stop[i]) (void)hipEventDestroy(c->t_stop[i]);
    }
    delete c;
}

int rto_ctx_width(const rto_ctx* c) { return c ? c->width : 0; }
int rto_ctx_height(const rto_ctx* c) { return c ? c->height : 0; }
float* rto_ctx_aux(rto_ctx* c) { return c ? c->aux + (size_t)c->sel * RTO_AUX_CHANNELS * frame_px(c) : nullptr; }
float* rto_ctx_noisy(rto_ctx* c) { return c ? c->noisy + (size_t)c->sel * 4 * frame_px(c) : nullptr; }
float* rto_ctx_image(rto_ctx* c) { return c ? c->image + (size_t)c->sel * 4 * frame_px(c) : nullptr; }
int rto_ctx_frames(const rto_ctx* c) { return c ? c->frames : 0; }
int rto_ctx_selected_frame(const rto_ctx* c) { return c ? c->sel : 0; }
int rto_ctx_select_frame(rto_ctx* c, int frame) {
    if (!c || frame < 0 || frame >= c->frames) return set_err(RTO_E_INVALID, "rto_ctx_select_frame: frame out of range");
    c->sel = frame;
    return RTO_OK;
}

void rto_ctx_rng_seed(rto_ctx* c, uint64_t initstate, uint64_t initseq) {
    if (c) pcg_seed(c->rng, initstate, initseq);
}
void rto_ctx_rng_advance(rto_ctx* c, int64_t delta) {
    if (!c) return;
    const rto::PcgJumpEntry j = pcg_jump(c->rng.inc, (uint64_t)delta);
    c->rng.state = j.mult * c->rng.state + j.plus;
}
void rto_ctx_rng_set(rto_ctx* c, uint64_t state, uint64_t inc) {
    if (!c) return;
    c->rng.state = state;
    c->rng.inc = inc;
}
void rto_ctx_rng_get(const rto_ctx* c, uint64_t* state, uint64_t* inc) {
    if (!c) return;
    if (state) *state = c->rng.state;
    if (inc) *inc = c->rng.inc;
}

int rto_ctx_set_layers(rto_ctx* c, const float* depth, const float* color) {
    if (!c) return set_err(RTO_E_INVALID, "rto_ctx_set_layers: null context");
    if ((uintptr_t)color % 16 != 0) return set_err(RTO_E_INVALID, "rto_ctx_set_layers: color must be 16-byte aligned");
    if ((uintptr_t)depth % 4 != 0) return set_err(RTO_E_INVALID, "rto_ctx_set_layers: depth must be 4-byte aligned");
    DeviceGuard guard(c->device);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    const size_t px = frame_px(c) * (size_t)c->frames;
    struct Range {
        const char* what;
        uintptr_t lo, hi;
    };
    const Range own[3] = {{"aux", (uintptr_t)c->aux, (uintptr_t)c->aux + px * RTO_AUX_CHANNELS * sizeof(float)},
                          {"noisy", (uintptr_t)c->noisy, (uintptr_t)c->noisy + px * 4 * sizeof(float)},
                          {"image", (uintptr_t)c->image, (uintptr_t)c->image + px * 4 * sizeof(float)}};
    const Range in[2] = {{"depth", (uintptr_t)depth, (uintptr_t)depth + px * sizeof(float)},
                         {"color", (uintptr_t)color, (uintptr_t)color + px * 4 * sizeof(float)}};
    for (const Range& l : in) {
        if (!l.lo) continue;
        if (pointer_device((const void*)l.lo) != c->device)
            return set_err(RTO_E_INVALID, std::string("rto_ctx_set_layers: ") + l.what + " is not memory of the context's device");
        // (in-place use, the reference's surf_obj, is not offered: the batched path stores a pixel from another kernel than the
        //  one that would have to read it)
        for (const Range& o : own)
            if (l.lo < o.hi && o.lo < l.hi)
                return set_err(RTO_E_INVALID, std::string("rto_ctx_set_layers: ") + l.what + " overlaps the context's " + o.what +
                                                  " buffer (keep the layers in buffers of their own)");
    }
    c->layer_depth = depth;
    c->layer_color = color;
    return RTO_OK;
}

int rto_ctx_layers(const rto_ctx* c, const float** depth, const float** color) {
    if (!c) return set_err(RTO_E_INVALID, "rto_ctx_layers: null context");
    if (depth) *depth = c->layer_depth;
    if (color) *color = c->layer_color;
    return RTO_OK;
}

int rto_ctx_enable_depth(rto_ctx* c, int enable) {
    if (!c) return set_err(RTO_E_INVALID, "rto_ctx_enable_depth: null context");
    // (1 = frame by frame, RTO_DEPTH_BATCHED = through the persistent kernels, anything else non-zero = 1; between the two the
    //  planes stay: the mode is all that changes)
    const int mode = enable == 0 ? 0 : enable == RTO_DEPTH_BATCHED ? RTO_DEPTH_BATCHED : 1;
    if ((enable != 0) == (c->depth != nullptr)) {
        c->depth_mode = mode;
        return RTO_OK;
    }
    DeviceGuard guard(c->device);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    if (!enable) {  // (launches in flight may still write the planes)
        HIP_TRY(hipDeviceSynchronize());
        float* const d = c->depth;
        float* const t = c->t_near;
        c->depth = c->t_near = nullptr;
        c->depth_mode = 0;
        const hipError_t e1 = hipFree(d), e2 = hipFree(t);  // (both planes, whatever the first call says)
        if (e1 != hipSuccess || e2 != hipSuccess)
            return set_err(RTO_E_HIP, std::string("hipFree(depth outputs): ") + hipGetErrorString(e1 != hipSuccess ? e1 : e2));
        return RTO_OK;
    }
    const size_t bytes = frame_px(c) * (size_t)c->frames * sizeof(float);
    float *d = nullptr, *t = nullptr;
    if (hipMalloc((void**)&d, bytes) != hipSuccess || hipMalloc((void**)&t, bytes) != hipSuccess) {
        if (d) (void)hipFree(d);
        return set_err(RTO_E_HIP, "hipMalloc(depth outputs) failed");
    }
    // until a launch writes a slot it reads as "no hit": depth 0, t_near +inf (0x7f800000 has no byte pattern: a copy)
    const std::vector<float> inf(frame_px(c) * (size_t)c->frames, INFINITY);
    if (hipMemset(d, 0, bytes) != hipSuccess || hipMemcpy(t, inf.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        (void)hipFree(t);
        return set_err(RTO_E_HIP, "initialising the depth outputs failed");
    }
    c->depth = d;
    c->t_near = t;
    c->depth_mode = mode;
    return RTO_OK;
}
int rto_ctx_depth_enabled(const rto_ctx* c) { return c && c->depth ? c->depth_mode : 0; }
float* rto_ctx_depth(rto_ctx* c) { return c && c->depth ? c->depth + (size_t)c->sel * frame_px(c) : nullptr; }
float* rto_ctx_t_near(rto_ctx* c) { return c && c->t_near ? c->t_near + (size_t)c->sel * frame_px(c) : nullptr; }

int rto_ctx_set_kernel(rto_ctx* c, int kernel) {
    if (!c || kernel < RTO_KERNEL_AUTO || kernel > RTO_KERNEL_FAST)
        return set_err(RTO_E_INVALID, "rto_ctx_set_kernel: bad argument");
    c->kernel = kernel;
    return RTO_OK;
}

#ifdef RTO_DBG_COUNTERS
extern "C" int rto_debug_read_queue(rto_ctx* c, uint64_t out[24]) {
    return hipMemcpy(out, c->queue, 24 * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -4;
}
extern "C" int rto_debug_zero_queue(rto_ctx* c) { return hipMemset(c->queue + 2, 0, 48) == hipSuccess ? 0 : -4; }
extern "C" int rto_debug_shade_phases(uint64_t* out /* 2^19 waves x 8 words */, int reset) {
    return rto::debug_shade_phases((unsigned long long*)out, reset != 0) == hipSuccess ? 0 : -4;
}
#endif

int rto_ctx_set_lean_outputs(rto_ctx* c, int level) {
    if (!c) return set_err(RTO_E_INVALID, "rto_ctx_set_lean_outputs: null context");
    if (level < 0 || level > 2) return set_err(RTO_E_INVALID, "rto_ctx_set_lean_outputs: level 0 (full), 1 (lean) or 2 (lean + sparse)");
    c->lean = level;
    return RTO_OK;
}

int rto_ctx_frames_lean_level(const rto_ctx* c, int first_slot, int n) {
    if (!c || n < 1 || first_slot < 0 || first_slot + n > c->frames) return 0;
    const int l0 = c->lean_slot[(size_t)first_slot];
    for (int i = first_slot + 1; i < first_slot + n; ++i)
        if (c->lean_slot[(size_t)i] != l0) return -1;
    return l0;
}

int rto_ctx_frames_are_lean(const rto_ctx* c, int first_slot, int n) {
    if (!c || n < 1 || first_slot < 0 || first_slot + n > c->frames) return 0;
    int lean = 0;
    for (int i = first_slot; i < first_slot + n; ++i) lean += c->lean_slot[(size_t)i] ? 1 : 0;
    return lean == n ? 1 : lean == 0 ? 0 : -1;  // -1: a mixed range -- no one route reads all of its slots correctly
}

int rto_ctx_set_tuning(rto_ctx* c, const char* key, int value) {
    if (!c || !key) return set_err(RTO_E_INVALID, "rto_ctx_set_tuning: null argument");
    const std::string k(key);
    if (k == "tile_order") {
        c->tile_order_on = value != 0;
    } else if (k == "xcd_queues") {
        c->xcd_queues = value != 0;
    } else if (k == "tile_major") {
        c->tile_major = value != 0;
    } else if (k == "tile_block") {
        if (value < 1 || value > 64) return set_err(RTO_E_INVALID, "tile_block must be 1..64");
        c->tile_block = value;
        DeviceGuard guard(c->device);
        if (hipDeviceSynchronize() != hipSuccess) return set_err(RTO_E_HIP, "hipDeviceSynchronize failed");
        return build_tile_tables(c);
    } else if (k == "queue_bands") {  // XCD queues by bands of `value` tile rows (0: angular wedges); same pixels
        if (value < 0 || value > 64) return set_err(RTO_E_INVALID, "queue_bands must be 0..64");
        c->queue_bands = value;
        DeviceGuard guard(c->device);
        if (hipDeviceSynchronize() != hipSuccess) return set_err(RTO_E_HIP, "hipDeviceSynchronize failed");
        return build_tile_tables(c);
    } else if (k == "refill") {
        c->refill = value;
    } else if (k == "wide_bits") {  // test hook (fast_path_for_spp): 0 = the real budget
        c->test_wide_bits = value;
    } else if (k == "cull") {  // empty-space culling of the batched path (1 = on; same pixels either way)
        c->cull_on = value != 0;
    } else if (k == "cull_cubes") {  // A/B and test hook: culling cells as whole cubes, not the bounds of their dense leaves (more marks, same pixels)
        c->cull_cubes = value != 0;
    } else if (k == "cull_single") {  // rto_launch_renderer's fast kernel skips the tiles no culling cell projects into (same pixels)
        c->cull_single = value != 0;
    } else if (k == "frame_via_batch") {  // rto_launch_renderer as a batch of one (culling + tile marks); same pixels
        c->frame_via_batch = value != 0;
    } else if (k == "blocks_per_cu") {  // occupancy of the persistent traversal kernel: 0 = what fits, else a cap (1..8)
        if (value < 0 || value > 8) return set_err(RTO_E_INVALID, "blocks_per_cu must be 0..8");
        c->occ.cap = value;
    } else if (k == "batch_fallback") {  // test hook: 1 = batched launches take the per-frame generic fallback (as a tree with too
        c->batch_fallback = value;       // many leaf slots for the SPP does), 2 = as if the device refused the traversal kernel's LDS
    } else if (k == "ray_order") {  // rto_launch_rays: 0 = consecutive blocks of 256 rays, 1 = one contiguous range of rays per XCD
        if (value < 0 || value > 1) return set_err(RTO_E_INVALID, "ray_order must be 0 or 1");
        c->ray_order = value;
    } else if (k == "strip_rows") {
        if (value < 1) return set_err(RTO_E_INVALID, "strip_rows must be >= 1");
        c->strip_rows = value;
    } else {
        return set_err(RTO_E_INVALID, "unknown tuning key '" + k + "'");
    }
    return RTO_OK;
}

int rto_ctx_kernel_timing(rto_ctx* c, int enable) {
    if (!c) return set_err(RTO_E_INVALID, "rto_ctx_kernel_timing: null context");
    DeviceGuard guard(c->device);
    if (enable && c->kt_ev.empty()) {
        c->kt_ev.resize((size_t)kKtRing * 4);
        for (auto& e : c->kt_ev) HIP_TRY(hipEventCreate(&e));
    }
    c->kt_on = enable != 0;
    c->kt_count = 0;
    return RTO_OK;
}

int rto_ctx_kernel_timing_read(rto_ctx* c, float* traverse_ms, float* shade_ms, int* launches) {
    return rto_ctx_kernel_timing_read3(c, nullptr, traverse_ms, shade_ms, launches);
}

int rto_ctx_kernel_timing_read3(rto_ctx* c, float* raygen_ms, float* traverse_ms, float* shade_ms, int* launches) {
    if (!c) return set_err(RTO_E_INVALID, "rto_ctx_kernel_timing_read: null context");
    DeviceGuard guard(c->device);
    double g = 0, t = 0, s = 0;
    for (int i = 0; i < c->kt_count; ++i) {
        float r = 0, a = 0, b = 0;
        const hipEvent_t* e = &c->kt_ev[(size_t)i * 4];
        HIP_TRY(hipEventSynchronize(e[3]));
        HIP_TRY(hipEventElapsedTime(&r, e[0], e[1]));
        HIP_TRY(hipEventElapsedTime(&a, e[1], e[2]));
        HIP_TRY(hipEventElapsedTime(&b, e[2], e[3]));
        g += r;
        t += a;
        s += b;
    }
    if (raygen_ms) *raygen_ms = c->kt_count ? (float)(g / c->kt_count) : 0.f;
    if (traverse_ms) *traverse_ms = c->kt_count ? (float)(t / c->kt_count) : 0.f;
    if (shade_ms) *shade_ms = c->kt_count ? (float)(s / c->kt_count) : 0.f;
    if (launches) *launches = c->kt_count;
    c->kt_count = 0;
    return RTO_OK;
}

int rto_ctx_queue_stats(rto_ctx* c, int64_t* live_tile_slots, int64_t* all_tile_slots) {
    if (!c || !live_tile_slots || !all_tile_slots) return set_err(RTO_E_INVALID, "rto_ctx_queue_stats: null argument");
    if (!c->qscratch || c->last_n_queues < 1) return set_err(RTO_E_INVALID, "rto_ctx_queue_stats: no batched launch yet");
    DeviceGuard guard(c->device);
    HIP_TRY(hipDeviceSynchronize());
    uint32_t cnt[rto::kMaxQueues] = {0};
    HIP_TRY(hipMemcpy(cnt, c->qscratch + 2 * (size_t)c->q_chunks_cap, sizeof(cnt), hipMemcpyDeviceToHost));
    int64_t live = 0;
    for (int k = 0; k < c->last_n_queues; ++k) live += cnt[k];
    *live_tile_slots = live;
    *all_tile_slots = c->last_slots;
    return RTO_OK;
}

int rto_ctx_tile_marks(const rto_ctx* c, const uint32_t** marks, int* words_per_frame, int* first_slot, int* frames, float* background) {
    if (!c || !marks || !words_per_frame || !first_slot || !frames || !background)
        return set_err(RTO_E_INVALID, "rto_ctx_tile_marks: null argument");
    if (c->marks_n < 1 || !c->tile_mask) return set_err(RTO_E_INVALID, "rto_ctx_tile_marks: the last launch on this context was not a batched one");
    *marks = c->tile_mask;
    *words_per_frame = c->mask_words;
    *first_slot = c->marks_slot0;
    *frames = c->marks_n;
    *background = c->marks_bg;
    return RTO_OK;
}

int rto_ctx_enable_stats(rto_ctx* c, int enable) {
    if (!c) return set_err(RTO_E_INVALID, "rto_ctx_enable_stats: null context");
    DeviceGuard guard(c->device);
    if (enable && !c->stats) {
        HIP_TRY(hipMalloc((void**)&c->stats, rto::kStatsWords * sizeof(unsigned long long)));
        HIP_TRY(hipMemset(c->stats, 0, rto::kStatsWords * sizeof(unsigned long long)));
    }
    c->stats_on = enable != 0;
    c->stats_marks = enable == 2;
    return RTO_OK;
}

// counters [first, first + count) of the context's block to the host, optionally zeroed behind the copy
static int read_stats(rto_ctx* c, void* stream_, uint64_t* out, int first, int count, int reset, const char* who) {
    if (!c || !out) return set_err(RTO_E_INVALID, std::string(who) + ": null argument");
    if (!c->stats) return set_err(RTO_E_INVALID, std::string(who) + ": counters were never enabled");
    DeviceGuard guard(c->device);
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipMemcpyAsync(out, c->stats + first, count * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    if (reset) HIP_TRY(hipMemsetAsync(c->stats + first, 0, count * sizeof(uint64_t), stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return RTO_OK;
}
int rto_ctx_get_march_stats(rto_ctx* c, void* stream, uint64_t out[8], int reset) {
    return read_stats(c, stream, out, 6, 8, reset, "rto_ctx_get_march_stats");
}
int rto_ctx_get_stats(rto_ctx* c, void* stream, uint64_t out[6], int reset) {
    return read_stats(c, stream, out, 0, 6, reset, "rto_ctx_get_stats");
}

int rto_filtering_batch(void* stream, const float* weight_map, const float* guidance_map, int L, int H, int W, int n,
                        const float* img_in, float* img_out) {
    return rto_filtering_batch_mode(stream, weight_map, guidance_map, L, H, W, n, img_in, img_out, RTO_FILTER_EXACT);
}

int rto_filtering_batch_mode(void* stream, const float* weight_map, const float* guidance_map, int L, int H, int W, int n,
                             const float* img_in, float* img_out, int mode) {
    if (mode != RTO_FILTER_EXACT && mode != RTO_FILTER_FACTORISED) return set_err(RTO_E_INVALID, "rto_filtering_batch_mode: unknown mode");
    return filter_call("rto_filtering", {weight_map, guidance_map, img_in, img_out}, L, H, W, n, img_in, img_out, img_out, "filter", [&] {
        return (mode == RTO_FILTER_EXACT ? rto::launch_filter : rto::launch_filter_fast)(weight_map, guidance_map, L, H, W, n, img_in, img_out,
                                                                                       (hipStream_t)stream);
    });
}

int rto_filtering_train_forward(void* stream, const float* weight_map, const float* guidance_map, int L, int H, int W,
                                int n, const float* img_in, float* img_out, float* rgb_filtered, float* max_map,
                                float* inv_kernel_sum) {
    return filter_call("rto_filtering_train_forward", {weight_map, guidance_map, img_in, img_out, rgb_filtered, max_map, inv_kernel_sum}, L,
                       H, W, n, img_in, img_out, img_out, "filter", [&] {
                           return rto::launch_filter_train(weight_map, guidance_map, L, H, W, n, img_in, img_out, rgb_filtered, max_map,
                                                           inv_kernel_sum, (hipStream_t)stream);
                       });
}

int rto_filtering_backward(void* stream, const float* grad_output, const float* img_in, const float* weight_map,
                           const float* guidance_map, const float* rgb_filtered, const float* max_map,
                           const float* inv_kernel_sum, int L, int H, int W, int n, float* grad_weight,
                           float* grad_guidance) {
    return filter_call("rto_filtering_backward",
                       {grad_output, img_in, weight_map, guidance_map, rgb_filtered, max_map, inv_kernel_sum, grad_weight, grad_guidance}, L, H, W,
                       n, nullptr, nullptr, grad_guidance, "filter backward", [&] {
                           return rto::launch_filter_backward(grad_output, img_in, weight_map, guidance_map, rgb_filtered, max_map,
                                                              inv_kernel_sum, L, H, W, n, grad_weight, grad_guidance, (hipStream_t)stream);
                       });
}

int rto_filtering(void* stream, const float* weight_map, const float* guidance_map, int L, int H, int W,
                  const float* img_in, float* img_out) {
    return rto_filtering_batch(stream, weight_map, guidance_map, L, H, W, 1, img_in, img_out);
}

int rto_ctx_filtering(rto_ctx* c, void* stream, const float* weight_map, const float* guidance_map, int L) {
    if (!c) return set_err(RTO_E_INVALID, "rto_ctx_filtering: null context");
    DeviceGuard guard(c->device);
    return rto_filtering(stream, weight_map, guidance_map, L, c->height, c->width, rto_ctx_noisy(c), rto_ctx_image(c));
}

// The noisy image of a SPARSE lean frame holds nothing in the tiles its launch left unmarked: they are the background (colour =
// the launch's background brightness, alpha 0 -- a lean frame's alpha is aux plane 3).  Filled in on the host after the copy,
// from the marks the launch left on the device; T = float (x4 per pixel) or uint8_t (the truncated bytes, main_headless.cpp:535-538).
}  // extern "C"
template <class T>
static int fill_unmarked_tiles(rto_ctx* c, hipStream_t stream, T* host, T colour) {
    if (c->lean_slot[(size_t)c->sel] != 2) return RTO_OK;
    if (c->marks_n < 1 || !c->tile_mask || c->sel < c->marks_slot0 || c->sel >= c->marks_slot0 + c->marks_n)
        return set_err(RTO_E_INVALID, "the selected slot holds a sparse lean frame whose tile marks a later launch replaced: its noisy image "
                                      "cannot be completed");
    std::vector<uint32_t> m((size_t)c->mask_words);
    HIP_TRY(hipMemcpyAsync(m.data(), c->tile_mask + (size_t)(c->sel - c->marks_slot0) * c->mask_words, m.size() * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (m.back() & 1u) return RTO_OK;  // keep-all frame: every tile was rendered
    const int tx_n = (c->width + 7) / 8, ty_n = (c->height + 7) / 8;
    for (int ty = 0; ty < ty_n; ++ty)
        for (int tx = 0; tx < tx_n; ++tx) {
            const uint32_t t = (uint32_t)(ty * tx_n + tx);
            if ((m[t >> 5] >> (t & 31u)) & 1u) continue;
            for (int y = ty * 8; y < std::min(ty * 8 + 8, c->height); ++y)
                for (int x = tx * 8; x < std::min(tx * 8 + 8, c->width); ++x) {
                    T* p = host + ((size_t)y * c->width + x) * 4;
                    p[0] = p[1] = p[2] = colour;
                    p[3] = T(0);
                }
        }
    return RTO_OK;
}
extern "C" {

int rto_ctx_download_rgba8(rto_ctx* c, void* stream_, int which, uint8_t* host_out) {
    if (!c || !host_out) return set_err(RTO_E_INVALID, "rto_ctx_download_rgba8: null argument");
    DeviceGuard guard(c->device);
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t px = (int64_t)c->width * c->height;
    HIP_TRY(rto::launch_rgba8(which ? rto_ctx_noisy(c) : rto_ctx_image(c), c->rgba8, px, stream));
    HIP_TRY(hipMemcpyAsync(host_out, c->rgba8, (size_t)px * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (which) return fill_unmarked_tiles<uint8_t>(c, stream, host_out, (uint8_t)(c->marks_bg * 255));
    return RTO_OK;
}

int rto_ctx_download_image(rto_ctx* c, void* stream_, int which, float* host_out) {
    if (!c || !host_out) return set_err(RTO_E_INVALID, "rto_ctx_download_image: null argument");
    DeviceGuard guard(c->device);
    hipStream_t stream = (hipStream_t)stream_;
    const size_t bytes = (size_t)c->width * c->height * 4 * sizeof(float);
    HIP_TRY(hipMemcpyAsync(host_out, which ? rto_ctx_noisy(c) : rto_ctx_image(c), bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (which) return fill_unmarked_tiles<float>(c, stream, host_out, c->marks_bg);
    return RTO_OK;
}

int rto_ctx_download_aux(rto_ctx* c, void* stream_, float* host_out) {
    if (!c || !host_out) return set_err(RTO_E_INVALID, "rto_ctx_download_aux: null argument");
    DeviceGuard guard(c->device);
    hipStream_t stream = (hipStream_t)stream_;
    const size_t bytes = (size_t)c->width * c->height * RTO_AUX_CHANNELS * sizeof(float);
    HIP_TRY(hipMemcpyAsync(host_out, rto_ctx_aux(c), bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return RTO_OK;
}

int rto_ctx_download_depth(rto_ctx* c, void* stream_, float* host_depth, float* host_t_near) {
    if (!c) return set_err(RTO_E_INVALID, "rto_ctx_download_depth: null context");
    if (!c->depth) return set_err(RTO_E_INVALID, "rto_ctx_download_depth: the context keeps no depth outputs (rto_ctx_enable_depth)");
    DeviceGuard guard(c->device);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t bytes = frame_px(c) * sizeof(float);
    if (host_depth) HIP_TRY(hipMemcpyAsync(host_depth, rto_ctx_depth(c), bytes, hipMemcpyDeviceToHost, stream));
    if (host_t_near) HIP_TRY(hipMemcpyAsync(host_t_near, rto_ctx_t_near(c), bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return RTO_OK;
}

// ---- Timer (render_context.hpp:122-213) ----
int rto_timer_reset(rto_ctx* c, void* stream) {
    if (!c) return set_err(RTO_E_INVALID, "rto_timer_reset: null context");
    c->t_stream = (hipStream_t)stream;
    c->t_cnt = 0;
    for (int i = 0; i < 3; ++i) {
        c->t_sum[i] = 0;
        c->t_used[i] = false;
    }
    return RTO_OK;
}
int rto_timer_start(rto_ctx* c, int which) {
    if (!c || which < 0 || which > 2) return set_err(RTO_E_INVALID, "rto_timer_start: bad argument");
    DeviceGuard guard(c->device);
    HIP_TRY(hipEventRecord(c->t_start[which], c->t_stream));
    return RTO_OK;
}
int rto_timer_stop(rto_ctx* c, int which) {
    if (!c || which < 0 || which > 2) return set_err(RTO_E_INVALID, "rto_timer_stop: bad argument");
    DeviceGuard guard(c->device);
    HIP_TRY(hipEventRecord(c->t_stop[which], c->t_stream));
    c->t_used[which] = true;
    return RTO_OK;
}
int rto_timer_record(rto_ctx* c, int denoise) {
    if (!c) return set_err(RTO_E_INVALID, "rto_timer_record: null context");
    DeviceGuard guard(c->device);
    const int last = denoise ? RTO_T_FILTER : RTO_T_RENDER;
    if (!c->t_used[last]) return set_err(RTO_E_INVALID, "rto_timer_record: the closing event was never recorded");
    HIP_TRY(hipEventSynchronize(c->t_stop[last]));
    c->t_cnt++;
    for (int i = 0; i < 3; ++i) {
        // the reference reads all three pairs every frame; buckets that never ran stay at 0 here
        if (!c->t_used[i] || (!denoise && i != RTO_T_RENDER)) continue;
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->t_start[i], c->t_stop[i]));
        c->t_sum[i] += ms;
    }
    return RTO_OK;
}
int rto_timer_report(const rto_ctx* c, float ms_out[3], float* fps_out, int* frames_out) {
    if (!c) return set_err(RTO_E_INVALID, "rto_timer_report: null context");
    float all = 0;
    for (int i = 0; i < 3; ++i) {
        const float t = c->t_cnt ? c->t_sum[i] / c->t_cnt : 0.f;
        if (ms_out) ms_out[i] = t;
        all += t;
    }
    if (fps_out) *fps_out = all > 0 ? 1000.f / all : 0.f;
    if (frames_out) *frames_out = c->t_cnt;
    return RTO_OK;
}

}  // extern "C"
