// host/fit_grad.cpp -- the host twin of rto_tree_fit_grad, rto_tree_fit_grad_rays (with or without the touched bitmap) and rto_fit_sgd_step: the marches of
// rto_fit_march.h over child[] / data[] with the root-restart float descent, det_expf restated in plain C++.  Same bits as the
// kernels (tests/test_fit_gpu.py, tests/test_fit_rays_gpu.py) and as the numpy restatements (tests/fit_ref.py,
// tests/fit_rays_ref.py).  No HIP header.
#include "fit_grad.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../rto_fit_march.h"
#include "leaf_weights.h"

namespace rto {

int fit_basis_of_tree(int format, int basis_dim, int data_dim) {
    if (format == RTO_FMT_RGBA) return data_dim == 4 ? 0 : -1;
    if (format != RTO_FMT_SH) return -1;
    if (basis_dim != 1 && basis_dim != 4 && basis_dim != 9 && basis_dim != 16 && basis_dim != 25) return -1;
    return data_dim == 3 * basis_dim + 1 ? basis_dim : -1;
}

int fit_basis_of_format(const char* data_format, int data_dim) {
    if (!data_format) return -1;
    if (!std::strcmp(data_format, "RGBA")) return fit_basis_of_tree(RTO_FMT_RGBA, -1, data_dim);
    if (!std::strncmp(data_format, "SH", 2) && data_format[2] >= '1' && data_format[2] <= '9') {
        char* end = nullptr;
        const long b = std::strtol(data_format + 2, &end, 10);
        if (*end == 0 && b <= 25) return fit_basis_of_tree(RTO_FMT_SH, (int)b, data_dim);
    }
    return -1;
}

namespace {

bool overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

}  // namespace

std::string fit_check_call(const float* params, const rto_camera* cams, const float* const* targets, float* const* images, int n,
                           const rto_options* opt, const int64_t* grad, const uint64_t* stats, int64_t param_count) {
    if (!params) return "null params";
    if (!opt) return "null options";
    if ((uintptr_t)params % 4 != 0) return "params must be 4-byte aligned";
    if ((uintptr_t)grad % 8 != 0) return "grad must be 8-byte aligned";
    if ((uintptr_t)stats % 8 != 0) return "stats must be 8-byte aligned";
    if (!targets && (grad || stats)) return "null targets with grad or stats set";
    const std::string bad = leaf_weights_check_cams(cams, n, params);
    if (!bad.empty()) return bad;
    if (opt->basis_minmax[0] != 0 || opt->basis_minmax[1] != RTO_BASIS_MAX - 1)
        return "options: basis_minmax is not read by the fit and must keep its default {0, 24}";
    if (opt->rot_dirs[0] != 0.f || opt->rot_dirs[1] != 0.f || opt->rot_dirs[2] != 0.f)
        return "options: rot_dirs is not read by the fit and must keep its default {0, 0, 0}";
    for (int f = 0; f < n; ++f) {
        const std::string at = "camera " + std::to_string(f) + ": ";
        const int64_t bytes = (int64_t)cams[f].width * cams[f].height * 12;
        if (targets) {
            if (!targets[f]) return at + "null target";
            if ((uintptr_t)targets[f] % 4 != 0) return at + "target must be 4-byte aligned";
            if (overlap(params, param_count * 4, targets[f], bytes)) return at + "params overlaps the target";
            if (grad && overlap(grad, param_count * 8, targets[f], bytes)) return at + "grad overlaps the target";
        }
        if (images && images[f]) {
            if ((uintptr_t)images[f] % 4 != 0) return at + "image must be 4-byte aligned";
            if (overlap(params, param_count * 4, images[f], bytes)) return at + "params overlaps the image";
            if (grad && overlap(grad, param_count * 8, images[f], bytes)) return at + "grad overlaps the image";
        }
    }
    return "";
}

std::string fit_check_rays_call(const float* params, const float* origins, const float* dirs, const float* targets, const float* out, int64_t n,
                                const rto_options* opt, const int64_t* grad, const uint64_t* stats, int64_t param_count) {
    if (!params) return "null params";
    if (!opt) return "null options";
    if (n < 0) return "n must be >= 0";
    if (!origins && n > 0) return "null origins with n > 0";
    if (!dirs && n > 0) return "null dirs with n > 0";
    if ((uintptr_t)params % 4 != 0) return "params must be 4-byte aligned";
    if ((uintptr_t)grad % 8 != 0) return "grad must be 8-byte aligned";
    if ((uintptr_t)stats % 8 != 0) return "stats must be 8-byte aligned";
    if (!targets && (grad || stats)) return "null targets with grad or stats set";
    if (opt->basis_minmax[0] != 0 || opt->basis_minmax[1] != RTO_BASIS_MAX - 1)
        return "options: basis_minmax is not read by the fit and must keep its default {0, 24}";
    if (opt->rot_dirs[0] != 0.f || opt->rot_dirs[1] != 0.f || opt->rot_dirs[2] != 0.f)
        return "options: rot_dirs is not read by the fit and must keep its default {0, 0, 0}";
    const struct {
        const float* p;
        const char* name;
    } arrays[4] = {{origins, "origins"}, {dirs, "dirs"}, {targets, "targets"}, {out, "out"}};
    const int64_t bytes = n * 12;
    for (const auto& a : arrays) {
        if (!a.p) continue;
        if ((uintptr_t)a.p % 4 != 0) return std::string(a.name) + " must be 4-byte aligned";
        if (overlap(params, param_count * 4, a.p, bytes)) return std::string("params overlaps ") + a.name;
        if (grad && overlap(grad, param_count * 8, a.p, bytes)) return std::string("grad overlaps ") + a.name;
    }
    if (out)
        for (int k = 0; k < 3; ++k)
            if (arrays[k].p && overlap(out, bytes, arrays[k].p, bytes)) return std::string("out overlaps ") + arrays[k].name;
    return "";
}

std::string fit_check_touched(const float* params, const float* origins, const float* dirs, const float* targets, const float* out, int64_t n,
                              const int64_t* grad, const uint64_t* stats, const uint32_t* touched, int64_t slots, int D) {
    if (!grad) return "null grad: a forward-only call uses the entry without the bitmap";
    if (!touched) return "null touched";
    if ((uintptr_t)touched % 4 != 0) return "touched must be 4-byte aligned";
    const int64_t t_bytes = ((slots + 31) >> 5) * 4;
    const struct {
        const void* p;
        int64_t bytes;
        const char* name;
    } arrays[7] = {{params, slots * D * 4, "params"}, {grad, slots * D * 8, "grad"}, {stats, 16, "stats"},   {origins, n * 12, "origins"},
                   {dirs, n * 12, "dirs"},            {targets, n * 12, "targets"},  {out, n * 12, "out"}};
    for (const auto& a : arrays)
        if (a.p && overlap(touched, t_bytes, a.p, a.bytes)) return std::string("touched overlaps ") + a.name;
    return "";
}

namespace {

template <int B>
void fit_cameras(const int32_t* child, const uint16_t* data, const float* params, int N, const lm::Frame& fr, const fm::Opt& o,
                 const rto_camera* cams, const float* const* targets, float* const* images, int n, int nt, int64_t* grad, uint64_t* stats) {
    constexpr int D = fm::data_dim_of<B>();
    const auto locate = [&](const float* pos, lm::Leaf& leaf) -> bool {
        for (int i = 0; i < 3; ++i) leaf.local[i] = pos[i];
        const int64_t slot = lm::descend_child(child, N, leaf.local, leaf.cube_sz);
        leaf.index = (uint32_t)slot;
        leaf.sigma_bits = data[slot * D + D - 1];
        return true;
    };
    const auto exp_ = [](float v) -> float { return lm::det_expf(v); };
    const auto slot_of = [](uint32_t index) -> uint32_t { return index; };
    const auto add = [&](int64_t index, float g) {
        const int64_t q = fm::to_fixed(g);
        if (q != 0) __atomic_fetch_add((uint64_t*)grad + index, (uint64_t)q, __ATOMIC_RELAXED);
    };
    for (int f = 0; f < n; ++f) {
        lm::Cam cam;
        cam.width = cams[f].width;
        cam.height = cams[f].height;
        cam.fx = cams[f].fx;
        cam.fy = cams[f].fy;
        for (int i = 0; i < 12; ++i) cam.transform[i] = cams[f].transform[i];
        const float* target = targets ? targets[f] : nullptr;
        float* image = images ? images[f] : nullptr;
        const auto rows = [&](int k) {
            uint64_t loss = 0, rays = 0;
            for (int y = k; y < cam.height; y += nt)
                for (int x = 0; x < cam.width; ++x) {
                    const int64_t px = ((int64_t)y * cam.width + x) * 3;
                    int64_t q;
                    if (fm::fit_pixel<B>(fr, o, cam, x, y, params, target ? target + px : nullptr, image ? image + px : nullptr, grad != nullptr,
                                         locate, exp_, slot_of, add, q)) {
                        loss += (uint64_t)q;
                        ++rays;
                    }
                }
            if (stats && target) {
                __atomic_fetch_add(stats, loss, __ATOMIC_RELAXED);
                __atomic_fetch_add(stats + 1, rays, __ATOMIC_RELAXED);
            }
        };
        if (nt == 1) {
            rows(0);
        } else {
            std::vector<std::thread> pool;
            for (int k = 0; k < nt; ++k) pool.emplace_back(rows, k);
            for (auto& t : pool) t.join();
        }
    }
}

// the rays [i0, i1) of thread k of nt; integer sums, so the split changes no bit
template <int B>
void fit_rays(const int32_t* child, const uint16_t* data, const float* params, int N, const lm::Frame& fr, const fm::Opt& o, const float* origins,
              const float* dirs, const float* targets, float* out, int64_t n, int nt, int64_t* grad, uint64_t* stats, uint32_t* touched) {
    constexpr int D = fm::data_dim_of<B>();
    const auto locate = [&](const float* pos, lm::Leaf& leaf) -> bool {
        for (int i = 0; i < 3; ++i) leaf.local[i] = pos[i];
        const int64_t slot = lm::descend_child(child, N, leaf.local, leaf.cube_sz);
        leaf.index = (uint32_t)slot;
        leaf.sigma_bits = data[slot * D + D - 1];
        return true;
    };
    const auto exp_ = [](float v) -> float { return lm::det_expf(v); };
    const auto slot_of = [](uint32_t index) -> uint32_t { return index; };
    const auto add = [&](int64_t index, float g) {
        if (touched && index % D == D - 1) {  // the density's contribution, the first of a dense sample: mark the slot
            const int64_t slot = index / D;
            __atomic_fetch_or(touched + (slot >> 5), 1u << (slot & 31), __ATOMIC_RELAXED);
        }
        const int64_t q = fm::to_fixed(g);
        if (q != 0) __atomic_fetch_add((uint64_t*)grad + index, (uint64_t)q, __ATOMIC_RELAXED);
    };
    const auto range = [&](int k) {
        const int64_t i0 = n / nt * k + (k < n % nt ? k : n % nt), i1 = i0 + n / nt + (k < n % nt ? 1 : 0);
        uint64_t loss = 0, rays = 0;
        for (int64_t i = i0; i < i1; ++i) {
            int64_t q;
            if (fm::fit_ray<B>(fr, o, origins + i * 3, dirs + i * 3, params, targets ? targets + i * 3 : nullptr, out ? out + i * 3 : nullptr,
                               grad != nullptr, locate, exp_, slot_of, add, q)) {
                loss += (uint64_t)q;
                ++rays;
            }
        }
        if (stats && targets) {
            __atomic_fetch_add(stats, loss, __ATOMIC_RELAXED);
            __atomic_fetch_add(stats + 1, rays, __ATOMIC_RELAXED);
        }
    };
    if (nt == 1) {
        range(0);
    } else {
        std::vector<std::thread> pool;
        for (int k = 0; k < nt; ++k) pool.emplace_back(range, k);
        for (auto& t : pool) t.join();
    }
}

void host_frame_and_opt(const float scale[3], const float offset[3], const float* ndc, const rto_options* opt, lm::Frame& fr, fm::Opt& o) {
    for (int i = 0; i < 3; ++i) {
        fr.offset[i] = offset[i];
        fr.scale[i] = scale[i];
    }
    fr.ndc_width = ndc && ndc[0] > 0 ? ndc[0] : -1.f;
    fr.ndc_height = ndc ? ndc[1] : 0.f;
    fr.ndc_focal = ndc ? ndc[2] : 0.f;
    o.m.step_size = opt->step_size;
    o.m.sigma_thresh = opt->sigma_thresh;
    o.m.stop_thresh = opt->stop_thresh;
    for (int i = 0; i < 6; ++i) o.m.render_bbox[i] = opt->render_bbox[i];
    o.bg = opt->background_brightness;
}

}  // namespace

int fit_grad_host(const int32_t* child, const uint16_t* data, const float* params, int64_t capacity, int N, int D, const char* data_format,
                  const float scale[3], const float offset[3], const float* ndc, const rto_camera* cams, const float* const* targets,
                  float* const* images, int n, const rto_options* opt, int threads, int64_t* grad, uint64_t* stats, std::string* err) {
    const auto fail = [&](int code, const std::string& msg) {
        if (err) *err = msg;
        return code;
    };
    if (!child || !data || !scale || !offset || !data_format) return fail(RTO_E_INVALID, "null argument");
    if (capacity < 1 || N < 2 || D < 1) return fail(RTO_E_INVALID, "capacity >= 1, N >= 2 and data_dim >= 1 are required");
    const int64_t N3 = (int64_t)N * N * N;
    if (capacity > (((int64_t)1 << 31) - 1) / N3) return fail(RTO_E_INVALID, "capacity * N^3 must stay below 2^31");
    const int B = fit_basis_of_format(data_format, D);
    if (B < 0)
        return fail(RTO_E_UNSUPPORTED, std::string("the fit takes RGBA and SH trees of basis_dim 1, 4, 9, 16 or 25, not ") + data_format +
                                           " with data_dim " + std::to_string(D));
    const std::string bad = fit_check_call(params, cams, targets, images, n, opt, grad, stats, capacity * N3 * D);
    if (!bad.empty()) return fail(RTO_E_INVALID, bad);
    const std::string links = leaf_weights_check_links(child, capacity, N3);
    if (!links.empty()) return fail(RTO_E_FORMAT, links);
    if (n == 0) return RTO_OK;

    lm::Frame fr;
    fm::Opt o;
    host_frame_and_opt(scale, offset, ndc, opt, fr, o);
    const int nt = threads <= 0 ? 1 : threads;
#define RTO_FIT_CASE(B_) \
    case B_: fit_cameras<B_>(child, data, params, N, fr, o, cams, targets, images, n, nt, grad, stats); break
    switch (B) {
        RTO_FIT_CASE(0);
        RTO_FIT_CASE(1);
        RTO_FIT_CASE(4);
        RTO_FIT_CASE(9);
        RTO_FIT_CASE(16);
        RTO_FIT_CASE(25);
    }
#undef RTO_FIT_CASE
    return RTO_OK;
}

int fit_grad_rays_host(const int32_t* child, const uint16_t* data, const float* params, int64_t capacity, int N, int D, const char* data_format,
                       const float scale[3], const float offset[3], const float* ndc, const float* origins, const float* dirs,
                       const float* targets, float* out, int64_t n, const rto_options* opt, int threads, int64_t* grad, uint64_t* stats,
                       std::string* err) {
    return fit_grad_rays_touched_host(child, data, params, capacity, N, D, data_format, scale, offset, ndc, origins, dirs, targets, out, n, opt,
                                      threads, grad, stats, nullptr, false, err);
}

int fit_grad_rays_touched_host(const int32_t* child, const uint16_t* data, const float* params, int64_t capacity, int N, int D,
                               const char* data_format, const float scale[3], const float offset[3], const float* ndc, const float* origins,
                               const float* dirs, const float* targets, float* out, int64_t n, const rto_options* opt, int threads,
                               int64_t* grad, uint64_t* stats, uint32_t* touched, bool marking, std::string* err) {
    const auto fail = [&](int code, const std::string& msg) {
        if (err) *err = msg;
        return code;
    };
    if (!child || !data || !scale || !offset || !data_format) return fail(RTO_E_INVALID, "null argument");
    if (capacity < 1 || N < 2 || D < 1) return fail(RTO_E_INVALID, "capacity >= 1, N >= 2 and data_dim >= 1 are required");
    const int64_t N3 = (int64_t)N * N * N;
    if (capacity > (((int64_t)1 << 31) - 1) / N3) return fail(RTO_E_INVALID, "capacity * N^3 must stay below 2^31");
    const int B = fit_basis_of_format(data_format, D);
    if (B < 0)
        return fail(RTO_E_UNSUPPORTED, std::string("the fit takes RGBA and SH trees of basis_dim 1, 4, 9, 16 or 25, not ") + data_format +
                                           " with data_dim " + std::to_string(D));
    const std::string bad = fit_check_rays_call(params, origins, dirs, targets, out, n, opt, grad, stats, capacity * N3 * D);
    if (!bad.empty()) return fail(RTO_E_INVALID, bad);
    if (marking) {
        const std::string bad_t = fit_check_touched(params, origins, dirs, targets, out, n, grad, stats, touched, capacity * N3, D);
        if (!bad_t.empty()) return fail(RTO_E_INVALID, bad_t);
    }
    const std::string links = leaf_weights_check_links(child, capacity, N3);
    if (!links.empty()) return fail(RTO_E_FORMAT, links);
    if (n == 0) return RTO_OK;

    lm::Frame fr;
    fm::Opt o;
    host_frame_and_opt(scale, offset, ndc, opt, fr, o);
    const int nt = (int)std::min<int64_t>(threads <= 0 ? 1 : threads, n);
#define RTO_FIT_CASE(B_) \
    case B_: fit_rays<B_>(child, data, params, N, fr, o, origins, dirs, targets, out, n, nt, grad, stats, marking ? touched : nullptr); break
    switch (B) {
        RTO_FIT_CASE(0);
        RTO_FIT_CASE(1);
        RTO_FIT_CASE(4);
        RTO_FIT_CASE(9);
        RTO_FIT_CASE(16);
        RTO_FIT_CASE(25);
    }
#undef RTO_FIT_CASE
    return RTO_OK;
}

int fit_sgd_step_host(float* params, int64_t* grad, int64_t count, float lr, std::string* err) {
    const auto fail = [&](int code, const std::string& msg) {
        if (err) *err = msg;
        return code;
    };
    if (!params || !grad) return fail(RTO_E_INVALID, "null params or grad");
    if (count < 0) return fail(RTO_E_INVALID, "count must be >= 0");
    if ((uintptr_t)params % 4 != 0 || (uintptr_t)grad % 8 != 0) return fail(RTO_E_INVALID, "params must be 4-byte and grad 8-byte aligned");
    for (int64_t i = 0; i < count; ++i) {
        params[i] = fm::sgd_step(params[i], grad[i], lr);
        grad[i] = 0;
    }
    return RTO_OK;
}

}  // namespace rto
