// rto_fit_abi.cpp -- C ABI of the tree fit (include/rto.h "tree fit"): the device entries (fit_kernels.hip, fit_rays_kernels.hip,
// fit_sparse_kernels.hip) and the host twins (host/fit_grad.cpp, host/fit_sparse.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>

#include "host/fit_grad.h"
#include "host/fit_sparse.h"
#include "rto_fit_launch.h"
#include "rto_internal.h"

namespace {

// threads per workgroup of the ray kernel: kFitRaysBlock; RTO_FIT_RAYS_BLOCK=128|256 is the measuring hook of
// tools/fit_rays_bench.py (the bytes do not depend on it)
int fit_rays_block() {
    const char* e = std::getenv("RTO_FIT_RAYS_BLOCK");
    const int b = e ? std::atoi(e) : 0;
    return b == 128 || b == 256 ? b : rto::kFitRaysBlock;
}

// RTO_FIT_MARK_NOREAD=1: the marking kernel issues its atomicOr without reading the word first -- the measuring hook of
// tools/fit_sparse_bench.py (the bytes do not depend on it)
bool fit_mark_read() {
    const char* e = std::getenv("RTO_FIT_MARK_NOREAD");
    return !(e && e[0] == '1');
}

// rto_tree_fit_grad_rays and rto_tree_fit_grad_rays_touched (marking: grad and touched required)
int fit_grad_rays_entry(const std::string& w, const rto_tree* tree, const float* params, const float* origins, const float* dirs,
                        const float* targets, float* out, int64_t n, const rto_options* opt, int64_t* grad, uint64_t* stats, uint32_t* touched,
                        bool marking, void* stream) {
    if (!tree) return set_err(RTO_E_INVALID, w + "null tree");
    const rto_tree_info& ti = tree->info;
    const int basis = rto::fit_basis_of_tree(ti.format, ti.basis_dim, ti.data_dim);
    if (basis < 0) return set_err(RTO_E_UNSUPPORTED, w + "the fit takes RGBA and SH trees of basis_dim 1, 4, 9, 16 or 25");
    if (tree->quant) return set_err(RTO_E_UNSUPPORTED, w + "a tree loaded with RTO_TREE_QUANT_DIRECT has no leaf values to fit");
    if (tree->d_recidx) return set_err(RTO_E_UNSUPPORTED, w + "a tree loaded with RTO_TREE_COMPACT_RECORDS is not taken");
    int walk;
    rto::ValuesSrc vs;
    (void)query_plan(tree, false, &walk, &vs);
    if (walk == rto::kWalkChild && !(tree->dev.child && tree->dev.data))
        return set_err(RTO_E_UNSUPPORTED, w + "the tree has neither a traversal image nor child[] / data[] resident");
    const int64_t slots = ti.capacity * tree->dev.N3;
    const int64_t count = slots * ti.data_dim;
    const std::string bad = rto::fit_check_rays_call(params, origins, dirs, targets, out, n, opt, grad, stats, count);
    if (!bad.empty()) return set_err(RTO_E_INVALID, w + bad);
    if (marking) {
        const std::string bad_t = rto::fit_check_touched(params, origins, dirs, targets, out, n, grad, stats, touched, slots, ti.data_dim);
        if (!bad_t.empty()) return set_err(RTO_E_INVALID, w + bad_t);
    }
    const struct {
        const void* p;
        const char* name;
    } mem[8] = {{params, "params"}, {grad, "grad"},       {stats, "stats"}, {origins, "origins"},
                {dirs, "dirs"},     {targets, "targets"}, {out, "out"},     {marking ? touched : nullptr, "touched"}};
    for (const auto& m : mem)
        if (m.p && pointer_device(m.p) != tree->device) return set_err(RTO_E_INVALID, w + m.name + " is not memory of the tree's device");
    if (n == 0) return RTO_OK;
    DeviceGuard guard(tree->device);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    rto::fm::Opt o;
    o.m.step_size = opt->step_size;
    o.m.sigma_thresh = opt->sigma_thresh;
    o.m.stop_thresh = opt->stop_thresh;
    for (int i = 0; i < 6; ++i) o.m.render_bbox[i] = opt->render_bbox[i];
    o.bg = opt->background_brightness;
    // a launch takes at most kFitRaysPerLaunch rays: the pointers advance, so every index inside a launch stays small
    for (int64_t i0 = 0; i0 < n; i0 += rto::kFitRaysPerLaunch) {
        const int64_t k = std::min(n - i0, rto::kFitRaysPerLaunch);
        const uint32_t* node_old = (const uint32_t*)tree->d_node_old;
        const float* tg = targets ? targets + i0 * 3 : nullptr;
        float* ou = out ? out + i0 * 3 : nullptr;
        const hipError_t e =
            marking ? rto::launch_fit_grad_rays_touched(tree->dev, walk, basis, o, node_old, params, origins + i0 * 3, dirs + i0 * 3, tg, ou, k,
                                                        fit_rays_block(), grad, stats, touched, fit_mark_read(), (hipStream_t)stream)
                    : rto::launch_fit_grad_rays(tree->dev, walk, basis, o, node_old, params, origins + i0 * 3, dirs + i0 * 3, tg, ou, k,
                                                fit_rays_block(), grad, stats, (hipStream_t)stream);
        if (e != hipSuccess) return set_err(RTO_E_HIP, w + "launch failed: " + hipGetErrorString(e));
    }
    return RTO_OK;
}

}  // namespace

extern "C" {

int rto_tree_fit_grad(const rto_tree* tree, const float* params, const rto_camera* cams, const float* const* targets, float* const* images,
                      int n, const rto_options* opt, int64_t* grad, uint64_t* stats, void* stream) {
    const std::string w = "rto_tree_fit_grad: ";
    if (!tree) return set_err(RTO_E_INVALID, w + "null tree");
    const rto_tree_info& ti = tree->info;
    const int basis = rto::fit_basis_of_tree(ti.format, ti.basis_dim, ti.data_dim);
    if (basis < 0) return set_err(RTO_E_UNSUPPORTED, w + "the fit takes RGBA and SH trees of basis_dim 1, 4, 9, 16 or 25");
    if (tree->quant) return set_err(RTO_E_UNSUPPORTED, w + "a tree loaded with RTO_TREE_QUANT_DIRECT has no leaf values to fit");
    if (tree->d_recidx) return set_err(RTO_E_UNSUPPORTED, w + "a tree loaded with RTO_TREE_COMPACT_RECORDS is not taken");
    int walk;
    rto::ValuesSrc vs;
    (void)query_plan(tree, false, &walk, &vs);
    if (walk == rto::kWalkChild && !(tree->dev.child && tree->dev.data))
        return set_err(RTO_E_UNSUPPORTED, w + "the tree has neither a traversal image nor child[] / data[] resident");
    const int64_t count = ti.capacity * tree->dev.N3 * ti.data_dim;
    const std::string bad = rto::fit_check_call(params, cams, targets, images, n, opt, grad, stats, count);
    if (!bad.empty()) return set_err(RTO_E_INVALID, w + bad);
    if (pointer_device(params) != tree->device) return set_err(RTO_E_INVALID, w + "params is not memory of the tree's device");
    if (grad && pointer_device(grad) != tree->device) return set_err(RTO_E_INVALID, w + "grad is not memory of the tree's device");
    if (stats && pointer_device(stats) != tree->device) return set_err(RTO_E_INVALID, w + "stats is not memory of the tree's device");
    for (int f = 0; f < n; ++f) {
        if (targets && pointer_device(targets[f]) != tree->device)
            return set_err(RTO_E_INVALID, w + "camera " + std::to_string(f) + ": target is not memory of the tree's device");
        if (images && images[f] && pointer_device(images[f]) != tree->device)
            return set_err(RTO_E_INVALID, w + "camera " + std::to_string(f) + ": image is not memory of the tree's device");
    }
    if (n == 0) return RTO_OK;
    DeviceGuard guard(tree->device);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    rto::fm::Opt o;
    o.m.step_size = opt->step_size;
    o.m.sigma_thresh = opt->sigma_thresh;
    o.m.stop_thresh = opt->stop_thresh;
    for (int i = 0; i < 6; ++i) o.m.render_bbox[i] = opt->render_bbox[i];
    o.bg = opt->background_brightness;
    // a launch takes a run of consecutive cameras of one size, at most kLayerCamChunk of them (the unused slots hold the first)
    for (int f0 = 0; f0 < n;) {
        int k = 1;
        while (k < rto::kLayerCamChunk && f0 + k < n && cams[f0 + k].width == cams[f0].width && cams[f0 + k].height == cams[f0].height) ++k;
        rto::LayerCams lc;
        rto::FitPlanes pl;
        for (int f = 0; f < rto::kLayerCamChunk; ++f) {
            const int g = f0 + (f < k ? f : 0);
            lc.c[f] = cam_dev(cams[g]);
            pl.target[f] = targets ? targets[g] : nullptr;
            pl.image[f] = images ? images[g] : nullptr;
        }
        const hipError_t e = rto::launch_fit_grad(tree->dev, walk, basis, o, lc, pl, k, (const uint32_t*)tree->d_node_old, params, grad, stats,
                                                  (hipStream_t)stream);
        if (e != hipSuccess) return set_err(RTO_E_HIP, w + "launch failed: " + hipGetErrorString(e));
        f0 += k;
    }
    return RTO_OK;
}

int rto_tree_fit_grad_rays(const rto_tree* tree, const float* params, const float* origins, const float* dirs, const float* targets, float* out,
                           int64_t n, const rto_options* opt, int64_t* grad, uint64_t* stats, void* stream) {
    return fit_grad_rays_entry("rto_tree_fit_grad_rays: ", tree, params, origins, dirs, targets, out, n, opt, grad, stats, nullptr, false, stream);
}

int rto_tree_fit_grad_rays_touched(const rto_tree* tree, const float* params, const float* origins, const float* dirs, const float* targets,
                                   float* out, int64_t n, const rto_options* opt, int64_t* grad, uint64_t* stats, uint32_t* touched,
                                   void* stream) {
    return fit_grad_rays_entry("rto_tree_fit_grad_rays_touched: ", tree, params, origins, dirs, targets, out, n, opt, grad, stats, touched, true,
                               stream);
}

int rto_fit_touched_block_words(void) { return rto::kFitTouchedBlockWords; }

int64_t rto_fit_touched_scratch_bytes(int64_t slots) { return rto::fit_touched_scratch_bytes(slots); }

int rto_fit_touched_list(uint32_t* touched, int64_t slots, int clear, uint32_t* list, int64_t list_capacity, uint64_t* count, void* scratch,
                         int64_t scratch_bytes, void* stream) {
    const std::string w = "rto_fit_touched_list: ";
    const std::string bad = rto::fit_check_list_call(touched, slots, list, list_capacity, count, scratch, scratch_bytes, true);
    if (!bad.empty()) return set_err(RTO_E_INVALID, w + bad);
    const int dev = pointer_device(touched);
    if (dev < 0 || pointer_device(count) != dev || pointer_device(scratch) != dev || (list && pointer_device(list) != dev))
        return set_err(RTO_E_INVALID, w + "touched, list, count and scratch must be memory of one device");
    DeviceGuard guard(dev);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    const hipError_t e = rto::launch_fit_touched_list(touched, slots, clear != 0, list, list_capacity, count, (uint32_t*)scratch, (hipStream_t)stream);
    if (e != hipSuccess) return set_err(RTO_E_HIP, w + "launch failed: " + hipGetErrorString(e));
    return RTO_OK;
}

int rto_fit_step_sparse(float* params, int64_t* grad, float* m, float* v, int64_t slots, int row, const uint32_t* list, const uint64_t* count,
                        int64_t list_capacity, const rto_fit_optim* o, void* stream) {
    const std::string w = "rto_fit_step_sparse: ";
    const std::string bad = rto::fit_check_step_call(params, grad, m, v, slots, row, list, count, list_capacity, o);
    if (!bad.empty()) return set_err(RTO_E_INVALID, w + bad);
    const int dev = pointer_device(params);
    const bool has_m = o->kind == RTO_FIT_ADAM, has_v = o->kind != RTO_FIT_SGD;
    if (dev < 0 || pointer_device(grad) != dev || pointer_device(list) != dev || pointer_device(count) != dev ||
        (has_m && pointer_device(m) != dev) || (has_v && pointer_device(v) != dev))
        return set_err(RTO_E_INVALID, w + "params, grad, m, v, list and count must be memory of one device");
    DeviceGuard guard(dev);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    const hipError_t e = rto::launch_fit_step_sparse(params, grad, has_m ? m : nullptr, has_v ? v : nullptr, slots, row, list, count,
                                                     list_capacity, *o, (hipStream_t)stream);
    if (e != hipSuccess) return set_err(RTO_E_HIP, w + "launch failed: " + hipGetErrorString(e));
    return RTO_OK;
}

int rto_fit_sgd_step(float* params, int64_t* grad, int64_t count, float lr, void* stream) {
    const std::string w = "rto_fit_sgd_step: ";
    if (!params || !grad) return set_err(RTO_E_INVALID, w + "null params or grad");
    if (count < 0) return set_err(RTO_E_INVALID, w + "count must be >= 0");
    if ((uintptr_t)params % 4 != 0 || (uintptr_t)grad % 8 != 0) return set_err(RTO_E_INVALID, w + "params must be 4-byte and grad 8-byte aligned");
    const int dev = pointer_device(params);
    if (dev < 0 || pointer_device(grad) != dev) return set_err(RTO_E_INVALID, w + "params and grad must be memory of one device");
    if (count == 0) return RTO_OK;
    DeviceGuard guard(dev);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    const hipError_t e = rto::launch_fit_sgd_step(params, grad, count, lr, (hipStream_t)stream);
    if (e != hipSuccess) return set_err(RTO_E_HIP, w + "launch failed: " + hipGetErrorString(e));
    return RTO_OK;
}

int rto_fit_grad_host(const int32_t* child, const uint16_t* data, const float* params, int64_t capacity, int N, int data_dim,
                      const char* data_format, const float scale[3], const float offset[3], const float* ndc, const rto_camera* cams,
                      const float* const* targets, float* const* images, int n, const rto_options* opt, int threads, int64_t* grad,
                      uint64_t* stats) {
    std::string err;
    const int rc = rto::fit_grad_host(child, data, params, capacity, N, data_dim, data_format, scale, offset, ndc, cams, targets, images, n, opt,
                                      threads, grad, stats, &err);
    if (rc != RTO_OK) return set_err(rc, "rto_fit_grad_host: " + err);
    return RTO_OK;
}

int rto_fit_grad_rays_host(const int32_t* child, const uint16_t* data, const float* params, int64_t capacity, int N, int data_dim,
                           const char* data_format, const float scale[3], const float offset[3], const float* ndc, const float* origins,
                           const float* dirs, const float* targets, float* out, int64_t n, const rto_options* opt, int threads, int64_t* grad,
                           uint64_t* stats) {
    std::string err;
    const int rc = rto::fit_grad_rays_host(child, data, params, capacity, N, data_dim, data_format, scale, offset, ndc, origins, dirs, targets, out,
                                           n, opt, threads, grad, stats, &err);
    if (rc != RTO_OK) return set_err(rc, "rto_fit_grad_rays_host: " + err);
    return RTO_OK;
}

int rto_fit_grad_rays_touched_host(const int32_t* child, const uint16_t* data, const float* params, int64_t capacity, int N, int data_dim,
                                   const char* data_format, const float scale[3], const float offset[3], const float* ndc,
                                   const float* origins, const float* dirs, const float* targets, float* out, int64_t n,
                                   const rto_options* opt, int threads, int64_t* grad, uint64_t* stats, uint32_t* touched) {
    std::string err;
    const int rc = rto::fit_grad_rays_touched_host(child, data, params, capacity, N, data_dim, data_format, scale, offset, ndc, origins, dirs,
                                                   targets, out, n, opt, threads, grad, stats, touched, true, &err);
    if (rc != RTO_OK) return set_err(rc, "rto_fit_grad_rays_touched_host: " + err);
    return RTO_OK;
}

int rto_fit_touched_list_host(uint32_t* touched, int64_t slots, int clear, uint32_t* list, int64_t list_capacity, uint64_t* count) {
    std::string err;
    const int rc = rto::fit_touched_list_host(touched, slots, clear, list, list_capacity, count, &err);
    if (rc != RTO_OK) return set_err(rc, "rto_fit_touched_list_host: " + err);
    return RTO_OK;
}

int rto_fit_step_sparse_host(float* params, int64_t* grad, float* m, float* v, int64_t slots, int row, const uint32_t* list,
                             const uint64_t* count, int64_t list_capacity, const rto_fit_optim* o) {
    std::string err;
    const int rc = rto::fit_step_sparse_host(params, grad, m, v, slots, row, list, count, list_capacity, o, &err);
    if (rc != RTO_OK) return set_err(rc, "rto_fit_step_sparse_host: " + err);
    return RTO_OK;
}

int rto_fit_sgd_step_host(float* params, int64_t* grad, int64_t count, float lr) {
    std::string err;
    const int rc = rto::fit_sgd_step_host(params, grad, count, lr, &err);
    if (rc != RTO_OK) return set_err(rc, "rto_fit_sgd_step_host: " + err);
    return RTO_OK;
}

}  // extern "C"
