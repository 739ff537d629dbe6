// host/leaf_weights.cpp -- the host twin of rto_tree_leaf_weights: the march of rto_leaf_march.h over child[] / data[] with the
// root-restart float descent, det_expf restated in plain C++.  Same bits as the kernel (tests/test_leaf_weights_gpu.py) and as
// the numpy restatement (tests/leaf_weights_ref.py).  No HIP header.
#include "leaf_weights.h"

#include <cmath>
#include <thread>
#include <vector>

#include "../rto_leaf_march.h"

namespace rto {

std::string leaf_weights_check_cams(const rto_camera* cams, int n, const void* weights) {
    if (n < 0) return "n must be >= 0";
    if (!cams && n > 0) return "null cams with n > 0";
    if (!weights) return "null weights";
    if ((uintptr_t)weights % 4 != 0) return "weights must be 4-byte aligned";
    for (int f = 0; f < n; ++f) {
        const rto_camera& c = cams[f];
        if (c.width < 1 || c.height < 1 || c.height > 65535 * 16 || !std::isfinite(c.fx) || !std::isfinite(c.fy) || c.fx == 0.f || c.fy == 0.f)
            return "camera " + std::to_string(f) + ": width, height (<= 1048560), fx or fy is out of range";
    }
    return "";
}

// every link of the walk from the root stays inside [1, capacity) and no node is reached twice
std::string leaf_weights_check_links(const int32_t* child, int64_t capacity, int64_t N3) {
    std::vector<uint8_t> seen((size_t)capacity, 0);
    std::vector<int64_t> stack{0};
    seen[0] = 1;
    while (!stack.empty()) {
        const int64_t node = stack.back();
        stack.pop_back();
        for (int64_t s = 0; s < N3; ++s) {
            const int64_t c = child[node * N3 + s];
            if (c == 0) continue;
            const int64_t t = node + c;
            if (t < 1 || t >= capacity)
                return "node " + std::to_string(node) + " slot " + std::to_string(s) + ": the offset refers outside [1, " +
                       std::to_string(capacity) + ")";
            if (seen[(size_t)t]) return "node " + std::to_string(t) + " is reached twice by the walk from the root";
            seen[(size_t)t] = 1;
            stack.push_back(t);
        }
    }
    return "";
}

namespace {

void atomic_max_u32(uint32_t* p, uint32_t v) {
    uint32_t cur = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v > cur && !__atomic_compare_exchange_n(p, &cur, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
}

}  // namespace

int leaf_weights_host(const int32_t* child, const uint16_t* data, int64_t capacity, int N, int data_dim, const float scale[3],
                      const float offset[3], const float* ndc, const rto_camera* cams, int n, const rto_options* opt, int threads,
                      uint32_t* weights, std::string* err) {
    const auto fail = [&](int code, const std::string& msg) {
        if (err) *err = msg;
        return code;
    };
    if (!child || !data || !scale || !offset || !opt) return fail(RTO_E_INVALID, "null argument");
    if (capacity < 1 || N < 2 || data_dim < 1) return fail(RTO_E_INVALID, "capacity >= 1, N >= 2 and data_dim >= 1 are required");
    const int64_t N3 = (int64_t)N * N * N;
    if (capacity > (((int64_t)1 << 31) - 1) / N3) return fail(RTO_E_INVALID, "capacity * N^3 must stay below 2^31");
    const std::string bad = leaf_weights_check_cams(cams, n, weights);
    if (!bad.empty()) return fail(RTO_E_INVALID, bad);
    const std::string links = leaf_weights_check_links(child, capacity, N3);
    if (!links.empty()) return fail(RTO_E_FORMAT, links);
    if (n == 0) return RTO_OK;

    lm::Frame fr;
    for (int i = 0; i < 3; ++i) {
        fr.offset[i] = offset[i];
        fr.scale[i] = scale[i];
    }
    fr.ndc_width = ndc && ndc[0] > 0 ? ndc[0] : -1.f;
    fr.ndc_height = ndc ? ndc[1] : 0.f;
    fr.ndc_focal = ndc ? ndc[2] : 0.f;
    lm::Opt o;
    o.step_size = opt->step_size;
    o.sigma_thresh = opt->sigma_thresh;
    o.stop_thresh = opt->stop_thresh;
    for (int i = 0; i < 6; ++i) o.render_bbox[i] = opt->render_bbox[i];

    const auto locate = [&](const float* pos, lm::Leaf& leaf) -> bool {
        for (int i = 0; i < 3; ++i) leaf.local[i] = pos[i];
        const int64_t slot = lm::descend_child(child, N, leaf.local, leaf.cube_sz);
        leaf.index = (uint32_t)slot;
        leaf.sigma_bits = data[slot * data_dim + data_dim - 1];
        return true;
    };
    const auto exp_ = [](float v) -> float { return lm::det_expf(v); };
    const auto update = [&](uint32_t slot, float w) { atomic_max_u32(weights + slot, lm::f_bits(w)); };

    const int nt = threads <= 0 ? 1 : threads;
    for (int f = 0; f < n; ++f) {
        lm::Cam cam;
        cam.width = cams[f].width;
        cam.height = cams[f].height;
        cam.fx = cams[f].fx;
        cam.fy = cams[f].fy;
        for (int i = 0; i < 12; ++i) cam.transform[i] = cams[f].transform[i];
        const auto rows = [&](int k) {
            for (int y = k; y < cam.height; y += nt)
                for (int x = 0; x < cam.width; ++x) lm::march_pixel(fr, o, cam, x, y, locate, exp_, update);
        };
        if (nt == 1) {
            rows(0);
        } else {
            std::vector<std::thread> pool;
            for (int k = 0; k < nt; ++k) pool.emplace_back(rows, k);
            for (auto& t : pool) t.join();
        }
    }
    return RTO_OK;
}

}  // namespace rto
