// leaf_weights_fuzz.cpp -- the host twin of the per-leaf peak weights (host/leaf_weights.cpp, rto_leaf_march.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer (tools/sanitize/run_leaf_weights.sh): seeded random small trees (N = 2 and 3,
// shuffled node order, NaN / infinite / negative densities) and cameras, degenerate ones included (non-finite and zero
// transforms, a camera inside the box, far away, behind, negative and tiny focal lengths), random options (step_size 0,
// stop_thresh 0, negative sigma_thresh, inverted and empty crop boxes, NDC).  Every call returns (the march terminates), every
// weight is the bit pattern of a float in [0, 1], internal slots stay 0, the thread count does not change a bit, accumulation
// only raises values; mutated child arrays are RTO_OK or RTO_E_FORMAT, never a report.  A stand-alone program: CPU only.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "host/leaf_weights.h"

namespace {

std::mt19937_64 rng;
double U(double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); }
int I(int a, int b) { return std::uniform_int_distribution<int>(a, b)(rng); }

uint16_t half_bits(float f) {  // round to nearest even; enough range handling for the values drawn here
    uint32_t u;
    std::memcpy(&u, &f, 4);
    const uint32_t s = (u >> 16) & 0x8000u;
    if (f != f) return (uint16_t)(s | 0x7e00u);
    const float a = std::fabs(f);
    if (a >= 65520.f) return (uint16_t)(s | 0x7c00u);
    if (a < 6.103515625e-5f) return (uint16_t)(s | (uint16_t)std::lrint(a * 16777216.f));
    const uint32_t e = ((u >> 23) & 0xffu) - 112u, m = u & 0x7fffffu;
    uint32_t h = (e << 10) | (m >> 13);
    const uint32_t rest = m & 0x1fffu;
    if (rest > 0x1000u || (rest == 0x1000u && (h & 1u))) ++h;
    return (uint16_t)(s | h);
}

struct Tree {
    int N, D;
    int64_t cap;
    std::vector<int32_t> child;
    std::vector<uint16_t> data;
};

Tree random_tree() {
    Tree t;
    t.N = I(0, 3) ? 2 : 3;
    t.D = I(1, 5);
    const int N3 = t.N * t.N * t.N, max_depth = I(1, t.N == 2 ? 4 : 2);
    // nodes in creation order, then a random permutation of all but the root
    std::vector<std::vector<int64_t>> kids(1, std::vector<int64_t>(N3, 0));  // target node per slot, 0 = leaf
    std::vector<int> depth(1, 0);
    for (size_t n = 0; n < kids.size() && kids.size() < 300; ++n)
        for (int s = 0; s < N3; ++s)
            if (depth[n] < max_depth && U(0, 1) < (depth[n] == 0 ? 0.7 : 0.3)) {
                kids[n][s] = (int64_t)kids.size();
                kids.emplace_back(N3, 0);
                depth.push_back(depth[n] + 1);
            }
    t.cap = (int64_t)kids.size();
    std::vector<int64_t> where(t.cap);
    for (int64_t i = 0; i < t.cap; ++i) where[i] = i;
    if (I(0, 1))
        for (int64_t i = t.cap - 1; i > 1; --i) std::swap(where[i], where[1 + (int64_t)(U(0, 1) * (double)i) % i]);
    t.child.assign((size_t)t.cap * N3, 0);
    t.data.assign((size_t)t.cap * N3 * t.D, 0);
    for (int64_t n = 0; n < t.cap; ++n)
        for (int s = 0; s < N3; ++s) {
            const int64_t at = where[n] * N3 + s;
            if (kids[n][s]) t.child[at] = (int32_t)(where[kids[n][s]] - where[n]);
            for (int k = 0; k < t.D; ++k) t.data[at * t.D + k] = half_bits((float)U(-2, 2));
            float sig = U(0, 1) < 0.5 ? 0.f : (float)std::exp(U(-6, 8));
            const int odd = I(0, 40);
            if (odd == 0) sig = std::numeric_limits<float>::quiet_NaN();
            if (odd == 1) sig = std::numeric_limits<float>::infinity();
            if (odd == 2) sig = -std::numeric_limits<float>::infinity();
            if (odd == 3) sig = -sig;
            if (odd == 4) sig = 1e-7f;  // a subnormal half
            t.data[at * t.D + t.D - 1] = half_bits(sig);
        }
    return t;
}

rto_camera random_camera(const float scale[3], const float offset[3]) {
    rto_camera c;
    c.width = I(1, 9);
    c.height = I(1, 7);
    c.fx = (float)(c.width * U(0.3, 3));
    c.fy = I(0, 3) ? c.fx : (float)U(0.5, 20);
    const int kind = I(0, 11);
    // a position in tree space, then to the world; look roughly at the box centre
    double p[3];
    for (int i = 0; i < 3; ++i) p[i] = kind == 0 ? U(0.05, 0.95) : kind == 1 ? U(-2000, 2000) : U(-3, 4);
    double f[3] = {0.5 - p[0] + U(-0.3, 0.3), 0.5 - p[1] + U(-0.3, 0.3), 0.5 - p[2] + U(-0.3, 0.3)};
    if (kind == 2) f[0] = f[1] = 0;  // axis-aligned: zero direction components
    for (int i = 0; i < 3; ++i) f[i] /= scale[i];  // the world direction whose tree-space image points at the box
    double nf = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    if (nf == 0) f[2] = nf = 1;
    double back[3] = {-f[0] / nf, -f[1] / nf, -f[2] / nf};
    double up[3] = {U(-1, 1), U(-1, 1), U(-1, 1)};
    double right[3] = {up[1] * back[2] - up[2] * back[1], up[2] * back[0] - up[0] * back[2], up[0] * back[1] - up[1] * back[0]};
    double nr = std::sqrt(right[0] * right[0] + right[1] * right[1] + right[2] * right[2]);
    if (nr < 1e-9) right[0] = nr = 1;
    for (double& v : right) v /= nr;
    double upv[3] = {back[1] * right[2] - back[2] * right[1], back[2] * right[0] - back[0] * right[2], back[0] * right[1] - back[1] * right[0]};
    for (int i = 0; i < 3; ++i) {
        c.transform[i] = (float)right[i];
        c.transform[3 + i] = (float)upv[i];
        c.transform[6 + i] = (float)back[i];
        c.transform[9 + i] = (float)((p[i] - offset[i]) / scale[i]);
    }
    if (kind == 3) c.transform[I(0, 11)] = std::numeric_limits<float>::quiet_NaN();
    if (kind == 4) c.transform[I(0, 11)] = I(0, 1) ? std::numeric_limits<float>::infinity() : -std::numeric_limits<float>::infinity();
    if (kind == 5)
        for (int i = 0; i < 9; ++i) c.transform[i] = 0.f;  // no direction at all
    if (kind == 6) c.fx = -c.fx;
    if (kind == 7) c.fx = 1e-30f;
    if (kind == 8) c.fy = 3e38f;
    if (kind == 9)
        for (int i = 0; i < 9; ++i) c.transform[i] *= 1e20f;  // a squared length that overflows
    return c;
}

int fails = 0;
void expect(bool ok, const char* what, int it) {
    if (!ok) {
        std::fprintf(stderr, "FAIL (iteration %d): %s\n", it, what);
        ++fails;
    }
}

}  // namespace

int main(int argc, char** argv) {
    const int iters = argc > 1 ? std::atoi(argv[1]) : 300;
    const uint64_t seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    rng.seed(seed);
    int64_t rays = 0, seen = 0, refused = 0;
    for (int it = 0; it < iters; ++it) {
        const Tree t = random_tree();
        const int64_t n_slots = t.cap * t.N * t.N * t.N;
        float scale[3], offset[3];
        for (int i = 0; i < 3; ++i) {
            scale[i] = (float)std::exp(U(-3, 3));
            offset[i] = (float)U(0.2, 0.8);
        }
        rto_options o;
        std::memset(&o, 0, sizeof(o));
        const int ok = I(0, 5);
        o.step_size = ok == 0 ? 0.f : ok == 1 ? -1e-4f : (float)std::exp(U(-10, -3));
        o.sigma_thresh = I(0, 5) ? (float)U(0, 0.1) : (float)U(-1, 0);
        o.stop_thresh = I(0, 2) ? (float)U(0, 0.2) : 0.f;
        const bool wide_box = o.step_size >= 1e-4f && I(0, 3) == 0;  // (a crop box beyond the volume with a zero step is a march of ~1e6 clamped steps per ray)
        for (int i = 0; i < 3; ++i) {
            o.render_bbox[i] = I(0, 2) ? 0.f : (float)U(wide_box ? -0.05 : 0, 0.6);
            o.render_bbox[i + 3] = I(0, 2) ? 1.f : (float)U(0.3, wide_box ? 1.05 : 1);  // (may be inverted or empty)
        }
        float ndc[3] = {(float)U(4, 64), (float)U(4, 64), (float)U(2, 64)};
        const float* ndc_p = I(0, 5) == 0 ? ndc : nullptr;
        std::vector<rto_camera> cams((size_t)I(0, 4));
        for (auto& c : cams) c = random_camera(scale, offset);
        for (const auto& c : cams) rays += (int64_t)c.width * c.height;

        std::vector<uint32_t> w1((size_t)n_slots, 0u), w3((size_t)n_slots, 0u);
        std::string err;
        int rc = rto::leaf_weights_host(t.child.data(), t.data.data(), t.cap, t.N, t.D, scale, offset, ndc_p, cams.data(), (int)cams.size(), &o, 1,
                                        w1.data(), &err);
        expect(rc == RTO_OK, err.c_str(), it);
        rc = rto::leaf_weights_host(t.child.data(), t.data.data(), t.cap, t.N, t.D, scale, offset, ndc_p, cams.data(), (int)cams.size(), &o, 3,
                                    w3.data(), &err);
        expect(rc == RTO_OK && w1 == w3, "the thread count changed the result", it);
        for (int64_t s = 0; s < n_slots; ++s) {
            expect(w1[(size_t)s] <= 0x3f800000u, "a weight outside [0, 1]", it);
            if (t.child[(size_t)s] != 0) expect(w1[(size_t)s] == 0u, "an internal slot carries a weight", it);
            seen += w1[(size_t)s] != 0u;
        }
        // accumulation only raises values, and a second pass over the same cameras changes nothing
        std::vector<uint32_t> acc((size_t)n_slots, 0x3e000000u);  // 0.125
        rc = rto::leaf_weights_host(t.child.data(), t.data.data(), t.cap, t.N, t.D, scale, offset, ndc_p, cams.data(), (int)cams.size(), &o, 2,
                                    acc.data(), &err);
        for (int64_t s = 0; s < n_slots; ++s) expect(acc[(size_t)s] == std::max(w1[(size_t)s], 0x3e000000u), "accumulation is not a max", it);
        // a mutated child array: refused or marched, never a report
        std::vector<int32_t> bad = t.child;
        for (int k = I(1, 3); k > 0; --k) bad[(size_t)(U(0, 1) * (double)n_slots) % (size_t)n_slots] = I(0, 1) ? 0 : I(0, 3) ? I(-(int)t.cap - 2, (int)t.cap + 2) : I(-2000000000, 2000000000);  // (0: a subtree cut off, still a tree)
        std::fill(w3.begin(), w3.end(), 0u);
        rc = rto::leaf_weights_host(bad.data(), t.data.data(), t.cap, t.N, t.D, scale, offset, ndc_p, cams.data(), (int)cams.size(), &o, 1, w3.data(), &err);
        expect(rc == RTO_OK || rc == RTO_E_FORMAT, "a mutated child array is neither marched nor refused as malformed", it);
        refused += rc == RTO_E_FORMAT;
        for (int64_t s = 0; s < n_slots; ++s) expect(w3[(size_t)s] <= 0x3f800000u, "a weight outside [0, 1] (mutated tree)", it);
    }
    // argument refusals
    {
        const Tree t = random_tree();
        const float one[3] = {1, 1, 1}, zero[3] = {0, 0, 0};
        rto_options o;
        std::memset(&o, 0, sizeof(o));
        o.render_bbox[3] = o.render_bbox[4] = o.render_bbox[5] = 1.f;
        rto_camera c = random_camera(one, zero);
        std::vector<uint32_t> w((size_t)(t.cap * t.N * t.N * t.N) + 1, 0u);
        std::string err;
        const auto call = [&](const int32_t* ch, const rto_camera* cm, int n, const rto_options* op, uint32_t* wp, int64_t cap, int N, int D) {
            return rto::leaf_weights_host(ch, t.data.data(), cap, N, D, one, zero, nullptr, cm, n, op, 1, wp, &err);
        };
        expect(call(nullptr, &c, 1, &o, w.data(), t.cap, t.N, t.D) == RTO_E_INVALID, "null child", -1);
        expect(call(t.child.data(), nullptr, 1, &o, w.data(), t.cap, t.N, t.D) == RTO_E_INVALID, "null cams", -1);
        expect(call(t.child.data(), &c, -1, &o, w.data(), t.cap, t.N, t.D) == RTO_E_INVALID, "n < 0", -1);
        expect(call(t.child.data(), &c, 1, nullptr, w.data(), t.cap, t.N, t.D) == RTO_E_INVALID, "null options", -1);
        expect(call(t.child.data(), &c, 1, &o, nullptr, t.cap, t.N, t.D) == RTO_E_INVALID, "null weights", -1);
        expect(call(t.child.data(), &c, 1, &o, (uint32_t*)((char*)w.data() + 1), t.cap, t.N, t.D) == RTO_E_INVALID, "misaligned weights", -1);
        expect(call(t.child.data(), &c, 1, &o, w.data(), 0, t.N, t.D) == RTO_E_INVALID, "capacity 0", -1);
        expect(call(t.child.data(), &c, 1, &o, w.data(), t.cap, 1, t.D) == RTO_E_INVALID, "N 1", -1);
        expect(call(t.child.data(), &c, 1, &o, w.data(), t.cap, t.N, 0) == RTO_E_INVALID, "data_dim 0", -1);
        rto_camera b = c;
        b.width = 0;
        expect(call(t.child.data(), &b, 1, &o, w.data(), t.cap, t.N, t.D) == RTO_E_INVALID, "width 0", -1);
        b = c;
        b.fx = 0.f;
        expect(call(t.child.data(), &b, 1, &o, w.data(), t.cap, t.N, t.D) == RTO_E_INVALID, "fx 0", -1);
        b = c;
        b.fy = std::numeric_limits<float>::quiet_NaN();
        expect(call(t.child.data(), &b, 1, &o, w.data(), t.cap, t.N, t.D) == RTO_E_INVALID, "fy NaN", -1);
        for (uint32_t v : w) expect(v == 0u, "a refused call wrote weights", -1);
    }
    std::printf("leaf_weights_fuzz: %d iterations (seed %llu), %lld rays, %lld weights above 0, %lld mutated trees refused, %d failures\n", iters,
                (unsigned long long)seed, (long long)rays, (long long)seen, (long long)refused, fails);
    return fails ? 1 : 0;
}
