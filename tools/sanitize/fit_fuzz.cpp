// fit_fuzz.cpp -- the host twin of the tree fit (host/fit_grad.cpp, rto_fit_march.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer (tools/sanitize/run_fit.sh): seeded random small trees (RGBA, SH1, SH4, SH9; shuffled node order;
// NaN / infinite / negative densities in the support and in params) and cameras, degenerate ones included (non-finite and zero
// transforms, inside the box, far away, tiny focal lengths), random options (step_size 0, stop_thresh 0, inverted crop boxes,
// NDC), targets with masked (NaN) pixels, infinite and huge values.  Every call returns; the thread count changes no bit of
// grad, stats or images; internal slots receive no gradient; stats[1] counts the unmasked pixels; a forward-only call writes
// the same images; the step zeroes grad; mutated child arrays are RTO_OK or RTO_E_FORMAT, never a report.  Stand-alone: CPU only.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "host/fit_grad.h"

namespace {

std::mt19937_64 rng;
double U(double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); }
int I(int a, int b) { return std::uniform_int_distribution<int>(a, b)(rng); }
const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

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

float odd_sigma(float sig) {
    switch (I(0, 40)) {
        case 0: return kNaN;
        case 1: return kInf;
        case 2: return -kInf;
        case 3: return -sig;
        case 4: return 1e-7f;
        default: return sig;
    }
}

struct Tree {
    int N, D;
    std::string fmt;
    int64_t cap;
    std::vector<int32_t> child;
    std::vector<uint16_t> data;
    std::vector<float> params;
};

Tree random_tree() {
    Tree t;
    t.N = I(0, 3) ? 2 : 3;
    const int basis[4] = {0, 1, 4, 9};
    const int B = basis[I(0, 3)];
    t.D = B ? 3 * B + 1 : 4;
    t.fmt = B ? "SH" + std::to_string(B) : "RGBA";
    const int N3 = t.N * t.N * t.N, max_depth = I(1, t.N == 2 ? 4 : 2);
    std::vector<std::vector<int64_t>> kids(1, std::vector<int64_t>(N3, 0));  // target node per slot, 0 = leaf
    std::vector<int> depth(1, 0);
    for (size_t n = 0; n < kids.size() && kids.size() < 200; ++n)
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
    t.params.assign((size_t)t.cap * N3 * t.D, 0.f);
    for (int64_t n = 0; n < t.cap; ++n)
        for (int s = 0; s < N3; ++s) {
            const int64_t at = where[n] * N3 + s;
            if (kids[n][s]) t.child[at] = (int32_t)(where[kids[n][s]] - where[n]);
            for (int k = 0; k < t.D - 1; ++k) {
                float v = (float)U(-2, 2);
                const int odd = I(0, 400);
                if (odd == 0) v = kNaN;
                if (odd == 1) v = I(0, 1) ? kInf : -kInf;
                if (odd == 2) v = 3e38f;
                t.params[at * t.D + k] = v;
            }
            const float sig = U(0, 1) < 0.4 ? 0.f : (float)std::exp(U(-6, 8));
            t.data[at * t.D + t.D - 1] = half_bits(odd_sigma(sig));
            t.params[at * t.D + t.D - 1] = odd_sigma(I(0, 6) ? sig * (float)U(0.5, 1.5) : 0.f);  // (the field is what params says)
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
    double p[3];
    for (int i = 0; i < 3; ++i) p[i] = kind == 0 ? U(0.05, 0.95) : kind == 1 ? U(-2000, 2000) : U(-3, 4);
    double f[3] = {0.5 - p[0] + U(-0.3, 0.3), 0.5 - p[1] + U(-0.3, 0.3), 0.5 - p[2] + U(-0.3, 0.3)};
    if (kind == 2) f[0] = f[1] = 0;
    for (int i = 0; i < 3; ++i) f[i] /= scale[i];
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
    if (kind == 3) c.transform[I(0, 11)] = kNaN;
    if (kind == 4) c.transform[I(0, 11)] = I(0, 1) ? kInf : -kInf;
    if (kind == 5)
        for (int i = 0; i < 9; ++i) c.transform[i] = 0.f;
    if (kind == 6) c.fx = -c.fx;
    if (kind == 7) c.fx = 1e-30f;
    if (kind == 8) c.fy = 3e38f;
    if (kind == 9)
        for (int i = 0; i < 9; ++i) c.transform[i] *= 1e20f;
    return c;
}

int fails = 0;
void expect(bool ok, const char* what, int it) {
    if (!ok) {
        std::fprintf(stderr, "FAIL (iteration %d): %s\n", it, what);
        ++fails;
    }
}

bool same_bits(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * 4));
}

}  // namespace

int main(int argc, char** argv) {
    const int iters = argc > 1 ? std::atoi(argv[1]) : 300;
    const uint64_t seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    rng.seed(seed);
    int64_t rays = 0, masked = 0, touched = 0, refused = 0;
    for (int it = 0; it < iters; ++it) {
        Tree t = random_tree();
        const int64_t n_slots = t.cap * t.N * t.N * t.N, count = n_slots * t.D;
        float scale[3], offset[3];
        for (int i = 0; i < 3; ++i) {
            scale[i] = (float)std::exp(U(-3, 3));
            offset[i] = (float)U(0.2, 0.8);
        }
        rto_options o;
        std::memset(&o, 0, sizeof(o));
        o.basis_minmax[1] = RTO_BASIS_MAX - 1;
        const int ok = I(0, 5);
        o.step_size = ok == 0 ? 0.f : ok == 1 ? -1e-4f : (float)std::exp(U(-10, -3));
        o.sigma_thresh = I(0, 5) ? (float)U(0, 0.1) : (float)U(-1, 0);
        o.stop_thresh = I(0, 2) ? (float)U(0, 0.2) : 0.f;
        o.background_brightness = I(0, 3) ? (float)U(0, 1) : (I(0, 1) ? kNaN : 1e30f);
        const bool wide_box = o.step_size >= 1e-4f && I(0, 3) == 0;
        for (int i = 0; i < 3; ++i) {
            o.render_bbox[i] = I(0, 2) ? 0.f : (float)U(wide_box ? -0.05 : 0, 0.6);
            o.render_bbox[i + 3] = I(0, 2) ? 1.f : (float)U(0.3, wide_box ? 1.05 : 1);
        }
        float ndc[3] = {(float)U(4, 64), (float)U(4, 64), (float)U(2, 64)};
        const float* ndc_p = I(0, 5) == 0 ? ndc : nullptr;
        const int n = I(0, 4);
        std::vector<rto_camera> cams((size_t)n);
        std::vector<std::vector<float>> tg((size_t)n), im1((size_t)n), im3((size_t)n), imf((size_t)n);
        std::vector<const float*> tp((size_t)n);
        tp.reserve(1);  // (n == 0: targets is still a pointer)
        std::vector<float*> ip1((size_t)n), ip3((size_t)n), ipf((size_t)n);
        int64_t unmasked = 0;
        for (int f = 0; f < n; ++f) {
            cams[f] = random_camera(scale, offset);
            const size_t px = (size_t)cams[f].width * cams[f].height;
            tg[f].resize(px * 3);
            for (size_t p = 0; p < px; ++p) {
                for (int ch = 0; ch < 3; ++ch) tg[f][p * 3 + ch] = (float)U(0, 1);
                const int odd = I(0, 30);
                if (odd == 0) tg[f][p * 3 + I(0, 2)] = kNaN;  // masked
                if (odd == 1) tg[f][p * 3 + I(0, 2)] = I(0, 1) ? kInf : -3e38f;
                unmasked += odd != 0;
                masked += odd == 0;
            }
            im1[f].assign(px * 3, -7.f);
            im3[f] = imf[f] = im1[f];
            tp[f] = tg[f].data();
            ip1[f] = im1[f].data();
            ip3[f] = I(0, 3) ? im3[f].data() : nullptr;  // (entries of images may be null)
            ipf[f] = imf[f].data();
            rays += (int64_t)px;
        }
        std::vector<int64_t> g1((size_t)count, 0), g3((size_t)count, 0);
        uint64_t s1[2] = {0, 0}, s3[2] = {0, 0}, sf[2] = {0, 0};
        std::string err;
        const auto call = [&](const int32_t* child, float* const* images, int threads, int64_t* grad, uint64_t* stats) {
            return rto::fit_grad_host(child, t.data.data(), t.params.data(), t.cap, t.N, t.D, t.fmt.c_str(), scale, offset, ndc_p, cams.data(),
                                      tp.data(), images, n, &o, threads, grad, stats, &err);
        };
        int rc = call(t.child.data(), ip1.data(), 1, g1.data(), s1);
        expect(rc == RTO_OK, err.c_str(), it);
        rc = call(t.child.data(), ip3.data(), 3, g3.data(), s3);
        expect(rc == RTO_OK && g1 == g3 && s1[0] == s3[0] && s1[1] == s3[1], "the thread count changed grad or stats", it);
        for (int f = 0; f < n; ++f) expect(!ip3[f] || same_bits(im1[f], im3[f]), "the thread count changed an image", it);
        expect(s1[1] == (uint64_t)unmasked, "stats[1] is not the number of unmasked pixels", it);
        rc = call(t.child.data(), ipf.data(), 2, nullptr, sf);
        expect(rc == RTO_OK && sf[0] == s1[0] && sf[1] == s1[1], "a forward-only call gives other stats", it);
        for (int f = 0; f < n; ++f) expect(same_bits(im1[f], imf[f]), "a forward-only call gives another image", it);
        for (int64_t s = 0; s < n_slots; ++s)
            for (int k = 0; k < t.D; ++k) {
                const int64_t g = g1[(size_t)(s * t.D + k)];
                touched += g != 0;
                if (t.child[(size_t)s] != 0) expect(g == 0, "an internal slot carries a gradient", it);
            }
        // the step: every grad word zero afterwards, a parameter without gradient keeps its bits
        std::vector<float> before = t.params;
        rc = rto::fit_sgd_step_host(t.params.data(), g3.data(), count, (float)U(0, 2), &err);
        expect(rc == RTO_OK, err.c_str(), it);
        for (int64_t i = 0; i < count; ++i) {
            expect(g3[(size_t)i] == 0, "the step left a grad word", it);
            if (g1[(size_t)i] == 0 && before[(size_t)i] == before[(size_t)i])
                expect(before[(size_t)i] == t.params[(size_t)i], "a parameter without gradient moved", it);
        }
        // a mutated child array: refused or marched, never a report
        std::vector<int32_t> bad = t.child;
        for (int k = I(1, 3); k > 0; --k)
            bad[(size_t)(U(0, 1) * (double)n_slots) % (size_t)n_slots] =
                I(0, 1) ? 0 : I(0, 3) ? I(-(int)t.cap - 2, (int)t.cap + 2) : I(-2000000000, 2000000000);
        rc = call(bad.data(), ip1.data(), 1, g1.data(), s1);
        expect(rc == RTO_OK || rc == RTO_E_FORMAT, "a mutated child array is neither marched nor refused as malformed", it);
        refused += rc == RTO_E_FORMAT;
    }
    // argument refusals
    {
        const Tree t = random_tree();
        const float one[3] = {1, 1, 1}, zero[3] = {0, 0, 0};
        rto_options o;
        std::memset(&o, 0, sizeof(o));
        o.basis_minmax[1] = RTO_BASIS_MAX - 1;
        o.render_bbox[3] = o.render_bbox[4] = o.render_bbox[5] = 1.f;
        rto_camera c = random_camera(one, zero);
        std::vector<float> tg((size_t)c.width * c.height * 3, 0.5f);
        const float* tp = tg.data();
        std::vector<int64_t> g(t.params.size() + 1, 0);
        uint64_t s[2] = {0, 0};
        std::string err;
        const auto call = [&](const float* params, const rto_camera* cm, const float* const* targets, int n, const rto_options* op, int64_t* grad,
                              uint64_t* stats, const char* fmt) {
            return rto::fit_grad_host(t.child.data(), t.data.data(), params, t.cap, t.N, t.D, fmt, one, zero, nullptr, cm, targets, nullptr, n, op, 1,
                                      grad, stats, &err);
        };
        const char* fmt = t.fmt.c_str();
        expect(call(nullptr, &c, &tp, 1, &o, g.data(), s, fmt) == RTO_E_INVALID, "null params", -1);
        expect(call(t.params.data(), nullptr, &tp, 1, &o, g.data(), s, fmt) == RTO_E_INVALID, "null cams", -1);
        expect(call(t.params.data(), &c, nullptr, 1, &o, g.data(), s, fmt) == RTO_E_INVALID, "null targets", -1);
        expect(call(t.params.data(), &c, &tp, -1, &o, g.data(), s, fmt) == RTO_E_INVALID, "n < 0", -1);
        expect(call(t.params.data(), &c, &tp, 1, nullptr, g.data(), s, fmt) == RTO_E_INVALID, "null options", -1);
        expect(call(t.params.data(), &c, &tp, 1, &o, (int64_t*)((char*)g.data() + 4), s, fmt) == RTO_E_INVALID, "misaligned grad", -1);
        expect(call(t.params.data(), &c, &tp, 1, &o, g.data(), s, "SG4") == RTO_E_UNSUPPORTED, "an SG tree", -1);
        const float* inside = t.params.data();
        expect(call(t.params.data(), &c, &inside, 1, &o, g.data(), s, fmt) == RTO_E_INVALID, "params overlapping a target", -1);
        rto_options r = o;
        r.rot_dirs[1] = 0.5f;
        expect(call(t.params.data(), &c, &tp, 1, &r, g.data(), s, fmt) == RTO_E_INVALID, "rot_dirs set", -1);
        r = o;
        r.basis_minmax[0] = 1;
        expect(call(t.params.data(), &c, &tp, 1, &r, g.data(), s, fmt) == RTO_E_INVALID, "basis_minmax set", -1);
        for (int64_t v : g) expect(v == 0, "a refused call wrote grad", -1);
        expect(s[0] == 0 && s[1] == 0, "a refused call wrote stats", -1);
    }
    std::printf("fit_fuzz: %d iterations (seed %llu), %lld rays (%lld masked), %lld grad words touched, %lld mutated trees refused, %d failures\n",
                iters, (unsigned long long)seed, (long long)rays, (long long)masked, (long long)touched, (long long)refused, fails);
    return fails ? 1 : 0;
}
