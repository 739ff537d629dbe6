// fit_rays_fuzz.cpp -- the host twin of the tree fit on rays the caller supplies (rto::fit_grad_rays_host, host/fit_grad.cpp over
// fm::ray_begin_ray / fit_ray of rto_fit_march.h) under AddressSanitizer + UndefinedBehaviorSanitizer
// (tools/sanitize/run_fit_rays.sh): seeded random small trees (RGBA, SH1, SH4, SH9; NaN / infinite / negative densities in the
// support and in params) and rays -- through the box, from inside it, far away, parallel to an axis, of length 1e-30 .. 1e30,
// zero, NaN and infinite directions, non-finite origins --, random options (step_size 0, stop_thresh 0, inverted crop boxes,
// NDC), targets with masked (NaN), infinite and huge values, n = 0.  Every call returns; the thread count, the order of the rays
// and a split over two calls change no bit of grad and stats, and out follows the rays; internal slots receive no gradient;
// stats[1] counts the unmasked rays; a masked ray's out keeps its bytes; a forward-only call writes the same out.
// Stand-alone: CPU only.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
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
    t.child.assign((size_t)t.cap * N3, 0);
    t.data.assign((size_t)t.cap * N3 * t.D, 0);
    t.params.assign((size_t)t.cap * N3 * t.D, 0.f);
    for (int64_t n = 0; n < t.cap; ++n)
        for (int s = 0; s < N3; ++s) {
            const int64_t at = n * N3 + s;
            if (kids[n][s]) t.child[at] = (int32_t)(kids[n][s] - n);
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
            t.params[at * t.D + t.D - 1] = odd_sigma(I(0, 6) ? sig * (float)U(0.5, 1.5) : 0.f);
        }
    return t;
}

// one ray in world space: tree = offset + scale * world
void random_ray(const float scale[3], const float offset[3], float* org, float* dir) {
    const int kind = I(0, 15);
    double p[3], a[3];
    for (int i = 0; i < 3; ++i) {
        p[i] = kind == 0 ? U(0.05, 0.95) : kind == 1 ? U(-2000, 2000) : U(-3, 4);
        a[i] = U(0.1, 0.9);
    }
    for (int i = 0; i < 3; ++i) {
        org[i] = (float)((p[i] - offset[i]) / scale[i]);
        dir[i] = (float)((a[i] - p[i]) / scale[i]);
    }
    if (kind == 2) {  // parallel to an axis
        const int ax = I(0, 2);
        for (int i = 0; i < 3; ++i)
            if (i != ax) dir[i] = 0.f;
    }
    if (kind == 3) dir[0] = dir[1] = dir[2] = 0.f;
    if (kind == 4) dir[I(0, 2)] = kNaN;
    if (kind == 5) dir[I(0, 2)] = I(0, 1) ? kInf : -kInf;
    if (kind == 6) org[I(0, 2)] = I(0, 1) ? kNaN : kInf;
    if (kind == 7 || kind == 8) {
        const float s = kind == 7 ? (float)std::exp(U(-70, -5)) : (float)std::exp(U(5, 70));
        for (int i = 0; i < 3; ++i) dir[i] *= s;
    }
}

int fails = 0;
void expect(bool ok, const char* what, int it) {
    if (!ok) {
        std::fprintf(stderr, "FAIL (iteration %d): %s\n", it, what);
        ++fails;
    }
}

bool same_bits(const float* a, const float* b, size_t count) { return count == 0 || !std::memcmp(a, b, count * 4); }

}  // namespace

int main(int argc, char** argv) {
    const int iters = argc > 1 ? std::atoi(argv[1]) : 300;
    const uint64_t seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    rng.seed(seed);
    int64_t rays = 0, masked = 0, touched = 0;
    for (int it = 0; it < iters; ++it) {
        const Tree t = random_tree();
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
        const int64_t n = I(0, 8) ? I(1, 150) : 0;
        // (+ 1 float: data() of an empty vector may be null, which the entry refuses only for n > 0 -- keep the pointers real)
        std::vector<float> org((size_t)n * 3 + 1), dir((size_t)n * 3 + 1), tg((size_t)n * 3 + 1);
        int64_t unmasked = 0;
        std::vector<char> is_masked((size_t)n, 0);
        for (int64_t r = 0; r < n; ++r) {
            random_ray(scale, offset, &org[(size_t)r * 3], &dir[(size_t)r * 3]);
            for (int ch = 0; ch < 3; ++ch) tg[(size_t)r * 3 + ch] = (float)U(0, 1);
            const int odd = I(0, 30);
            if (odd == 0) tg[(size_t)r * 3 + I(0, 2)] = kNaN;  // masked
            if (odd == 1) tg[(size_t)r * 3 + I(0, 2)] = I(0, 1) ? kInf : -3e38f;
            is_masked[(size_t)r] = odd == 0;
            unmasked += odd != 0;
            masked += odd == 0;
        }
        rays += n;
        std::string err;
        const auto call = [&](const float* og, const float* dr, const float* tp, float* out, int64_t k, int threads, int64_t* grad,
                              uint64_t* stats) {
            return rto::fit_grad_rays_host(t.child.data(), t.data.data(), t.params.data(), t.cap, t.N, t.D, t.fmt.c_str(), scale, offset, ndc_p,
                                           og, dr, tp, out, k, &o, threads, grad, stats, &err);
        };
        std::vector<int64_t> g1((size_t)count, 0), g3((size_t)count, 0), gp((size_t)count, 0), gs((size_t)count, 0);
        uint64_t s1[2] = {0, 0}, s3[2] = {0, 0}, sp[2] = {0, 0}, ss[2] = {0, 0}, sf[2] = {0, 0};
        std::vector<float> o1((size_t)n * 3 + 1, -7.f), o3 = o1, of = o1, os = o1;
        int rc = call(org.data(), dir.data(), tg.data(), o1.data(), n, 1, g1.data(), s1);
        expect(rc == RTO_OK, err.c_str(), it);
        rc = call(org.data(), dir.data(), tg.data(), o3.data(), n, I(2, 9), g3.data(), s3);
        expect(rc == RTO_OK && g1 == g3 && s1[0] == s3[0] && s1[1] == s3[1], "the thread count changed grad or stats", it);
        expect(same_bits(o1.data(), o3.data(), (size_t)n * 3), "the thread count changed out", it);
        expect(s1[1] == (uint64_t)unmasked, "stats[1] is not the number of unmasked rays", it);
        for (int64_t r = 0; r < n; ++r)
            if (is_masked[(size_t)r])
                expect(o1[(size_t)r * 3] == -7.f && o1[(size_t)r * 3 + 1] == -7.f && o1[(size_t)r * 3 + 2] == -7.f, "a masked ray's out was written", it);
        // forward only
        rc = call(org.data(), dir.data(), tg.data(), of.data(), n, 2, nullptr, sf);
        expect(rc == RTO_OK && sf[0] == s1[0] && sf[1] == s1[1] && same_bits(o1.data(), of.data(), (size_t)n * 3),
               "a forward-only call gives other stats or another out", it);
        // a permutation of the rays: the same grad and stats, out follows the rays
        std::vector<int64_t> perm((size_t)n);
        std::iota(perm.begin(), perm.end(), 0);
        std::shuffle(perm.begin(), perm.end(), rng);
        std::vector<float> porg((size_t)n * 3 + 1), pdir((size_t)n * 3 + 1), ptg((size_t)n * 3 + 1), po((size_t)n * 3 + 1, -7.f);
        for (int64_t r = 0; r < n; ++r)
            for (int ch = 0; ch < 3; ++ch) {
                porg[(size_t)r * 3 + ch] = org[(size_t)perm[(size_t)r] * 3 + ch];
                pdir[(size_t)r * 3 + ch] = dir[(size_t)perm[(size_t)r] * 3 + ch];
                ptg[(size_t)r * 3 + ch] = tg[(size_t)perm[(size_t)r] * 3 + ch];
            }
        rc = call(porg.data(), pdir.data(), ptg.data(), po.data(), n, 3, gp.data(), sp);
        expect(rc == RTO_OK && gp == g1 && sp[0] == s1[0] && sp[1] == s1[1], "the order of the rays changed grad or stats", it);
        for (int64_t r = 0; r < n; ++r)
            expect(same_bits(&po[(size_t)r * 3], &o1[(size_t)perm[(size_t)r] * 3], 3), "out does not follow the permuted rays", it);
        // a split over two calls, accumulating
        const int64_t cut = n ? I(0, (int)n) : 0;
        rc = call(org.data(), dir.data(), tg.data(), os.data(), cut, 2, gs.data(), ss);
        expect(rc == RTO_OK, err.c_str(), it);
        rc = call(org.data() + cut * 3, dir.data() + cut * 3, tg.data() + cut * 3, os.data() + cut * 3, n - cut, 2, gs.data(), ss);
        expect(rc == RTO_OK && gs == g1 && ss[0] == s1[0] && ss[1] == s1[1] && same_bits(o1.data(), os.data(), (size_t)n * 3),
               "a split over two calls changed a bit", it);
        for (int64_t s = 0; s < n_slots; ++s)
            for (int k = 0; k < t.D; ++k) {
                const int64_t g = g1[(size_t)(s * t.D + k)];
                touched += g != 0;
                if (t.child[(size_t)s] != 0) expect(g == 0, "an internal slot carries a gradient", it);
            }
    }
    // argument refusals
    {
        const Tree t = random_tree();
        const float one[3] = {1, 1, 1}, zero[3] = {0, 0, 0};
        rto_options o;
        std::memset(&o, 0, sizeof(o));
        o.basis_minmax[1] = RTO_BASIS_MAX - 1;
        o.render_bbox[3] = o.render_bbox[4] = o.render_bbox[5] = 1.f;
        std::vector<float> org(12, 0.f), dir(12, 1.f), tg(12, 0.5f), out(12, 0.f);
        std::vector<int64_t> g(t.params.size() + 1, 0);
        uint64_t s[2] = {0, 0};
        std::string err;
        const auto call = [&](const float* params, const float* og, const float* dr, const float* tp, float* ou, int64_t n, const rto_options* op,
                              int64_t* grad, uint64_t* stats, const char* fmt) {
            return rto::fit_grad_rays_host(t.child.data(), t.data.data(), params, t.cap, t.N, t.D, fmt, one, zero, nullptr, og, dr, tp, ou, n, op,
                                           1, grad, stats, &err);
        };
        const char* fmt = t.fmt.c_str();
        const float* P = t.params.data();
        expect(call(nullptr, org.data(), dir.data(), tg.data(), out.data(), 4, &o, g.data(), s, fmt) == RTO_E_INVALID, "null params", -1);
        expect(call(P, nullptr, dir.data(), tg.data(), out.data(), 4, &o, g.data(), s, fmt) == RTO_E_INVALID, "null origins", -1);
        expect(call(P, org.data(), nullptr, tg.data(), out.data(), 4, &o, g.data(), s, fmt) == RTO_E_INVALID, "null dirs", -1);
        expect(call(P, org.data(), dir.data(), nullptr, out.data(), 4, &o, g.data(), s, fmt) == RTO_E_INVALID, "null targets", -1);
        expect(call(P, org.data(), dir.data(), tg.data(), out.data(), -1, &o, g.data(), s, fmt) == RTO_E_INVALID, "n < 0", -1);
        expect(call(P, org.data(), dir.data(), tg.data(), out.data(), 4, nullptr, g.data(), s, fmt) == RTO_E_INVALID, "null options", -1);
        expect(call(P, org.data(), dir.data(), tg.data(), out.data(), 4, &o, (int64_t*)((char*)g.data() + 4), s, fmt) == RTO_E_INVALID,
               "misaligned grad", -1);
        expect(call(P, (const float*)((const char*)org.data() + 2), dir.data(), tg.data(), out.data(), 3, &o, g.data(), s, fmt) == RTO_E_INVALID,
               "misaligned origins", -1);
        expect(call(P, org.data(), dir.data(), tg.data(), out.data(), 4, &o, g.data(), s, "SG4") == RTO_E_UNSUPPORTED, "an SG tree", -1);
        expect(call(P, org.data(), dir.data(), P, out.data(), 4, &o, g.data(), s, fmt) == RTO_E_INVALID, "params overlapping targets", -1);
        expect(call(P, org.data(), dir.data(), tg.data(), (float*)g.data(), 4, &o, g.data(), s, fmt) == RTO_E_INVALID, "grad overlapping out", -1);
        expect(call(P, org.data(), dir.data(), tg.data(), dir.data() + 3, 3, &o, g.data(), s, fmt) == RTO_E_INVALID, "out overlapping dirs", -1);
        rto_options r = o;
        r.rot_dirs[1] = 0.5f;
        expect(call(P, org.data(), dir.data(), tg.data(), out.data(), 4, &r, g.data(), s, fmt) == RTO_E_INVALID, "rot_dirs set", -1);
        r = o;
        r.basis_minmax[0] = 1;
        expect(call(P, org.data(), dir.data(), tg.data(), out.data(), 4, &r, g.data(), s, fmt) == RTO_E_INVALID, "basis_minmax set", -1);
        for (int64_t v : g) expect(v == 0, "a refused call wrote grad", -1);
        for (float v : out) expect(v == 0.f, "a refused call wrote out", -1);
        expect(s[0] == 0 && s[1] == 0, "a refused call wrote stats", -1);
    }
    std::printf("fit_rays_fuzz: %d iterations (seed %llu), %lld rays (%lld masked), %lld grad words touched, %d failures\n", iters,
                (unsigned long long)seed, (long long)rays, (long long)masked, (long long)touched, fails);
    return fails ? 1 : 0;
}
