// fit_sparse_fuzz.cpp -- the host twins of the sparse step of the tree fit (rto::fit_grad_rays_touched_host of host/fit_grad.cpp;
// rto::fit_touched_list_host and rto::fit_step_sparse_host of host/fit_sparse.cpp over rto_fit_optim.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer (tools/sanitize/run_fit_sparse.sh): seeded random small trees (RGBA, SH1, SH4, SH9; NaN / infinite /
// negative densities) and rays, degenerate and masked ones included.  Per iteration: the marking twin gives the old twin's out,
// grad and stats; the bitmap does not depend on the thread count or on a split over two calls, covers every non-zero grad row and
// no internal slot, and holds no bit at or beyond slots; the list is ascending, complete, cut at its capacity and clears; the
// SGD step over the list leaves the dense step's bytes; RMSProp and Adam steps on random moments (NaN, infinite, negative v
// included) return, change no row that is not listed and zero the listed rows' grad.  Then the refusals.  Stand-alone: CPU only.
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
#include "host/fit_sparse.h"

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

float odd_value(float v) {
    switch (I(0, 60)) {
        case 0: return kNaN;
        case 1: return kInf;
        case 2: return -kInf;
        case 3: return -v;
        default: return v;
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
            for (int k = 0; k < t.D - 1; ++k) t.params[at * t.D + k] = I(0, 400) ? (float)U(-2, 2) : kNaN;
            const float sig = U(0, 1) < 0.4 ? 0.f : (float)std::exp(U(-6, 8));
            t.data[at * t.D + t.D - 1] = half_bits(odd_value(sig));
            t.params[at * t.D + t.D - 1] = odd_value(I(0, 6) ? sig * (float)U(0.5, 1.5) : 0.f);
        }
    return t;
}

void random_ray(const float scale[3], const float offset[3], float* org, float* dir) {
    const int kind = I(0, 12);
    for (int i = 0; i < 3; ++i) {
        const double p = kind == 0 ? U(0.05, 0.95) : U(-3, 4), a = U(0.1, 0.9);
        org[i] = (float)((p - offset[i]) / scale[i]);
        dir[i] = (float)((a - p) / scale[i]);
    }
    if (kind == 1) dir[0] = dir[1] = dir[2] = 0.f;
    if (kind == 2) dir[I(0, 2)] = kNaN;
    if (kind == 3) org[I(0, 2)] = kInf;
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

bool bit(const std::vector<uint32_t>& w, int64_t s) { return (w[(size_t)(s >> 5)] >> (s & 31)) & 1u; }

rto_fit_optim optim(int kind) {
    rto_fit_optim o;
    o.kind = kind;
    o.lr = (float)std::exp(U(-8, 2));
    o.grad_scale = I(0, 3) ? (float)std::exp(U(-8, 2)) : 1.f;
    o.beta1 = (float)U(0, 0.99);
    o.beta2 = (float)U(0, 0.9999);
    o.eps = I(0, 4) ? 1e-8f : 0.f;
    const int t = I(1, 50);
    o.bias1 = (float)(1.0 - std::pow((double)o.beta1, t));
    o.bias2 = (float)(1.0 - std::pow((double)o.beta2, t));
    return o;
}

}  // namespace

int main(int argc, char** argv) {
    const int iters = argc > 1 ? std::atoi(argv[1]) : 300;
    const uint64_t seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    rng.seed(seed);
    int64_t rays = 0, marked = 0, stepped = 0;
    for (int it = 0; it < iters; ++it) {
        const Tree t = random_tree();
        const int64_t slots = t.cap * t.N * t.N * t.N, count = slots * t.D, words = (slots + 31) / 32;
        float scale[3], offset[3];
        for (int i = 0; i < 3; ++i) {
            scale[i] = (float)std::exp(U(-3, 3));
            offset[i] = (float)U(0.2, 0.8);
        }
        rto_options o;
        std::memset(&o, 0, sizeof(o));
        o.basis_minmax[1] = RTO_BASIS_MAX - 1;
        o.step_size = I(0, 5) ? (float)std::exp(U(-10, -3)) : 0.f;
        o.sigma_thresh = (float)U(0, 0.1);
        o.stop_thresh = I(0, 2) ? (float)U(0, 0.2) : 0.f;
        o.background_brightness = (float)U(0, 1);
        for (int i = 0; i < 3; ++i) {
            o.render_bbox[i] = I(0, 2) ? 0.f : (float)U(0, 0.6);
            o.render_bbox[i + 3] = I(0, 2) ? 1.f : (float)U(0.3, 1);
        }
        const int64_t n = I(0, 8) ? I(1, 150) : 0;
        std::vector<float> org((size_t)n * 3 + 1), dir((size_t)n * 3 + 1), tg((size_t)n * 3 + 1);
        for (int64_t r = 0; r < n; ++r) {
            random_ray(scale, offset, &org[(size_t)r * 3], &dir[(size_t)r * 3]);
            for (int ch = 0; ch < 3; ++ch) tg[(size_t)r * 3 + ch] = (float)U(0, 1);
            if (I(0, 30) == 0) tg[(size_t)r * 3 + I(0, 2)] = kNaN;  // masked
        }
        rays += n;
        std::string err;
        const auto call = [&](int64_t r0, int64_t k, float* out, int threads, int64_t* grad, uint64_t* stats, uint32_t* touched, bool marking) {
            return rto::fit_grad_rays_touched_host(t.child.data(), t.data.data(), t.params.data(), t.cap, t.N, t.D, t.fmt.c_str(), scale, offset,
                                                   nullptr, org.data() + r0 * 3, dir.data() + r0 * 3, tg.data() + r0 * 3, out + r0 * 3, k, &o,
                                                   threads, grad, stats, touched, marking, &err);
        };
        std::vector<int64_t> g0((size_t)count, 0), g1((size_t)count, 0), g2((size_t)count, 0);
        uint64_t s0[2] = {0, 0}, s1[2] = {0, 0}, s2[2] = {0, 0};
        std::vector<float> o0((size_t)n * 3 + 1, -7.f), o1 = o0, o2 = o0;
        // (one word more than the bitmap, which must stay clear)
        std::vector<uint32_t> t1((size_t)words + 1, 0u), t2((size_t)words + 1, 0u);
        expect(call(0, n, o0.data(), 2, g0.data(), s0, nullptr, false) == RTO_OK, err.c_str(), it);
        expect(call(0, n, o1.data(), 1, g1.data(), s1, t1.data(), true) == RTO_OK, err.c_str(), it);
        expect(g0 == g1 && s0[0] == s1[0] && s0[1] == s1[1] && same_bits(o0, o1), "the marking twin changed out, grad or stats", it);
        const int64_t cut = n ? I(0, (int)n) : 0;
        expect(call(0, cut, o2.data(), I(2, 9), g2.data(), s2, t2.data(), true) == RTO_OK, err.c_str(), it);
        expect(call(cut, n - cut, o2.data(), I(2, 9), g2.data(), s2, t2.data(), true) == RTO_OK, err.c_str(), it);
        expect(g2 == g1 && t2 == t1 && same_bits(o1, o2), "threads or a split over two calls changed the bitmap, grad or out", it);
        expect(t1[(size_t)words] == 0u, "a word past the bitmap was written", it);
        int64_t set = 0;
        for (int64_t s = 0; s < words * 32; ++s) {
            const bool b = bit(t1, s);
            set += b;
            if (s >= slots) {
                expect(!b, "a bit at or beyond slots is set", it);
                continue;
            }
            if (t.child[(size_t)s] != 0) expect(!b, "an internal slot is marked", it);
            bool any = false;
            for (int k = 0; k < t.D; ++k) any = any || g1[(size_t)(s * t.D + k)] != 0;
            if (any) expect(b, "a slot with a non-zero grad word is not marked", it);
        }
        marked += set;
        // the list: some stray bits beyond slots, which are ignored and cleared
        std::vector<uint32_t> tb = t1;
        tb.resize((size_t)words);
        if (slots % 32 != 0 && I(0, 1)) tb[(size_t)words - 1] |= 0xffffffffu << (slots % 32);
        const int64_t cap = I(0, 2) ? slots : I(0, (int)set);
        std::vector<uint32_t> list((size_t)cap + 1, 0xffffffffu), full((size_t)slots + 1, 0xffffffffu);
        uint64_t c1 = 99, c2 = 99;
        std::vector<uint32_t> keep = tb;
        expect(rto::fit_touched_list_host(keep.data(), slots, 0, full.data(), slots, &c1, &err) == RTO_OK && keep == tb, "the list without clear", it);
        expect(rto::fit_touched_list_host(tb.data(), slots, 1, list.data(), cap, &c2, &err) == RTO_OK, err.c_str(), it);
        expect(c1 == (uint64_t)set && c2 == c1, "the count is not the number of set bits", it);
        for (uint32_t w : tb) expect(w == 0u, "clear left a bit", it);
        for (int64_t j = 0; j < (int64_t)c1; ++j) {
            expect(bit(t1, full[(size_t)j]) && (j == 0 || full[(size_t)j] > full[(size_t)j - 1]), "the list is not the ascending set bits", it);
            if (j < cap) expect(list[(size_t)j] == full[(size_t)j], "the cut list differs", it);
        }
        expect(full[(size_t)c1] == 0xffffffffu && list[(size_t)(cap < (int64_t)c1 ? cap : (int64_t)c1)] == 0xffffffffu, "written past the count", it);
        // the SGD identity
        const float lr = (float)std::exp(U(-3, 8));
        std::vector<float> pd = t.params, ps = t.params;
        std::vector<int64_t> gd = g1, gsp = g1;
        expect(rto::fit_sgd_step_host(pd.data(), gd.data(), count, lr, &err) == RTO_OK, err.c_str(), it);
        rto_fit_optim sgd = optim(RTO_FIT_SGD);
        sgd.lr = lr;
        sgd.grad_scale = 1.f;
        expect(rto::fit_step_sparse_host(ps.data(), gsp.data(), nullptr, nullptr, slots, t.D, full.data(), &c1, slots, &sgd, &err) == RTO_OK,
               err.c_str(), it);
        expect(same_bits(pd, ps) && gsp == gd, "the sparse SGD step does not leave the dense step's bytes", it);
        // RMSProp and Adam on random moments; some list entries beyond slots
        for (int kind = RTO_FIT_RMSPROP; kind <= RTO_FIT_ADAM; ++kind) {
            std::vector<float> p = t.params, m((size_t)count), v((size_t)count);
            for (int64_t i = 0; i < count; ++i) {
                m[(size_t)i] = odd_value((float)U(-1e-3, 1e-3));
                v[(size_t)i] = odd_value((float)std::exp(U(-30, 2)));
            }
            const std::vector<float> p0 = p, m0 = m, v0 = v;
            std::vector<int64_t> g = g1;
            std::vector<uint32_t> l = full;
            l.resize((size_t)c1 + 2);
            l[(size_t)c1] = (uint32_t)slots;
            l[(size_t)c1 + 1] = 0xfffffffeu;
            const uint64_t cl = c1 + 2 + (uint64_t)I(0, 3);  // (a count beyond the capacity is cut)
            const rto_fit_optim ok = optim(kind);
            expect(rto::fit_step_sparse_host(p.data(), g.data(), kind == RTO_FIT_ADAM ? m.data() : nullptr, v.data(), slots, t.D, l.data(), &cl,
                                             (int64_t)c1 + 2, &ok, &err) == RTO_OK, err.c_str(), it);
            for (int64_t s = 0; s < slots; ++s)
                for (int k = 0; k < t.D; ++k) {
                    const size_t i = (size_t)(s * t.D + k);
                    if (bit(t1, s)) {
                        expect(g[i] == 0, "a listed row's grad word was not zeroed", it);
                        ++stepped;
                    } else {
                        expect(!std::memcmp(&p[i], &p0[i], 4) && !std::memcmp(&m[i], &m0[i], 4) && !std::memcmp(&v[i], &v0[i], 4) && g[i] == g1[i],
                               "a row that is not listed changed", it);
                    }
                }
        }
    }
    // argument refusals
    {
        float p[8] = {0}, m[8] = {0}, v[8] = {0};
        int64_t g[8] = {0};
        uint32_t tw[2] = {0, 0}, l[4] = {0, 1, 0, 0};
        uint64_t c[2] = {2, 0};
        std::string err;
        rto_fit_optim o = optim(RTO_FIT_ADAM);
        using rto::fit_step_sparse_host;
        using rto::fit_touched_list_host;
        expect(fit_touched_list_host(nullptr, 8, 0, l, 4, c, &err) == RTO_E_INVALID, "null touched", -1);
        expect(fit_touched_list_host(tw, 8, 0, nullptr, 4, c, &err) == RTO_E_INVALID, "null list", -1);
        expect(fit_touched_list_host(tw, 8, 0, l, 4, nullptr, &err) == RTO_E_INVALID, "null count", -1);
        expect(fit_touched_list_host(tw, -1, 0, l, 4, c, &err) == RTO_E_INVALID, "slots < 0", -1);
        expect(fit_touched_list_host(tw, (int64_t)1 << 31, 0, l, 4, c, &err) == RTO_E_INVALID, "slots >= 2^31", -1);
        expect(fit_touched_list_host(tw, 8, 0, l, -1, c, &err) == RTO_E_INVALID, "list_capacity < 0", -1);
        expect(fit_touched_list_host((uint32_t*)((char*)tw + 2), 8, 0, l, 4, c, &err) == RTO_E_INVALID, "misaligned touched", -1);
        expect(fit_touched_list_host(tw, 8, 0, l, 4, (uint64_t*)((char*)c + 4), &err) == RTO_E_INVALID, "misaligned count", -1);
        expect(rto::fit_touched_scratch_bytes(-1) == -1 && rto::fit_touched_scratch_bytes(0) == 4, "scratch bytes", -1);
        expect(fit_step_sparse_host(nullptr, g, m, v, 2, 4, l, c, 4, &o, &err) == RTO_E_INVALID, "null params", -1);
        expect(fit_step_sparse_host(p, nullptr, m, v, 2, 4, l, c, 4, &o, &err) == RTO_E_INVALID, "null grad", -1);
        expect(fit_step_sparse_host(p, g, nullptr, v, 2, 4, l, c, 4, &o, &err) == RTO_E_INVALID, "null m for Adam", -1);
        expect(fit_step_sparse_host(p, g, m, nullptr, 2, 4, l, c, 4, &o, &err) == RTO_E_INVALID, "null v for Adam", -1);
        expect(fit_step_sparse_host(p, g, m, v, 2, 0, l, c, 4, &o, &err) == RTO_E_INVALID, "row < 1", -1);
        expect(fit_step_sparse_host(p, g, m, v, 2, 4, nullptr, c, 4, &o, &err) == RTO_E_INVALID, "null list", -1);
        expect(fit_step_sparse_host(p, g, m, v, 2, 4, l, nullptr, 4, &o, &err) == RTO_E_INVALID, "null count", -1);
        expect(fit_step_sparse_host(p, g, m, v, 2, 4, l, c, 4, nullptr, &err) == RTO_E_INVALID, "null options", -1);
        expect(fit_step_sparse_host((float*)((char*)p + 2), g, m, v, 2, 4, l, c, 4, &o, &err) == RTO_E_INVALID, "misaligned params", -1);
        o.kind = 3;
        expect(fit_step_sparse_host(p, g, m, v, 2, 4, l, c, 4, &o, &err) == RTO_E_INVALID, "unknown kind", -1);
        for (int i = 0; i < 8; ++i) expect(p[i] == 0.f && m[i] == 0.f && v[i] == 0.f && g[i] == 0, "a refused call wrote", -1);
        // the marking twin's own refusals
        const Tree t = random_tree();
        const float one[3] = {1, 1, 1}, zero[3] = {0, 0, 0};
        rto_options ro;
        std::memset(&ro, 0, sizeof(ro));
        ro.basis_minmax[1] = RTO_BASIS_MAX - 1;
        ro.render_bbox[3] = ro.render_bbox[4] = ro.render_bbox[5] = 1.f;
        std::vector<float> org(12, 0.f), dir(12, 1.f), tg(12, 0.5f), out(12, 0.f);
        std::vector<int64_t> gg(t.params.size(), 0);
        std::vector<uint32_t> tt(t.child.size() / 32 + 2, 0u);
        uint64_t s[2] = {0, 0};
        const auto call = [&](int64_t* grad, uint32_t* touched) {
            return rto::fit_grad_rays_touched_host(t.child.data(), t.data.data(), t.params.data(), t.cap, t.N, t.D, t.fmt.c_str(), one, zero, nullptr,
                                                   org.data(), dir.data(), tg.data(), out.data(), 4, &ro, 1, grad, s, touched, true, &err);
        };
        expect(call(nullptr, tt.data()) == RTO_E_INVALID, "null grad with the bitmap", -1);
        expect(call(gg.data(), nullptr) == RTO_E_INVALID, "null touched", -1);
        expect(call(gg.data(), (uint32_t*)((char*)tt.data() + 1)) == RTO_E_INVALID, "misaligned touched", -1);
        expect(call(gg.data(), (uint32_t*)gg.data()) == RTO_E_INVALID, "touched overlapping grad", -1);
        expect(call(gg.data(), (uint32_t*)out.data()) == RTO_E_INVALID, "touched overlapping out", -1);
        for (float x : out) expect(x == 0.f, "a refused call wrote out", -1);
    }
    std::printf("fit_sparse_fuzz: %d iterations (seed %llu), %lld rays, %lld slots marked, %lld elements stepped, %d failures\n", iters,
                (unsigned long long)seed, (long long)rays, (long long)marked, (long long)stepped, fails);
    return fails ? 1 : 0;
}
