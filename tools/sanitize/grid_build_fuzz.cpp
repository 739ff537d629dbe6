// grid_build_fuzz.cpp -- the host twin of the grid builder (host/grid_build.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer (tools/sanitize/run_grid_build.sh): seeded random grids of L = 1 .. 4 and D = 1 .. 49 with uniform
// regions of every size, every result held to the invariants of the definition (include/rto.h "grid builder") -- the field at
// every voxel, breadth-first links, no uniform node but the root, the counts -- in outputs of exactly the size the count-only
// call reported (a write beyond them is a report), the edge cases, `room` too small and the argument refusals.  Stand-alone,
// CPU only.
//   grid_build_fuzz [iters] [seed]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "host/grid_build.h"

namespace {

int failures = 0;
#define EXPECT(cond, ...)                      \
    do {                                       \
        if (!(cond)) {                         \
            std::fprintf(stderr, "FAIL: ");    \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");        \
            ++failures;                        \
        }                                      \
    } while (0)

struct Grid {
    int L = 1, D = 1;
    std::vector<uint16_t> v;
    int R() const { return 1 << L; }
    uint16_t* at(int x, int y, int z) { return &v[((((size_t)x << L) + (size_t)y) << L) * (size_t)D + (size_t)z * (size_t)D]; }
    const uint16_t* at(int x, int y, int z) const { return const_cast<Grid*>(this)->at(x, y, z); }
};

// a random record per block of a random size at every level, coarse to fine: uniform regions of every size; few values
Grid random_grid(std::mt19937_64& rng, int L, int D) {
    static const uint16_t density[7] = {0x0000, 0x0000, 0x3C00, 0x4900, 0x7E00, 0x8000, 0x7C00};  // 0, 0, 1, 10, NaN, -0, inf
    Grid g;
    g.L = L, g.D = D;
    const int R = g.R();
    g.v.assign((size_t)R * R * R * D, 0);
    std::vector<uint16_t> rec((size_t)D);
    for (int l = 0; l <= L; ++l) {
        const int side = R >> l;  // voxels per cell side
        const uint64_t share = l == 0 ? 1 : 2 + rng() % 4u;
        for (int cx = 0; cx < R; cx += side)
            for (int cy = 0; cy < R; cy += side)
                for (int cz = 0; cz < R; cz += side) {
                    if (l && rng() % share) continue;
                    for (int j = 0; j + 1 < D; ++j) rec[(size_t)j] = (uint16_t)(rng() % 3u ? 0x0000 : 0x3800);
                    rec[(size_t)D - 1] = density[rng() % 7u];
                    for (int x = cx; x < cx + side; ++x)
                        for (int y = cy; y < cy + side; ++y)
                            for (int z = cz; z < cz + side; ++z)
                                for (int j = 0; j < D; ++j) g.at(x, y, z)[j] = rec[(size_t)j];
                }
    }
    return g;
}

struct Result {
    int rc = 0;
    int64_t cap = 0;
    std::vector<int32_t> child;
    std::vector<uint16_t> data;
    rto_grid_build_stats st{};
    std::string err;
};

// count first, then outputs of exactly that many nodes
Result run(const Grid& g, float kill) {
    Result r;
    rto_grid_build_stats counted{};
    r.rc = rto::grid_build_host(g.v.data(), g.L, g.D, kill, nullptr, nullptr, 0, &r.cap, &counted, &r.err);
    if (r.rc != RTO_OK) return r;
    r.child.assign((size_t)r.cap * 8, 0x5A5A5A5A);
    r.data.assign((size_t)r.cap * 8 * (size_t)g.D, 0xABCD);
    int64_t again = 0;
    r.rc = rto::grid_build_host(g.v.data(), g.L, g.D, kill, r.child.data(), r.data.data(), r.cap, &again, &r.st, &r.err);
    EXPECT(again == r.cap && counted.nodes == r.st.nodes && counted.killed == r.st.killed && counted.levels == r.st.levels,
           "the counting call and the writing call disagree");
    return r;
}

void check_valid(const Grid& g, float kill, const char* what, uint64_t it) {
    const int D = g.D, R = g.R();
    const Result r = run(g, kill);
    EXPECT(r.rc == RTO_OK, "%s it %llu: refused: %s", what, (unsigned long long)it, r.err.c_str());
    if (r.rc != RTO_OK) return;
    const unsigned long long id = (unsigned long long)it;
    EXPECT(r.cap >= 1 && r.st.nodes == r.cap && r.st.levels >= 1 && r.st.levels <= g.L, "%s it %llu: counts", what, id);
    const bool killing = !std::isnan(kill);
    const uint32_t th = killing ? rto::simp_thresh_half(kill) : 0;
    // links: breadth-first means the targets of all slots, in node and slot order, are 1, 2, 3, ...; no uniform node but the root
    int64_t expect = 1;
    for (int64_t n = 0; n < r.cap; ++n) {
        bool leaves = true, same = true;
        for (int s = 0; s < 8; ++s) {
            const int32_t c = r.child[(size_t)(n * 8 + s)];
            if (c) {
                EXPECT(n + c == expect, "%s it %llu: node %lld slot %d refers to %lld, not %lld", what, id, (long long)n, s, (long long)(n + c), (long long)expect);
                ++expect;
                EXPECT(rto::simp_rec_zero(&r.data[(size_t)(n * 8 + s) * D], D), "%s it %llu: an interior slot is not zero", what, id);
            }
            leaves = leaves && c == 0;
            same = same && rto::simp_rec_equal(&r.data[(size_t)(n * 8 + s) * D], &r.data[(size_t)(n * 8) * D], D);
        }
        EXPECT(n == 0 || !(leaves && same), "%s it %llu: node %lld is uniform", what, id, (long long)n);
    }
    EXPECT(expect == r.cap, "%s it %llu: %lld nodes are referred to, the tree has %lld", what, id, (long long)expect - 1, (long long)r.cap);
    // the field at every voxel, and the dead ones
    int64_t dead = 0, deepest = 0;
    for (int x = 0; x < R; ++x)
        for (int y = 0; y < R; ++y)
            for (int z = 0; z < R; ++z) {
                int64_t n = 0;
                int l = 0;
                size_t slot = 0;
                for (;; ++l) {
                    const int b = g.L - 1 - l;
                    slot = (size_t)n * 8 + (size_t)((((x >> b) & 1) << 2) | (((y >> b) & 1) << 1) | ((z >> b) & 1));
                    const int32_t c = r.child[slot];
                    if (!c || b == 0) {
                        EXPECT(!c, "%s it %llu: a link below the voxels", what, id);
                        break;
                    }
                    n += c;
                }
                if (l > deepest) deepest = l;
                const uint16_t* in = g.at(x, y, z);
                const bool d = killing && !rto::simp_half_gt(in[D - 1], th);
                dead += d ? 1 : 0;
                const bool ok = d ? rto::simp_rec_zero(&r.data[slot * D], D) : rto::simp_rec_equal(&r.data[slot * D], in, D);
                EXPECT(ok, "%s it %llu: the field differs at voxel %d %d %d", what, id, x, y, z);
            }
    EXPECT(dead == r.st.killed, "%s it %llu: %lld dead voxels, stats say %lld", what, id, (long long)dead, (long long)r.st.killed);
    EXPECT(deepest + 1 == r.st.levels, "%s it %llu: levels", what, id);
    // room too small: refused, the count reported, nothing written
    if (r.cap > 1) {
        std::vector<int32_t> co((size_t)(r.cap - 1) * 8, 7);
        std::vector<uint16_t> dout((size_t)(r.cap - 1) * 8 * (size_t)D, 7);
        int64_t cap = 0;
        std::string err;
        const int rc = rto::grid_build_host(g.v.data(), g.L, D, kill, co.data(), dout.data(), r.cap - 1, &cap, nullptr, &err);
        EXPECT(rc == RTO_E_INVALID && cap == r.cap && !err.empty() && co[0] == 7 && dout[0] == 7, "%s it %llu: room too small", what, id);
    }
}

void check_edges() {
    static const int dims[6] = {1, 4, 5, 13, 28, 49};
    for (const int D : dims)
        for (int L = 1; L <= 3; ++L) {
            Grid g;
            g.L = L, g.D = D;
            g.v.assign(((size_t)1 << (3 * L)) * (size_t)D, 0);
            Result r = run(g, NAN);
            EXPECT(r.rc == RTO_OK && r.cap == 1 && r.st.killed == 0, "the zero grid, L %d D %d", L, D);
            r = run(g, 0.0f);
            EXPECT(r.rc == RTO_OK && r.cap == 1 && r.st.killed == (int64_t)1 << (3 * L), "the zero grid killed, L %d D %d", L, D);
            g.at(g.R() - 1, g.R() - 1, g.R() - 1)[D / 2] = 0x8000;  // -0 in one half of the far corner: a chain of L nodes
            r = run(g, NAN);
            EXPECT(r.rc == RTO_OK && r.cap == L && r.st.levels == L, "the chain, L %d D %d: %lld nodes", L, D, (long long)r.cap);
            check_valid(g, NAN, "chain", (uint64_t)(L * 100 + D));
            for (uint16_t& h : g.v) h = 0x7E00;  // equal NaNs merge
            r = run(g, NAN);
            EXPECT(r.rc == RTO_OK && r.cap == 1, "equal NaN records, L %d D %d", L, D);
        }
}

void check_refusals() {
    Grid g;
    g.L = 1, g.D = 2;
    g.v.assign(16, 0);
    std::vector<int32_t> co(8);
    std::vector<uint16_t> dout(16);
    int64_t cap = 0;
    std::string err;
    const auto call = [&](const uint16_t* grid, int L, int D, int32_t* c, uint16_t* d, int64_t room, int64_t* oc) {
        err.clear();
        return rto::grid_build_host(grid, L, D, NAN, c, d, room, oc, nullptr, &err);
    };
    EXPECT(call(g.v.data(), 1, 2, co.data(), dout.data(), 1, &cap) == RTO_OK && cap == 1, "the smallest grid");
    EXPECT(call(nullptr, 1, 2, co.data(), dout.data(), 1, &cap) == RTO_E_INVALID, "null grid");
    EXPECT(call(g.v.data(), 1, 2, co.data(), dout.data(), 1, nullptr) == RTO_E_INVALID, "null out_capacity");
    EXPECT(call(g.v.data(), 1, 2, co.data(), nullptr, 1, &cap) == RTO_E_INVALID, "one output null");
    EXPECT(call(g.v.data(), 0, 2, co.data(), dout.data(), 1, &cap) == RTO_E_INVALID, "L 0");
    EXPECT(call(g.v.data(), 11, 2, co.data(), dout.data(), 1, &cap) == RTO_E_INVALID, "L 11");
    EXPECT(call(g.v.data(), 1, 0, co.data(), dout.data(), 1, &cap) == RTO_E_INVALID, "D 0");
    EXPECT(call(g.v.data(), 1, 2, co.data(), dout.data(), 0, &cap) == RTO_E_INVALID && cap == 1, "room 0");
    EXPECT(call(g.v.data(), 1, 2, co.data(), dout.data(), -1, &cap) == RTO_E_INVALID, "room -1");
    EXPECT(call(g.v.data(), 1, 2, co.data(), g.v.data() + 2, 1, &cap) == RTO_E_INVALID, "data_out inside the grid");
    EXPECT(call(g.v.data(), 1, 2, reinterpret_cast<int32_t*>(dout.data()), dout.data(), 1, &cap) == RTO_E_INVALID, "the outputs on one buffer");
    EXPECT(call(reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(g.v.data()) + 1), 1, 2, co.data(), dout.data(), 1, &cap) == RTO_E_INVALID,
           "a misaligned grid");
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t iters = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 300;
    const uint64_t seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    std::mt19937_64 rng(seed);
    check_refusals();
    check_edges();
    static const float kills[6] = {NAN, 0.0f, 1.0f, -1.0f, 1e9f, 65504.0f};
    static const int dims[6] = {1, 4, 5, 13, 28, 49};
    for (uint64_t it = 0; it < iters; ++it) {
        const int L = it % 13 == 0 ? 4 : 1 + (int)(rng() % 3u);
        const Grid g = random_grid(rng, L, dims[rng() % 6u]);
        check_valid(g, kills[rng() % 6u], "random", it);
    }
    if (failures) {
        std::fprintf(stderr, "grid_build_fuzz: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("grid_build_fuzz: %llu iterations, seed %llu: ok\n", (unsigned long long)iters, (unsigned long long)seed);
    return 0;
}
