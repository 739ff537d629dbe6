// simplify_fuzz.cpp -- the host twin of the tree simplifier (host/tree_simplify.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer (tools/sanitize/run_simplify.sh): seeded random trees of N = 2 and 3, shuffled and padded with
// garbage nodes, every result held to the invariants of the definition (include/rto.h "simplifier") -- the field at every
// leaf of the input, no uniform node left, idempotence -- and the same trees with mutated `child` arrays, which must end in
// RTO_OK or RTO_E_FORMAT and never in a report of the sanitizers.  Stand-alone, CPU only.
//   simplify_fuzz [iters] [seed]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "host/tree_simplify.h"

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

struct Tree {
    int N = 2, D = 1;
    std::vector<int32_t> child;
    std::vector<uint16_t> data;
    int64_t cap() const { return (int64_t)child.size() / (N * N * N); }
};

// a random tree: nodes are appended while a random leaf slot of a random earlier node is refined; few record values, so that
// uniform nodes and cascades are common; then the nodes behind the root are permuted and garbage nodes appended
Tree random_tree(std::mt19937_64& rng, int N, int D, int nodes, int garbage) {
    Tree t;
    t.N = N, t.D = D;
    const int S = N * N * N;
    const int64_t cap = nodes + garbage;
    std::vector<int64_t> parent_slot((size_t)nodes, -1);
    for (int n = 1; n < nodes; ++n)
        for (;;) {
            const int64_t slot = (int64_t)(rng() % (uint64_t)n) * S + (int64_t)(rng() % (uint64_t)S);
            bool taken = false;
            for (int k = 1; k < n && !taken; ++k) taken = parent_slot[(size_t)k] == slot;
            if (!taken) {
                parent_slot[(size_t)n] = slot;
                break;
            }
        }
    std::vector<int64_t> place((size_t)nodes);
    for (int n = 0; n < nodes; ++n) place[(size_t)n] = n;
    for (int n = nodes - 1; n > 1; --n) std::swap(place[(size_t)n], place[(size_t)(1 + rng() % (uint64_t)n)]);
    t.child.assign((size_t)cap * S, 0);
    t.data.assign((size_t)cap * S * D, 0);
    for (int n = 1; n < nodes; ++n) {
        const int64_t p = parent_slot[(size_t)n] / S, s = parent_slot[(size_t)n] % S;
        t.child[(size_t)(place[(size_t)p] * S + s)] = (int32_t)(place[(size_t)n] - place[(size_t)p]);
    }
    static const uint16_t density[6] = {0x0000, 0x0000, 0x3C00, 0x4900, 0x7E00, 0x8000};  // 0, 0, 1, 10, NaN, -0
    for (size_t i = 0; i < (size_t)cap * S; ++i) {
        for (int j = 0; j + 1 < D; ++j) t.data[i * D + j] = (uint16_t)(rng() % 2u ? 0x3800 : 0x0000);
        t.data[i * D + D - 1] = density[rng() % 6u];
    }
    return t;
}

// the leaf record of the slot path `path` (slot per level) in a tree: walks until a leaf; out: D halves
void walk(const int32_t* child, const uint16_t* data, int S, int D, const std::vector<int>& path, std::vector<uint16_t>& out, int* depth) {
    int64_t n = 0;
    for (size_t l = 0;; ++l) {
        const int s = path[l < path.size() ? l : path.size() - 1];
        const int32_t c = child[n * S + s];
        if (!c || l + 1 >= path.size() + 40) {
            out.assign(data + (n * S + s) * D, data + (n * S + s) * D + D);
            *depth = (int)l;
            return;
        }
        n += c;
    }
}

struct Result {
    int rc = 0;
    int64_t cap = 0;
    std::vector<int32_t> child;
    std::vector<uint16_t> data;
    std::vector<int64_t> map;
    rto_simplify_stats st{};
    std::string err;
};

Result run(const Tree& t, float kill) {
    Result r;
    const size_t S = (size_t)t.N * t.N * t.N;
    r.child.assign((size_t)t.cap() * S, 0x5A5A5A5A);
    r.data.assign((size_t)t.cap() * S * t.D, 0xABCD);
    r.map.assign((size_t)t.cap(), -9);
    r.rc = rto::tree_simplify_host(t.child.data(), t.data.data(), t.cap(), t.N, t.D, kill, r.child.data(), r.data.data(), &r.cap,
                                   r.map.data(), &r.st, &r.err);
    return r;
}

void check_valid(const Tree& t, float kill, std::mt19937_64& rng, const char* what, uint64_t it) {
    const int S = t.N * t.N * t.N;
    const Result r = run(t, kill);
    EXPECT(r.rc == RTO_OK, "%s it %llu: refused: %s", what, (unsigned long long)it, r.err.c_str());
    if (r.rc != RTO_OK) return;
    EXPECT(r.cap >= 1 && r.cap <= t.cap() && r.cap == r.st.reachable - r.st.merged, "%s it %llu: capacity %lld", what,
           (unsigned long long)it, (long long)r.cap);
    EXPECT(r.st.reachable + r.st.unreachable == t.cap(), "%s it %llu: reachable + unreachable != cap", what, (unsigned long long)it);
    // node_map ascends; behind the result nothing was written to child_out / node_map guard values beyond cap nodes is not promised
    for (int64_t k = 1; k < r.cap; ++k) EXPECT(r.map[(size_t)k] > r.map[(size_t)k - 1], "%s it %llu: node_map not ascending", what, (unsigned long long)it);
    // links of the output stay inside it, and no surviving non-root node is uniform
    const bool killing = !std::isnan(kill);
    const uint32_t th = killing ? rto::simp_thresh_half(kill) : 0;
    for (int64_t n = 0; n < r.cap; ++n) {
        bool leaves = true, same = true;
        for (int s = 0; s < S; ++s) {
            const int32_t c = r.child[(size_t)(n * S + s)];
            EXPECT(c == 0 || (n + c >= 1 && n + c < r.cap), "%s it %llu: output link outside the output", what, (unsigned long long)it);
            leaves = leaves && c == 0;
            same = same && rto::simp_rec_equal(&r.data[(size_t)(n * S + s) * t.D], &r.data[(size_t)(n * S) * t.D], t.D);
        }
        EXPECT(n == 0 || !(leaves && same), "%s it %llu: node %lld of the output is uniform", what, (unsigned long long)it, (long long)n);
    }
    // the field along random slot paths
    std::vector<uint16_t> a, b;
    for (int k = 0; k < 200; ++k) {
        std::vector<int> path(12);
        for (int& s : path) s = (int)(rng() % (uint64_t)S);
        int da = 0, db = 0;
        walk(t.child.data(), t.data.data(), S, t.D, path, a, &da);
        walk(r.child.data(), r.data.data(), S, t.D, path, b, &db);
        if (killing && !rto::simp_half_gt(a[(size_t)t.D - 1], th)) a.assign((size_t)t.D, 0);
        EXPECT(a == b && db <= da, "%s it %llu: the field differs along a path", what, (unsigned long long)it);
    }
    // idempotence
    Tree again;
    again.N = t.N, again.D = t.D;
    again.child.assign(r.child.begin(), r.child.begin() + r.cap * S);
    again.data.assign(r.data.begin(), r.data.begin() + r.cap * S * t.D);
    const Result r2 = run(again, kill);
    EXPECT(r2.rc == RTO_OK && r2.cap == r.cap && r2.st.merged == 0 && r2.st.unreachable == 0, "%s it %llu: not idempotent", what, (unsigned long long)it);
    if (r2.rc == RTO_OK && r2.cap == r.cap) {
        EXPECT(std::equal(again.child.begin(), again.child.end(), r2.child.begin()) && std::equal(again.data.begin(), again.data.end(), r2.data.begin()),
               "%s it %llu: the second pass changed bytes", what, (unsigned long long)it);
    }
}

void check_mutated(Tree t, std::mt19937_64& rng, uint64_t it) {
    static const int32_t wild[8] = {INT32_MAX, INT32_MIN, -1, 1, 2, -2, 1 << 30, -(1 << 30)};
    const int n_mut = 1 + (int)(rng() % 4u);
    for (int k = 0; k < n_mut; ++k) {
        const size_t i = (size_t)(rng() % (uint64_t)t.child.size());
        const uint64_t how = rng() % 3u;
        t.child[i] = how == 0 ? wild[rng() % 8u] : how == 1 ? (int32_t)(rng() % (uint64_t)(2 * t.cap() + 1)) - (int32_t)t.cap() : (int32_t)rng();
    }
    const Result r = run(t, (rng() & 1u) ? 0.0f : NAN);
    EXPECT(r.rc == RTO_OK || (r.rc == RTO_E_FORMAT && !r.err.empty()), "mutated it %llu: rc %d (%s)", (unsigned long long)it, r.rc, r.err.c_str());
}

void check_refusals() {
    Tree t;
    t.child.assign(8, 0);
    t.data.assign(8, 0);
    std::vector<int32_t> co(8);
    std::vector<uint16_t> dout(8);
    int64_t cap = 0;
    std::string err;
    const auto call = [&](const int32_t* c, const uint16_t* d, int64_t n, int N, int D, int32_t* c2, uint16_t* d2, int64_t* oc) {
        err.clear();
        return rto::tree_simplify_host(c, d, n, N, D, NAN, c2, d2, oc, nullptr, nullptr, &err);
    };
    EXPECT(call(t.child.data(), t.data.data(), 1, 2, 1, co.data(), dout.data(), &cap) == RTO_OK && cap == 1, "the one-node tree");
    EXPECT(call(nullptr, t.data.data(), 1, 2, 1, co.data(), dout.data(), &cap) == RTO_E_INVALID, "null child");
    EXPECT(call(t.child.data(), t.data.data(), 1, 2, 1, co.data(), dout.data(), nullptr) == RTO_E_INVALID, "null out_capacity");
    EXPECT(call(t.child.data(), t.data.data(), 0, 2, 1, co.data(), dout.data(), &cap) == RTO_E_INVALID, "cap 0");
    EXPECT(call(t.child.data(), t.data.data(), (int64_t)1 << 28, 2, 1, co.data(), dout.data(), &cap) == RTO_E_INVALID, "cap * 8 = 2^31");
    EXPECT(call(t.child.data(), t.data.data(), 1, 1, 1, co.data(), dout.data(), &cap) == RTO_E_INVALID, "N 1");
    EXPECT(call(t.child.data(), t.data.data(), 1, 1 << 30, 1, co.data(), dout.data(), &cap) == RTO_E_INVALID, "N 2^30");
    EXPECT(call(t.child.data(), t.data.data(), 1, 2, 0, co.data(), dout.data(), &cap) == RTO_E_INVALID, "D 0");
    EXPECT(call(t.child.data(), t.data.data(), 1, 2, 1, t.child.data(), dout.data(), &cap) == RTO_E_INVALID, "child_out == child");
    EXPECT(call(t.child.data(), t.data.data(), 1, 2, 1, co.data(), t.data.data() + 1, &cap) == RTO_E_INVALID, "data_out inside data");
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t iters = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 300;
    const uint64_t seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    std::mt19937_64 rng(seed);
    check_refusals();
    static const float kills[5] = {NAN, 0.0f, 1.0f, -1.0f, 1e9f};
    static const int dims[5] = {1, 4, 5, 13, 28};
    for (uint64_t it = 0; it < iters; ++it) {
        const int N = it % 7 == 6 ? 3 : 2;
        const int D = dims[rng() % 5u];
        const int nodes = 1 + (int)(rng() % (it % 11 == 0 ? 400u : 40u));
        const Tree t = random_tree(rng, N, D, nodes, (int)(rng() % 4u));
        check_valid(t, kills[rng() % 5u], rng, "random", it);
        check_mutated(t, rng, it);
    }
    // a chain of 31 nodes below the root is taken, one of 32 refused
    for (int links = 31; links <= 32; ++links) {
        Tree t;
        t.child.assign((size_t)(links + 1) * 8, 0);
        t.data.assign((size_t)(links + 1) * 8, 0x3C00);
        for (int k = 0; k < links; ++k) t.child[(size_t)k * 8 + (size_t)(k % 8)] = 1;
        const Result r = run(t, NAN);
        EXPECT(r.rc == (links == 31 ? RTO_OK : RTO_E_FORMAT), "chain of %d: rc %d", links, r.rc);
        EXPECT(links != 31 || (r.cap == 1 && r.st.merged == 31), "chain of 31 does not collapse");
    }
    if (failures) {
        std::fprintf(stderr, "simplify_fuzz: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("simplify_fuzz: %llu iterations, seed %llu: ok\n", (unsigned long long)iters, (unsigned long long)seed);
    return 0;
}
