// refine_fuzz.cpp -- the host twin of the tree refiner (host/tree_refine.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer (tools/sanitize/run_refine.sh): seeded random trees of N = 2 and 3, shuffled and padded with
// garbage nodes, random keys, thresholds, budgets and level bounds, every result held to the invariants of the definition
// (include/rto.h "refiner") -- the counts, the order of the selection, slot_src, the field along random slot paths -- and the
// same trees with mutated `child` arrays, which must end in RTO_OK or RTO_E_FORMAT and never in a report of the sanitizers.
// Stand-alone, CPU only.
//   refine_fuzz [iters] [seed]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "host/tree_refine.h"

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
    std::vector<uint32_t> key;
    int64_t cap() const { return (int64_t)child.size() / (N * N * N); }
};

// a random tree: nodes are appended while a random leaf slot of a random earlier node is refined; then the nodes behind the
// root are permuted and garbage nodes appended; keys from a small or a wide set
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
    t.data.resize((size_t)cap * S * D);
    t.key.resize((size_t)cap * S);
    for (int n = 1; n < nodes; ++n) {
        const int64_t p = parent_slot[(size_t)n] / S, s = parent_slot[(size_t)n] % S;
        t.child[(size_t)(place[(size_t)p] * S + s)] = (int32_t)(place[(size_t)n] - place[(size_t)p]);
    }
    for (uint16_t& h : t.data) h = (uint16_t)rng();
    const uint64_t kinds = rng() % 3u;
    for (uint32_t& k : t.key) k = kinds == 0 ? (uint32_t)(rng() % 4u) : kinds == 1 ? 0x3F000000u + (uint32_t)(rng() % 256u) : (uint32_t)rng();
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
    std::vector<int32_t> child, src;
    std::vector<uint16_t> data;
    rto_refine_stats st{};
    std::string err;
};

Result run(const Tree& t, bool with_key, uint32_t thresh, int64_t max_new, int max_level) {
    Result r;
    const size_t S = (size_t)t.N * t.N * t.N;
    const uint32_t* key = with_key ? t.key.data() : nullptr;
    // pass 1 counts; the outputs are then sized exactly, so that a write past the result is a report
    r.rc = rto::tree_refine_host(t.child.data(), t.data.data(), key, t.cap(), t.N, t.D, thresh, max_new, max_level, nullptr, nullptr, 0,
                                 &r.cap, nullptr, &r.st, &r.err);
    if (r.rc != RTO_OK) return r;
    const int64_t counted = r.cap;
    const rto_refine_stats st = r.st;
    r.child.assign((size_t)counted * S, 0x5A5A5A5A);
    r.src.assign((size_t)counted * S, -77);
    r.data.assign((size_t)counted * S * t.D, 0xABCD);
    r.rc = rto::tree_refine_host(t.child.data(), t.data.data(), key, t.cap(), t.N, t.D, thresh, max_new, max_level, r.child.data(),
                                 r.data.data(), counted, &r.cap, r.src.data(), &r.st, &r.err);
    EXPECT(r.rc == RTO_OK && r.cap == counted && r.st.selected == st.selected && r.st.candidates == st.candidates && r.st.levels == st.levels &&
               r.st.cut_key == st.cut_key && r.st.reachable == st.reachable,
           "the writing pass disagrees with the counting pass (rc %d)", r.rc);
    return r;
}

void check_valid(const Tree& t, std::mt19937_64& rng, uint64_t it) {
    const int S = t.N * t.N * t.N;
    const bool with_key = rng() % 4u != 0;
    const uint32_t thresh = rng() % 3u == 0 ? 0u : rng() % 2u ? 1u : t.key[rng() % t.key.size()];
    const int max_level = rng() % 3u == 0 ? 1 + (int)(rng() % 31u) : 31;
    // the candidates by the definition, from the result of an unbounded call
    const Result all = run(t, with_key, thresh, -1, max_level);
    EXPECT(all.rc == RTO_OK, "it %llu: refused: %s", (unsigned long long)it, all.err.c_str());
    if (all.rc != RTO_OK) return;
    const int64_t C = all.st.candidates;
    EXPECT(all.st.selected == C && all.cap == t.cap() + C, "it %llu: the unbounded call does not take every candidate", (unsigned long long)it);
    const int64_t budgets[6] = {0, 1, C - 1, C, C + 1, C ? (int64_t)(rng() % (uint64_t)C) : 0};
    const int64_t max_new = budgets[rng() % 6u];
    const Result r = max_new < 0 ? all : run(t, with_key, thresh, max_new, max_level);
    if (r.rc != RTO_OK) {
        EXPECT(false, "it %llu: budget %lld refused: %s", (unsigned long long)it, (long long)max_new, r.err.c_str());
        return;
    }
    const int64_t K = max_new < 0 ? C : std::min(C, max_new);
    EXPECT(r.st.selected == K && r.cap == t.cap() + K && r.st.candidates == C, "it %llu: K", (unsigned long long)it);
    // the first cap nodes: the input's bytes but for the selected offsets; slot_src the identity
    const size_t old_slots = (size_t)t.cap() * S;
    int64_t j = 0;
    uint32_t smallest = 0xFFFFFFFFu;
    std::vector<char> taken(old_slots, 0);
    for (size_t i = 0; i < old_slots; ++i) {
        EXPECT(r.src[i] == (int32_t)i, "it %llu: slot_src of an old slot", (unsigned long long)it);
        if (r.child[i] == t.child[i]) continue;
        EXPECT(t.child[i] == 0 && (int64_t)(i / S) + r.child[i] == t.cap() + j, "it %llu: a new offset out of order", (unsigned long long)it);
        taken[i] = 1;
        smallest = std::min(smallest, with_key ? t.key[i] : 1u);
        ++j;
    }
    EXPECT(j == K, "it %llu: %lld offsets changed, K = %lld", (unsigned long long)it, (long long)j, (long long)K);
    EXPECT(std::equal(t.data.begin(), t.data.end(), r.data.begin()), "it %llu: old records changed", (unsigned long long)it);
    EXPECT(r.st.cut_key == (K ? (int64_t)smallest : 0), "it %llu: cut_key", (unsigned long long)it);
    // the order: every candidate left out (a slot the unbounded call took) has a smaller key than the cut, or the same key and
    // a larger index than every taken slot of that key
    int64_t last_equal = -1;
    for (size_t i = 0; i < old_slots; ++i)
        if (taken[i] && (with_key ? t.key[i] : 1u) == smallest) last_equal = (int64_t)i;
    for (size_t i = 0; i < old_slots; ++i) {
        if (taken[i] || all.child[i] == t.child[i]) continue;
        const uint32_t k = with_key ? t.key[i] : 1u;
        EXPECT(K == 0 || k < smallest || (k == smallest && (int64_t)i > last_equal), "it %llu: a better candidate was left out", (unsigned long long)it);
    }
    // the new nodes
    for (int64_t m = t.cap(); m < r.cap; ++m)
        for (int s = 0; s < S; ++s) {
            const size_t g = (size_t)(m * S + s);
            const int32_t from = r.src[g];
            const bool ok = r.child[g] == 0 && from >= 0 && (size_t)from < old_slots && taken[(size_t)from] &&
                            (int64_t)(from / S) + r.child[(size_t)from] == m;
            EXPECT(ok, "it %llu: slot_src of a new slot", (unsigned long long)it);
            if (ok) EXPECT(std::equal(&r.data[g * t.D], &r.data[g * t.D] + t.D, &t.data[(size_t)from * t.D]), "it %llu: a new record", (unsigned long long)it);
        }
    // the field along random slot paths
    std::vector<uint16_t> a, b;
    for (int k = 0; k < 100; ++k) {
        std::vector<int> path(12);
        for (int& s : path) s = (int)(rng() % (uint64_t)S);
        int da = 0, db = 0;
        walk(t.child.data(), t.data.data(), S, t.D, path, a, &da);
        walk(r.child.data(), r.data.data(), S, t.D, path, b, &db);
        EXPECT(a == b && db >= da && db <= da + 1 && db < r.st.levels, "it %llu: the field differs along a path", (unsigned long long)it);
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
    const Result r = run(t, rng() & 1u, (uint32_t)(rng() % 3u), (rng() & 1u) ? -1 : (int64_t)(rng() % 50u), 31);
    EXPECT(r.rc == RTO_OK || (r.rc == RTO_E_FORMAT && !r.err.empty()), "mutated it %llu: rc %d (%s)", (unsigned long long)it, r.rc, r.err.c_str());
}

void check_refusals() {
    Tree t;
    t.child.assign(8, 0);
    t.data.assign(8, 0);
    t.key.assign(8, 1);
    std::vector<int32_t> co(9 * 8), ss(9 * 8);
    std::vector<uint16_t> dout(9 * 8);
    int64_t cap = 0;
    std::string err;
    rto_refine_stats st{};
    const auto call = [&](const int32_t* c, const uint16_t* d, const uint32_t* k, int64_t n, int N, int D, int max_level, int32_t* c2, uint16_t* d2,
                          int64_t room, int64_t* oc, int32_t* s2) {
        err.clear();
        return rto::tree_refine_host(c, d, k, n, N, D, 1u, -1, max_level, c2, d2, room, oc, s2, &st, &err);
    };
    const int32_t* c = t.child.data();
    const uint16_t* d = t.data.data();
    EXPECT(call(c, d, t.key.data(), 1, 2, 1, 31, co.data(), dout.data(), 9, &cap, ss.data()) == RTO_OK && cap == 9 && st.levels == 2, "the one-node tree");
    EXPECT(call(c, d, nullptr, 1, 2, 1, 31, nullptr, nullptr, 0, &cap, nullptr) == RTO_OK && cap == 9, "counting only");
    EXPECT(call(c, d, nullptr, 1, 2, 1, 31, co.data(), dout.data(), 8, &cap, nullptr) == RTO_E_INVALID && cap == 9 && st.selected == 8, "room too small");
    EXPECT(call(nullptr, d, nullptr, 1, 2, 1, 31, co.data(), dout.data(), 9, &cap, nullptr) == RTO_E_INVALID, "null child");
    EXPECT(call(c, nullptr, nullptr, 1, 2, 1, 31, co.data(), dout.data(), 9, &cap, nullptr) == RTO_E_INVALID, "null data");
    EXPECT(call(c, d, nullptr, 1, 2, 1, 31, co.data(), nullptr, 9, &cap, nullptr) == RTO_E_INVALID, "null data_out alone");
    EXPECT(call(c, d, nullptr, 1, 2, 1, 31, co.data(), dout.data(), 9, nullptr, nullptr) == RTO_E_INVALID, "null out_capacity");
    EXPECT(call(c, d, nullptr, 0, 2, 1, 31, co.data(), dout.data(), 9, &cap, nullptr) == RTO_E_INVALID, "cap 0");
    EXPECT(call(c, d, nullptr, (int64_t)1 << 28, 2, 1, 31, co.data(), dout.data(), 9, &cap, nullptr) == RTO_E_INVALID, "cap * 8 = 2^31");
    EXPECT(call(c, d, nullptr, 1, 1, 1, 31, co.data(), dout.data(), 9, &cap, nullptr) == RTO_E_INVALID, "N 1");
    EXPECT(call(c, d, nullptr, 1, 1 << 30, 1, 31, co.data(), dout.data(), 9, &cap, nullptr) == RTO_E_INVALID, "N 2^30");
    EXPECT(call(c, d, nullptr, 1, 2, 0, 31, co.data(), dout.data(), 9, &cap, nullptr) == RTO_E_INVALID, "D 0");
    EXPECT(call(c, d, nullptr, 1, 2, 1, 0, co.data(), dout.data(), 9, &cap, nullptr) == RTO_E_INVALID, "max_level 0");
    EXPECT(call(c, d, nullptr, 1, 2, 1, 32, co.data(), dout.data(), 9, &cap, nullptr) == RTO_E_INVALID, "max_level 32");
    EXPECT(call(c, d, nullptr, 1, 2, 1, 31, co.data(), dout.data(), -1, &cap, nullptr) == RTO_E_INVALID, "negative room");
    EXPECT(call(c, d, nullptr, 1, 2, 1, 31, t.child.data(), dout.data(), 1, &cap, nullptr) == RTO_E_INVALID, "child_out == child");
    EXPECT(call(c, d, nullptr, 1, 2, 1, 31, co.data(), t.data.data() + 1, 1, &cap, nullptr) == RTO_E_INVALID, "data_out inside data");
    EXPECT(call(c, d, nullptr, 1, 2, 1, 31, co.data(), dout.data(), 9, &cap, co.data() + 8) == RTO_E_INVALID, "slot_src inside child_out");
    EXPECT(call(c, d, t.key.data(), 1, 2, 1, 31, co.data(), dout.data(), 9, &cap, reinterpret_cast<int32_t*>(t.key.data())) == RTO_E_INVALID,
           "slot_src == key");
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t iters = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 300;
    const uint64_t seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    std::mt19937_64 rng(seed);
    check_refusals();
    static const int dims[5] = {1, 4, 5, 13, 28};
    for (uint64_t it = 0; it < iters; ++it) {
        const int N = it % 7 == 6 ? 3 : 2;
        const int D = dims[rng() % 5u];
        const int nodes = 1 + (int)(rng() % (it % 11 == 0 ? 400u : 40u));
        const Tree t = random_tree(rng, N, D, nodes, (int)(rng() % 4u));
        check_valid(t, rng, it);
        check_mutated(t, rng, it);
    }
    // a chain of 31 nodes below the root is taken (its deepest leaves are no candidates), one of 32 refused
    for (int links = 31; links <= 32; ++links) {
        Tree t;
        t.child.assign((size_t)(links + 1) * 8, 0);
        t.data.assign((size_t)(links + 1) * 8, 0x3C00);
        t.key.assign((size_t)(links + 1) * 8, 1);
        for (int k = 0; k < links; ++k) t.child[(size_t)k * 8 + (size_t)(k % 8)] = 1;
        const Result r = run(t, true, 1, -1, 31);
        EXPECT(r.rc == (links == 31 ? RTO_OK : RTO_E_FORMAT), "chain of %d: rc %d", links, r.rc);
        EXPECT(links != 31 || (r.st.candidates == 31 * 7 && r.st.levels == 32), "chain of 31: the leaves of level 31 were split");
    }
    if (failures) {
        std::fprintf(stderr, "refine_fuzz: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("refine_fuzz: %llu iterations, seed %llu: ok\n", (unsigned long long)iters, (unsigned long long)seed);
    return 0;
}
