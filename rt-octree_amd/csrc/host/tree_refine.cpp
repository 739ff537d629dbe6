// tree_refine.cpp -- the host twin of the tree refiner (include/rto.h "refiner"): links and levels as the simplifier's twin walks
// them, the candidates, the first K of them by (key descending, slot ascending), the appended nodes.  No HIP: compiled alone by
// tools/sanitize/run_refine.sh.
#include "host/tree_refine.h"

#include <algorithm>
#include <cstring>
#include <functional>
#include <vector>

namespace rto {

namespace {

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

}  // namespace

std::string refine_check_inputs(const int32_t* child, const uint32_t* key, int64_t cap, int N, int max_level) {
    if (!child) return "null argument";
    if (N < 2) return "N must be at least 2, not " + std::to_string(N);
    if (cap < 1) return "cap must be at least 1, not " + std::to_string(cap);
    if (N > 1290) return "cap * N^3 must stay below 2^31";
    const int64_t S = (int64_t)N * N * N;
    if (cap >= ((int64_t)1 << 31) / S + (((int64_t)1 << 31) % S ? 1 : 0)) return "cap * N^3 must stay below 2^31, cap = " + std::to_string(cap);
    if (max_level < 1 || max_level > kSimplifyMaxLevels - 1)
        return "max_level must lie in 1 .. " + std::to_string(kSimplifyMaxLevels - 1) + ", not " + std::to_string(max_level);
    if ((uintptr_t)child & 3u) return "child is not aligned to 4 bytes";
    if ((uintptr_t)key & 3u) return "key is not aligned to 4 bytes";
    return std::string();
}

std::string refine_check_outputs(const int32_t* child, const uint16_t* data, const uint32_t* key, int64_t cap, int N, int D,
                                 const int32_t* child_out, const uint16_t* data_out, const int32_t* slot_src, int64_t nodes) {
    if (!data || !child_out || !data_out) return "null argument";
    if (D < 1) return "D must be at least 1, not " + std::to_string(D);
    if (nodes < 0) return "room must not be negative";
    if ((uintptr_t)data & 1u) return "data is not aligned to 2 bytes";
    if ((uintptr_t)child_out & 3u) return "child_out is not aligned to 4 bytes";
    if ((uintptr_t)data_out & 1u) return "data_out is not aligned to 2 bytes";
    if ((uintptr_t)slot_src & 3u) return "slot_src is not aligned to 4 bytes";
    const int64_t S = (int64_t)N * N * N;
    if (refine_too_large(nodes, S)) nodes = (((int64_t)1 << 31) - 1) / S;  // (no result is larger: room beyond it is never written)
    const size_t cb = (size_t)cap * S * 4, db = (size_t)cap * S * (size_t)D * 2, kb = key ? cb : 0;
    const size_t ocb = (size_t)nodes * S * 4, odb = (size_t)nodes * S * (size_t)D * 2, osb = slot_src ? ocb : 0;
    const void* in[3] = {child, data, key};
    const size_t in_b[3] = {cb, db, kb};
    const void* out[3] = {child_out, data_out, slot_src};
    const size_t out_b[3] = {ocb, odb, osb};
    for (int o = 0; o < 3; ++o) {
        if (!out_b[o]) continue;
        for (int i = 0; i < 3; ++i)
            if (in_b[i] && ranges_overlap(out[o], out_b[o], in[i], in_b[i])) return "an output overlaps an input";
        for (int p = o + 1; p < 3; ++p)
            if (out_b[p] && ranges_overlap(out[o], out_b[o], out[p], out_b[p])) return "two outputs overlap";
    }
    return std::string();
}

int tree_refine_host(const int32_t* child, const uint16_t* data, const uint32_t* key, int64_t cap, int N, int D, uint32_t key_thresh,
                     int64_t max_new, int max_level, int32_t* child_out, uint16_t* data_out, int64_t room, int64_t* out_capacity,
                     int32_t* slot_src, rto_refine_stats* stats, std::string* err) {
    if (!out_capacity) {
        *err = "null argument";
        return RTO_E_INVALID;
    }
    const bool count_only = !child_out && !data_out;
    std::string bad = refine_check_inputs(child, key, cap, N, max_level);
    if (bad.empty() && count_only && (!data || D < 1)) bad = !data ? "null argument" : "D must be at least 1, not " + std::to_string(D);
    if (bad.empty() && !count_only) bad = refine_check_outputs(child, data, key, cap, N, D, child_out, data_out, slot_src, room);
    if (!bad.empty()) {
        *err = bad;
        return RTO_E_INVALID;
    }
    const int S = N * N * N;
    // 1. links: every slot of every node, bounds-checked before the target is used as an index
    std::vector<int32_t> parent((size_t)cap, -1);
    for (int64_t n = 0; n < cap; ++n)
        for (int s = 0; s < S; ++s) {
            const int32_t c = child[n * S + s];
            if (!c) continue;
            const int64_t t = simp_link_target(n, c, cap);
            const std::string where = "node " + std::to_string(n) + " slot " + std::to_string(s);
            if (t < 0) {
                *err = where + ": offset " + std::to_string(c) + " refers outside [1, " + std::to_string(cap) + ")";
                return RTO_E_FORMAT;
            }
            if (parent[t] >= 0) {
                *err = where + ": node " + std::to_string(t) + " is referred to by more than one slot";
                return RTO_E_FORMAT;
            }
            parent[t] = (int32_t)(n * S + s);
        }
    // levels: the walk from the root, level by level
    std::vector<int32_t> level((size_t)cap, -1), order;
    level[0] = 0;
    order.push_back(0);
    size_t lo = 0;
    int n_levels = 0;
    for (int l = 0;; ++l) {
        const size_t hi = order.size();
        if (lo == hi) break;
        if (l >= kSimplifyMaxLevels) {
            *err = "the walk from the root does not end within " + std::to_string(kSimplifyMaxLevels) + " levels";
            return RTO_E_FORMAT;
        }
        for (size_t i = lo; i < hi; ++i) {
            const int64_t n = order[i];
            for (int s = 0; s < S; ++s)
                if (const int32_t c = child[n * S + s]) {
                    level[n + c] = l + 1;
                    order.push_back((int32_t)(n + c));
                }
        }
        lo = hi;
        n_levels = l + 1;
    }
    const int64_t reachable = (int64_t)order.size();
    // 2. candidates, in slot order
    std::vector<int32_t> cand;
    for (int64_t n = 0; n < cap; ++n) {
        if (level[n] < 0) continue;
        for (int s = 0; s < S; ++s) {
            const int64_t i = n * S + s;
            if (refine_candidate(child[i], level[n], max_level, key ? key[i] : 1u, key_thresh)) cand.push_back((int32_t)i);
        }
    }
    // 3. selection: the K-th largest key is the cut; of the candidates that hold it the first rem in slot order are taken
    const int64_t C = (int64_t)cand.size();
    const int64_t K = max_new < 0 ? C : std::min(C, max_new);
    uint32_t cut_key = 0;
    uint64_t rem = 0;
    if (K > 0) {
        std::vector<uint32_t> keys((size_t)C);
        for (int64_t j = 0; j < C; ++j) keys[(size_t)j] = key ? key[cand[(size_t)j]] : 1u;
        std::nth_element(keys.begin(), keys.begin() + (K - 1), keys.end(), std::greater<uint32_t>());
        cut_key = keys[(size_t)K - 1];
        int64_t above = 0;
        for (int64_t j = 0; j < C; ++j) above += keys[(size_t)j] > cut_key ? 1 : 0;
        rem = (uint64_t)(K - above);
    }
    std::vector<int32_t> sel;  // the selected slots, ascending
    sel.reserve((size_t)K);
    int64_t deepest = n_levels - 1;
    uint64_t eq_rank = 0;
    for (int64_t j = 0; j < C && K > 0; ++j) {
        const int32_t i = cand[(size_t)j];
        const uint32_t k = key ? key[i] : 1u;
        if (refine_selected(k, cut_key, eq_rank, rem)) {
            sel.push_back(i);
            deepest = std::max<int64_t>(deepest, level[i / S] + 1);
        }
        if (k == cut_key) ++eq_rank;
    }
    const int64_t cap_out = cap + K;
    *out_capacity = cap_out;
    if (stats) *stats = rto_refine_stats{reachable, C, K, deepest + 1, (int64_t)cut_key};
    if (refine_too_large(cap_out, S)) {
        *err = "the result's cap * N^3 must stay below 2^31, cap = " + std::to_string(cap_out);
        return RTO_E_INVALID;
    }
    if (count_only) return RTO_OK;
    if (room < cap_out) {
        *err = "room for " + std::to_string(room) + " nodes, the result has " + std::to_string(cap_out);
        return RTO_E_INVALID;
    }
    // 4. the output: the input's bytes, the selected slots' offsets, the appended nodes
    const size_t slots = (size_t)cap * S;
    std::memcpy(child_out, child, slots * 4);
    std::memcpy(data_out, data, slots * (size_t)D * 2);
    if (slot_src)
        for (size_t i = 0; i < slots; ++i) slot_src[i] = (int32_t)i;
    for (int64_t j = 0; j < K; ++j) {
        const int32_t i = sel[(size_t)j];
        const int64_t m = cap + j;
        child_out[i] = (int32_t)(m - i / S);
        for (int s = 0; s < S; ++s) {
            child_out[m * S + s] = 0;
            std::memcpy(data_out + (m * S + s) * D, data + (int64_t)i * D, (size_t)D * 2);
            if (slot_src) slot_src[m * S + s] = i;
        }
    }
    return RTO_OK;
}

}  // namespace rto
