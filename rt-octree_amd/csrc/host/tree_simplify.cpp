// tree_simplify.cpp -- the host twin of the tree simplifier (include/rto.h "simplifier"): links, kill, merge, compact, one node
// at a time in the order the definition gives.  No HIP: compiled alone by tools/sanitize/run_simplify.sh.
#include "host/tree_simplify.h"

#include <cmath>
#include <vector>

namespace rto {

namespace {

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

}  // namespace

std::string simplify_check_args(const int32_t* child, const uint16_t* data, int64_t cap, int N, int D, const int32_t* child_out,
                                const uint16_t* data_out, const int64_t* out_capacity, const int64_t* node_map) {
    if (!child || !data || !child_out || !data_out || !out_capacity) return "null argument";
    if (N < 2) return "N must be at least 2, not " + std::to_string(N);
    if (D < 1) return "D must be at least 1, not " + std::to_string(D);
    if (cap < 1) return "cap must be at least 1, not " + std::to_string(cap);
    if (N > 1290) return "cap * N^3 must stay below 2^31";
    const int64_t S = (int64_t)N * N * N;
    if (cap >= ((int64_t)1 << 31) / S + (((int64_t)1 << 31) % S ? 1 : 0)) return "cap * N^3 must stay below 2^31, cap = " + std::to_string(cap);
    if (((uintptr_t)child | (uintptr_t)child_out) & 3u) return "child or child_out is not aligned to 4 bytes";
    if (((uintptr_t)data | (uintptr_t)data_out) & 1u) return "data or data_out is not aligned to 2 bytes";
    if ((uintptr_t)node_map & 7u) return "node_map is not aligned to 8 bytes";
    const size_t cb = (size_t)cap * S * 4, db = (size_t)cap * S * (size_t)D * 2, mb = node_map ? (size_t)cap * 8 : 0;
    const void* in[2] = {child, data};
    const size_t in_b[2] = {cb, db};
    const void* out[3] = {child_out, data_out, node_map};
    const size_t out_b[3] = {cb, db, mb};
    for (int o = 0; o < 3; ++o) {
        if (!out_b[o]) continue;
        for (int i = 0; i < 2; ++i)
            if (ranges_overlap(out[o], out_b[o], in[i], in_b[i])) return "an output overlaps an input";
        for (int p = o + 1; p < 3; ++p)
            if (out_b[p] && ranges_overlap(out[o], out_b[o], out[p], out_b[p])) return "two outputs overlap";
    }
    return std::string();
}

int tree_simplify_host(const int32_t* child, const uint16_t* data, int64_t cap, int N, int D, float kill_thresh, int32_t* child_out,
                       uint16_t* data_out, int64_t* out_capacity, int64_t* node_map, rto_simplify_stats* stats, std::string* err) {
    const std::string bad = simplify_check_args(child, data, cap, N, D, child_out, data_out, out_capacity, node_map);
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
    // levels: the walk from the root, level by level (order[] holds the reachable nodes by level)
    std::vector<int32_t> level((size_t)cap, -1), order;
    std::vector<size_t> level_start;
    level[0] = 0;
    order.push_back(0);
    level_start.push_back(0);
    for (int l = 0;; ++l) {
        const size_t lo = level_start[l], hi = order.size();
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
        level_start.push_back(hi);
    }
    const int n_levels = (int)level_start.size() - 1;  // levels 0 .. n_levels - 1 hold nodes
    const int64_t reachable = (int64_t)order.size();
    std::vector<int32_t> wchild(child, child + (size_t)cap * S), src((size_t)cap * S);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (int32_t)i;
    // 2. kill
    int64_t killed = 0, merged = 0;
    if (!std::isnan(kill_thresh)) {
        const uint32_t th = simp_thresh_half(kill_thresh);
        for (int64_t n = 0; n < cap; ++n) {
            if (level[n] < 0) continue;
            for (int s = 0; s < S; ++s) {
                const int64_t i = n * S + s;
                if (wchild[i] == 0 && !simp_half_gt(data[i * D + D - 1], th)) src[i] = kSimplifyZero, ++killed;
            }
        }
    }
    // 3. merge, deepest level first
    for (int l = n_levels - 1; l >= 1; --l)
        for (size_t i = level_start[l]; i < level_start[l + 1]; ++i) {
            const int64_t n = order[i];
            bool leaves = true;
            for (int s = 0; s < S && leaves; ++s) leaves = wchild[n * S + s] == 0;
            if (!leaves || !simp_node_uniform(data, D, &src[n * S], S)) continue;
            level[n] = -2;
            wchild[parent[n]] = 0;
            src[parent[n]] = src[n * S];
            ++merged;
        }
    // 4. compact
    std::vector<int32_t> newidx((size_t)cap, -1);
    int64_t m = 0, deepest = 0;
    for (int64_t n = 0; n < cap; ++n)
        if (level[n] >= 0) {
            newidx[n] = (int32_t)m++;
            if (level[n] > deepest) deepest = level[n];
        }
    for (int64_t n = 0; n < cap; ++n) {
        if (level[n] < 0) continue;
        const int64_t k = newidx[n];
        if (node_map) node_map[k] = n;
        bool own = true;
        for (int s = 0; s < S; ++s) {
            const int64_t i = n * S + s;
            child_out[k * S + s] = wchild[i] ? newidx[n + wchild[i]] - (int32_t)k : 0;
            own = own && src[i] == (int32_t)i;
        }
        if (own) {
            std::memcpy(data_out + k * S * D, data + n * S * D, (size_t)S * D * 2);
            continue;
        }
        for (int s = 0; s < S; ++s) {
            uint16_t* dst = data_out + (k * S + s) * D;
            const int32_t from = src[n * S + s];
            if (from == kSimplifyZero)
                std::memset(dst, 0, (size_t)D * 2);
            else
                std::memcpy(dst, data + (int64_t)from * D, (size_t)D * 2);
        }
    }
    *out_capacity = m;
    if (stats) *stats = rto_simplify_stats{reachable, cap - reachable, killed, merged, deepest + 1};
    return RTO_OK;
}

}  // namespace rto
