// median_cut.cpp -- the host twin of the quantiser (median_cut.h; the definition: include/rto.h "quantiser").  Serial, plain
// C++17.  Boxes are contiguous segments of a row permutation; a round selects, per box, the first (cnt + 1) / 2 rows in the
// order (key on the split axis, row index) with std::nth_element over 64-bit words key << 32 | row -- a strict total order, so
// the two halves are the definition's whatever the order inside them.
#include "median_cut.h"

#include <algorithm>
#include <vector>

namespace rto {

bool median_cut_host(const uint16_t* rows, int64_t m, int bits, uint16_t* palette, uint16_t* ids, std::string* err) {
    const auto fail = [&](const std::string& msg) {
        if (err) *err = msg;
        return false;
    };
    if (!rows || !palette || !ids) return fail("null argument");
    if (m < 1 || m > (int64_t)INT32_MAX) return fail("m must be in 1 .. 2^31 - 1, not " + std::to_string(m));
    if (bits < 1 || bits > kMedianCutMaxBits) return fail("bits must be in 1 .. 16, not " + std::to_string(bits));
    uint32_t max_abs = 0;
    for (int64_t i = 0; i < 3 * m; ++i) {
        if (!mc_finite(rows[i])) return fail("row " + std::to_string(i / 3) + " holds a NaN or an infinity");
        max_abs = std::max<uint32_t>(max_abs, rows[i] & 0x7FFFu);
    }
    if (mc_sum_overflows(m, max_abs)) return fail("m * max|value| * 2^24 reaches 2^63: a box sum could overflow");

    std::vector<uint32_t> perm((size_t)m), start{0u, (uint32_t)m}, next;
    for (int64_t i = 0; i < m; ++i) perm[(size_t)i] = (uint32_t)i;
    std::vector<uint64_t> words;
    for (int level = 0; level < bits; ++level) {
        const size_t nb = (size_t)1 << level;
        next.assign(2 * nb + 1, 0u);
        for (size_t b = 0; b < nb; ++b) {
            const uint32_t s = start[b], e = start[b + 1], cnt = e - s, half = (cnt + 1) / 2;
            next[2 * b] = s, next[2 * b + 1] = s + half;
            if (cnt < 2) continue;
            uint32_t lo[3] = {0xFFFFu, 0xFFFFu, 0xFFFFu}, hi[3] = {0u, 0u, 0u};
            for (uint32_t p = s; p < e; ++p)
                for (int c = 0; c < 3; ++c) {
                    const uint32_t k = mc_key(rows[(size_t)perm[p] * 3 + c]);
                    lo[c] = std::min(lo[c], k), hi[c] = std::max(hi[c], k);
                }
            const int axis = mc_widest_axis(lo, hi);
            words.resize(cnt);
            for (uint32_t p = s; p < e; ++p) words[p - s] = (uint64_t)mc_key(rows[(size_t)perm[p] * 3 + axis]) << 32 | perm[p];
            std::nth_element(words.begin(), words.begin() + half, words.end());
            for (uint32_t p = s; p < e; ++p) perm[p] = (uint32_t)words[p - s];
        }
        next[2 * nb] = (uint32_t)m;
        start.swap(next);
    }
    const size_t nb = (size_t)1 << bits;
    for (size_t b = 0; b < nb; ++b) {
        int64_t sum[3] = {0, 0, 0};
        for (uint32_t p = start[b]; p < start[b + 1]; ++p) {
            ids[perm[p]] = (uint16_t)b;
            for (int c = 0; c < 3; ++c) sum[c] += mc_fixed(rows[(size_t)perm[p] * 3 + c]);
        }
        for (int c = 0; c < 3; ++c) palette[b * 3 + c] = mc_palette_entry(sum[c], (int64_t)start[b + 1] - start[b]);
    }
    return true;
}

}  // namespace rto
