// quantize_fuzz.cpp -- the host twin of the median-cut quantiser (host/median_cut.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer (tools/sanitize/run_quantize.sh): seeded random and tie-heavy inputs, every result held to the
// invariants of the definition (include/rto.h "quantiser"), and the refusals.  Stand-alone, CPU only.
//   quantize_fuzz [iters] [seed]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "host/median_cut.h"

namespace {

int failures = 0;
#define EXPECT(cond, ...)                   \
    do {                                    \
        if (!(cond)) {                      \
            std::fprintf(stderr, "FAIL: "); \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");     \
            ++failures;                     \
        }                                   \
    } while (0)

uint16_t finite_half(std::mt19937_64& rng) {
    for (;;) {
        const uint16_t h = (uint16_t)rng();
        if (rto::mc_finite(h)) return h;
    }
}

void check(const std::vector<uint16_t>& rows, int bits, const char* what, uint64_t it) {
    const int64_t m = (int64_t)rows.size() / 3;
    const size_t nb = (size_t)1 << bits;
    // guard words around the outputs: the sanitizer sees heap overruns, these see writes to the wrong element
    std::vector<uint16_t> palette(nb * 3, 0xABCD), ids((size_t)m, 0xFFFF);
    std::string err;
    const bool ok = rto::median_cut_host(rows.data(), m, bits, palette.data(), ids.data(), &err);
    EXPECT(ok, "%s it %llu: refused: %s", what, (unsigned long long)it, err.c_str());
    if (!ok) return;
    std::vector<int64_t> cnt(nb, 0), sum(nb * 3, 0);
    for (int64_t i = 0; i < m; ++i) {
        EXPECT(ids[(size_t)i] < nb, "%s it %llu: id %u of row %lld >= 2^%d", what, (unsigned long long)it, ids[(size_t)i], (long long)i, bits);
        if (ids[(size_t)i] >= nb) return;
        ++cnt[ids[(size_t)i]];
        for (int c = 0; c < 3; ++c) sum[(size_t)ids[(size_t)i] * 3 + c] += rto::mc_fixed(rows[(size_t)i * 3 + c]);
    }
    // the counts of every level: siblings differ by at most 1, the lower one never the smaller
    std::vector<int64_t> level(cnt);
    for (int l = bits; l > 0; --l) {
        std::vector<int64_t> up(level.size() / 2);
        for (size_t b = 0; b < up.size(); ++b) {
            EXPECT(level[2 * b] - level[2 * b + 1] == ((level[2 * b] + level[2 * b + 1]) & 1), "%s it %llu: level %d boxes %zu, %zu hold %lld and %lld rows",
                   what, (unsigned long long)it, l, 2 * b, 2 * b + 1, (long long)level[2 * b], (long long)level[2 * b + 1]);
            up[b] = level[2 * b] + level[2 * b + 1];
        }
        level.swap(up);
    }
    EXPECT(level[0] == m, "%s: rows lost", what);
    for (size_t b = 0; b < nb; ++b)
        for (int c = 0; c < 3; ++c) {
            const uint16_t p = palette[b * 3 + c];
            EXPECT(p == rto::mc_palette_entry(sum[b * 3 + c], cnt[b]), "%s it %llu: palette[%zu][%d] = %#06x", what, (unsigned long long)it, b, c, p);
            if (cnt[b] == 0) EXPECT(p == 0, "%s: the palette of an empty box is %#06x", what, p);
        }
    for (int64_t i = 0; i < m; ++i)
        if (cnt[ids[(size_t)i]] == 1)  // the palette of a one-row box is the row (a -0 becomes +0: the sum is an integer)
            for (int c = 0; c < 3; ++c) {
                const uint16_t h = rows[(size_t)i * 3 + c], p = palette[(size_t)ids[(size_t)i] * 3 + c];
                EXPECT(p == (h == 0x8000 ? 0 : h), "%s it %llu: one-row box of row %lld: %#06x != %#06x", what, (unsigned long long)it, (long long)i, p, h);
            }
}

void refusals() {
    std::vector<uint16_t> rows(30, 0x3C00), palette(6), ids(10);
    std::string err;
    const auto refused = [&](const uint16_t* r, int64_t m, int bits, uint16_t* p, uint16_t* i, const char* what) {
        err.clear();
        EXPECT(!rto::median_cut_host(r, m, bits, p, i, &err) && !err.empty(), "%s was not refused", what);
    };
    refused(nullptr, 10, 1, palette.data(), ids.data(), "null rows");
    refused(rows.data(), 10, 1, nullptr, ids.data(), "null palette");
    refused(rows.data(), 10, 1, palette.data(), nullptr, "null ids");
    refused(rows.data(), 0, 1, palette.data(), ids.data(), "m = 0");
    refused(rows.data(), -5, 1, palette.data(), ids.data(), "m < 0");
    refused(rows.data(), (int64_t)1 << 31, 1, palette.data(), ids.data(), "m = 2^31");
    refused(rows.data(), 10, 0, palette.data(), ids.data(), "bits = 0");
    refused(rows.data(), 10, 17, palette.data(), ids.data(), "bits = 17");
    for (uint16_t bad : {(uint16_t)0x7C00, (uint16_t)0xFC00, (uint16_t)0x7E00, (uint16_t)0xFFFF}) {
        rows[17] = bad;
        refused(rows.data(), 10, 1, palette.data(), ids.data(), "a non-finite value");
        rows[17] = 0x3C00;
    }
    // m * 65504 * 2^24 reaches 2^63 from m = 8392707 rows
    const int64_t m = 8392707;
    std::vector<uint16_t> big((size_t)m * 3, 0x3C00), big_ids((size_t)m);
    big[5] = 0xFBFF;
    refused(big.data(), m, 1, palette.data(), big_ids.data(), "a sum that could overflow");
    EXPECT(rto::median_cut_host(big.data(), m - 1, 1, palette.data(), big_ids.data(), &err), "one row below the overflow bound: %s", err.c_str());
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t iters = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 300;
    const uint64_t seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    refusals();
    std::mt19937_64 rng(seed);
    const uint16_t few[] = {0xBC00, 0x8000, 0x0000, 0x3400, 0x7BFF, 0xFBFF, 0x0001, 0x8001};  // -1, -0, +0, 0.25, +-65504, +-2^-24
    for (uint64_t it = 0; it < iters; ++it) {
        const int bits = 1 + (int)(rng() % 16);
        const int64_t m = 1 + (int64_t)(rng() % (it % 16 == 0 ? 70000 : 3000));
        std::vector<uint16_t> rows((size_t)m * 3);
        for (auto& h : rows) h = finite_half(rng);
        check(rows, bits, "random", it);
        const size_t kinds = 1 + rng() % 8;
        for (auto& h : rows) h = few[rng() % kinds];
        check(rows, bits, "tie-heavy", it);
        if (it % 8 == 0) {
            const uint16_t col = finite_half(rng);  // one constant column among random ones
            for (int64_t i = 0; i < m; ++i) rows[(size_t)i * 3] = finite_half(rng), rows[(size_t)i * 3 + 1] = col, rows[(size_t)i * 3 + 2] = (uint16_t)(rng() % 4);
            check(rows, bits, "constant column", it);
        }
    }
    if (failures) {
        std::fprintf(stderr, "quantize_fuzz: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("quantize_fuzz ok: %llu iterations, seed %llu\n", (unsigned long long)iters, (unsigned long long)seed);
    return 0;
}
