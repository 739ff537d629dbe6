// median_cut.h -- the deterministic median cut of include/rto.h "quantiser": the arithmetic both implementations share (the key
// of an fp16 value, its exact integer value, the widest axis of a box, the palette entry of a box) and the host twin.
// Plain C++17, no HIP include: g++ compiles host/median_cut.cpp alone (tools/sanitize/run_quantize.sh); the kernels
// (quantize_kernels.hip) include this header for the RTO_MC_HD functions, so both sides run the same statements.
#pragma once
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define RTO_MC_HD __host__ __device__ inline
#else
#define RTO_MC_HD inline
#endif

namespace rto {

constexpr int kMedianCutMaxBits = 16;

// order-preserving key of the fp16 bit pattern h: -0 sorts before +0
RTO_MC_HD uint32_t mc_key(uint32_t h) { return (h & 0x8000u) ? (~h & 0xFFFFu) : (h | 0x8000u); }
RTO_MC_HD uint32_t mc_unkey(uint32_t k) { return (k & 0x8000u) ? (k & 0x7FFFu) : (~k & 0xFFFFu); }
RTO_MC_HD bool mc_finite(uint32_t h) { return (h & 0x7C00u) != 0x7C00u; }

// the finite fp16 value h in units of 2^-24: an integer of magnitude below 2^41
RTO_MC_HD int64_t mc_fixed(uint32_t h) {
    const uint32_t e = (h >> 10) & 31u, f = h & 1023u;
    const int64_t mag = e ? (int64_t)(1024u + f) << (e - 1u) : (int64_t)f;
    return (h & 0x8000u) ? -mag : mag;
}

RTO_MC_HD float mc_bits_float(uint32_t u) { return __builtin_bit_cast(float, u); }
RTO_MC_HD uint32_t mc_float_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

// finite fp16 -> float32, exact
RTO_MC_HD float mc_half_to_float(uint32_t h) {
    const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 31u, f = h & 1023u;
    if (e) return mc_bits_float(s | ((e + 112u) << 23) | (f << 13));
    const float mag = (float)f * 5.9604644775390625e-8f;  // f * 2^-24, exact
    return (h & 0x8000u) ? -mag : mag;
}

// float32 -> fp16, round to nearest even (finite input of magnitude at most 65504)
RTO_MC_HD uint32_t mc_float_to_half(float x) {
    const uint32_t u = mc_float_bits(x), s = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
    if (a >= 0x47800000u) return s | 0x7C00u;  // (2^16 and above: not reached by a mean of fp16 values)
    if (a < 0x38800000u) {                     // below 2^-14: a subnormal half or zero
        if (a < 0x33000000u) return s;         // below 2^-25: rounds to zero (2^-25 itself is a tie to even = 0)
        const uint32_t e = a >> 23, man = (a & 0x7FFFFFu) | 0x800000u, shift = 126u - e;  // 14 .. 24
        const uint32_t q = man >> shift, rem = man & ((1u << shift) - 1u), halfway = 1u << (shift - 1u);
        return s | (q + ((rem > halfway || (rem == halfway && (q & 1u))) ? 1u : 0u));
    }
    const uint32_t v = a - 0x38000000u, q = v >> 13, rem = v & 0x1FFFu;  // exponent rebased, 13 mantissa bits dropped
    return s | (q + ((rem > 0x1000u || (rem == 0x1000u && (q & 1u))) ? 1u : 0u));
}

// the split axis of a box from its minimum and maximum keys per axis: the lowest c with the largest hi[c] - lo[c], one float32
// subtraction each
RTO_MC_HD int mc_widest_axis(const uint32_t lo_key[3], const uint32_t hi_key[3]) {
    int axis = 0;
    float best = mc_half_to_float(mc_unkey(hi_key[0])) - mc_half_to_float(mc_unkey(lo_key[0]));
    for (int c = 1; c < 3; ++c) {
        const float ext = mc_half_to_float(mc_unkey(hi_key[c])) - mc_half_to_float(mc_unkey(lo_key[c]));
        if (ext > best) best = ext, axis = c;
    }
    return axis;
}

// the palette entry of a box: sum = exact sum of mc_fixed over its cnt rows
RTO_MC_HD uint16_t mc_palette_entry(int64_t sum, int64_t cnt) {
    if (cnt <= 0) return 0;
    const double mean = (double)sum / (double)cnt * 5.9604644775390625e-8;
    return (uint16_t)mc_float_to_half((float)mean);
}

// m rows of magnitude max_abs_bits (an fp16 pattern without its sign): could a box sum leave an int64?
inline bool mc_sum_overflows(int64_t m, uint32_t max_abs_bits) {
    return (unsigned __int128)(uint64_t)m * (unsigned __int128)(uint64_t)mc_fixed(max_abs_bits) >= ((unsigned __int128)1 << 63);
}

// The host twin: the definition followed literally (per box a selection by (key, row index), int64 sums).  rows [m][3] fp16
// patterns, palette [2^bits][3], ids [m], host memory.  false with *err set: a null argument, m < 1 or above 2^31 - 1, bits
// outside 1..16, a NaN or an infinity, m * max|value| * 2^24 >= 2^63.
bool median_cut_host(const uint16_t* rows, int64_t m, int bits, uint16_t* palette, uint16_t* ids, std::string* err);

}  // namespace rto
