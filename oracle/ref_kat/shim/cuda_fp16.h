// Stand-in for NVIDIA's <cuda_fp16.h>, written for oracle/ref_kat only: the few names the reference's host-compilable
// headers use (__half / half as a storage type, __half2float).  IEEE binary16, conversions exact (half -> float) and
// round-to-nearest-even (float -> half).  Nothing here comes from the reference or from the CUDA toolkit.
#ifndef RTO_REF_KAT_SHIM_CUDA_FP16_H
#define RTO_REF_KAT_SHIM_CUDA_FP16_H
#include <cstdint>
#include <cstring>

struct __half {
    uint16_t bits;

    __half() = default;
    explicit __half(float f) : bits(from_float(f)) {}
    operator float() const { return to_float(bits); }

    static float to_float(uint16_t h) {
        const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
        const uint32_t e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
        uint32_t u;
        if (e == 0) {
            if (m == 0) {
                u = sign;
            } else {  // subnormal half: m * 2^-24, normalised for binary32
                int sh = 0;
                uint32_t mm = m;
                while (!(mm & 0x400u)) { mm <<= 1; ++sh; }
                u = sign | ((uint32_t)(113 - sh) << 23) | ((mm & 0x3ffu) << 13);
            }
        } else if (e == 31) {
            u = sign | 0x7f800000u | (m << 13);
        } else {
            u = sign | ((e + 112u) << 23) | (m << 13);
        }
        float f;
        std::memcpy(&f, &u, 4);
        return f;
    }

    static uint16_t from_float(float f) {
        uint32_t u;
        std::memcpy(&u, &f, 4);
        const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
        const uint32_t a = u & 0x7fffffffu;
        if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((a >> 13) & 0x3ffu));  // NaN stays NaN
        if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // >= 65520 rounds to infinity
        if (a < 0x33000001u) return sign;                         // <= 2^-25 rounds to zero (ties to even)
        int e = (int)(a >> 23) - 127;
        uint32_t m = (a & 0x7fffffu) | 0x800000u;  // 24-bit significand
        int shift = e < -14 ? 13 + (-14 - e) : 13;  // bits dropped; a subnormal result drops more
        uint32_t kept = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1u), half_ulp = 1u << (shift - 1);
        if (rem > half_ulp || (rem == half_ulp && (kept & 1u))) ++kept;
        // kept carries the implicit bit for normal results: adding the biased exponent minus one lets a rounding carry
        // move into the exponent field on its own
        const uint32_t h = e < -14 ? kept : (((uint32_t)(e + 15 - 1) << 10) + kept);
        return (uint16_t)(sign | h);
    }
};

typedef __half half;

static inline float __half2float(const __half h) { return __half::to_float(h.bits); }
static inline __half __float2half(const float f) { return __half(f); }

#endif
