// tree_simplify.h -- the tree simplifier of include/rto.h "simplifier": the arithmetic both implementations share (the fp16
// threshold and its comparison, the bit compare of two records, the bounds check of a link) and the host twin.
// Plain C++17, no HIP include: g++ compiles host/tree_simplify.cpp alone (tools/sanitize/run_simplify.sh); the kernels
// (simplify_kernels.hip) include this header for the RTO_MC_HD functions, so both sides run the same statements.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#include "host/median_cut.h"
#include "rto.h"

namespace rto {

constexpr int kSimplifyMaxLevels = 32;  // nodes live at levels 0 .. 31
constexpr int32_t kSimplifyZero = -1;   // the source of a dead slot: a record of D halves +0

// the kill threshold as an fp16 pattern: float32 -> fp16 to nearest even, beyond 65504 an infinity (a NaN never gets here)
RTO_MC_HD uint32_t simp_thresh_half(float t) { return mc_float_to_half(t); }

// IEEE a > b on fp16 patterns: false when either is a NaN, -0 == +0
RTO_MC_HD bool simp_half_gt(uint32_t a, uint32_t b) {
    if ((a & 0x7FFFu) > 0x7C00u || (b & 0x7FFFu) > 0x7C00u) return false;
    const int32_t va = (a & 0x8000u) ? -(int32_t)(a & 0x7FFFu) : (int32_t)(a & 0x7FFFu);
    const int32_t vb = (b & 0x8000u) ? -(int32_t)(b & 0x7FFFu) : (int32_t)(b & 0x7FFFu);
    return va > vb;
}

// the node slot s of node n refers to through the offset c != 0, or -1 when it lies outside [1, cap): decided on 64-bit
// integers BEFORE anything is indexed with it
RTO_MC_HD int64_t simp_link_target(int64_t n, int32_t c, int64_t cap) {
    const int64_t t = n + (int64_t)c;
    return (t >= 1 && t < cap) ? t : -1;
}

RTO_MC_HD uint32_t simp_load32(const uint16_t* p) {  // p is 4-byte aligned
    return *reinterpret_cast<const uint32_t*>(p);
}

// D halves at a == D halves at b, bit for bit.  Two records of one tree are both 2-byte aligned only; where they share their
// alignment modulo 4 (always for records an even number of records apart) the body is compared as 32-bit words.
RTO_MC_HD bool simp_rec_equal(const uint16_t* a, const uint16_t* b, int D) {
    int i = 0;
    if ((((uintptr_t)a ^ (uintptr_t)b) & 2u) == 0) {
        if (((uintptr_t)a & 2u) && D > 0) {
            if (a[0] != b[0]) return false;
            i = 1;
        }
        for (; i + 2 <= D; i += 2)
            if (simp_load32(a + i) != simp_load32(b + i)) return false;
    }
    for (; i < D; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

// D halves at a are all +0
RTO_MC_HD bool simp_rec_zero(const uint16_t* a, int D) {
    int i = 0;
    if (((uintptr_t)a & 2u) && D > 0) {
        if (a[0]) return false;
        i = 1;
    }
    for (; i + 2 <= D; i += 2)
        if (simp_load32(a + i)) return false;
    for (; i < D; ++i)
        if (a[i]) return false;
    return true;
}

// The records of slots x and y through their sources (a slot index of the input, or kSimplifyZero): equal bit for bit?
RTO_MC_HD bool simp_src_equal(const uint16_t* data, int D, int32_t x, int32_t y) {
    if (x == y) return true;
    if (x == kSimplifyZero) return simp_rec_zero(data + (int64_t)y * D, D);
    if (y == kSimplifyZero) return simp_rec_zero(data + (int64_t)x * D, D);
    return simp_rec_equal(data + (int64_t)x * D, data + (int64_t)y * D, D);
}

// Is the node whose S slots have the sources src[0 .. S) uniform?  (All its slots are known to be leaves.)  Slot 1 is held to
// slot 0 and every later slot to the slot two before it: an even number of records apart, so simp_rec_equal takes words.
RTO_MC_HD bool simp_node_uniform(const uint16_t* data, int D, const int32_t* src, int S) {
    // the density first: it separates almost every pair of records that differ
    for (int s = 1; s < S; ++s) {
        const int32_t x = src[s], y = src[0];
        const uint32_t dx = x == kSimplifyZero ? 0u : data[(int64_t)x * D + D - 1];
        const uint32_t dy = y == kSimplifyZero ? 0u : data[(int64_t)y * D + D - 1];
        if (dx != dy) return false;
    }
    if (!simp_src_equal(data, D, src[1], src[0])) return false;
    for (int s = 2; s < S; ++s)
        if (!simp_src_equal(data, D, src[s], src[s - 2])) return false;
    return true;
}

// The argument refusals both entries share (everything but the device checks); an empty string = accepted.
std::string simplify_check_args(const int32_t* child, const uint16_t* data, int64_t cap, int N, int D, const int32_t* child_out,
                                const uint16_t* data_out, const int64_t* out_capacity, const int64_t* node_map);

// The host twin: the definition followed literally, one node at a time.  Host memory; node_map and stats may be null.
// RTO_OK, or RTO_E_INVALID / RTO_E_FORMAT with *err set.
int tree_simplify_host(const int32_t* child, const uint16_t* data, int64_t cap, int N, int D, float kill_thresh, int32_t* child_out,
                       uint16_t* data_out, int64_t* out_capacity, int64_t* node_map, rto_simplify_stats* stats, std::string* err);

}  // namespace rto
