// rto_tree_bits.h -- bit layout of the traversal images' words: what the kernels (rto_kernel_types.h) and the host code that
// builds the images (host/tree_layout.cpp, which compiles without HIP) both state them with.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define RTO_HD __host__ __device__
#else  // a plain C++ compiler
#define RTO_HD
#endif

namespace rto {

// Leaf tag of the traversal image `nodew` (see build_nodew_kernel in tree_image_kernels.hip):
//   internal slot: the reference's child[] value (relative node offset, |v| < 2^30)
//   leaf slot:     0x80000000 | fp16 bits of the slot's sigma  -> top two bits are 0b10
constexpr uint32_t kLeafTag = 0x80000000u;
// A leaf word of the TWO-LEVEL image also carries its leaf's level (< 32), at the bits a float's exponent field starts at:
// the march step's 2^(level + c) factors are then one integer add / subtract on (word & kWideLevelMask) -- no field extract
constexpr int kWideLevelShift = 23;
constexpr uint32_t kWideLevelMask = 31u << kWideLevelShift;
constexpr int kOccLevel = 7;  // finest cube of the culling cells: 2^-7 of the volume (6 pixels across at 800 x 800)
// (the bit budgets of the packed words: rto_kernel_types.h)
constexpr int kGridSlotBits = 29;
constexpr uint32_t kGridSlotMask = (1u << kGridSlotBits) - 1u;
RTO_HD inline bool nodew_is_leaf(uint32_t w) { return (w >> 30) == 2u; }

}  // namespace rto
