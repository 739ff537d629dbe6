// fit_rays_kernels.hip -- the tree fit on rays the caller supplies (rto_tree_fit_grad_rays, include/rto.h "tree fit"): what
// fit_kernels.hip does for the pixels of cameras, for n rays given by origin and direction, with a target and an output colour
// per ray.  A unit of its own so that fit_kernels.hip keeps its code (tests/test_fit_codegen.py).
//
// One lane per ray, ray i = blockIdx.x * blockDim.x + threadIdx.x of the launch; the host splits a call into launches of at most
// kFitRaysPerLaunch rays and advances the pointers, so every index is 64-bit.  Workgroups are single waves (kFitRaysBlock = 64,
// DESIGN.md 7q): the rays of a shuffled batch end at very different times, and a wave that ends frees its slot at once.  The
// marches are rto_fit_march.h (fit_ray); locate, slot_of, exp_ and add are fit_grad_kernel's, restated.  The loss and the ray
// count are summed over the wave in integers before lane 0's one pair of atomics; lanes past n take part in the shuffles and
// touch no memory.  No LDS, no scratch.
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"
#include "rto_tree_device.h"
#include "rto_launch.h"

#pragma clang fp contract(off)

#include "rto_fit_launch.h"
#include "rto_fit_march.h"
#include "rto_tree_walk.h"

namespace rto {

template <int WALK, int B>
__global__ void __launch_bounds__(256) fit_grad_rays_kernel(const TreeDev tree, const fm::Opt opt, const uint32_t* __restrict__ node_old,
                                                            const float* __restrict__ params, const float* __restrict__ origins,
                                                            const float* __restrict__ dirs, const float* __restrict__ targets, float* out,
                                                            const int64_t n, unsigned long long* grad, unsigned long long* stats) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    long long loss_q = 0;
    unsigned counted = 0u;
    if (i < n) {
        lm::Frame fr;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            fr.offset[k] = tree.offset[k];
            fr.scale[k] = tree.scale[k];
        }
        fr.ndc_width = tree.ndc_width;
        fr.ndc_height = tree.ndc_height;
        fr.ndc_focal = tree.ndc_focal;

        const auto locate = [&](const float* pos, lm::Leaf& leaf) -> bool {
            if constexpr (WALK == kWalkChild) {
#pragma unroll
                for (int k = 0; k < 3; ++k) leaf.local[k] = pos[k];
                const int64_t slot = lm::descend_child(tree.child, tree.N, leaf.local, leaf.cube_sz);
                leaf.index = (uint32_t)slot;
                leaf.sigma_bits = tree.data[slot * tree.data_dim + tree.data_dim - 1];
                return true;
            } else {
                float p[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) p[k] = f_max(f_min(pos[k], 1.f - 1e-6f), 0.f);
                const Leaf r = walk_point<true>(tree, WALK, p);
                if (r.level < 1) return false;  // (cannot happen, see walk_point)
                leaf.index = r.index;
                leaf.sigma_bits = r.sigma;
                leaf.cube_sz = __uint_as_float((uint32_t)(127 + r.level) << 23);  // 2^level
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float u = p[k] * leaf.cube_sz;  // (exact, as is the subtraction)
                    leaf.local[k] = u - floorf(u);
                }
                return true;
            }
        };
        const auto exp_ = [](float v) -> float { return (v >= -87.f && v <= 0.f) ? det_expf_mid(v) : det_expf(v); };
        const auto slot_of = [&](uint32_t index) -> uint32_t {
            uint32_t slot = WALK == kWalkWide ? wide_to_slot(tree, index) : index;
            if (node_old) {  // (uniform) the upload re-laid the nodes: back to the caller's numbering
                const uint32_t N3 = (uint32_t)tree.N3, node = slot / N3;
                slot = node_old[node] * N3 + (slot - node * N3);
            }
            return slot;
        };
        const auto add = [&](int64_t index, float g) {
            const int64_t q = fm::to_fixed(g);
            if (q != 0) atomicAdd(grad + index, (unsigned long long)q);
        };
        const int64_t at = i * 3;
        const float org[3] = {origins[at], origins[at + 1], origins[at + 2]};
        const float dir[3] = {dirs[at], dirs[at + 1], dirs[at + 2]};
        int64_t q;
        if (fm::fit_ray<B>(fr, opt, org, dir, params, targets ? targets + at : nullptr, out ? out + at : nullptr, grad != nullptr, locate, exp_,
                           slot_of, add, q)) {
            loss_q = q;
            counted = 1u;
        }
    }
    if (stats) {  // (uniform) every lane of the wave is here: the sums over the wave, then one pair of atomics
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            loss_q += __shfl_xor(loss_q, m, 64);
            counted += __shfl_xor(counted, m, 64);
        }
        if (lane == 0 && counted != 0u) {
            if (loss_q != 0) atomicAdd(stats, (unsigned long long)loss_q);
            atomicAdd(stats + 1, (unsigned long long)counted);
        }
    }
}

namespace {

template <int WALK>
hipError_t launch_fit_rays_walk(const TreeDev& tree, int basis, const fm::Opt& opt, const uint32_t* node_old, const float* params,
                                const float* origins, const float* dirs, const float* targets, float* out, int64_t n, int block,
                                int64_t* grad, uint64_t* stats, hipStream_t stream) {
    unsigned long long* g = reinterpret_cast<unsigned long long*>(grad);
    unsigned long long* s = reinterpret_cast<unsigned long long*>(stats);
    const dim3 grid((unsigned)((n + block - 1) / block));
#define RTO_FIT_CASE(B_)                                                                                                                 \
    case B_:                                                                                                                             \
        hipLaunchKernelGGL((fit_grad_rays_kernel<WALK, B_>), grid, dim3((unsigned)block), 0, stream, tree, opt, node_old, params, origins, dirs, \
                           targets, out, n, g, s);                                                                                       \
        break
    switch (basis) {
        RTO_FIT_CASE(0);
        RTO_FIT_CASE(1);
        RTO_FIT_CASE(4);
        RTO_FIT_CASE(9);
        RTO_FIT_CASE(16);
        RTO_FIT_CASE(25);
        default: return hipErrorInvalidValue;
    }
#undef RTO_FIT_CASE
    return hipGetLastError();
}

}  // namespace

hipError_t launch_fit_grad_rays(const TreeDev& tree, int walk, int basis, const fm::Opt& opt, const uint32_t* node_old, const float* params,
                                const float* origins, const float* dirs, const float* targets, float* out, int64_t n, int block,
                                int64_t* grad, uint64_t* stats, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (n > kFitRaysPerLaunch || !params || !origins || !dirs) return hipErrorInvalidValue;
    if (block != 64 && block != 128 && block != 256) return hipErrorInvalidValue;
    if (tree.data_dim != (basis ? 3 * basis + 1 : 4)) return hipErrorInvalidValue;
    if (walk == kWalkChild && !(tree.child && tree.data)) return hipErrorInvalidValue;
    if (walk == kWalkNodew && !tree.nodew) return hipErrorInvalidValue;
    if (walk == kWalkWide && !(tree.widew && tree.nodew && tree.wgslot && tree.worig)) return hipErrorInvalidValue;
#define RTO_FIT_WALK(W_) \
    if (walk == W_) return launch_fit_rays_walk<W_>(tree, basis, opt, node_old, params, origins, dirs, targets, out, n, block, grad, stats, stream)
    RTO_FIT_WALK(kWalkWide);
    RTO_FIT_WALK(kWalkNodew);
    RTO_FIT_WALK(kWalkChild);
#undef RTO_FIT_WALK
    return hipErrorInvalidValue;
}

}  // namespace rto
