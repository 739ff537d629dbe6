// fit_kernels.hip -- fine-tuning a tree's leaf values against training images (rto_tree_fit_grad / rto_fit_sgd_step, include/rto.h
// "tree fit"): the deterministic composited render of the field `params`, its squared error against the targets, and the
// gradient with respect to params, accumulated in 64-bit fixed point.
//
// One lane per pixel's ray; a wave covers an 8x8 pixel tile, a workgroup 16x16, blockIdx.z is the camera of the launch -- the
// cameras and their target / image pointers travel by value, kLayerCamChunk per launch.  The two marches are rto_fit_march.h,
// the text the host twin compiles too; here they are given
//   locate:  the walk over what the tree has resident, exactly leaf_weights_kernel's (the two-level image, the one-level image,
//            or child[] with the reference's float descent); the walk returns the uploaded density half, the support's first test.
//   slot_of: a dense leaf's slot in the numbering of params -- wide_to_slot for an entry of the two-level image, node_old where
//            the upload re-laid the nodes.  Only a leaf of the support pays for it.
//   exp:     det_expf_mid for an argument in [-87, 0], det_expf elsewhere: the same float.
//   add:     one 64-bit integer atomic add per non-zero contribution.  Integer adds commute, so the words do not depend on the
//            order the rays run in.
// basis_dim is a template parameter: Y[] and the per-channel loops are unrolled into registers.  The loss and the ray count are
// summed over the wave in integers before lane 0's one pair of atomics.  No LDS, no scratch.
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
__global__ void __launch_bounds__(256) fit_grad_kernel(const TreeDev tree, const fm::Opt opt, const LayerCams cams, const FitPlanes planes,
                                                       const uint32_t* __restrict__ node_old, const float* __restrict__ params,
                                                       unsigned long long* grad, unsigned long long* stats) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const CamDev& cd = cams.c[blockIdx.z];
    const int x = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    const int y = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    long long loss_q = 0;
    unsigned counted = 0u;
    if (x < cd.width && y < cd.height) {
        lm::Cam cam;
        cam.width = cd.width;
        cam.height = cd.height;
        cam.fx = cd.fx;
        cam.fy = cd.fy;
#pragma unroll
        for (int i = 0; i < 12; ++i) cam.transform[i] = cd.transform[i];
        lm::Frame fr;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            fr.offset[i] = tree.offset[i];
            fr.scale[i] = tree.scale[i];
        }
        fr.ndc_width = tree.ndc_width;
        fr.ndc_height = tree.ndc_height;
        fr.ndc_focal = tree.ndc_focal;

        const auto locate = [&](const float* pos, lm::Leaf& leaf) -> bool {
            if constexpr (WALK == kWalkChild) {
#pragma unroll
                for (int i = 0; i < 3; ++i) leaf.local[i] = pos[i];
                const int64_t slot = lm::descend_child(tree.child, tree.N, leaf.local, leaf.cube_sz);
                leaf.index = (uint32_t)slot;
                leaf.sigma_bits = tree.data[slot * tree.data_dim + tree.data_dim - 1];
                return true;
            } else {
                float p[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) p[i] = f_max(f_min(pos[i], 1.f - 1e-6f), 0.f);
                const Leaf r = walk_point<true>(tree, WALK, p);
                if (r.level < 1) return false;  // (cannot happen, see walk_point)
                leaf.index = r.index;
                leaf.sigma_bits = r.sigma;
                leaf.cube_sz = __uint_as_float((uint32_t)(127 + r.level) << 23);  // 2^level
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float u = p[i] * leaf.cube_sz;  // (exact, as is the subtraction)
                    leaf.local[i] = u - floorf(u);
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
        const int64_t px = ((int64_t)y * cd.width + x) * 3;
        const float* target = planes.target[blockIdx.z];
        float* image = planes.image[blockIdx.z];
        int64_t q;
        if (fm::fit_pixel<B>(fr, opt, cam, x, y, params, target ? target + px : nullptr, image ? image + px : nullptr, grad != nullptr, locate,
                             exp_, slot_of, add, q)) {
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

// 4 parameters per thread: one 16-byte access to params, two to grad (read, then zeroed); the last count % 4 by single accesses
__global__ void __launch_bounds__(256) fit_sgd_step_kernel(float* __restrict__ params, long long* __restrict__ grad, int64_t quads,
                                                           int64_t count, float lr) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < quads) {
        float4 p = reinterpret_cast<float4*>(params)[i];
        longlong2* g = reinterpret_cast<longlong2*>(grad) + 2 * i;
        const longlong2 g0 = g[0], g1 = g[1];
        p.x = fm::sgd_step(p.x, g0.x, lr);
        p.y = fm::sgd_step(p.y, g0.y, lr);
        p.z = fm::sgd_step(p.z, g1.x, lr);
        p.w = fm::sgd_step(p.w, g1.y, lr);
        reinterpret_cast<float4*>(params)[i] = p;
        g[0] = make_longlong2(0, 0);
        g[1] = make_longlong2(0, 0);
    } else {
        const int64_t j = quads * 4 + (i - quads);
        if (j < count) {
            params[j] = fm::sgd_step(params[j], grad[j], lr);
            grad[j] = 0;
        }
    }
}

namespace {

template <int WALK>
hipError_t launch_fit_walk(const TreeDev& tree, int basis, const fm::Opt& opt, const LayerCams& cams, const FitPlanes& planes, dim3 grid,
                           const uint32_t* node_old, const float* params, int64_t* grad, uint64_t* stats, hipStream_t stream) {
    unsigned long long* g = reinterpret_cast<unsigned long long*>(grad);
    unsigned long long* s = reinterpret_cast<unsigned long long*>(stats);
#define RTO_FIT_CASE(B_) \
    case B_: hipLaunchKernelGGL((fit_grad_kernel<WALK, B_>), grid, dim3(256), 0, stream, tree, opt, cams, planes, node_old, params, g, s); break
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

hipError_t launch_fit_grad(const TreeDev& tree, int walk, int basis, const fm::Opt& opt, const LayerCams& cams, const FitPlanes& planes,
                           int frames, const uint32_t* node_old, const float* params, int64_t* grad, uint64_t* stats, hipStream_t stream) {
    if (frames <= 0) return hipSuccess;
    if (frames > kLayerCamChunk || cams.c[0].width <= 0 || cams.c[0].height <= 0 || !params) return hipErrorInvalidValue;
    if (tree.data_dim != (basis ? 3 * basis + 1 : 4)) return hipErrorInvalidValue;
    if (walk == kWalkChild && !(tree.child && tree.data)) return hipErrorInvalidValue;
    if (walk == kWalkNodew && !tree.nodew) return hipErrorInvalidValue;
    if (walk == kWalkWide && !(tree.widew && tree.nodew && tree.wgslot && tree.worig)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((cams.c[0].width + 15) / 16), (unsigned)((cams.c[0].height + 15) / 16), (unsigned)frames);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    if (walk == kWalkWide) return launch_fit_walk<kWalkWide>(tree, basis, opt, cams, planes, grid, node_old, params, grad, stats, stream);
    if (walk == kWalkNodew) return launch_fit_walk<kWalkNodew>(tree, basis, opt, cams, planes, grid, node_old, params, grad, stats, stream);
    if (walk == kWalkChild) return launch_fit_walk<kWalkChild>(tree, basis, opt, cams, planes, grid, node_old, params, grad, stats, stream);
    return hipErrorInvalidValue;
}

hipError_t launch_fit_sgd_step(float* params, int64_t* grad, int64_t count, float lr, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    // the 16-byte form needs both arrays 16-byte aligned; else every parameter goes the single way
    const int64_t quads = ((uintptr_t)params % 16 == 0 && (uintptr_t)grad % 16 == 0) ? count / 4 : 0;
    const int64_t threads = quads + (count - 4 * quads);
    const int64_t blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fit_sgd_step_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, params, reinterpret_cast<long long*>(grad), quads, count,
                       lr);
    return hipGetLastError();
}

}  // namespace rto
