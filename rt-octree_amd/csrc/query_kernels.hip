// query_kernels.hip -- what the tree holds at a point (rto_tree_query), and the operator's probe built on it.
//
// What the reference computes (relative to /root/reference):
//   query_single_from_root             renderer/include/volrend/internal/n3tree_query.hpp:13-48   point -> leaf, cube_sz
//   retrieve_cursor_lumisphere_kernel  renderer/src/cuda/volrend.cu:215-231                       the probe point's coefficients
//   render_kernel, enable_probe        renderer/src/cuda/volrend.cu:100-134                       the lumisphere disc
//
// query_kernel: one thread per point walks whatever the tree has resident -- the two-level image (one load per two levels), the
// one-level image (top grid + nodew) or, for a tree without traversal image (N != 2), child[] with the reference's float
// descent -- and stores sigma, level and cube from the walk alone: the leaf word carries the sigma bits, so an occupancy query
// reads neither data[] nor a record.  The [n][data_dim] `values` rows are not stored by the thread that walked: it leaves where
// its leaf's coefficients are in LDS, and each wave then runs its lanes over the data_dim * 64 contiguous floats of its 64 points
// (consecutive lanes = consecutive halves of one record -> consecutive floats of the output).
//
// The walk itself (walk_point) lives in rto_tree_walk.h, shared with grid_kernels.hip.
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"
#include "rto_tree_device.h"
#include "rto_launch.h"

#pragma clang fp contract(off)

#include "rto_tree_walk.h"

namespace rto {


// where `values` of a leaf come from: half k of its row is vs.src[(uint64_t)row * vs.stride + k]
RTO_DEV uint32_t values_row(const TreeDev& tree, int walk, const ValuesSrc& vs, const Leaf& r) {
    if (vs.by_entry) return r.index;
    return walk == kWalkWide ? wide_to_slot(tree, r.index) : r.index;
}

constexpr uint32_t kAnswered = 1u << 16;

__global__ void __launch_bounds__(256) query_kernel(const TreeDev tree, const int walk, const ValuesSrc vs, const float* __restrict__ points,
                                                    const int64_t n, const QueryOut out) {
    __shared__ uint2 s_row[256];  // per point: {row of its values, sigma bits | kAnswered}
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
        const Leaf r = walk_point(tree, walk, p);
        const bool ok = r.level >= 0;
        if (out.sigma) out.sigma[i] = ok ? half_bits_to_float((uint16_t)r.sigma) : 0.f;
        if (out.level) out.level[i] = r.level;
        if (out.cube) reinterpret_cast<float4*>(out.cube)[i] = make_float4(r.cube[0], r.cube[1], r.cube[2], r.cube[3]);
        if (out.values) s_row[threadIdx.x] = make_uint2(ok ? values_row(tree, walk, vs, r) : 0u, r.sigma | (ok ? kAnswered : 0u));
    }
    if (!out.values) return;  // (uniform)
    __syncthreads();
    // the wave's 64 points own DD * 64 consecutive floats of `values`: lane j takes floats j, j + 64, ...
    const int DD = tree.data_dim;
    const int lane = threadIdx.x & 63, wave0 = threadIdx.x & ~63;
    const int64_t first = (int64_t)blockIdx.x * 256 + wave0;
    if (first >= n) return;
    const int cnt = n - first < 64 ? (int)(n - first) : 64;
    const uint16_t* __restrict__ src = vs.src;
    const uint32_t stride = vs.stride;
    float* __restrict__ dst = out.values + (uint64_t)first * (uint64_t)DD;
    const int dq = 64 / DD, dk = 64 % DD;  // a step of 64 floats in (point, channel) terms
    int q = lane / DD, k = lane % DD;
    for (int f = lane; f < cnt * DD; f += 64) {
        const uint2 e = s_row[wave0 + q];
        float v = 0.f;
        if (e.y & kAnswered) v = half_bits_to_float(k == DD - 1 ? (uint16_t)(e.y & 0xffffu) : src[(uint64_t)e.x * stride + (uint32_t)k]);
        dst[f] = v;
        q += dq;
        k += dk;
        if (k >= DD) {
            k -= DD;
            ++q;
        }
    }
}

// ---- the probe (volrend.cu:100-134, 215-231) ----

// retrieve_cursor_lumisphere_kernel: the coefficients of the leaf that holds `point` -> coeffs[0 .. min(data_dim - 1, cap) - 1].
// One wave; every lane walks the same point.
__global__ void __launch_bounds__(64) probe_fetch_kernel(const TreeDev tree, const int walk, const ValuesSrc vs, const float px, const float py,
                                                         const float pz, float* __restrict__ coeffs, const int cap) {
    const float p[3] = {px, py, pz};
    const Leaf r = walk_point(tree, walk, p);
    const bool ok = r.level >= 0;  // (a non-finite probe point reads as zeros)
    const uint32_t row = ok ? values_row(tree, walk, vs, r) : 0u;
    const uint16_t* __restrict__ src = vs.src;
    const uint32_t stride = vs.stride;
    const int m = tree.data_dim - 1 < cap ? tree.data_dim - 1 : cap;
    for (int k = threadIdx.x; k < m; k += 64) coeffs[k] = ok ? half_bits_to_float(src[(uint64_t)row * stride + (uint32_t)k]) : 0.f;
}

// The disc's pixels of every frame the launch wrote (volrend.cu:100-131 in float arithmetic, every operation rounded; the outputs
// of :174-212 with nalpha = 0).  One thread per pixel of the probe's square clipped to the image, blockIdx.z = frame.
__global__ void __launch_bounds__(256) probe_overlay_kernel(const TreeDev tree, const OptDev opt, const ProbeDraw pd,
                                                            const float* __restrict__ coeffs) {
    const int x = pd.x0 + (int)(blockIdx.x * 16 + (threadIdx.x & 15)), y = (int)(blockIdx.y * 16 + (threadIdx.x >> 4));
    if (x >= pd.width || y >= pd.y1) return;
    const int xx = x - (pd.width - pd.disp) + 5;
    const int yy = y - 5;
    float cen[3];
    cen[0] = -(xx / (0.5f * pd.disp) - 1.f);
    cen[1] = (yy / (0.5f * pd.disp) - 1.f);
    const float c = cen[0] * cen[0] + cen[1] * cen[1];
    if (!(c <= 1.f)) return;  // outside the disc: the traced pixel stays
    const FrameDesc* __restrict__ fd = pd.table ? pd.table + blockIdx.z : &pd.one;
    float o[3];
    if (tree.basis_dim >= 0) {
        cen[2] = -sqrtf(1 - c);
        const float* m = fd->transform;
        const float dir[3] = {m[0] * cen[0] + m[3] * cen[1] + m[6] * cen[2], m[1] * cen[0] + m[4] * cen[1] + m[7] * cen[2],
                              m[2] * cen[0] + m[5] * cen[1] + m[8] * cen[2]};
        float basis_fn[RTO_BASIS_MAX_DEV];
        ray_basis_any(tree, opt, dir, basis_fn);  // (opt.rot_on = 0: the probe applies no rot_dirs rotation)
        // the reference sums i = basis_minmax[0] .. [1] whatever the tree's basis_dim; here i stays inside the tree's basis
        const int lo = opt.basis_minmax[0] > 0 ? opt.basis_minmax[0] : 0;
        const int hi = opt.basis_minmax[1] < tree.basis_dim - 1 ? opt.basis_minmax[1] : tree.basis_dim - 1;
        for (int t = 0; t < 3; ++t) {
            const int off = t * tree.basis_dim;
            float tmp = 0.f;
#pragma unroll
            for (int i = 0; i < RTO_BASIS_MAX_DEV; ++i)
                if (i >= lo && i <= hi) tmp += basis_fn[i] * coeffs[off + i];
            o[t] = 1.f / (1.f + det_expf(-tmp));
        }
    } else {
        for (int t = 0; t < 3; ++t) o[t] = coeffs[t];
    }
    const int64_t SIZE = (int64_t)pd.width * pd.height, idx = (int64_t)y * pd.width + x;
    if (!pd.lean) {
        float* a = fd->aux + idx;
        a[0] = o[0];
        a[SIZE] = o[1];
        a[2 * SIZE] = o[2];
        a[3 * SIZE] = 1.f;
        a[4 * SIZE] = o[0] * o[0];
        a[5 * SIZE] = o[1] * o[1];
        a[6 * SIZE] = o[2] * o[2];
        a[7 * SIZE] = 1.f;
    }
    reinterpret_cast<float4*>(fd->image)[idx] = make_float4(o[0], o[1], o[2], 1.0f);
}

// ---- launchers ----

hipError_t launch_query(const TreeDev& tree, int walk, const ValuesSrc& vs, const float* points, int64_t n, const QueryOut& out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const int64_t blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(query_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, tree, walk, vs, points, n, out);
    return hipGetLastError();
}

hipError_t launch_probe_fetch(const TreeDev& tree, int walk, const ValuesSrc& vs, const float point[3], float* coeffs, int cap, hipStream_t stream) {
    hipLaunchKernelGGL(probe_fetch_kernel, dim3(1), dim3(64), 0, stream, tree, walk, vs, point[0], point[1], point[2], coeffs, cap);
    return hipGetLastError();
}

hipError_t launch_probe_overlay(const TreeDev& tree, const OptDev& opt, ProbeDraw pd, int frames, const float* coeffs, hipStream_t stream) {
    // volrend.cu:100-101: y < disp + 5 && x >= width - disp - 5, clipped to the image
    const int64_t x0 = (int64_t)pd.width - pd.disp - 5, y1 = (int64_t)pd.disp + 5;
    pd.x0 = x0 > 0 ? (int)x0 : 0;
    pd.y1 = y1 < pd.height ? (int)y1 : pd.height;
    if (pd.x0 >= pd.width || pd.y1 <= 0 || frames < 1) return hipSuccess;
    const dim3 grid((unsigned)((pd.width - pd.x0 + 15) / 16), (unsigned)((pd.y1 + 15) / 16), (unsigned)frames);
    hipLaunchKernelGGL(probe_overlay_kernel, grid, dim3(256), 0, stream, tree, opt, pd, coeffs);
    return hipGetLastError();
}

}  // namespace rto
