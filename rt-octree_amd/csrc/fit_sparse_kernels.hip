// fit_sparse_kernels.hip -- the sparse step of the tree fit (include/rto.h "tree fit"): the ray kernel that also
// marks the leaves it reached (rto_tree_fit_grad_rays_touched), the list of the marked slots (rto_fit_touched_list) and the step
// over the listed rows (rto_fit_step_sparse).  A unit of its own so that fit_kernels.hip and fit_rays_kernels.hip keep their
// code (tests/test_fit_codegen.py, tests/test_fit_rays_codegen.py).
//
// fit_grad_rays_touched_kernel is fit_grad_rays_kernel (fit_rays_kernels.hip) word for word -- one lane per ray, locate, slot_of,
// exp_ restated -- but for its add: rto_fit_march.h calls add once per dense sample with the density's index, slot * D + D - 1,
// before the colour contributions, and there the lane marks the slot.  slot_of leaves the slot it returned in a register, so add
// knows the density's index without a division.  Marking: the lane reads the bitmap word and issues atomicOr only when the bit
// is clear; a stale read can only miss a set bit (one redundant atomic), never invent one.  No LDS, no scratch.
//
// The list is reduce-then-scan in three launches (no workgroup waits for another): touched_sum_kernel, touched_scan_kernel (one
// workgroup), touched_scatter_kernel.  A thread owns kFitTouchedThreadWords consecutive words, so thread order is slot order.
//
// fit_step_sparse_kernel: a fixed grid strides over (list position, k) flattened, so consecutive lanes touch consecutive
// addresses of a row; the count is read on the device; no atomics.  The arithmetic is rto_fit_optim.h.
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"
#include "rto_tree_device.h"
#include "rto_launch.h"

#pragma clang fp contract(off)

#include "rto_fit_launch.h"
#include "rto_fit_march.h"
#include "rto_fit_optim.h"
#include "rto_tree_walk.h"

namespace rto {

template <int WALK, int B>
__global__ void __launch_bounds__(256) fit_grad_rays_touched_kernel(const TreeDev tree, const fm::Opt opt, const uint32_t* __restrict__ node_old,
                                                                    const float* __restrict__ params, const float* __restrict__ origins,
                                                                    const float* __restrict__ dirs, const float* __restrict__ targets,
                                                                    float* out, const int64_t n, unsigned long long* grad,
                                                                    unsigned long long* stats, uint32_t* touched, const int mark_read) {
    constexpr int D = fm::data_dim_of<B>();
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
        uint32_t cur_slot = 0u;  // the slot slot_of returned last: the sample add is called for
        const auto slot_of = [&](uint32_t index) -> uint32_t {
            uint32_t slot = WALK == kWalkWide ? wide_to_slot(tree, index) : index;
            if (node_old) {  // (uniform) the upload re-laid the nodes: back to the caller's numbering
                const uint32_t N3 = (uint32_t)tree.N3, node = slot / N3;
                slot = node_old[node] * N3 + (slot - node * N3);
            }
            cur_slot = slot;
            return slot;
        };
        const auto add = [&](int64_t index, float g) {
            if (index == (int64_t)cur_slot * D + (D - 1)) {  // the density's contribution, the first of a dense sample: mark the slot
                uint32_t* word = touched + (cur_slot >> 5);
                const uint32_t bit = 1u << (cur_slot & 31u);
                if (!mark_read || !(__atomic_load_n(word, __ATOMIC_RELAXED) & bit)) atomicOr(word, bit);
            }
            const int64_t q = fm::to_fixed(g);
            if (q != 0) atomicAdd(grad + index, (unsigned long long)q);
        };
        const int64_t at = i * 3;
        const float org[3] = {origins[at], origins[at + 1], origins[at + 2]};
        const float dir[3] = {dirs[at], dirs[at + 1], dirs[at + 2]};
        int64_t q;
        if (fm::fit_ray<B>(fr, opt, org, dir, params, targets + at, out ? out + at : nullptr, true, locate, exp_, slot_of, add, q)) {
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

// ---- the list ----

// the kFitTouchedThreadWords words of thread t of block b, masked to the valid bits; w0: the first word's index
__device__ inline void touched_load(const uint32_t* touched, int64_t words, int64_t slots, int64_t w0, uint32_t* raw, uint32_t* bits) {
#pragma unroll
    for (int k = 0; k < kFitTouchedThreadWords; ++k) {
        const int64_t w = w0 + k;
        raw[k] = w < words ? touched[w] : 0u;
        bits[k] = raw[k] & fo::touched_valid_mask(w, slots);
    }
}

// the sum of v over the 256 threads of the block in every thread, and the sum over the threads before this one in `before`
__device__ inline uint32_t block_scan_256(uint32_t v, uint32_t* lds4, uint32_t& before) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) lds4[wave] = inc;
    __syncthreads();
    uint32_t base = 0u, total = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t s = lds4[k];
        if (k < wave) base += s;
        total += s;
    }
    before = base + inc - v;
    return total;
}

__global__ void __launch_bounds__(256) touched_sum_kernel(const uint32_t* __restrict__ touched, int64_t words, int64_t slots,
                                                          uint32_t* __restrict__ sums) {
    __shared__ uint32_t lds4[4];
    const int64_t w0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * kFitTouchedThreadWords;
    uint32_t raw[kFitTouchedThreadWords], bits[kFitTouchedThreadWords];
    touched_load(touched, words, slots, w0, raw, bits);
    uint32_t c = 0u;
#pragma unroll
    for (int k = 0; k < kFitTouchedThreadWords; ++k) c += (uint32_t)__popc(bits[k]);
    uint32_t before;
    const uint32_t total = block_scan_256(c, lds4, before);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// ONE workgroup of 1024 threads: sums[b] -> the sum of the blocks before b, in place; count[0] = the total.  A thread owns
// `per` consecutive blocks (per <= 32 for 2^15 blocks)
__global__ void __launch_bounds__(1024) touched_scan_kernel(uint32_t* sums, int blocks, unsigned long long* count) {
    __shared__ uint32_t part[1024];
    const int t = threadIdx.x;
    const int per = (blocks + 1023) / 1024;
    const int b0 = t * per, b1 = min(b0 + per, blocks);
    uint32_t c = 0u;
    for (int b = b0; b < b1; ++b) c += sums[b];
    part[t] = c;
    __syncthreads();
    // Hillis-Steele over the 1024 partial sums
    for (int d = 1; d < 1024; d <<= 1) {
        const uint32_t o = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += o;
        __syncthreads();
    }
    uint32_t run = part[t] - c;
    for (int b = b0; b < b1; ++b) {
        const uint32_t s = sums[b];
        sums[b] = run;
        run += s;
    }
    if (t == 1023) count[0] = (unsigned long long)part[1023];
}

__global__ void __launch_bounds__(256) touched_scatter_kernel(uint32_t* touched, int64_t words, int64_t slots, int clear,
                                                              const uint32_t* __restrict__ offsets, uint32_t* __restrict__ list,
                                                              int64_t list_capacity) {
    __shared__ uint32_t lds4[4];
    const int64_t w0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * kFitTouchedThreadWords;
    uint32_t raw[kFitTouchedThreadWords], bits[kFitTouchedThreadWords];
    touched_load(touched, words, slots, w0, raw, bits);
    uint32_t c = 0u;
#pragma unroll
    for (int k = 0; k < kFitTouchedThreadWords; ++k) c += (uint32_t)__popc(bits[k]);
    uint32_t before;
    (void)block_scan_256(c, lds4, before);
    int64_t pos = (int64_t)offsets[blockIdx.x] + before;
#pragma unroll
    for (int k = 0; k < kFitTouchedThreadWords; ++k) {
        uint32_t b = bits[k];
        while (b != 0u && pos < list_capacity) {
            const int lo = __ffs((int)b) - 1;
            list[pos++] = (uint32_t)(((w0 + k) << 5) + lo);
            b &= b - 1u;
        }
        pos += __popc(b);  // (past the capacity: counted, not written)
        if (clear && raw[k] != 0u) touched[w0 + k] = 0u;  // (raw != 0 only for a word inside the bitmap)
    }
}

// ---- the step ----

template <int KIND, class Index>
__global__ void __launch_bounds__(256) fit_step_sparse_kernel(float* __restrict__ params, long long* __restrict__ grad, float* __restrict__ m,
                                                              float* __restrict__ v, int64_t slots, int row, const uint32_t* __restrict__ list,
                                                              const unsigned long long* __restrict__ count, int64_t list_capacity,
                                                              const rto_fit_optim o) {
    const unsigned long long cnt = count[0];
    const int64_t rows = cnt < (unsigned long long)list_capacity ? (int64_t)cnt : list_capacity;
    const int64_t total = rows * row;
    if (sizeof(Index) == 4 ? total > 0xffffffffLL : total <= 0xffffffffLL) return;  // (uniform) the other instantiation's call
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const Index j = (Index)e / (Index)row;
        const int k = (int)((Index)e - j * (Index)row);
        const uint32_t s = list[j];
        if ((int64_t)s >= slots) continue;
        const int64_t i = (int64_t)s * row + k;
        float p = params[i], mm = 0.f, vv = 0.f;
        if constexpr (KIND == RTO_FIT_ADAM) mm = m[i];
        if constexpr (KIND != RTO_FIT_SGD) vv = v[i];
        fo::step<KIND>(o, grad[i], p, mm, vv);
        grad[i] = 0;
        params[i] = p;
        if constexpr (KIND == RTO_FIT_ADAM) m[i] = mm;
        if constexpr (KIND != RTO_FIT_SGD) v[i] = vv;
    }
}

namespace {

template <int WALK>
hipError_t launch_fit_rays_touched_walk(const TreeDev& tree, int basis, const fm::Opt& opt, const uint32_t* node_old, const float* params,
                                        const float* origins, const float* dirs, const float* targets, float* out, int64_t n, int block,
                                        int64_t* grad, uint64_t* stats, uint32_t* touched, int mark_read, hipStream_t stream) {
    unsigned long long* g = reinterpret_cast<unsigned long long*>(grad);
    unsigned long long* s = reinterpret_cast<unsigned long long*>(stats);
    const dim3 grid((unsigned)((n + block - 1) / block));
#define RTO_FIT_CASE(B_)                                                                                                                \
    case B_:                                                                                                                            \
        hipLaunchKernelGGL((fit_grad_rays_touched_kernel<WALK, B_>), grid, dim3((unsigned)block), 0, stream, tree, opt, node_old, params, \
                           origins, dirs, targets, out, n, g, s, touched, mark_read);                                                   \
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

template <int KIND>
hipError_t launch_step_kind(float* params, int64_t* grad, float* m, float* v, int64_t slots, int row, const uint32_t* list,
                            const uint64_t* count, int64_t list_capacity, const rto_fit_optim& o, hipStream_t stream) {
    long long* g = reinterpret_cast<long long*>(grad);
    const unsigned long long* c = reinterpret_cast<const unsigned long long*>(count);
    // both index widths are enqueued; the one whose range does not hold the device's count returns at once
    hipLaunchKernelGGL((fit_step_sparse_kernel<KIND, uint32_t>), dim3(kFitStepSparseBlocks), dim3(256), 0, stream, params, g, m, v, slots, row,
                       list, c, list_capacity, o);
    if (list_capacity * row > 0xffffffffLL)
        hipLaunchKernelGGL((fit_step_sparse_kernel<KIND, uint64_t>), dim3(kFitStepSparseBlocks), dim3(256), 0, stream, params, g, m, v, slots,
                           row, list, c, list_capacity, o);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_fit_grad_rays_touched(const TreeDev& tree, int walk, int basis, const fm::Opt& opt, const uint32_t* node_old,
                                        const float* params, const float* origins, const float* dirs, const float* targets, float* out,
                                        int64_t n, int block, int64_t* grad, uint64_t* stats, uint32_t* touched, bool mark_read,
                                        hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (n > kFitRaysPerLaunch || !params || !origins || !dirs || !targets || !grad || !touched) return hipErrorInvalidValue;
    if (block != 64 && block != 128 && block != 256) return hipErrorInvalidValue;
    if (tree.data_dim != (basis ? 3 * basis + 1 : 4)) return hipErrorInvalidValue;
    if (walk == kWalkChild && !(tree.child && tree.data)) return hipErrorInvalidValue;
    if (walk == kWalkNodew && !tree.nodew) return hipErrorInvalidValue;
    if (walk == kWalkWide && !(tree.widew && tree.nodew && tree.wgslot && tree.worig)) return hipErrorInvalidValue;
#define RTO_FIT_WALK(W_)                                                                                                                   \
    if (walk == W_)                                                                                                                        \
    return launch_fit_rays_touched_walk<W_>(tree, basis, opt, node_old, params, origins, dirs, targets, out, n, block, grad, stats, touched, \
                                            mark_read ? 1 : 0, stream)
    RTO_FIT_WALK(kWalkWide);
    RTO_FIT_WALK(kWalkNodew);
    RTO_FIT_WALK(kWalkChild);
#undef RTO_FIT_WALK
    return hipErrorInvalidValue;
}

hipError_t launch_fit_touched_list(uint32_t* touched, int64_t slots, bool clear, uint32_t* list, int64_t list_capacity, uint64_t* count,
                                   uint32_t* scratch, hipStream_t stream) {
    if (!touched || !count || !scratch || slots < 0 || slots > 0x7fffffffLL || list_capacity < 0 || (!list && list_capacity > 0))
        return hipErrorInvalidValue;
    const int64_t words = fo::touched_words(slots);
    const int blocks = (int)fit_touched_blocks(slots);
    if (blocks > 0) hipLaunchKernelGGL(touched_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, touched, words, slots, scratch);
    hipLaunchKernelGGL(touched_scan_kernel, dim3(1), dim3(1024), 0, stream, scratch, blocks, reinterpret_cast<unsigned long long*>(count));
    if (blocks > 0)
        hipLaunchKernelGGL(touched_scatter_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, touched, words, slots, clear ? 1 : 0, scratch,
                           list, list_capacity);
    return hipGetLastError();
}

hipError_t launch_fit_step_sparse(float* params, int64_t* grad, float* m, float* v, int64_t slots, int row, const uint32_t* list,
                                  const uint64_t* count, int64_t list_capacity, const rto_fit_optim& o, hipStream_t stream) {
    if (!params || !grad || !list || !count || row < 1 || slots < 0 || list_capacity < 0) return hipErrorInvalidValue;
    if (list_capacity == 0 || slots == 0) return hipSuccess;
    switch (o.kind) {
        case RTO_FIT_SGD: return launch_step_kind<RTO_FIT_SGD>(params, grad, m, v, slots, row, list, count, list_capacity, o, stream);
        case RTO_FIT_RMSPROP:
            if (!v) return hipErrorInvalidValue;
            return launch_step_kind<RTO_FIT_RMSPROP>(params, grad, m, v, slots, row, list, count, list_capacity, o, stream);
        case RTO_FIT_ADAM:
            if (!m || !v) return hipErrorInvalidValue;
            return launch_step_kind<RTO_FIT_ADAM>(params, grad, m, v, slots, row, list, count, list_capacity, o, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace rto
