// rto_fit_optim.h -- the sparse step of the tree fit (rto_fit_step_sparse, include/rto.h "tree fit"), stated ONCE for the kernel
// (fit_sparse_kernels.hip) and for the host twin (host/fit_sparse.cpp), and the bit arithmetic of the touched bitmap both share.
//
// All arithmetic is float32; every operation is rounded once: each product, sum, quotient and square root below is its own
// statement, so nothing is left to contract (compile with -ffp-contract=off all the same).  Division and sqrtf are the IEEE,
// correctly rounded ones: hipcc's default for gfx950 (-fhip-fp32-correctly-rounded-divide-sqrt) and g++'s on the host.
//   * bias1 and bias2 are the CALLER's floats, 1 - beta^t for step t.  The entry does no step counting.
//   * The moments of a leaf that was not listed do not decay: the lazy rule of torch.optim.SparseAdam and of Plenoxels.
//   * With grad_scale == 1.f and a finite lr >= 0, RTO_FIT_SGD over a list that covers every non-zero grad row leaves the bytes of
//     rto_fit_sgd_step in params and an all-zero grad: g * 1.f is g, and the dense step on a zero word subtracts lr * 0.f = +0.f.
#pragma once
#include "rto.h"
#include "rto_fit_march.h"

namespace rto {
namespace fo {

// g = from_fixed(q) * grad_scale: the gradient every kind steps with
RTO_HD inline float grad_of(int64_t q, const rto_fit_optim& o) {
    const float g = fm::from_fixed(q);
    return g * o.grad_scale;
}

// KIND: RTO_FIT_SGD / RTO_FIT_RMSPROP / RTO_FIT_ADAM.  p, m, v: the element's parameter and moments (m, v read and written only
// by the kinds that have them)
template <int KIND>
RTO_HD inline void step(const rto_fit_optim& o, int64_t q, float& p, float& m, float& v) {
    const float g = grad_of(q, o);
    if constexpr (KIND == RTO_FIT_SGD) {
        const float s = o.lr * g;
        p = p - s;
    } else {
        if constexpr (KIND == RTO_FIT_ADAM) {
            const float a = o.beta1 * m;
            const float c1 = 1.f - o.beta1;
            const float b = c1 * g;
            m = a + b;
        }
        const float a2 = o.beta2 * v;
        const float c2 = 1.f - o.beta2;
        const float b2 = c2 * g;
        const float b3 = b2 * g;
        v = a2 + b3;
        float num, root;
        if constexpr (KIND == RTO_FIT_ADAM) {
            num = m / o.bias1;
            const float vh = v / o.bias2;
            root = sqrtf(vh);
        } else {
            num = g;
            root = sqrtf(v);
        }
        const float den = root + o.eps;
        const float r = num / den;
        const float s = o.lr * r;
        p = p - s;
    }
}

// the touched bitmap: words of a bitmap of `slots` bits, and the valid bits of word w (all but the tail of the last word)
RTO_HD inline int64_t touched_words(int64_t slots) { return (slots + 31) >> 5; }
RTO_HD inline uint32_t touched_valid_mask(int64_t w, int64_t slots) {
    const int64_t left = slots - (w << 5);
    return left >= 32 ? 0xffffffffu : (left <= 0 ? 0u : ((1u << (int)left) - 1u));
}

}  // namespace fo
}  // namespace rto
