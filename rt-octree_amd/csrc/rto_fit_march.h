// rto_fit_march.h -- the two marches of rto_tree_fit_grad (include/rto.h "tree fit"), stated ONCE for the kernel
// (fit_kernels.hip) and for the host twin (host/fit_grad.cpp): the ray of rto_leaf_march.h, composited deterministically with a
// colour per dense leaf (the forward march), and marched a second time with the same operations for the gradient of
// 1/2 |out - target|^2 with respect to the leaf values (the backward march).  Gradients leave through add(index, g): the caller
// converts them to fixed point (to_fixed) and adds integers, so no order of rays, threads or calls can change a bit.
// rto_tree_fit_grad_rays (fit_rays_kernels.hip) marches the same ray from a caller's origin and direction: ray_begin_ray, fit_ray.
//
// Built on lm::ray_setup / ray_enter / dda_unit / half_to_float; the locate / exp functors are those of lm::march_pixel.  It
// carries its own RTO_HD copy of the SH basis (sh_basis of rto_tree_device.h, the same operations) so that a plain C++ compiler
// reads it.  Compile with -ffp-contract=off: every float operation is rounded once.
#pragma once
#include "rto_leaf_march.h"

namespace rto {
namespace fm {

struct Opt {
    lm::Opt m;
    float bg;  // background_brightness
};

// what a ray needs for both marches
struct Ray {
    float dir[3], cen[3], invdir[3];
    float delta_scale, tmin, tmax;
    bool hit;  // false: not marched (a non-finite set-up or a miss of the box), out = bg
};

// ---- fixed point: a float contribution as a 64-bit integer in units of 2^-36 ----
// NaN -> 0; clamped to +-2^16, so |q| <= 2^52 and the product, the rounding and the conversion are exact
RTO_HD inline int64_t to_fixed(float g) {
    if (g != g) return 0;
    const float c = g > 65536.f ? 65536.f : (g < -65536.f ? -65536.f : g);
    return (int64_t)rint((double)c * 68719476736.0);
}
RTO_HD inline float from_fixed(int64_t q) { return (float)((double)q * (1.0 / 68719476736.0)); }

// the SGD step on one parameter (rto_fit_sgd_step): two float roundings, no FMA
RTO_HD inline float sgd_step(float p, int64_t q, float lr) {
    const float g = from_fixed(q);
    const float s = lr * g;
    return p - s;
}

// sh_basis of rto_tree_device.h (lumisphere.hpp:38-80) for a basis_dim known at compile time: double literals, the products
// with them in double, one rounding per assignment
template <int B>
RTO_HD inline void sh_basis(const float* dir, float* out) {
    out[0] = (float)0.28209479177387814;
    const float x = dir[0], y = dir[1], z = dir[2];
    const float xx = x * x, yy = y * y, zz = z * z;
    const float xy = x * y, yz = y * z, xz = x * z;
    if constexpr (B >= 25) {
        out[16] = (float)(2.5033429417967046 * xy * (xx - yy));
        out[17] = (float)(-1.7701307697799304 * yz * (3 * xx - yy));
        out[18] = (float)(0.9461746957575601 * xy * (7 * zz - 1.f));
        out[19] = (float)(-0.6690465435572892 * yz * (7 * zz - 3.f));
        out[20] = (float)(0.10578554691520431 * (zz * (35 * zz - 30) + 3));
        out[21] = (float)(-0.6690465435572892 * xz * (7 * zz - 3));
        out[22] = (float)(0.47308734787878004 * (xx - yy) * (7 * zz - 1.f));
        out[23] = (float)(-1.7701307697799304 * xz * (xx - 3 * yy));
        out[24] = (float)(0.6258357354491761 * (xx * (xx - 3 * yy) - yy * (3 * xx - yy)));
    }
    if constexpr (B >= 16) {
        out[9] = (float)(-0.5900435899266435 * y * (3 * xx - yy));
        out[10] = (float)(2.890611442640554 * xy * z);
        out[11] = (float)(-0.4570457994644658 * y * (4 * zz - xx - yy));
        out[12] = (float)(0.3731763325901154 * z * (2 * zz - 3 * xx - 3 * yy));
        out[13] = (float)(-0.4570457994644658 * x * (4 * zz - xx - yy));
        out[14] = (float)(1.445305721320277 * z * (xx - yy));
        out[15] = (float)(-0.5900435899266435 * x * (xx - 3 * yy));
    }
    if constexpr (B >= 9) {
        out[4] = (float)(1.0925484305920792 * xy);
        out[5] = (float)(-1.0925484305920792 * yz);
        out[6] = (float)(0.31539156525252005 * (2.0 * zz - xx - yy));
        out[7] = (float)(-1.0925484305920792 * xz);
        out[8] = (float)(0.5462742152960396 * (xx - yy));
    }
    if constexpr (B >= 4) {
        out[1] = (float)(-0.4886025119029199 * y);
        out[2] = (float)(0.4886025119029199 * z);
        out[3] = (float)(-0.4886025119029199 * x);
    }
}

// lm::ray_setup's sibling: the same (dir, cen), and beside them vdir, the unit view direction before the NDC warp and before
// ray_enter scales it (the first normalised dir of ray_setup, by the same operations)
RTO_HD inline void ray_setup_vdir(int x, int y, const lm::Cam& cam, const lm::Frame& fr, float* dir, float* cen, float* vdir) {
    const float xyz[3] = {(x - 0.5f * cam.width) / cam.fx, -(y - 0.5f * cam.height) / cam.fy, -1.0f};
    const float* m = cam.transform;
    vdir[0] = m[0] * xyz[0] + m[3] * xyz[1] + m[6] * xyz[2];
    vdir[1] = m[1] * xyz[0] + m[4] * xyz[1] + m[7] * xyz[2];
    vdir[2] = m[2] * xyz[0] + m[5] * xyz[1] + m[8] * xyz[2];
    lm::normalize3(vdir);
    lm::ray_setup(x, y, cam, fr, dir, cen);
}

// B: basis_dim of an SH tree, 0 for RGBA.  values per leaf
template <int B>
constexpr int data_dim_of() {
    return B ? 3 * B + 1 : 4;
}

// the ray of pixel (x, y) and, for an SH tree, the basis Y[B] at its view direction
template <int B>
RTO_HD inline void ray_begin(const lm::Frame& fr, const Opt& o, const lm::Cam& cam, int x, int y, Ray& r, float* Y) {
    float vdir[3];
    ray_setup_vdir(x, y, cam, fr, r.dir, r.cen, vdir);
    r.hit = true;
    for (int i = 0; i < 3; ++i)
        if (!lm::finite_f(r.dir[i]) || !lm::finite_f(r.cen[i])) r.hit = false;
    if constexpr (B > 0) sh_basis<B>(vdir, Y);
    r.delta_scale = r.tmin = r.tmax = 0.f;
    r.invdir[0] = r.invdir[1] = r.invdir[2] = 0.f;
    if (r.hit) r.hit = lm::ray_enter(fr, o.m, r.dir, r.cen, r.invdir, r.delta_scale, r.tmin, r.tmax);
}

// ray_begin's sibling for a ray the caller supplies (rto_tree_fit_grad_rays): the ray of a pixel whose set-up produced
// dir = vdir = normalize3(direction) and cen = origin.  From there on lm::ray_setup's tail -- the NDC warp, then
// offset + scale * cen -- by ray_setup's operations in ray_setup's order, and ray_begin's own.  A zero or non-finite direction
// and a non-finite origin leave a non-finite dir or cen: the ray is not marched (hit = false), by arithmetic alone.
template <int B>
RTO_HD inline void ray_begin_ray(const lm::Frame& fr, const Opt& o, const float* origin, const float* direction, Ray& r, float* Y) {
    float vdir[3] = {direction[0], direction[1], direction[2]};
    lm::normalize3(vdir);
    float* dir = r.dir;
    float* cen = r.cen;
    for (int i = 0; i < 3; ++i) {
        dir[i] = vdir[i];
        cen[i] = origin[i];
    }
    if (fr.ndc_width > 0) {
        const float t = -(1.f + cen[2]) / dir[2];
        for (int i = 0; i < 3; ++i) cen[i] = cen[i] + t * dir[i];
        dir[0] = -((2 * fr.ndc_focal) / fr.ndc_width) * (dir[0] / dir[2] - cen[0] / cen[2]);
        dir[1] = -((2 * fr.ndc_focal) / fr.ndc_height) * (dir[1] / dir[2] - cen[1] / cen[2]);
        dir[2] = -2 / cen[2];
        cen[0] = -((2 * fr.ndc_focal) / fr.ndc_width) * (cen[0] / cen[2]);
        cen[1] = -((2 * fr.ndc_focal) / fr.ndc_height) * (cen[1] / cen[2]);
        cen[2] = 1 + 2 / cen[2];
        lm::normalize3(dir);
    }
    for (int i = 0; i < 3; ++i) cen[i] = fr.offset[i] + fr.scale[i] * cen[i];
    r.hit = true;
    for (int i = 0; i < 3; ++i)
        if (!lm::finite_f(r.dir[i]) || !lm::finite_f(r.cen[i])) r.hit = false;
    if constexpr (B > 0) sh_basis<B>(vdir, Y);
    r.delta_scale = r.tmin = r.tmax = 0.f;
    r.invdir[0] = r.invdir[1] = r.invdir[2] = 0.f;
    if (r.hit) r.hit = lm::ray_enter(fr, o.m, r.dir, r.cen, r.invdir, r.delta_scale, r.tmin, r.tmax);
}

// colour of a dense leaf from its values p[0 .. D-2]
template <int B, class Exp>
RTO_HD inline void leaf_colour(const float* p, const float* Y, Exp exp_, float* c) {
    if constexpr (B == 0) {
        c[0] = p[0];
        c[1] = p[1];
        c[2] = p[2];
    } else {
        for (int ch = 0; ch < 3; ++ch) {
            float z = Y[0] * p[ch * B];
            for (int k = 1; k < B; ++k) z = z + Y[k] * p[ch * B + k];
            c[ch] = 1.f / (1.f + exp_(-z));
        }
    }
}

// One march of the ray (the definition in include/rto.h).
//   BACKWARD false: out[3] = the composited colour
//   BACKWARD true:  out[3] and res[3] = out - target are given; add(index into params, g) receives every contribution
//   locate, exp_: as lm::march_pixel's;  slot_of(leaf.index) -> the leaf's slot in the numbering of params (dense leaves only)
template <int B, bool BACKWARD, class Locate, class Exp, class SlotOf, class Add>
RTO_HD inline void march(const Ray& r, const Opt& o, const float* Y, const float* params, Locate locate, Exp exp_, SlotOf slot_of,
                         float* out, const float* res, Add add) {
    constexpr int D = data_dim_of<B>();
    float T = 1.f;
    float acc[3] = {0.f, 0.f, 0.f};
    float t = r.tmin;
    while (r.hit && t < r.tmax) {
        float pos[3];
        for (int i = 0; i < 3; ++i) pos[i] = r.cen[i] + t * r.dir[i];
        lm::Leaf leaf;
        if (!locate(pos, leaf)) break;
        const float dt = lm::dda_unit(leaf.local, r.invdir) / leaf.cube_sz + o.m.step_size;
        if (lm::half_to_float((uint16_t)leaf.sigma_bits) > o.m.sigma_thresh) {  // the support: only such a leaf pays for its address
            const float* p = params + (int64_t)slot_of(leaf.index) * D;
            const float sigma = p[D - 1];
            if (sigma > o.m.sigma_thresh) {
                const float delta = dt * r.delta_scale;
                const float e = exp_(-(delta * sigma));
                const float att = e < 1.f ? e : 1.f;
                const float w = T * (1.f - att);
                float c[3];
                leaf_colour<B>(p, Y, exp_, c);
                for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + w * c[ch];
                if constexpr (BACKWARD) {
                    const int64_t base = p - params;
                    const float Ta = T * att;
                    float s = res[0] * (Ta * c[0] - (out[0] - acc[0]));
                    s = s + res[1] * (Ta * c[1] - (out[1] - acc[1]));
                    s = s + res[2] * (Ta * c[2] - (out[2] - acc[2]));
                    add(base + (D - 1), delta * s);
                    for (int ch = 0; ch < 3; ++ch) {
                        const float gc = res[ch] * w;
                        if constexpr (B == 0) {
                            add(base + ch, gc);
                        } else {
                            const float gz = gc * (c[ch] * (1.f - c[ch]));
                            for (int k = 0; k < B; ++k) add(base + ch * B + k, gz * Y[k]);
                        }
                    }
                }
                T = T * att;
                if (T < o.m.stop_thresh) break;
            }
        }
        const float tn = t + dt;
        if (!(tn > t)) break;
        t = tn;
    }
    if constexpr (!BACKWARD)
        for (int ch = 0; ch < 3; ++ch) out[ch] = acc[ch] + T * o.bg;
}

// One pixel of one camera.  target: its three floats or nullptr; image: where out goes, or nullptr; backward: march twice.
// false: masked (a NaN in the target) -- nothing is marched, written or counted.  loss_q: the pixel's loss in fixed point
template <int B, class Locate, class Exp, class SlotOf, class Add>
RTO_HD inline bool fit_pixel(const lm::Frame& fr, const Opt& o, const lm::Cam& cam, int x, int y, const float* params, const float* target,
                             float* image, bool backward, Locate locate, Exp exp_, SlotOf slot_of, Add add, int64_t& loss_q) {
    loss_q = 0;
    float tg[3] = {0.f, 0.f, 0.f};
    if (target) {
        for (int ch = 0; ch < 3; ++ch) tg[ch] = target[ch];
        if (tg[0] != tg[0] || tg[1] != tg[1] || tg[2] != tg[2]) return false;
    }
    Ray r;
    float Y[B > 0 ? B : 1];
    ray_begin<B>(fr, o, cam, x, y, r, Y);
    float out[3], res[3];
    march<B, false>(r, o, Y, params, locate, exp_, slot_of, out, res, add);
    if (image)
        for (int ch = 0; ch < 3; ++ch) image[ch] = out[ch];
    if (!target) return true;
    for (int ch = 0; ch < 3; ++ch) res[ch] = out[ch] - tg[ch];
    loss_q = to_fixed((res[0] * res[0] + res[1] * res[1]) + res[2] * res[2]);
    if (backward) march<B, true>(r, o, Y, params, locate, exp_, slot_of, out, res, add);
    return true;
}

// One ray of the caller's (rto_tree_fit_grad_rays): fit_pixel with ray_begin_ray in place of ray_begin, the same text after it.
// origin, direction: three floats each; target: three floats or nullptr; out: where the colour goes, or nullptr
template <int B, class Locate, class Exp, class SlotOf, class Add>
RTO_HD inline bool fit_ray(const lm::Frame& fr, const Opt& o, const float* origin, const float* direction, const float* params,
                           const float* target, float* out_px, bool backward, Locate locate, Exp exp_, SlotOf slot_of, Add add,
                           int64_t& loss_q) {
    loss_q = 0;
    float tg[3] = {0.f, 0.f, 0.f};
    if (target) {
        for (int ch = 0; ch < 3; ++ch) tg[ch] = target[ch];
        if (tg[0] != tg[0] || tg[1] != tg[1] || tg[2] != tg[2]) return false;
    }
    Ray r;
    float Y[B > 0 ? B : 1];
    ray_begin_ray<B>(fr, o, origin, direction, r, Y);
    float out[3], res[3];
    march<B, false>(r, o, Y, params, locate, exp_, slot_of, out, res, add);
    if (out_px)
        for (int ch = 0; ch < 3; ++ch) out_px[ch] = out[ch];
    if (!target) return true;
    for (int ch = 0; ch < 3; ++ch) res[ch] = out[ch] - tg[ch];
    loss_q = to_fixed((res[0] * res[0] + res[1] * res[1]) + res[2] * res[2]);
    if (backward) march<B, true>(r, o, Y, params, locate, exp_, slot_of, out, res, add);
    return true;
}

}  // namespace fm
}  // namespace rto
