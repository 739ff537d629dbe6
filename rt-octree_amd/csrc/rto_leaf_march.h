// rto_leaf_march.h -- the transmittance march of rto_tree_leaf_weights (include/rto.h "leaf weights"), stated ONCE for the
// kernel (leaf_weight_kernels.hip) and for the host twin (host/leaf_weights.cpp): a pixel's ray as the renderer sets it up, the
// walk from leaf to leaf, and per dense leaf the compositing weight T * (1 - exp(-sigma * delta)).  No colour, no image, no RNG.
//
// Self-contained on purpose: it holds its own copies of the few helpers it needs (ray set-up and entry of
// rto_render_shared.h, det_expf of rto_device_math.h, the float descent of rto_tree_device.h), written so that a plain C++
// compiler reads them too -- the existing headers stay device-only and every existing kernel keeps its code.  Under hipcc
// the functions are __host__ __device__ (RTO_HD, rto_tree_bits.h).  Compile with -ffp-contract=off: every float operation is
// rounded once, and the device, the host twin and the numpy restatement of tests/leaf_weights_ref.py give the same bits.
//
// What the reference computes (line numbers relative to the reference renderer):
//   ray set-up, NDC warp   src/cuda/volrend.cu:23-56,138-144
//   entry into the volume  src/cuda/rt_core.cuh:206-222 (_dda_world :19-36), tmax_bg = 1e9f
//   leaf step              src/cuda/rt_core.cuh:38-51 (_dda_unit), include/volrend/internal/n3tree_query.hpp:13-48
//   the bookkeeping        shaders/rt.frag:244-321 without its colour
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rto_tree_bits.h"

namespace rto {
namespace lm {

struct Cam {  // rto_camera
    int width, height;
    float fx, fy;
    float transform[12];
};
struct Frame {  // what a ray reads of the tree besides its nodes
    float offset[3], scale[3];
    float ndc_width, ndc_height, ndc_focal;  // ndc_width <= 0: no warp
};
struct Opt {  // the rto_options fields the march reads
    float step_size, sigma_thresh, stop_thresh;
    float render_bbox[6];
};
// what the walk from a point ends in: `index` names the leaf for the update (its slot, or whatever the locate functor's
// partner translates), cube_sz = N^level, local = the point in the leaf's own [0, 1)^3
struct Leaf {
    uint32_t index, sigma_bits;
    float cube_sz;
    float local[3];
};

RTO_HD inline float f_min(float a, float b) { return a < b ? a : b; }
RTO_HD inline float f_max(float a, float b) { return a > b ? a : b; }
RTO_HD inline uint32_t f_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
RTO_HD inline float bits_f(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
RTO_HD inline bool finite_f(float f) { return (f_bits(f) & 0x7f800000u) != 0x7f800000u; }

// fp16 bits -> float, exact (subnormals, infinities and NaN included)
RTO_HD inline float half_to_float(uint16_t h) {
    const uint32_t s = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    if (e == 31u) return bits_f(s | 0x7f800000u | (m << 13));
    if (e != 0u) return bits_f(s | ((e + 112u) << 23) | (m << 13));
    const float v = (float)m * 5.9604644775390625e-8f;  // m * 2^-24, exact
    return s ? -v : v;
}

// det_expf of rto_device_math.h (= orc_det_expf), full range, in plain C++
RTO_HD inline float det_expf(float x) {
    if (x != x) return x;
    if (x > 88.72283935546875f) return bits_f(0x7f800000u);
    if (x < -103.97208404541016f) return 0.0f;
    const double xd = (double)x;
    const double z = xd * 1.4426950408889634;
    const double kd = (z + 6755399441055744.0) - 6755399441055744.0;
    const double r = (xd - kd * 0.693147180558298016) - kd * 1.6465949582897082e-12;
    double p = 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    const int k = (int)kd;
    const uint64_t scb = (uint64_t)(k + 1023) << 52;
    double sc;
    memcpy(&sc, &scb, 8);
    return (float)(p * sc);
}

RTO_HD inline float norm3(const float* d) { return sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]); }
RTO_HD inline void normalize3(float* d) {
    const float invnorm = 1.f / norm3(d);
    d[0] *= invnorm;
    d[1] *= invnorm;
    d[2] *= invnorm;
}

// ray_setup of rto_render_shared.h: pixel -> (dir, cen) in tree space, the NDC warp included
RTO_HD inline void ray_setup(int x, int y, const Cam& cam, const Frame& fr, float* dir, float* cen) {
    const float xyz[3] = {(x - 0.5f * cam.width) / cam.fx, -(y - 0.5f * cam.height) / cam.fy, -1.0f};
    const float* m = cam.transform;
    dir[0] = m[0] * xyz[0] + m[3] * xyz[1] + m[6] * xyz[2];
    dir[1] = m[1] * xyz[0] + m[4] * xyz[1] + m[7] * xyz[2];
    dir[2] = m[2] * xyz[0] + m[5] * xyz[1] + m[8] * xyz[2];
    normalize3(dir);
    cen[0] = m[9];
    cen[1] = m[10];
    cen[2] = m[11];
    if (fr.ndc_width > 0) {
        const float t = -(1.f + cen[2]) / dir[2];
        for (int i = 0; i < 3; ++i) cen[i] = cen[i] + t * dir[i];
        dir[0] = -((2 * fr.ndc_focal) / fr.ndc_width) * (dir[0] / dir[2] - cen[0] / cen[2]);
        dir[1] = -((2 * fr.ndc_focal) / fr.ndc_height) * (dir[1] / dir[2] - cen[1] / cen[2]);
        dir[2] = -2 / cen[2];
        cen[0] = -((2 * fr.ndc_focal) / fr.ndc_width) * (cen[0] / cen[2]);
        cen[1] = -((2 * fr.ndc_focal) / fr.ndc_height) * (cen[1] / cen[2]);
        cen[2] = 1 + 2 / cen[2];
        normalize3(dir);
    }
    for (int i = 0; i < 3; ++i) cen[i] = fr.offset[i] + fr.scale[i] * cen[i];
}

// ray_enter of rto_render_shared.h with tmax_bg = 1e9f: double sub-expressions, render_bbox +- 1e-6.  false: a miss
RTO_HD inline bool ray_enter(const Frame& fr, const Opt& opt, float* dir, const float* cen, float* invdir, float& delta_scale,
                             float& tmin, float& tmax) {
    float tmax_bg = 1e9f;
    dir[0] *= fr.scale[0];
    dir[1] *= fr.scale[1];
    dir[2] *= fr.scale[2];
    delta_scale = 1.f / norm3(dir);
    dir[0] *= delta_scale;
    dir[1] *= delta_scale;
    dir[2] *= delta_scale;
    tmax_bg /= delta_scale;
    for (int i = 0; i < 3; ++i) invdir[i] = (float)(1.0 / ((double)dir[i] + 1e-9));
    tmin = 0.0f;
    tmax = 1e4f;
    for (int i = 0; i < 3; ++i) {
        const float t1 = (float)((((double)opt.render_bbox[i] + 1e-6) - (double)cen[i]) * (double)invdir[i]);
        const float t2 = (float)((((double)opt.render_bbox[i + 3] - 1e-6) - (double)cen[i]) * (double)invdir[i]);
        tmin = f_max(tmin, f_min(t1, t2));
        tmax = f_min(tmax, f_max(t1, t2));
    }
    tmax = f_min(tmax, tmax_bg);
    return !(tmax < 0 || tmin > tmax);
}

RTO_HD inline float dda_unit(const float* p, const float* invdir) {
    float tm = 1e4f;
    for (int i = 0; i < 3; ++i) {
        const float t1 = -p[i] * invdir[i];
        const float t2 = t1 + invdir[i];
        tm = f_min(tm, f_max(t1, t2));
    }
    return tm;
}

// query_single_from_root (n3tree_query.hpp:13-48) over child[]: the root-restart float descent, its clamp included.
// -> the leaf's slot; xyz becomes leaf-local
RTO_HD inline int64_t descend_child(const int32_t* child, int N, float* xyz, float& cube_sz) {
    const float fN = (float)N;
    const int64_t N3 = (int64_t)N * N * N;
    for (int i = 0; i < 3; ++i) xyz[i] = f_max(f_min(xyz[i], 1.f - 1e-6f), 0.f);
    int64_t ptr = 0;
    cube_sz = fN;
    while (true) {
        float index = 0.f;
        for (int i = 0; i < 3; ++i) {
            xyz[i] *= fN;
            const float idx_dimi = floorf(xyz[i]);
            index = index * fN + idx_dimi;
            xyz[i] -= idx_dimi;
        }
        const int64_t sub_ptr = ptr + (int32_t)index;
        const int64_t skip = child[sub_ptr];
        if (skip == 0) return sub_ptr;
        cube_sz *= fN;
        ptr += skip * N3;
    }
}

// The march of one pixel's ray (the definition in include/rto.h).
//   locate(pos, leaf) -> bool   the leaf that holds pos (false ends the ray: no walk here can say it)
//   exp_(x)           -> float  det_expf(x), by whatever route gives the same float
//   update(index, w)            weights[slot of index] = max(weights[..], w) on the bit patterns; w is never NaN nor negative
template <class Locate, class Exp, class Update>
RTO_HD inline void march_pixel(const Frame& fr, const Opt& opt, const Cam& cam, int x, int y, Locate locate, Exp exp_, Update update) {
    float dir[3], cen[3], invdir[3];
    ray_setup(x, y, cam, fr, dir, cen);
    for (int i = 0; i < 3; ++i)
        if (!finite_f(dir[i]) || !finite_f(cen[i])) return;
    float delta_scale, tmin, tmax;
    if (!ray_enter(fr, opt, dir, cen, invdir, delta_scale, tmin, tmax)) return;
    float T = 1.f;
    float t = tmin;
    while (t < tmax) {
        float pos[3];
        for (int i = 0; i < 3; ++i) pos[i] = cen[i] + t * dir[i];
        Leaf leaf;
        if (!locate(pos, leaf)) return;
        const float dt = dda_unit(leaf.local, invdir) / leaf.cube_sz + opt.step_size;
        const float sigma = half_to_float((uint16_t)leaf.sigma_bits);
        if (sigma > opt.sigma_thresh) {
            const float e = exp_(-((dt * delta_scale) * sigma));
            const float att = e < 1.f ? e : 1.f;  // fminf(e, 1.f): 1 for a NaN
            const float w = T * (1.f - att);
            update(leaf.index, w);
            T = T * att;
            if (T < opt.stop_thresh) break;
        }
        const float tn = t + dt;
        if (!(tn > t)) break;  // a step that does not advance ends the ray
        t = tn;
    }
}

}  // namespace lm
}  // namespace rto
