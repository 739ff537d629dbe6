// rto_render_shared.h -- the device pieces the render kernel bodies (rto_render_fast.inc, rto_render_generic.inc) are built from:
// ray set-up, the pixel / ray outputs, the workgroup tiles, hit-list entries and the packed leaf shading.  Included by
// the render units (frame_kernels.hip, render_kernels.hip, shade_kernels.hip) and by depth_kernels.hip (the depth-carrying
// instantiations of the same bodies): translation units of their own so that they compile side by side.  Everything here is RTO_DEV (forced inline) or constexpr.  Include it behind the
// translation unit's `#pragma clang fp contract(off)`: the bodies are compared bit for bit with the CPU oracle.
#pragma once
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"
#include "rto_tree_device.h"

namespace rto {

// ------------------------------------------------------------------ shared pieces

// A pointer loaded from device memory (the frame table's aux / image / hits) is generic to the compiler, which then issues
// flat_load / flat_store for it.  It is device memory: typed as a global-address-space pointer the accesses become
// global_load / global_store.
#define RTO_GLOBAL __attribute__((address_space(1)))
template <class T>
RTO_DEV RTO_GLOBAL T* as_global(T* p) {
    return (RTO_GLOBAL T*)p;
}

// cuda/common.cuh:16-27
RTO_DEV float norm3(const float* d) { return sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]); }
RTO_DEV void normalize3(float* d) {
    const float invnorm = 1.f / norm3(d);
    d[0] *= invnorm;
    d[1] *= invnorm;
    d[2] *= invnorm;
}

// volrend.cu:35-56,142-144: a ray's (dir, cen) in world space -> tree space (the NDC warp, then offset + scale * cen)
RTO_DEV void ray_to_tree(const TreeDev& tree, float* dir, float* cen) {
    if (tree.ndc_width > 0) {  // maybe_world2ndc :35-56
        const float t = -(1.f + cen[2]) / dir[2];
        for (int i = 0; i < 3; ++i) cen[i] = cen[i] + t * dir[i];
        dir[0] = -((2 * tree.ndc_focal) / tree.ndc_width) * (dir[0] / dir[2] - cen[0] / cen[2]);
        dir[1] = -((2 * tree.ndc_focal) / tree.ndc_height) * (dir[1] / dir[2] - cen[1] / cen[2]);
        dir[2] = -2 / cen[2];
        cen[0] = -((2 * tree.ndc_focal) / tree.ndc_width) * (cen[0] / cen[2]);
        cen[1] = -((2 * tree.ndc_focal) / tree.ndc_height) * (cen[1] / cen[2]);
        cen[2] = 1 + 2 / cen[2];
        normalize3(dir);
    }
    for (int i = 0; i < 3; ++i) cen[i] = tree.offset[i] + tree.scale[i] * cen[i];
}

// volrend.cu:23-56,138-144: pixel -> (dir, vdir, cen) in tree space
RTO_DEV void ray_setup(int x, int y, const CamDev& cam, const TreeDev& tree, float* dir, float* vdir,
                       float* cen) {
    const float xyz[3] = {(x - 0.5f * cam.width) / cam.fx, -(y - 0.5f * cam.height) / cam.fy, -1.0f};
    const float* m = cam.transform;
    dir[0] = m[0] * xyz[0] + m[3] * xyz[1] + m[6] * xyz[2];
    dir[1] = m[1] * xyz[0] + m[4] * xyz[1] + m[7] * xyz[2];
    dir[2] = m[2] * xyz[0] + m[5] * xyz[1] + m[8] * xyz[2];
    normalize3(dir);
    cen[0] = m[9];
    cen[1] = m[10];
    cen[2] = m[11];
    vdir[0] = dir[0];
    vdir[1] = dir[1];
    vdir[2] = dir[2];
    ray_to_tree(tree, dir, cen);
}

// rto_launch_rays: ray i of the batch -> (dir, vdir, cen) in tree space, the way ray_setup turns a pixel's (M xyz, centre)
// into them, and its depth limit and backdrop.  false: a degenerate ray, which is not traced (its result is the backdrop with
// alpha 0) -- a direction normalize3 cannot normalise (zero, NaN, infinite, or a squared length that under- / overflows),
// a non-finite origin or NDC image of it, a t_max that is not > 0 (NaN included)
RTO_DEV bool ray_from_batch(const RayBatch& rb, uint32_t i, const TreeDev& tree, float bg_default, float* dir, float* vdir,
                            float* cen, float& tmax_bg, float* bg) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        dir[c] = rb.dirs[3 * (uint64_t)i + c];
        cen[c] = rb.origins[3 * (uint64_t)i + c];
        bg[c] = rb.background ? rb.background[3 * (uint64_t)i + c] : bg_default;
    }
    tmax_bg = rb.t_max ? rb.t_max[i] : 1e9f;
    normalize3(dir);
    vdir[0] = dir[0];
    vdir[1] = dir[1];
    vdir[2] = dir[2];
    ray_to_tree(tree, dir, cen);
    bool ok = tmax_bg > 0.f && (dir[0] != 0.f || dir[1] != 0.f || dir[2] != 0.f);
#pragma unroll
    for (int c = 0; c < 3; ++c) ok = ok && __builtin_isfinite(dir[c]) && __builtin_isfinite(cen[c]);
    return ok;
}

// block b's ray for thread tid (RayBatch::per_xcd); >= rb.n: none
RTO_DEV uint32_t ray_index(const RayBatch& rb, uint32_t b, int tid) {
    const uint32_t chunk = rb.per_xcd ? (b & 7u) * rb.per_xcd + (b >> 3) : b;
    return chunk * 256u + (uint32_t)tid;
}

// volrend.cu:161-185 with offscreen = false, per ray: the result composited over the ray's backdrop, alpha = accumulated opacity
RTO_DEV void write_ray(const RayBatch& rb, uint32_t i, const float* bg, float* out) {
    const float nalpha = 1.f - out[3];
    out[0] += bg[0] * nalpha;
    out[1] += bg[1] * nalpha;
    out[2] += bg[2] * nalpha;
    rb.out[i] = make_float4(out[0], out[1], out[2], out[3]);
}

// rt_core.cuh:206-222: scale dir, invdir, slab test.  returns false when the ray misses the box.
// SEQ: one axis after the other (scheduling barriers): the three double-precision reciprocals and slab tests interleaved keep
// ~30 VGPRs busy, which the reservoir kernel -- it sets a tile up while its lanes hold rays in flight -- does not have
template <bool SEQ = false>
RTO_DEV bool ray_enter(const TreeDev& tree, const OptDev& opt, float* dir, const float* cen, float tmax_bg,
                       float* invdir, float& delta_scale, float& tmin, float& tmax) {
    dir[0] *= tree.scale[0];
    dir[1] *= tree.scale[1];
    dir[2] *= tree.scale[2];
    delta_scale = 1.f / norm3(dir);
    dir[0] *= delta_scale;
    dir[1] *= delta_scale;
    dir[2] *= delta_scale;
    tmax_bg /= delta_scale;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        invdir[i] = 1.f / (dir[i] + 1e-9);  // double
        if (SEQ) __builtin_amdgcn_sched_barrier(0);
    }
    tmin = 0.0;
    tmax = 1e4;
#pragma unroll
    for (int i = 0; i < 3; ++i) {  // _dda_world :19-36, double sub-expressions
        const float t1 = (opt.render_bbox[i] + 1e-6 - cen[i]) * invdir[i];
        const float t2 = (opt.render_bbox[i + 3] - 1e-6 - cen[i]) * invdir[i];
        tmin = f_max(tmin, f_min(t1, t2));
        tmax = f_min(tmax, f_max(t1, t2));
        if (SEQ) __builtin_amdgcn_sched_barrier(0);
    }
    tmax = f_min(tmax, tmax_bg);
    return !(tmax < 0 || tmin > tmax);
}

// min(max(x, 0), 1 - 1e-6) (n3tree_query.hpp:20-24 clamp) as one v_med3_f32: the same value for every
// finite x (the sign of a zero result may differ, which no later operation can observe: the
// fixed-point conversion, fract * invdir and the sums that follow give the same numbers)
RTO_DEV float clamp_unit(float x) { return __builtin_amdgcn_fmed3f(x, 0.f, 1.f - 1e-6f); }
// The batched kernels keep a ray's position SCALED by 2^24 (kPos24): cen and dir are multiplied by 2^24 once, at the ray's
// set-up, and cen24 + t * dir24 is then 2^24 times cen + t * dir bit for bit (a power of two commutes with every rounding),
// so the fixed-point coordinates are a bare float -> integer conversion of the clamped sum -- no multiply per march step --
// and the leaf-local point frac(pos * 2^(level + 1)) is frac(pos24 * 2^(level - 23)).
constexpr float kPos24 = 16777216.f;
RTO_DEV float clamp_unit24(float x) { return __builtin_amdgcn_fmed3f(x, 0.f, (1.f - 1e-6f) * kPos24); }

// _dda_unit rt_core.cuh:38-51
RTO_DEV float dda_unit(const float* p, const float* invdir) {
    float tm = 1e4;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float t1 = -p[i] * invdir[i];
        const float t2 = t1 + invdir[i];
        tm = f_min(tm, f_max(t1, t2));
    }
    return tm;
}

// ray_basis for a tree KNOWN to hold B SH basis functions per channel (the shading kernel's record layouts): the same values in
// basis_fn[0 .. B-1] -- the only ones shade_leaf_packed<3 B + 1> / shade_leaf_quant<B> read -- without the run-time switch over
// the basis size, the 25-entry clear and the 25 mask tests (a third of the ~220 instructions the basis cost per hit entry)
template <int B>
RTO_DEV void ray_basis_sh(const OptDev& opt, const float* vdir_in, float* basis_fn) {
    float vdir[3] = {vdir_in[0], vdir_in[1], vdir_in[2]};
    rotate_vdir(opt, vdir);
    float full[RTO_BASIS_MAX_DEV];
    sh_basis(B, vdir, full);  // (B is a constant: the switch folds)
#pragma unroll
    for (int i = 0; i < B; ++i) basis_fn[i] = full[i];
    if (opt.basis_minmax[0] > 0 || opt.basis_minmax[1] < B - 1) {  // (uniform; the default options mask nothing)
#pragma unroll
        for (int i = 0; i < B; ++i)
            if (i < opt.basis_minmax[0] || i > opt.basis_minmax[1]) basis_fn[i] = 0.f;
    }
}

// The same for an SG / ASG tree KNOWN to hold B lobes (LOBES = kFmtSG / kFmtASG; the shading kernel's record layouts, B = 9 /
// 16 / 25): ray_basis<LOBES>'s values in basis_fn[0 .. B-1], each lobe record at a constant offset of the kernel argument
template <int LOBES, int B>
RTO_DEV void ray_basis_lobes(const TreeDev& tree, const OptDev& opt, const float* vdir_in, float* basis_fn) {
    float vdir[3] = {vdir_in[0], vdir_in[1], vdir_in[2]};
    rotate_vdir(opt, vdir);
#pragma unroll
    for (int i = 0; i < B; ++i) basis_fn[i] = lobe_basis<LOBES>(tree, i, vdir, (float)B);
    if (opt.basis_minmax[0] > 0 || opt.basis_minmax[1] < B - 1) {
#pragma unroll
        for (int i = 0; i < B; ++i)
            if (i < opt.basis_minmax[0] || i > opt.basis_minmax[1]) basis_fn[i] = 0.f;
    }
}

// rt_core.cuh:286-325 for one hit leaf: out[0..2] += cnt * sigmoid(<basis, coeffs>), out[3] += cnt.
// The summation order (DC, then the 16..24 group, 9..15, 4..8, 1..3, each left to right) is part of
// the result.
RTO_DEV void shade_leaf(const TreeDev& tree, const uint16_t* __restrict__ tv, const float* basis_fn, float cnt,
                        float* out) {
    const int basis_dim = tree.basis_dim;
    if (basis_dim >= 0) {
        int off = 0;
        float t3[3], o3[3];
#define MUL_BASIS_I(k) (basis_fn[k] * half_bits_to_float(tv[off + (k)]))
        for (int c = 0; c < 3; ++c) {
            float tmp = basis_fn[0] * half_bits_to_float(tv[off]);
            switch (basis_dim) {
                case 25:
                    tmp += MUL_BASIS_I(16) + MUL_BASIS_I(17) + MUL_BASIS_I(18) + MUL_BASIS_I(19) + MUL_BASIS_I(20) +
                           MUL_BASIS_I(21) + MUL_BASIS_I(22) + MUL_BASIS_I(23) + MUL_BASIS_I(24);
                    [[fallthrough]];
                case 16:
                    tmp += MUL_BASIS_I(9) + MUL_BASIS_I(10) + MUL_BASIS_I(11) + MUL_BASIS_I(12) + MUL_BASIS_I(13) +
                           MUL_BASIS_I(14) + MUL_BASIS_I(15);
                    [[fallthrough]];
                case 9:
                    tmp += MUL_BASIS_I(4) + MUL_BASIS_I(5) + MUL_BASIS_I(6) + MUL_BASIS_I(7) + MUL_BASIS_I(8);
                    [[fallthrough]];
                case 4:
                    tmp += MUL_BASIS_I(1) + MUL_BASIS_I(2) + MUL_BASIS_I(3);
            }
            t3[c] = tmp;
            off += basis_dim;
        }
#undef MUL_BASIS_I
        sigmoid_cnt3(t3, cnt, o3);  // out[c] += cnt / (1.f + det_expf(-tmp)), rt_core.cuh:314-318
        for (int c = 0; c < 3; ++c) out[c] += o3[c];
    } else {
        for (int j = 0; j < 3; ++j) out[j] += half_bits_to_float(tv[j]) * cnt;
    }
    out[3] += cnt;
}

// volrend.cu:174-212 (offscreen): background composite, 8 aux planes, RGBA32F image, alpha = 1
RTO_DEV void write_pixel(const FrameOut& fo, int64_t SIZE, int idx, float bg, float* out) {
    const float nalpha = 1.f - out[3];
    const float remain = bg * nalpha;
    out[0] += remain;
    out[1] += remain;
    out[2] += remain;
    float* a = fo.aux + idx;
    a[0] = out[0];
    a[SIZE] = out[1];
    a[2 * SIZE] = out[2];
    a[3 * SIZE] = out[3];
    a[4 * SIZE] = out[0] * out[0];
    a[5 * SIZE] = out[1] * out[1];
    a[6 * SIZE] = out[2] * out[2];
    a[7 * SIZE] = out[3] * out[3];
    reinterpret_cast<float4*>(fo.image)[idx] = make_float4(out[0], out[1], out[2], 1.0f);
}

// ---- the layers of rto_ctx_set_layers (RenderContext::offscreen = false: surf_obj_depth / surf_obj, volrend.cu:146-153,162-184)
// backdrop of pixel i (an index into the launch's colour planes): its rgb, or the options' brightness without a colour layer
RTO_DEV void layer_backdrop(const LayerDev& layers, uint32_t i, float bg_default, float* bg) {
    bg[0] = bg[1] = bg[2] = bg_default;
    if (layers.color) {
        const float4 c = layers.color[i];
        bg[0] = c.x;
        bg[1] = c.y;
        bg[2] = c.z;
    }
}

// ray_from_batch's verdict on a pixel's ray after ray_setup (tree-space dir / cen) with the depth tmax_bg: false = not traced,
// the pixel is its backdrop with alpha 0 (a depth that is not > 0, NaN included; a camera that yields no finite ray)
RTO_DEV bool ray_is_live(float tmax_bg, const float* dir, const float* cen) {
    bool ok = tmax_bg > 0.f && (dir[0] != 0.f || dir[1] != 0.f || dir[2] != 0.f);
#pragma unroll
    for (int c = 0; c < 3; ++c) ok = ok && __builtin_isfinite(dir[c]) && __builtin_isfinite(cen[c]);
    return ok;
}

// write_pixel over a per-pixel backdrop (write_ray's composite: out += bg * (1 - alpha) per channel), same outputs
RTO_DEV void write_pixel_over(const FrameOut& fo, int64_t SIZE, int idx, const float* bg, float* out) {
    const float nalpha = 1.f - out[3];
    out[0] += bg[0] * nalpha;
    out[1] += bg[1] * nalpha;
    out[2] += bg[2] * nalpha;
    float* a = fo.aux + idx;
    a[0] = out[0];
    a[SIZE] = out[1];
    a[2 * SIZE] = out[2];
    a[3 * SIZE] = out[3];
    a[4 * SIZE] = out[0] * out[0];
    a[5 * SIZE] = out[1] * out[1];
    a[6 * SIZE] = out[2] * out[2];
    a[7 * SIZE] = out[3] * out[3];
    reinterpret_cast<float4*>(fo.image)[idx] = make_float4(out[0], out[1], out[2], 1.0f);
}

// the depth outputs of ray / pixel i (DepthOut): dsum is already scaled by 1 / SPP
RTO_DEV void write_depth(const DepthOut& d, uint32_t i, float dsum, float tnear) {
    if (d.depth) d.depth[i] = dsum;
    if (d.t_near) d.t_near[i] = tnear;
}

// ------------------------------------------------------------------ fast kernel (N == 2): tiles, hit entries, packed shading

constexpr int kTileW = 32, kTileH = 8;  // workgroup tile; each wave owns an 8x8 sub-tile

// workgroup -> tile (XCD-interleaved strips, rto_kernel_types.h TileMap)
RTO_DEV bool block_tile(const TileMap& tm, int b, int& tx, int& ty) {
    const int xcd = b & 7, q = b >> 3;
    const int per_strip = tm.strip_rows * tm.tiles_x;
    const int j = q / per_strip, rem = q - j * per_strip;
    ty = (j * 8 + xcd) * tm.strip_rows + rem / tm.tiles_x;
    tx = rem % tm.tiles_x;
    return ty < tm.tiles_y;
}

// Layout of the traversal -> shading hand-off buffer, per frame ("split", round 3): entry 0 of every pixel in a dense plane
// [H*W], entries 1.. pixel-major [H*W][SPP-1] behind it -- a pixel's thresholds / hit list behind entry 0 are one contiguous
// run (20 B at SPP 6), and the thresholds kernel writes entry 0 of an 8x8 tile as eight 32-byte row segments instead of 64
// dwords at a 24-byte stride (0.66 -> 0.43 ms per 100 frames for marks + lists + thresholds).  The planar [SPP][H*W] layout of
// round 1 and the plain pixel-major one of round 2 (shading 1.96 vs 2.17 ms) are history.
template <int SPP>
RTO_DEV uint32_t hit_index(uint32_t pixel, uint32_t i, uint32_t SIZE) {
    return i == 0u ? pixel : SIZE + pixel * (uint32_t)(SPP - 1) + (i - 1u);
}
// distance between entries i and i + 1 of a pixel for i >= 1
RTO_DEV uint32_t hit_stride(uint32_t) { return 1u; }

// Hit list entry: leaf slot in the low hit_slot_bits(SPP) bits, (count - 1) above, kHitValid on top (rto_kernel_types.h).
template <int SPP>
RTO_DEV uint32_t hit_pack(uint32_t slot, uint32_t cnt) { return kHitValid | slot | ((cnt - 1u) << hit_slot_bits(SPP)); }
template <int SPP>
RTO_DEV uint32_t hit_slot(uint32_t h) { return h & ((1u << hit_slot_bits(SPP)) - 1u); }
template <int SPP>
RTO_DEV uint32_t hit_count(uint32_t h) { return ((h & ~kHitValid) >> hit_slot_bits(SPP)) + 1u; }

// The record's DD - 1 coefficients as packed halves al[k >> 1] (half k at its packed position) -> the leaf's contribution.
template <int DD>
RTO_DEV void shade_leaf_words(const uint32_t* al, const float* basis_fn, float cnt, float* out) {
    constexpr int B = (DD - 1) / 3;
    // basis_fn[j] * (float)coefficient k, the half widened by the multiply itself (mul_half_lo / _hi: one instruction, same float)
    auto bc = [&](int j, int k) -> float { return (k & 1) ? mul_half_hi(al[k >> 1], basis_fn[j]) : mul_half_lo(al[k >> 1], basis_fn[j]); };
    float t3[3], o3[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int off = c * B;
        float tmp = bc(0, off);
        if constexpr (B >= 25) {
            tmp += bc(16, off + 16) + bc(17, off + 17) + bc(18, off + 18) + bc(19, off + 19) + bc(20, off + 20) + bc(21, off + 21) +
                   bc(22, off + 22) + bc(23, off + 23) + bc(24, off + 24);
        }
        if constexpr (B >= 16) {
            tmp += bc(9, off + 9) + bc(10, off + 10) + bc(11, off + 11) + bc(12, off + 12) + bc(13, off + 13) + bc(14, off + 14) +
                   bc(15, off + 15);
        }
        if constexpr (B >= 9) {
            tmp += bc(4, off + 4) + bc(5, off + 5) + bc(6, off + 6) + bc(7, off + 7) + bc(8, off + 8);
        }
        if constexpr (B >= 4) {
            tmp += bc(1, off + 1) + bc(2, off + 2) + bc(3, off + 3);
        }
        t3[c] = tmp;
    }
    sigmoid_cnt3(t3, cnt, o3);  // out[c] += cnt / (1.f + det_expf(-tmp)), rt_core.cuh:314-318
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] += o3[c];
    out[3] += cnt;
}

// Loads the `DD` fp16 values of one leaf record with aligned dword loads and shades it.
// DD = data_dim (28 for SH9, 49 for SH16); the record starts at a 2-byte aligned address.
// halves per record of the aligned SH-coefficient copy (TreeDev::shrec): the 3 B coefficients in a power-of-two stride,
// so that a record lies in ONE 128-byte line -- SH9 64 B, SH16 128 B.  (Measured, 100 frames of the bench scene: SH16
// shading 2.53 ms from data[], 2.36 with 96-byte records, 2.24 with 128-byte ones; SH25 records -- 150 B -- gain
// nothing at 160 B and lose at 256 B, so SH25 trees are shaded from data[].)
__host__ __device__ constexpr int shrec_halves(int basis_dim) { return 3 * basis_dim * 2 <= 64 ? 32 : 64; }

template <int DD>
RTO_DEV void shade_leaf_packed(const TreeDev& tree, uint32_t slot, const float* basis_fn, float cnt, float* out) {
    constexpr int B = (DD - 1) / 3;
    constexpr int NAL = (DD + 1) / 2;
    uint32_t al[NAL];
    if (B <= 16 && tree.shrec) {
        // the aligned copy: 16-byte loads, every coefficient already at its packed position, one 128-byte line per
        // record (a 98-byte record at a 2-byte aligned address straddles 1.76 lines on average)
        constexpr int NQ = (3 * B * 2 + 15) / 16;  // 16-byte loads that hold coefficients
        // (compact records: the slot's record index first -- one more dependent 4-byte gather per hit leaf)
        const uint32_t ridx = tree.recidx ? tree.recidx[slot] : slot;
        const uint4* __restrict__ q = reinterpret_cast<const uint4*>(tree.shrec + (uint64_t)ridx * shrec_halves(B));
        uint4 v[NQ];
#pragma unroll
        for (int i = 0; i < NQ; ++i) v[i] = q[i];
#pragma unroll
        for (int i = 0; i < NAL; ++i) {
            const uint4& w = v[i >> 2];
            al[i] = (i & 3) == 0 ? w.x : (i & 3) == 1 ? w.y : (i & 3) == 2 ? w.z : w.w;
        }
    } else {
        constexpr int NDW = (DD + 2) / 2;  // dwords covering DD halves at either alignment
        const uint64_t hoff = (uint64_t)slot * DD;  // in halves
        const uint32_t odd = (uint32_t)hoff & 1u;
        const uint32_t* __restrict__ p = reinterpret_cast<const uint32_t*>(tree.data + (hoff - odd));
        uint32_t dw[NDW];
#pragma unroll
        for (int i = 0; i < NDW; ++i) dw[i] = p[i];
        // bring half k of the record to packed position k: a funnel shift by 0 or 16 bits per dword
        // (v_alignbit_b32) instead of extracting every coefficient at both alignments and selecting
        const uint32_t sh = odd * 16u;
#pragma unroll
        for (int i = 0; i < NAL; ++i) al[i] = __builtin_amdgcn_alignbit(i + 1 < NDW ? dw[i + 1] : 0u, dw[i], sh);
    }
    shade_leaf_words<DD>(al, basis_fn, cnt, out);
}

// Waves per SIMD render_fast is built for.  A lone frame does not care (it waits for its longest rays on a nearly empty chip);
// callers with several frames in flight do: 5 waves (96 VGPRs; the spills are in the shading tail) lift the pipelined reference
// loop from 5.65 k to 6.07 k frames/s with the sequential one unchanged, 6 waves give 6.1 k and cost the lone frame 1 %
// (profiles/r4_w_ab_fast_wps.txt).  The large-SPP instantiations keep 4 (their threshold / hit arrays live in registers).
#ifndef RTO_FAST_WPS
#define RTO_FAST_WPS 5
#endif

// ------------------------------------------------------------------ persistent kernel (N == 2): what rto_render_persist.inc is built from
// (moved verbatim from render_kernels.hip: render_persist / render_persist_layers there and render_persist_depth in depth_kernels.hip
//  are the same body)

// the per-ray state that survives between march steps (thresholds live in LDS, hits go straight
// to the hand-off buffer)
struct RayState {
    float cen[3], dir[3], invdir[3];
    float pos[3];  // 2^24 * clamp(cen + t * dir, 0, 1 - 1e-6): the point the next march step starts from (scaled: kPos24)
    float delta_scale, t, tmax, src, cur;      // cur = next threshold to cross (dst[spp])
    uint32_t spp;
    uint32_t pix, piy, piz;
    int prev_lvl;   // level of the node about to be visited
    uint32_t hoff, hnext;  // index of this pixel's next free hit entry in the hand-off buffer, and of the one behind it
                           // (staged hit lists, the default: of its entries 0 and 1, fixed for the ray's life)
    uint32_t nh;           // staged hit lists: hit entries of this ray parked in LDS, not yet written out
    uint32_t node;  // node about to be visited; kGridNext = the top grid is visited next (two-level image: 0 = the grid)
    uint32_t woff;  // two-level image: lowest of the coordinate bits that index the node about to be visited
    uint32_t wb;    // two-level image: coordinate bits per axis that index it -- G at the grid, 2 at a wide node (round 5: kept with
                    // the ray instead of re-derived from `node` by a compare + select in every iteration)
    float cxy __attribute__((ext_vector_type(2)));  // cen[0], cen[1] as a register pair for the packed march arithmetic
    // _dda_unit's max(t1, t1 + invdir) per axis is t1 + (invdir > 0 ? invdir : 0): the sign of invdir is the ray's, not the
    // step's (exit_add below)
    float exit_add[3];
};
constexpr uint32_t kGridNext = 0xffffffffu;
constexpr int kCamFloats = 14;  // fx, fy, transform[12]: what a ray set-up reads of a FrameDesc

// Staged hit lists (round 4, VERDICT r3 task 5; -DRTO_HITS_DIRECT restores the store per hit): a ray's hit entries wait in LDS -- in the rows of its threshold column that
// its consumed thresholds left free -- and are written to the hand-off buffer when the ray has ended: entry 0 into the dense
// plane, entries 1.. as one contiguous run (4 * (n - 1) bytes of ONE 32-byte sector for SPP <= 9), back to back, instead of
// one 4-byte store per hit at the moment it happens (71.6 M scattered dwords per 100 frames cost 2.48 GB of line-granular
// HBM writes for 0.29 GB of payload: the L2 had evicted the sector long before the pixel's next entry arrived).
template <int SPP, bool WIDE>
RTO_DEV void flush_hits(RayState& rs, const TreeDev& tree, uint32_t* __restrict__ hits, const float* s_col, uint32_t hstride,
                        bool translate = true) {
    uint32_t e[SPP];
#pragma unroll
    for (int i = 0; i < SPP; ++i) {
        e[i] = 0u;
        if ((uint32_t)i < rs.nh) {
            e[i] = __float_as_uint(s_col[i * 256]);
            if constexpr (WIDE) {
                constexpr uint32_t smask = (1u << hit_slot_bits(SPP)) - 1u;
                // (off the march loop: the ray has ended; !translate: entry-ordered records, TreeDev::rec_by_entry -- the entry IS the record)
                if (translate) e[i] = (e[i] & ~smask) | wide_to_slot(tree, e[i] & smask);
            }
        }
    }
    hits[rs.hoff] = e[0];
    uint32_t* tp = hits + rs.hnext;
#pragma unroll
    for (int i = 1; i < SPP; ++i)
        if ((uint32_t)i < rs.nh) tp[(uint32_t)(i - 1) * hstride] = e[i];
    rs.nh = 0;
}

// Waves per SIMD the default instantiation is built for.  Round 3: 7 (72 VGPRs).  Round 4: 8 (64 VGPRs; the spills this forces are
// in the ray set-up) -- with the shorter two-level loop one more resident wave is worth more than the spills cost: C2 4.69 -> 4.57,
// C4 13.27 -> 12.71, C5 2.96 -> 2.88 ms per 100 frames in one box (profiles/r4_u_ab_wps8.txt).  Tuning key refill = 732: the 7-wave build.
#ifndef RTO_WPS_DEFAULT
#define RTO_WPS_DEFAULT 8
#endif

// render_persist_depth: a ray's index into the depth planes of a batched launch (DepthOut: plane f = batch frame f) from the offset
// of its first hit entry, rs.hoff = frame * SPP * SIZE + pixel (hit_index): frame * SIZE + pixel.  Derived at the ray's flush
// (one integer division per ray that hit something) instead of parked beside hoff / hnext
template <int SPP>
RTO_DEV uint32_t depth_plane_index(uint32_t hoff, uint32_t SIZE) {
    if constexpr (SPP == 1) return hoff;
    const uint32_t frame = hoff / ((uint32_t)SPP * SIZE);
    return hoff - frame * ((uint32_t)(SPP - 1) * SIZE);
}

// render_persist_depth, at a ray's flush (both sites, in front of flush_hits): the ray's two hand-off offsets back from the rows
// they were parked in at its set-up (s_offs), and its pixel's depth outputs from the two accumulator rows (s_acc: the sum over
// its hits, its first hit's distance) stored to plane `frame` of dout
template <int SPP>
RTO_DEV void depth_flush(RayState& rs, const uint32_t* s_offs, const float* s_acc, const DepthOut& dout, uint32_t SIZE) {
    rs.hoff = s_offs[0];
    rs.hnext = s_offs[256];
    write_depth(dout, depth_plane_index<SPP>(rs.hoff, SIZE), s_acc[0] * (1.0f / SPP), s_acc[256]);
}

}  // namespace rto
