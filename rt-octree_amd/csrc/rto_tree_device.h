// rto_tree_device.h -- device functions that more than one translation unit of the library states the tree's answers with:
// the view-direction basis (SH, SG / ASG, the basis_minmax mask), the reference's float descent over child[], and the
// entry <-> slot relations of the two-level traversal image.  The render units (render_kernels.hip's map) and query_kernels.hip include it; the
// functions are force-inlined, so each kernel's code is what it was when they stood beside the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"

#pragma clang fp contract(off)

namespace rto {

// lumisphere.hpp:38-80; double literals, one rounding per assignment
RTO_DEV void sh_basis(int basis_dim, const float* dir, float* out) {
    out[0] = 0.28209479177387814;
    const float x = dir[0], y = dir[1], z = dir[2];
    const float xx = x * x, yy = y * y, zz = z * z;
    const float xy = x * y, yz = y * z, xz = x * z;
    switch (basis_dim) {
        case 25:
            out[16] = 2.5033429417967046 * xy * (xx - yy);
            out[17] = -1.7701307697799304 * yz * (3 * xx - yy);
            out[18] = 0.9461746957575601 * xy * (7 * zz - 1.f);
            out[19] = -0.6690465435572892 * yz * (7 * zz - 3.f);
            out[20] = 0.10578554691520431 * (zz * (35 * zz - 30) + 3);
            out[21] = -0.6690465435572892 * xz * (7 * zz - 3);
            out[22] = 0.47308734787878004 * (xx - yy) * (7 * zz - 1.f);
            out[23] = -1.7701307697799304 * xz * (xx - 3 * yy);
            out[24] = 0.6258357354491761 * (xx * (xx - 3 * yy) - yy * (3 * xx - yy));
            [[fallthrough]];
        case 16:
            out[9] = -0.5900435899266435 * y * (3 * xx - yy);
            out[10] = 2.890611442640554 * xy * z;
            out[11] = -0.4570457994644658 * y * (4 * zz - xx - yy);
            out[12] = 0.3731763325901154 * z * (2 * zz - 3 * xx - 3 * yy);
            out[13] = -0.4570457994644658 * x * (4 * zz - xx - yy);
            out[14] = 1.445305721320277 * z * (xx - yy);
            out[15] = -0.5900435899266435 * x * (xx - 3 * yy);
            [[fallthrough]];
        case 9:
            out[4] = 1.0925484305920792 * xy;
            out[5] = -1.0925484305920792 * yz;
            out[6] = 0.31539156525252005 * (2.0 * zz - xx - yy);
            out[7] = -1.0925484305920792 * xz;
            out[8] = 0.5462742152960396 * (xx - yy);
            [[fallthrough]];
        case 4:
            out[1] = -0.4886025119029199 * y;
            out[2] = 0.4886025119029199 * z;
            out[3] = -0.4886025119029199 * x;
    }
}

// rodrigues (volrend.cu:58-73): only the view direction of the basis lookup turns
RTO_DEV void rotate_vdir(const OptDev& opt, float* vdir) {
    if (opt.rot_on) {
        const float* k = opt.rot_k;
        const float cross[3] = {k[1] * vdir[2] - k[2] * vdir[1], k[2] * vdir[0] - k[0] * vdir[2],
                                k[0] * vdir[1] - k[1] * vdir[0]};
        const float dot = k[0] * vdir[0] + k[1] * vdir[1] + k[2] * vdir[2];
#pragma unroll
        for (int i = 0; i < 3; ++i)  // float + float, then + (float * float) * double in double, one rounding
            vdir[i] = (float)((double)(vdir[i] * opt.rot_cos + cross[i] * opt.rot_sin) + (double)(k[i] * dot) * opt.rot_omc);
    }
}

// basis function i of an SG / ASG tree (LOBES = kFmtSG / kFmtASG) for the rotated view direction d; fB = (float)basis_dim
template <int LOBES>
RTO_DEV float lobe_basis(const TreeDev& tree, int i, const float* d, float fB) {
    const RTO_CONST float* lobes = (const RTO_CONST float*)tree.extra;
    if constexpr (LOBES == kFmtSG)
        return sg_lobe(d, lobes + 4 * i, fB);
    else
        return asg_lobe(d, lobes + 11 * i, fB);
}

// basis for the ray + the basis_minmax mask (rt_core.cuh:277-284).  LOBES = 0: SH and RGBA trees (the format is read at run
// time); kFmtSG / kFmtASG: a tree of that format -- a template argument, so that the SH instantiations carry no lobe code
template <int LOBES = 0>
RTO_DEV void ray_basis(const TreeDev& tree, const OptDev& opt, const float* vdir_in, float* basis_fn) {
#pragma unroll
    for (int i = 0; i < RTO_BASIS_MAX_DEV; ++i) basis_fn[i] = 0.f;
    float vdir[3] = {vdir_in[0], vdir_in[1], vdir_in[2]};
    rotate_vdir(opt, vdir);
    if constexpr (LOBES != 0) {
        const int B = tree.basis_dim;
        const float fB = (float)B;  // (maybe_precalc_basis divides by the int basis_dim)
#pragma unroll
        for (int i = 0; i < RTO_BASIS_MAX_DEV; ++i)
            if (i < B) basis_fn[i] = lobe_basis<LOBES>(tree, i, vdir, fB);
    } else {
        if (tree.format == kFmtSH) sh_basis(tree.basis_dim, vdir, basis_fn);
    }
#pragma unroll
    for (int i = 0; i < RTO_BASIS_MAX_DEV; ++i)
        if (i < opt.basis_minmax[0] || i > opt.basis_minmax[1]) basis_fn[i] = 0.f;
}

// ray_basis for any tree, the format read at run time (the generic kernel, the basis probe)
RTO_DEV void ray_basis_any(const TreeDev& tree, const OptDev& opt, const float* vdir_in, float* basis_fn) {
    if (tree.format == kFmtSG)
        ray_basis<kFmtSG>(tree, opt, vdir_in, basis_fn);
    else if (tree.format == kFmtASG)
        ray_basis<kFmtASG>(tree, opt, vdir_in, basis_fn);
    else
        ray_basis(tree, opt, vdir_in, basis_fn);
}

// n3tree_query.hpp:13-48
RTO_DEV int64_t query_from_root(const TreeDev& tree, float* xyz, float& cube_sz) {
    const float fN = (float)tree.N;
    xyz[0] = f_max(f_min(xyz[0], 1.f - 1e-6f), 0.f);
    xyz[1] = f_max(f_min(xyz[1], 1.f - 1e-6f), 0.f);
    xyz[2] = f_max(f_min(xyz[2], 1.f - 1e-6f), 0.f);
    int64_t ptr = 0;
    cube_sz = fN;
    while (true) {
        float index = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            xyz[i] *= fN;
            const float idx_dimi = floorf(xyz[i]);
            index = index * fN + idx_dimi;
            xyz[i] -= idx_dimi;
        }
        const int64_t sub_ptr = ptr + (int32_t)index;
        const int64_t skip = tree.child[sub_ptr];
        if (skip == 0) return sub_ptr;
        cube_sz *= fN;
        ptr += skip * tree.N3;
    }
}

// hit index of the wide image (= the index of the leaf's entry) -> the leaf's slot in data[] / shrec[] (what a hit entry
// names): a grid cell's leaf through wgslot; an entry of a wide node is child a of its octree node (when that is a leaf) or
// child b of that child
RTO_DEV uint32_t wide_to_slot(const TreeDev& tree, uint32_t u) {
    const uint32_t pad = tree.wide_grid_nodes * 64u;
    if (u < pad) return tree.wgslot[u];  // a leaf cell of the top grid
    const uint32_t v = u - pad, wn = v >> 6, x2 = (v >> 4) & 3u, y2 = (v >> 2) & 3u, z2 = v & 3u;
    const uint32_t a = (x2 >> 1) << 2 | (y2 >> 1) << 1 | (z2 >> 1), b = (x2 & 1u) << 2 | (y2 & 1u) << 1 | (z2 & 1u);
    const uint32_t N = tree.worig[wn];
    const uint32_t w0 = tree.nodew[N * 8u + a];
    return nodew_is_leaf(w0) ? N * 8u + a : (N + w0) * 8u + b;
}

// entry of the two-level image that holds the point (ix, iy, iz) (24-bit fixed point): the walk of render_fast, from the grid
RTO_DEV uint32_t wide_entry_of(const TreeDev& tree, uint32_t ix, uint32_t iy, uint32_t iz) {
    const int G = tree.top_levels;
    uint32_t node = 0u, slot;
    int pr = -1;
    for (;;) {
        const uint32_t b = node ? 2u : (uint32_t)G, msk = (1u << b) - 1u;
        const uint32_t off = node ? (uint32_t)(22 - G - 2 * pr) : 24u - (uint32_t)G;
        slot = (((node << b | ((ix >> off) & msk)) << b | ((iy >> off) & msk)) << b) | ((iz >> off) & msk);
        const uint32_t w = tree.widew[slot];
        if (nodew_is_leaf(w)) return slot;
        node = w;
        ++pr;
    }
}

}  // namespace rto
