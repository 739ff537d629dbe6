// grid_kernels.hip -- the octree grid (RenderOptions::show_grid) ray-traced into a depth and a colour layer (rto_draw_grid_layers).
//
// What the reference draws (relative to /root/reference): the wireframe of the tree cut off at grid_max_depth, as GL lines
//   N3Tree::gen_wireframe   renderer/src/n3tree.cpp:390-434          the cells: child == 0 || depth >= max_depth
//   the GL pass             renderer/src/cuda/cuda_renderer.cpp:112-124
// Here: one thread per pixel walks the truncated tree cell by cell along its ray and looks for cell edges at the faces it
// crosses (DESIGN.md section 7f holds the rule and why it measures the PERPENDICULAR distance to an edge's line).  A wave covers
// an 8x8 pixel tile, so that its lanes stay in the same cells; no LDS, no atomics.  Every operation is float32 and rounded once
// (contract off, IEEE division and square root): tests/grid_ref.py restates the kernel in numpy bit for bit.
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"
#include "rto_tree_device.h"
#include "rto_launch.h"

#pragma clang fp contract(off)

#include "rto_render_shared.h"
#include "rto_tree_walk.h"

namespace rto {

RTO_DEV float sel3(const float* v, int a) { return a == 0 ? v[0] : a == 1 ? v[1] : v[2]; }

// The edge test at the face point p (local coordinates of a cell of side 1 / cs) reached at ray parameter tau on a face whose
// normal is axis a: for each in-face axis j the nearer of the two edges that run along the third axis k.  -> the smallest world
// distance dc (along the unit ray, at closest approach) among the edges hit, +inf without one.
//   dw: the unit world direction; sc: the tree's scale; ds: delta_scale; kk = (0.5 line_px) / fx
RTO_DEV float grid_edge_test(const float* p, float tau, int a, float cs, const float* dw, const float* sc, float ds, float kk) {
    float best = __builtin_inff();
    const float tw = tau * ds;
    const float dn = sel3(dw, a);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int j = s == 0 ? (a == 0 ? 1 : 0) : (a == 2 ? 1 : 2);
        const int k = 3 - a - j;
        const float p_j = sel3(p, j);
        const float b = p_j >= 0.5f ? 1.f : 0.f;
        const float pj = ((p_j - b) / cs) / sel3(sc, j);  // signed world offset to the edge
        const float dj = sel3(dw, j);
        const float q = dj * dj + dn * dn;
        const float perp = (fabsf(pj) * fabsf(dn)) / sqrtf(q);  // the ray's perpendicular distance to the edge's line
        const float ts = (-(pj * dj)) / q;
        const float dc = tw + ts;
        const float r = kk * dc;
        const float pk = sel3(p, k) + ((ts * sel3(dw, k)) * sel3(sc, k)) * cs;
        const float wk = (r * sel3(sc, k)) * cs;
        const bool ok = dc > 0.f && perp <= r && pk >= -wk && pk <= 1.f + wk;  // (q == 0: NaN, every comparison false)
        if (ok && dc < best) best = dc;
    }
    return best;
}

// a layer pass (rto_layer_pass.h): the pixel frame around the walk of this pixel's ray
__global__ void __launch_bounds__(256) grid_layers_kernel(const TreeDev tree, const int walk, const GridDraw gd, const LayerCams cams) {
    int x, y;
    int64_t idx;
    float old;
    if (!layer_pixel_begin(gd.target, x, y, idx, old)) return;
    const CamDev& cam = cams.c[blockIdx.z];
    float dir[3], dw[3], cen[3];
    ray_setup(x, y, cam, tree, dir, dw, cen);  // (no NDC tree gets here: dw = dir = the unit world direction)
    // rt_core.cuh:206-211 in float: the direction in tree space, renormalised
#pragma unroll
    for (int i = 0; i < 3; ++i) dir[i] *= tree.scale[i];
    const float ds = 1.f / norm3(dir);
#pragma unroll
    for (int i = 0; i < 3; ++i) dir[i] *= ds;
    // slab test against [0, 1]^3; axp: the entry face's axis, -1 with the camera inside the box
    float tn[3], tf[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float t1 = (0.f - cen[i]) / dir[i], t2 = (1.f - cen[i]) / dir[i];
        tn[i] = f_min(t1, t2);
        tf[i] = f_max(t1, t2);
    }
    float tmin = tn[0];
    int axp = 0;
    if (tn[1] > tmin) {
        tmin = tn[1];
        axp = 1;
    }
    if (tn[2] > tmin) {
        tmin = tn[2];
        axp = 2;
    }
    const float tmax = f_min(f_min(tf[0], tf[1]), tf[2]);
    if (!(tmin > 0.f)) {
        tmin = 0.f;
        axp = -1;
    }
    const float kk = (0.5f * gd.line_px) / cam.fx;
    const int Lmax = gd.max_depth + 1;
    float best = __builtin_inff();
    float t = tmin;
    for (int it = 3 * (1 << Lmax) + 8; it > 0 && t < tmax; --it) {
        float pos[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) pos[i] = f_max(f_min(cen[i] + t * dir[i], 1.f - 1e-6f), 0.f);
        const int level = walk_point<true>(tree, walk, pos).level;
        if (level < 1) break;  // (cannot happen, see walk_point)
        const int L = level < Lmax ? level : Lmax;
        const float cs = __uint_as_float((uint32_t)(127 + L) << 23);  // cube_sz = 2^L
        float u[3], tu[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            u[i] = pos[i] * cs;
            u[i] -= floorf(u[i]);  // (both exact: the cell is pos's fixed point masked at L)
            tu[i] = dir[i] == 0.f ? __builtin_inff() : ((dir[i] > 0.f ? 1.f : 0.f) - u[i]) / dir[i];
        }
        float tsl = tu[0];
        int axo = 0;
        if (tu[1] < tsl) {
            tsl = tu[1];
            axo = 1;
        }
        if (tu[2] < tsl) {
            tsl = tu[2];
            axo = 2;
        }
        float e[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) e[i] = u[i] + tsl * dir[i];
        const float te = t + tsl / cs;
        if (axp >= 0) best = grid_edge_test(u, t, axp, cs, dw, tree.scale, ds, kk);
        best = f_min(best, grid_edge_test(e, te, axo, cs, dw, tree.scale, ds, kk));
        if (best < __builtin_inff()) break;
        t = te + 1e-5f;
        axp = axo;
    }
    const bool line = best < __builtin_inff();
    const float bg = gd.background;
    layer_pixel_end(gd.target, idx, old, best, line ? gd.color_rgb[0] : bg, line ? gd.color_rgb[1] : bg, line ? gd.color_rgb[2] : bg);
}

hipError_t launch_grid_layers(const TreeDev& tree, int walk, const GridDraw& gd, const LayerCams& cams, int frames, hipStream_t stream) {
    return launch_layer_pass(gd.target, frames, [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(grid_layers_kernel, grid, block, 0, stream, tree, walk, gd, cams);
    });
}

}  // namespace rto
