// rto_mesh_trace.h -- one ray against a mesh set (rto_meshes): the rule of DESIGN.md section 7g and the walk of the threaded BVH.
// __host__ __device__: mesh_kernels.hip (mesh_layers_kernel, mesh_rays_kernel) and rto_meshes_trace_rays_host (rto_mesh.cpp) run
// this same text.  Every operation is float32 and rounded once; include it behind `#pragma clang fp contract(off)` and build with
// -ffp-contract=off -fno-fast-math (IEEE division and square root).  tests/mesh_ref.py restates mesh_hit_* and mesh_shade in
// numpy, bit for bit, WITHOUT the BVH: the walk may only skip primitives that cannot win.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rto {

#define RTO_MESH_HD __host__ __device__ __forceinline__

// A primitive record: 32 floats = 8 float4 (128 B), world space.
//   [0..8]   positions p0 p1 p2   (segment: p0 p1; point: p0)
//   [9..17]  colours   c0 c1 c2
//   [18..26] normals   n0 n1 n2   (triangles; normalize(mat3(M) n), not renormalised after interpolation)
//   [27] kind (int: 3 triangle, 2 segment, 1 point)   [28] unlit (int)   [29] id (int: mesh order, then face order)
constexpr int kMeshPrimFloats = 32;
constexpr int kMeshKind = 27, kMeshUnlit = 28, kMeshId = 29;

// A node of the threaded BVH: 2 float4, depth-first order.
//   a = (lo.xyz, link)   link: bit 31 leaf, bit 30 the subtree holds segments or points, bits 0..29 the miss link (n_nodes = stop)
//   b = (hi.xyz, leaf)   leaf: first * 4 + (count - 1) into the records, which are stored in leaf order (internal nodes: 0)
// The node after a box hit is i + 1 (for a leaf that is its miss link too).
constexpr uint32_t kMeshLeaf = 0x80000000u, kMeshThick = 0x40000000u, kMeshLinkMask = 0x3fffffffu;

struct MeshSetDev {
    const float4* nodes;  // [n_nodes][2]
    const float4* prims;  // [n_prims][8]
    int n_nodes;
};

struct MeshHit {
    float t;      // +inf: none
    int id;       // the primitive's id, -1: none
    int rec;      // its record
    float u, v;   // triangle: barycentrics of p1, p2; segment / point: u = the clamped parameter
};

RTO_MESH_HD float mesh_as_float(uint32_t u) { return __builtin_bit_cast(float, u); }
RTO_MESH_HD uint32_t mesh_as_uint(float f) { return __builtin_bit_cast(uint32_t, f); }
RTO_MESH_HD float mesh_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
RTO_MESH_HD float mesh_min(float a, float b) { return a < b ? a : b; }
RTO_MESH_HD float mesh_max(float a, float b) { return a > b ? a : b; }

// Moeller-Trumbore, two-sided.  -> t (> 0) and (u, v), or t = +inf without a hit
RTO_MESH_HD float mesh_hit_triangle(const float* o, const float* d, const float* p0, const float* p1, const float* p2, float& u, float& v) {
    float e1[3], e2[3], tv[3], pv[3], qv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        e1[i] = p1[i] - p0[i];
        e2[i] = p2[i] - p0[i];
        tv[i] = o[i] - p0[i];
    }
    pv[0] = d[1] * e2[2] - d[2] * e2[1];
    pv[1] = d[2] * e2[0] - d[0] * e2[2];
    pv[2] = d[0] * e2[1] - d[1] * e2[0];
    const float det = mesh_dot(e1, pv);
    const float inv = 1.f / det;
    u = mesh_dot(tv, pv) * inv;
    qv[0] = tv[1] * e1[2] - tv[2] * e1[1];
    qv[1] = tv[2] * e1[0] - tv[0] * e1[2];
    qv[2] = tv[0] * e1[1] - tv[1] * e1[0];
    v = mesh_dot(d, qv) * inv;
    const float t = mesh_dot(e2, qv) * inv;
    const bool hit = det != 0.f && u >= 0.f && v >= 0.f && u + v <= 1.f && t > 0.f;
    return hit ? t : __builtin_inff();
}

// The closest approach of the ray's line to the segment a b, the segment's parameter clamped to [0, 1] (a point: a == b, s = 0).
// -> tc (> 0) and s when dist <= spread * tc, else +inf
RTO_MESH_HD float mesh_hit_segment(const float* o, const float* d, const float* a, const float* b, float spread, float& s) {
    float w[3], w0[3], c[3], diff[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        w[i] = b[i] - a[i];
        w0[i] = a[i] - o[i];
    }
    const float A = mesh_dot(w, w), bd = mesh_dot(w, d), f = mesh_dot(w0, d), g = mesh_dot(w0, w);
    const float den = A - bd * bd;
    s = den > 0.f ? (bd * f - g) / den : 0.f;
    s = mesh_min(mesh_max(s, 0.f), 1.f);  // (a NaN becomes 0)
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = w0[i] + s * w[i];
    const float tc = mesh_dot(c, d);
#pragma unroll
    for (int i = 0; i < 3; ++i) diff[i] = c[i] - tc * d[i];
    const float dist = sqrtf(mesh_dot(diff, diff));
    const bool hit = tc > 0.f && dist <= spread * tc;
    return hit ? tc : __builtin_inff();
}

// The colour of a hit (mesh.cpp's fragment shader with viewDir = -d: see include/rto.h)
RTO_MESH_HD void mesh_shade(const float* r /* the record */, const MeshHit& h, const float* d, float* rgb) {
    const int kind = (int)mesh_as_uint(r[kMeshKind]);
    if (kind != 3) {
        const float s = h.u, s0 = 1.f - s;
#pragma unroll
        for (int i = 0; i < 3; ++i) rgb[i] = s0 * r[9 + i] + s * r[12 + i];
        return;
    }
    const float b0 = (1.f - h.u) - h.v;
#pragma unroll
    for (int i = 0; i < 3; ++i) rgb[i] = (b0 * r[9 + i] + h.u * r[12 + i]) + h.v * r[15 + i];
    if (mesh_as_uint(r[kMeshUnlit]) != 0u) return;
    float n[3], l1[3], l2[3], rf[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] = (b0 * r[18 + i] + h.u * r[21 + i]) + h.v * r[24 + i];
    const float i1 = 1.f / sqrtf((0.5f * 0.5f + 0.2f * 0.2f) + 1.f * 1.f);
    const float i2 = 1.f / sqrtf((0.5f * 0.5f + 1.f * 1.f) + 0.5f * 0.5f);
    l1[0] = 0.5f * i1, l1[1] = 0.2f * i1, l1[2] = 1.f * i1;
    l2[0] = -0.5f * i2, l2[1] = -1.f * i2, l2[2] = -0.5f * i2;
    const float dn = mesh_dot(l1, n);
    const float diffuse = 0.7f * mesh_max(dn, 0.f);
    const float diffuse2 = 0.2f * mesh_max(mesh_dot(l2, n), 0.f);
#pragma unroll
    for (int i = 0; i < 3; ++i) rf[i] = (2.f * dn) * n[i] - l1[i];  // reflect(-l1, n)
    float sp = mesh_max(-mesh_dot(d, rf), 0.f);                     // dot(viewDir, reflectDir), viewDir = -d
#pragma unroll
    for (int i = 0; i < 5; ++i) sp = sp * sp;  // pow(x, 32)
    const float shade = ((0.3f + diffuse) + diffuse2) + 0.6f * sp;
#pragma unroll
    for (int i = 0; i < 3; ++i) rgb[i] = rgb[i] * shade;
}

// Does the ray reach the node's box before `best`?  Conservative against mesh_hit_*: the box is widened by pad (the float32
// error of the primitive tests, generously: 2^-12 of the largest coordinate involved) and, where the subtree holds segments or
// points, by spread * (the farthest projection of the box onto the ray) -- a hit's ray point o + tc d lies within spread * tc of
// a segment point inside the box, and tc is that point's projection.  The entry parameter may lie behind `best` by 2^-8 of it.
RTO_MESH_HD bool mesh_box_test(const float* o, const float* d, const float4& a, const float4& b, float spread, float oinf, float best) {
    const float lo[3] = {a.x, a.y, a.z}, hi[3] = {b.x, b.y, b.z};
    float m = 0.f, proj = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float l = lo[i] - o[i], h = hi[i] - o[i];
        m = mesh_max(m, mesh_max(fabsf(l), fabsf(h)));
        proj += mesh_max(l * d[i], h * d[i]);
    }
    float pad = (m + oinf) * 0x1p-12f;
    if (mesh_as_uint(a.w) & kMeshThick) pad += spread * mesh_max(proj, 0.f) * 1.0001f;
    float tn = 0.f, tf = __builtin_inff();
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float l = (lo[i] - pad) - o[i], h = (hi[i] + pad) - o[i];
        if (d[i] == 0.f) {
            if (l > 0.f || h < 0.f) return false;
        } else {
            const float inv = 1.f / d[i];
            const float t1 = l * inv, t2 = h * inv;
            tn = mesh_max(tn, mesh_min(t1, t2));
            tf = mesh_min(tf, mesh_max(t1, t2));
        }
    }
    return tn <= tf && tn <= best + best * 0x1p-8f;
}

// The nearest primitive along the ray o + t d (d unit): the smallest t, among equal t the lowest id.  Independent of the BVH's
// shape and of the visit order.
RTO_MESH_HD MeshHit mesh_trace(const MeshSetDev& ms, const float* o, const float* d, float line_spread, float point_spread) {
    MeshHit best;
    best.t = __builtin_inff();
    best.id = -1;
    best.rec = -1;
    best.u = best.v = 0.f;
    const float wide = mesh_max(line_spread, point_spread);
    const float oinf = mesh_max(mesh_max(fabsf(o[0]), fabsf(o[1])), fabsf(o[2]));
    int i = 0;
    while (i < ms.n_nodes) {
        const float4 na = ms.nodes[2 * (int64_t)i], nb = ms.nodes[2 * (int64_t)i + 1];
        const uint32_t link = mesh_as_uint(na.w);
        if (!mesh_box_test(o, d, na, nb, wide, oinf, best.t)) {
            i = (int)(link & kMeshLinkMask);
            continue;
        }
        if (link & kMeshLeaf) {
            const uint32_t leaf = mesh_as_uint(nb.w);
            const int first = (int)(leaf >> 2), count = (int)(leaf & 3u) + 1;
            for (int k = 0; k < count; ++k) {
                const float4* r = ms.prims + 8 * (int64_t)(first + k);
                const float4 q0 = r[0], q1 = r[1], q2 = r[2];
                const float4 q7 = r[6 + 1];  // [28..31]: unlit, id
                const float p0[3] = {q0.x, q0.y, q0.z}, p1[3] = {q0.w, q1.x, q1.y}, p2[3] = {q1.z, q1.w, q2.x};
                const int kind = (int)mesh_as_uint(r[6].w), id = (int)mesh_as_uint(q7.y);
                float u = 0.f, v = 0.f, t;
                if (kind == 3) {
                    t = mesh_hit_triangle(o, d, p0, p1, p2, u, v);
                } else {  // (a point is the segment p0 p0; selected by value: no pointer into a private array)
                    const bool seg = kind == 2;
                    const float pb[3] = {seg ? p1[0] : p0[0], seg ? p1[1] : p0[1], seg ? p1[2] : p0[2]};
                    t = mesh_hit_segment(o, d, p0, pb, seg ? line_spread : point_spread, u);
                }
                if (t < best.t || (t == best.t && id < best.id)) {
                    best.t = t;
                    best.id = id;
                    best.rec = first + k;
                    best.u = u;
                    best.v = v;
                }
            }
        }
        ++i;
    }
    return best;
}

// (t, rgb) of a ray: the hit's depth and colour, or (+inf, background)
RTO_MESH_HD float mesh_trace_shade(const MeshSetDev& ms, const float* o, const float* d, float line_spread, float point_spread,
                              float background, float* rgb) {
    const MeshHit h = mesh_trace(ms, o, d, line_spread, point_spread);
    if (h.id < 0) {
        rgb[0] = rgb[1] = rgb[2] = background;
        return __builtin_inff();
    }
    float r[kMeshPrimFloats];
    const float4* q = ms.prims + 8 * (int64_t)h.rec;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float4 x = q[k];
        r[4 * k] = x.x, r[4 * k + 1] = x.y, r[4 * k + 2] = x.z, r[4 * k + 3] = x.w;
    }
    mesh_shade(r, h, d, rgb);
    return h.t;
}

// rto_meshes_trace_rays' ray: the direction normalised as rto_launch_rays does; false = degenerate (a direction that cannot be
// normalised, a non-finite origin), which is a miss
RTO_MESH_HD bool mesh_ray_from(const float* origin, const float* dir, float* o, float* d) {
    const float inv = 1.f / sqrtf(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        d[i] = dir[i] * inv;
        o[i] = origin[i];
        ok = ok && __builtin_isfinite(d[i]) && __builtin_isfinite(o[i]);
    }
    return ok && (d[0] != 0.f || d[1] != 0.f || d[2] != 0.f);
}

}  // namespace rto
