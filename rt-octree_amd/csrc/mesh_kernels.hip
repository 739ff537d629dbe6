// mesh_kernels.hip -- meshes (triangles, lines, points) ray-traced into a depth and a colour layer (rto_draw_mesh_layers) and
// for arbitrary rays (rto_meshes_trace_rays).
//
// What the reference draws: Mesh::draw over its fragment shader (renderer/src/mesh.cpp:100-161, 366-397) in the GL pass of
// cuda_renderer.cpp:96-111.  Here there is no rasteriser: a pixel is a ray and the answer is the nearest primitive along it
// (DESIGN.md section 7g holds the rule).  One thread per pixel walks the threaded BVH of rto_mesh_trace.h -- no stack, no private
// array, no LDS, no atomics; a wave covers an 8x8 pixel tile so that its lanes visit the same nodes.  Every operation is float32
// and rounded once (contract off, IEEE division and square root): tests/mesh_ref.py restates the rule in numpy bit for bit.
#include <hip/hip_runtime.h>

#include "rto_mesh_launch.h"

#pragma clang fp contract(off)

#include "rto_mesh_trace.h"

namespace rto {

// A layer pass (rto_layer_pass.h: launch shape, LayerTarget, LayerCams) that keeps the text of the pixel frame and of ray_setup's
// pixel ray (volrend.cu:23-34) written out: built from layer_pixel_begin / layer_pixel_end, and from a ray helper shared with the
// render kernels, it ran 1.3 % (sphere, batched) to 2.6 % (frusta, lone frame) slower, each half about half of that
// (profiles/layer_pass_ab.txt).  wave w = the 8x8 tile (w & 1, w >> 1) of the 16x16 workgroup, lane l its pixel (l & 7, l >> 3)
__global__ void __launch_bounds__(256) mesh_layers_kernel(const MeshSetDev ms, const MeshDraw md, const LayerCams cams) {
    const LayerTarget& lt = md.target;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), y = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (x >= lt.width || y >= lt.height) return;
    const int64_t idx = ((int64_t)blockIdx.z * lt.height + y) * lt.width + x;
    float old = 0.f;
    if (lt.merge) {  // the GL depth test against what the buffers hold; a depth <= 0 or NaN (not traced) is left alone
        old = lt.depth[idx];
        if (!(old > 0.f)) return;
    }
    const CamDev& cam = cams.c[blockIdx.z];
    const float xyz[3] = {(x - 0.5f * cam.width) / cam.fx, -(y - 0.5f * cam.height) / cam.fy, -1.0f};
    const float* m = cam.transform;
    float d[3];
    d[0] = m[0] * xyz[0] + m[3] * xyz[1] + m[6] * xyz[2];
    d[1] = m[1] * xyz[0] + m[4] * xyz[1] + m[7] * xyz[2];
    d[2] = m[2] * xyz[0] + m[5] * xyz[1] + m[8] * xyz[2];
    const float inv = 1.f / sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    d[0] *= inv;
    d[1] *= inv;
    d[2] *= inv;
    const float o[3] = {m[9], m[10], m[11]};
    float rgb[3];
    const float t = mesh_trace_shade(ms, o, d, (0.5f * md.line_px) / cam.fx, (0.5f * md.point_px) / cam.fx, md.background, rgb);
    if (lt.merge) {
        if (!(old > t)) return;  // (a miss is +inf: never nearer)
    }
    if (lt.depth) lt.depth[idx] = t;
    if (lt.color) lt.color[idx] = make_float4(rgb[0], rgb[1], rgb[2], 1.f);
}

// one thread per ray
__global__ void __launch_bounds__(256) mesh_rays_kernel(const MeshSetDev ms, const MeshRays mr) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= mr.n) return;
    float og[3], dg[3], o[3], d[3], rgb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        og[c] = mr.origins[3 * i + c];
        dg[c] = mr.dirs[3 * i + c];
    }
    float t = __builtin_inff();
    rgb[0] = rgb[1] = rgb[2] = mr.background;
    if (mesh_ray_from(og, dg, o, d)) t = mesh_trace_shade(ms, o, d, mr.line_spread, mr.point_spread, mr.background, rgb);
    if (mr.t_hit) mr.t_hit[i] = t;
    if (mr.rgb) {
        mr.rgb[3 * i] = rgb[0];
        mr.rgb[3 * i + 1] = rgb[1];
        mr.rgb[3 * i + 2] = rgb[2];
    }
}

hipError_t launch_mesh_layers(const MeshSetDev& ms, const MeshDraw& md, const LayerCams& cams, int frames, hipStream_t stream) {
    return launch_layer_pass(md.target, frames, [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(mesh_layers_kernel, grid, block, 0, stream, ms, md, cams);
    });
}

hipError_t launch_mesh_rays(const MeshSetDev& ms, const MeshRays& mr, hipStream_t stream) {
    if (mr.n <= 0) return hipSuccess;
    const int64_t blocks = (mr.n + 255) / 256;
    if (blocks > (int64_t(1) << 30)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mesh_rays_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, ms, mr);
    return hipGetLastError();
}

}  // namespace rto
