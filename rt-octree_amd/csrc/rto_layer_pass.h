// rto_layer_pass.h -- what a layer pass is, for kernels and launchers alike: something (the octree grid, meshes) ray-traced for the
// cameras of a call into a depth and a colour plane per camera (DESIGN.md section 7f "Layer pass").
#pragma once
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"

namespace rto {

// The cameras of one launch travel BY VALUE in the kernel arguments (64 B each; a kernarg segment holds 4 KB): no table in
// device memory, so no copy and nothing for a handle to own.  A call of more frames is split into launches of kLayerCamChunk.
constexpr int kLayerCamChunk = 32;
struct LayerCams {
    CamDev c[kLayerCamChunk];
};
struct LayerTarget {  // what every pass draws into; a pass's launch struct holds one beside its own fields
    int width, height;  // of every camera of the launch
    int merge;          // RTO_GRID_MERGE / RTO_MESH_MERGE: depth-test against what depth holds (depth != nullptr then)
    float* depth;       // [frames][H][W] or nullptr, offset to the launch's first frame
    float4* color;      // [frames][H][W] or nullptr
};

// The launch shape: a workgroup = 16x16 pixels, blockIdx.z = frame of this launch (cams.c[z], plane z of depth / color).
// launch(grid, block) starts the pass's kernel; frames <= kLayerCamChunk
template <class Launch>
hipError_t launch_layer_pass(const LayerTarget& lt, int frames, Launch launch) {
    if (frames <= 0 || lt.width <= 0 || lt.height <= 0) return hipSuccess;
    if (frames > kLayerCamChunk) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((lt.width + 15) / 16), (unsigned)((lt.height + 15) / 16), (unsigned)frames);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    launch(grid, dim3(256));
    return hipGetLastError();
}

// The pixel frame: a pass's kernel is layer_pixel_begin, its own tracing of the pixel's ray, layer_pixel_end.
// Thread -> pixel: wave w takes the 8x8 tile (w & 1, w >> 1) of the workgroup, lane l its pixel (l & 7, l >> 3), so that a wave's
// rays stay together.  idx: the pixel's index into depth / color; old: the depth the buffer holds, read under merge only.
// false: no pixel here, or an existing depth <= 0 or NaN (not traced), which the GL depth test leaves alone
RTO_DEV bool layer_pixel_begin(const LayerTarget& lt, int& x, int& y, int64_t& idx, float& old) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    x = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    y = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (x >= lt.width || y >= lt.height) return false;
    idx = ((int64_t)blockIdx.z * lt.height + y) * lt.width + x;
    old = lt.merge ? lt.depth[idx] : 0.f;
    return !lt.merge || old > 0.f;
}

// t: the pixel's depth, +inf for a miss, which is never nearer: the depth test needs no "hit &&"; (r, g, b): its colour
RTO_DEV void layer_pixel_end(const LayerTarget& lt, int64_t idx, float old, float t, float r, float g, float b) {
    if (lt.merge && !(old > t)) return;
    if (lt.depth) lt.depth[idx] = t;
    if (lt.color) lt.color[idx] = make_float4(r, g, b, 1.f);
}

}  // namespace rto
