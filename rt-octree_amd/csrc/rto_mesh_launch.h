// rto_mesh_launch.h -- host-callable launchers of mesh_kernels.hip (rto_draw_mesh_layers, rto_meshes_trace_rays).
#pragma once
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"
#include "rto_mesh_trace.h"

namespace rto {

// As the grid's: the cameras of one launch travel BY VALUE in the kernel arguments, 32 per launch.
constexpr int kMeshCamChunk = 32;
struct MeshCams {
    CamDev c[kMeshCamChunk];
};
struct MeshDraw {
    int width, height;  // of every camera of the launch
    int merge;          // RTO_MESH_MERGE: depth-test against what depth holds (depth != nullptr then)
    float line_px, point_px;
    float background;
    float* depth;   // [frames][H][W] or nullptr, offset to the launch's first frame
    float4* color;  // [frames][H][W] or nullptr
};
// frames <= kMeshCamChunk
hipError_t launch_mesh_layers(const MeshSetDev& ms, const MeshDraw& md, const MeshCams& cams, int frames, hipStream_t stream);

struct MeshRays {
    const float* origins;  // [n][3]
    const float* dirs;     // [n][3]
    int64_t n;             // <= 2^38 per launch
    float line_spread, point_spread;
    float background;
    float* t_hit;  // [n] or nullptr
    float* rgb;    // [n][3] or nullptr
};
hipError_t launch_mesh_rays(const MeshSetDev& ms, const MeshRays& mr, hipStream_t stream);

}  // namespace rto
