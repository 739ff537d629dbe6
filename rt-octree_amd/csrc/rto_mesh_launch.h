// rto_mesh_launch.h -- host-callable launchers of mesh_kernels.hip (rto_draw_mesh_layers, rto_meshes_trace_rays).
#pragma once
#include <hip/hip_runtime.h>

#include "rto_layer_pass.h"
#include "rto_mesh_trace.h"

namespace rto {

// rto_draw_mesh_layers, a layer pass (rto_layer_pass.h)
struct MeshDraw {
    LayerTarget target;
    float line_px, point_px;
    float background;
};
// frames <= kLayerCamChunk
hipError_t launch_mesh_layers(const MeshSetDev& ms, const MeshDraw& md, const LayerCams& cams, int frames, hipStream_t stream);

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
