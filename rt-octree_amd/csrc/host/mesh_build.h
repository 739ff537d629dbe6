// host/mesh_build.h -- rto_meshes on the host: the model transform baked into world-space primitive records, and the threaded BVH
// over them (rto_mesh_trace.h has the two layouts).  No device code, no HIP: tools/sanitize/host_fuzz.cpp builds it with g++.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace rto {

// rto_mesh_desc (include/rto.h) without the header: the builder is compiled into programs that do not include it
struct MeshDescHost {
    const float* vert;
    int64_t n_verts;
    const uint32_t* faces;
    int64_t n_faces;
    int face_size;
    int unlit;
    int estimate_normals;
    float rotation[3];
    float translation[3];
    float scale;
};

struct MeshSetHost {
    std::vector<float> prims;  // [n_prims][32], in LEAF order (record k of a leaf: first + k)
    std::vector<float> nodes;  // [n_nodes][8]
    int64_t triangles = 0, segments = 0, points = 0;
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};  // world bounds of the positions (zeros for an empty set)
    int64_t n_prims() const { return (int64_t)prims.size() / 32; }
    int64_t n_nodes() const { return (int64_t)nodes.size() / 8; }
};

constexpr int64_t kMeshMaxPrims = int64_t(1) << 30;

// mesh.cpp estimate_normals: the normals of `vert` ([n][9]) overwritten by the normalised sum of the cross products of the faces
// at each vertex (double accumulation in face order, rounded to float once).  faces == nullptr: consecutive vertices.
void mesh_estimate_normals(float* vert, int64_t n_verts, const uint32_t* faces, int64_t n_faces);

// Checks the descriptions (-> false and *err: null pointers, face_size outside 1..3, an index >= n_verts, a non-finite position,
// transform or scale, more than 2^30 primitives), bakes and builds.  Deterministic: the same bytes for the same input.
bool mesh_build(const MeshDescHost* meshes, int n, MeshSetHost* out, std::string* err);

}  // namespace rto
