// host/mesh_io.h -- the two mesh file formats of the reference viewer, read on the host: a basic OBJ reader (Mesh::load_basic_obj)
// and the drawlist npz (Mesh::open_drawlist, mesh.cpp _load_npz's schema).  No device code: tools/sanitize/host_fuzz.cpp builds
// it with g++.  Every function throws std::runtime_error on malformed input and never leaves an index out of range.
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "mesh_build.h"
#include "npz.h"

namespace rto {

struct MeshData {  // one mesh as the files describe it: volrend::Mesh's fields
    std::string name;
    std::vector<float> vert;      // [n][9]: position, rgb, normal
    std::vector<uint32_t> faces;  // [m][face_size]; empty: consecutive vertices
    int face_size = 3;
    bool unlit = false, visible = true, estimate_normals = false;
    float rotation[3] = {0, 0, 0}, translation[3] = {0, 0, 0}, scale = 1.f;
    MeshDescHost desc() const;  // (points into this object)
};

// OBJ text: `v x y z [r g b]`, `vn x y z`, `f` with a, a/b, a/b/c, a//c and negative indices; polygons that are no triangles are
// dropped; colours / normals are taken only when there is one per vertex, else (1, 0.5, 0.2) and estimated normals.
void parse_obj(const char* text, size_t n, MeshData* out);
void load_obj_file(const std::string& path, MeshData* out);

// drawlist: entries `<name>` = type string, `<name>__<field>` = value; meshes in the order of their names
void parse_drawlist(const std::map<std::string, NpyArray>& arrays, std::vector<MeshData>* out);
void load_drawlist_file(const std::string& path, std::vector<MeshData>* out);

// the presets the drawlist names (fresh generators; meshes.py has the same shapes)
MeshData mesh_cube(const float color[3]);
MeshData mesh_sphere(int rings, int sectors, const float color[3]);
MeshData mesh_frustum(float focal, float width, float height, float z, const float color[3]);

}  // namespace rto
