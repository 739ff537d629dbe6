// rto_mesh.cpp -- the mesh part of the C ABI (include/rto.h "meshes"): rto_meshes handles, rto_draw_mesh_layers,
// rto_meshes_trace_rays and its host twin.  The baking and the BVH are host/mesh_build.cpp, the rule is rto_mesh_trace.h.
#include <cmath>
#include <cstring>

#include <stdexcept>

#include "host/mesh_build.h"
#include "host/mesh_io.h"
#include "rto_internal.h"
#include "rto_mesh_launch.h"

#pragma clang fp contract(off)

#include "rto_mesh_trace.h"

struct rto_meshes {
    int device = -1;  // < 0: host only
    rto::MeshSetHost host;
    void* d_nodes = nullptr;
    void* d_prims = nullptr;
    int64_t device_bytes = 0;
};

namespace {

rto::MeshSetDev dev_view(const rto_meshes* m) {
    rto::MeshSetDev v;
    v.nodes = (const float4*)m->d_nodes;
    v.prims = (const float4*)m->d_prims;
    v.n_nodes = (int)m->host.n_nodes();
    return v;
}

}  // namespace

extern "C" {

int rto_meshes_create(const rto_mesh_desc* meshes, int n, int device, rto_meshes** out) {
    if (!out) return set_err(RTO_E_INVALID, "rto_meshes_create: null out");
    *out = nullptr;
    if (n < 0) return set_err(RTO_E_INVALID, "rto_meshes_create: n must be >= 0");
    if (n > 0 && !meshes) return set_err(RTO_E_INVALID, "rto_meshes_create: null meshes with n > 0");
    std::vector<rto::MeshDescHost> descs((size_t)n);
    for (int i = 0; i < n; ++i) {
        rto::MeshDescHost& d = descs[i];
        d.vert = meshes[i].vert;
        d.n_verts = meshes[i].n_verts;
        d.faces = meshes[i].faces;
        d.n_faces = meshes[i].n_faces;
        d.face_size = meshes[i].face_size;
        d.unlit = meshes[i].unlit;
        d.estimate_normals = meshes[i].estimate_normals;
        std::memcpy(d.rotation, meshes[i].rotation, sizeof(d.rotation));
        std::memcpy(d.translation, meshes[i].translation, sizeof(d.translation));
        d.scale = meshes[i].scale;
    }
    rto_meshes* m = new rto_meshes;
    std::string err;
    if (!rto::mesh_build(descs.data(), n, &m->host, &err)) {
        delete m;
        return set_err(RTO_E_INVALID, "rto_meshes_create: " + err);
    }
    m->device = device < 0 ? -1 : device;
    if (device >= 0 && m->host.n_prims() > 0) {
        DeviceGuard guard(device);
        const size_t nb = m->host.nodes.size() * sizeof(float), pb = m->host.prims.size() * sizeof(float);
        hipError_t e = guard.ok ? hipSuccess : hipErrorInvalidDevice;
        if (e == hipSuccess) e = hipMalloc(&m->d_nodes, nb);
        if (e == hipSuccess) e = hipMalloc(&m->d_prims, pb);
        if (e == hipSuccess) e = hipMemcpy(m->d_nodes, m->host.nodes.data(), nb, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(m->d_prims, m->host.prims.data(), pb, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (m->d_nodes) (void)hipFree(m->d_nodes);
            if (m->d_prims) (void)hipFree(m->d_prims);
            delete m;
            return set_err(RTO_E_HIP, std::string("rto_meshes_create: upload failed: ") + hipGetErrorString(e));
        }
        m->device_bytes = (int64_t)(nb + pb);
    }
    *out = m;
    return RTO_OK;
}

int rto_meshes_load_files(const char* const* paths, int n, int device, rto_meshes** out) {
    if (!out) return set_err(RTO_E_INVALID, "rto_meshes_load: null out");
    *out = nullptr;
    if (n < 0 || (n > 0 && !paths)) return set_err(RTO_E_INVALID, "rto_meshes_load: null paths or n < 0");
    std::vector<rto::MeshData> all;
    for (int i = 0; i < n; ++i) {
        if (!paths[i]) return set_err(RTO_E_INVALID, "rto_meshes_load: null path");
        const std::string path = paths[i];
        std::string ext = path.size() >= 4 ? path.substr(path.size() - 4) : "";
        for (char& c : ext) c = (char)tolower((unsigned char)c);
        if (ext != ".obj" && ext != ".npz")
            return set_err(RTO_E_FORMAT, "rto_meshes_load: " + path + ": the extension must be .obj or .npz (a drawlist)");
        FILE* f = fopen(path.c_str(), "rb");
        if (!f) return set_err(RTO_E_IO, "rto_meshes_load: cannot open " + path);
        fclose(f);
        try {
            if (ext == ".obj") {
                rto::MeshData m;
                rto::load_obj_file(path, &m);
                all.push_back(std::move(m));
            } else {
                std::vector<rto::MeshData> list;
                rto::load_drawlist_file(path, &list);
                for (rto::MeshData& m : list)
                    if (m.visible) all.push_back(std::move(m));
            }
        } catch (const std::exception& e) {
            return set_err(RTO_E_FORMAT, "rto_meshes_load: " + path + ": " + e.what());
        }
    }
    std::vector<rto_mesh_desc> descs(all.size());
    for (size_t i = 0; i < all.size(); ++i) {
        const rto::MeshDescHost h = all[i].desc();
        rto_mesh_desc& d = descs[i];
        d.vert = h.vert;
        d.n_verts = h.n_verts;
        d.faces = h.faces;
        d.n_faces = h.n_faces;
        d.face_size = h.face_size;
        d.unlit = h.unlit;
        d.estimate_normals = h.estimate_normals;
        std::memcpy(d.rotation, h.rotation, sizeof(d.rotation));
        std::memcpy(d.translation, h.translation, sizeof(d.translation));
        d.scale = h.scale;
    }
    const int rc = rto_meshes_create(descs.data(), (int)descs.size(), device, out);
    return rc == RTO_E_INVALID ? set_err(RTO_E_FORMAT, std::string("rto_meshes_load: ") + rto_last_error()) : rc;
}

int rto_meshes_load(const char* path, int device, rto_meshes** out) { return rto_meshes_load_files(&path, 1, device, out); }

int rto_meshes_get_info(const rto_meshes* m, rto_meshes_info* info) {
    if (!m || !info) return set_err(RTO_E_INVALID, "rto_meshes_get_info: null argument");
    info->triangles = m->host.triangles;
    info->segments = m->host.segments;
    info->points = m->host.points;
    info->nodes = m->host.n_nodes();
    info->device_bytes = m->device_bytes;
    for (int i = 0; i < 3; ++i) {
        info->lo[i] = m->host.lo[i];
        info->hi[i] = m->host.hi[i];
    }
    info->device = m->device;
    return RTO_OK;
}

int rto_meshes_download(const rto_meshes* m, float* prims, float* nodes) {
    if (!m) return set_err(RTO_E_INVALID, "rto_meshes_download: null set");
    if (prims && !m->host.prims.empty()) std::memcpy(prims, m->host.prims.data(), m->host.prims.size() * sizeof(float));
    if (nodes && !m->host.nodes.empty()) std::memcpy(nodes, m->host.nodes.data(), m->host.nodes.size() * sizeof(float));
    return RTO_OK;
}

void rto_meshes_free(rto_meshes* m) {
    if (!m) return;
    if (m->d_nodes || m->d_prims) {
        DeviceGuard guard(m->device);
        if (m->d_nodes) (void)hipFree(m->d_nodes);
        if (m->d_prims) (void)hipFree(m->d_prims);
    }
    delete m;
}

void rto_mesh_params_default(rto_mesh_params* p, const rto_options* o) {
    if (!p) return;
    rto_options def;
    if (!o) {
        rto_options_default(&def);
        o = &def;
    }
    p->line_px = 1.f;
    p->point_px = 1.f;
    p->background = o->background_brightness;
    p->flags = 0;
}

int rto_draw_mesh_layers(const rto_meshes* m, const rto_camera* cams, int n, const rto_mesh_params* p, float* depth, float* color,
                         void* stream_) {
    static_assert(RTO_MESH_MERGE == 1, "check_layer_call takes bit 0 of the flags for the merge flag");
    const int rc = check_layer_call("rto_draw_mesh_layers", "set", "RTO_MESH_MERGE", m, cams, n, p, depth, color, [&]() -> const char* {
        if (!(std::isfinite(p->line_px) && p->line_px > 0.f && std::isfinite(p->point_px) && p->point_px > 0.f))
            return "line_px and point_px must be finite and > 0";
        if (!std::isfinite(p->background)) return "the background must be finite";
        return nullptr;
    });
    if (rc != RTO_OK) return rc;
    if (m->device < 0) return set_err(RTO_E_INVALID, "rto_draw_mesh_layers: a host-only set (device < 0) cannot be drawn on a GPU");
    if (n == 0) return RTO_OK;
    DeviceGuard guard(m->device);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    const rto::MeshSetDev ms = dev_view(m);
    rto::MeshDraw md;
    md.line_px = p->line_px;
    md.point_px = p->point_px;
    md.background = p->background;
    return launch_layer_chunks("mesh", cams, n, p->flags, depth, color, [&](const rto::LayerTarget& lt, const rto::LayerCams& lc, int k) {
        md.target = lt;
        return rto::launch_mesh_layers(ms, md, lc, k, (hipStream_t)stream_);
    });
}

static int check_rays(const char* fn, const rto_meshes* m, const rto_mesh_rays* r, const float* t_hit, const float* rgb) {
    const std::string at = std::string(fn) + ": ";
    if (!m || !r) return set_err(RTO_E_INVALID, at + "null set or rays");
    if (!t_hit && !rgb) return set_err(RTO_E_INVALID, at + "t_hit and rgb are both null");
    if (r->n < 0) return set_err(RTO_E_INVALID, at + "n must be >= 0");
    if (r->n > 0 && (!r->origins || !r->dirs)) return set_err(RTO_E_INVALID, at + "null origins or dirs with n > 0");
    if (!(std::isfinite(r->line_spread) && r->line_spread >= 0.f && std::isfinite(r->point_spread) && r->point_spread >= 0.f))
        return set_err(RTO_E_INVALID, at + "line_spread and point_spread must be finite and >= 0");
    if (!std::isfinite(r->background)) return set_err(RTO_E_INVALID, at + "the background must be finite");
    return RTO_OK;
}

int rto_meshes_trace_rays(const rto_meshes* m, const rto_mesh_rays* r, float* t_hit, float* rgb, void* stream_) {
    const int rc = check_rays("rto_meshes_trace_rays", m, r, t_hit, rgb);
    if (rc != RTO_OK) return rc;
    if (m->device < 0) return set_err(RTO_E_INVALID, "rto_meshes_trace_rays: a host-only set (device < 0) cannot be traced on a GPU");
    if (r->n == 0) return RTO_OK;
    DeviceGuard guard(m->device);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    const rto::MeshSetDev ms = dev_view(m);
    const int64_t per_launch = int64_t(1) << 38;
    for (int64_t i0 = 0; i0 < r->n; i0 += per_launch) {
        rto::MeshRays mr;
        mr.origins = r->origins + 3 * i0;
        mr.dirs = r->dirs + 3 * i0;
        mr.n = std::min(per_launch, r->n - i0);
        mr.line_spread = r->line_spread;
        mr.point_spread = r->point_spread;
        mr.background = r->background;
        mr.t_hit = t_hit ? t_hit + i0 : nullptr;
        mr.rgb = rgb ? rgb + 3 * i0 : nullptr;
        const hipError_t e = rto::launch_mesh_rays(ms, mr, (hipStream_t)stream_);
        if (e != hipSuccess) return set_err(RTO_E_HIP, std::string("mesh rays launch failed: ") + hipGetErrorString(e));
    }
    return RTO_OK;
}

int rto_meshes_trace_rays_host(const rto_meshes* m, const rto_mesh_rays* r, float* t_hit, float* rgb) {
    const int rc = check_rays("rto_meshes_trace_rays_host", m, r, t_hit, rgb);
    if (rc != RTO_OK) return rc;
    rto::MeshSetDev ms;
    ms.nodes = (const float4*)m->host.nodes.data();
    ms.prims = (const float4*)m->host.prims.data();
    ms.n_nodes = (int)m->host.n_nodes();
    for (int64_t i = 0; i < r->n; ++i) {
        float o[3], d[3], c[3] = {r->background, r->background, r->background};
        float t = __builtin_inff();
        if (rto::mesh_ray_from(r->origins + 3 * i, r->dirs + 3 * i, o, d))
            t = rto::mesh_trace_shade(ms, o, d, r->line_spread, r->point_spread, r->background, c);
        if (t_hit) t_hit[i] = t;
        if (rgb) {
            rgb[3 * i] = c[0];
            rgb[3 * i + 1] = c[1];
            rgb[3 * i + 2] = c[2];
        }
    }
    return RTO_OK;
}

}  // extern "C"
