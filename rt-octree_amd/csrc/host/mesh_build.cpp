// host/mesh_build.cpp -- see mesh_build.h.  DESIGN.md section 7g has the bake (double precision, rounded to float once) and the
// BVH (median split of the centroids along their longest axis, leaves of at most 4, depth-first with miss links).
#include "mesh_build.h"

#include <math.h>
#include <string.h>

#include <algorithm>

namespace rto {
namespace {

struct Item {
    float lo[3], hi[3];
    float cen[3];
    int64_t id;  // index of the primitive in draw order = of its record in `recs`
};

struct Builder {
    std::vector<Item> items;
    const std::vector<float>* recs;  // draw order
    MeshSetHost* out;

    static uint32_t f2u(float f) {
        uint32_t u;
        memcpy(&u, &f, 4);
        return u;
    }
    static float u2f(uint32_t u) {
        float f;
        memcpy(&f, &u, 4);
        return f;
    }

    // -> whether the subtree holds a segment or a point
    bool build(int64_t b, int64_t e) {
        const int64_t idx = out->n_nodes();
        out->nodes.resize(out->nodes.size() + 8);
        float lo[3], hi[3], clo[3], chi[3];
        for (int a = 0; a < 3; ++a) {
            lo[a] = clo[a] = INFINITY;
            hi[a] = chi[a] = -INFINITY;
        }
        for (int64_t i = b; i < e; ++i)
            for (int a = 0; a < 3; ++a) {
                lo[a] = std::min(lo[a], items[i].lo[a]);
                hi[a] = std::max(hi[a], items[i].hi[a]);
                clo[a] = std::min(clo[a], items[i].cen[a]);
                chi[a] = std::max(chi[a], items[i].cen[a]);
            }
        bool thick = false;
        uint32_t leafw = 0, leaf = 0;
        if (e - b <= 4) {
            std::sort(items.begin() + b, items.begin() + e, [](const Item& x, const Item& y) { return x.id < y.id; });
            const int64_t first = out->n_prims();
            for (int64_t i = b; i < e; ++i) {
                const float* r = recs->data() + 32 * items[i].id;
                out->prims.insert(out->prims.end(), r, r + 32);
                if (f2u(r[27]) != 3u) thick = true;
            }
            leaf = 0x80000000u;
            leafw = (uint32_t)(first * 4 + (e - b - 1));
        } else {
            int ax = 0;
            if (chi[1] - clo[1] > chi[ax] - clo[ax]) ax = 1;
            if (chi[2] - clo[2] > chi[ax] - clo[ax]) ax = 2;
            std::sort(items.begin() + b, items.begin() + e, [ax](const Item& x, const Item& y) {
                return x.cen[ax] < y.cen[ax] || (x.cen[ax] == y.cen[ax] && x.id < y.id);
            });
            const int64_t mid = b + (e - b) / 2;
            const bool t1 = build(b, mid);
            const bool t2 = build(mid, e);
            thick = t1 || t2;
        }
        float* n = out->nodes.data() + 8 * idx;
        for (int a = 0; a < 3; ++a) {
            n[a] = lo[a];
            n[4 + a] = hi[a];
        }
        n[3] = u2f(leaf | (thick ? 0x40000000u : 0u) | (uint32_t)out->n_nodes());  // the miss link: the node after this subtree
        n[7] = u2f(leafw);
        return thick;
    }
};

bool fail(std::string* err, const std::string& msg) {
    if (err) *err = msg;
    return false;
}

bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

}  // namespace

void mesh_estimate_normals(float* vert, int64_t n_verts, const uint32_t* faces, int64_t n_faces) {
    if (!faces) n_faces = n_verts / 3;
    std::vector<double> acc((size_t)n_verts * 3, 0.0);
    for (int64_t f = 0; f < n_faces; ++f) {
        int64_t ix[3];
        for (int j = 0; j < 3; ++j) ix[j] = faces ? (int64_t)faces[3 * f + j] : 3 * f + j;
        if (ix[0] >= n_verts || ix[1] >= n_verts || ix[2] >= n_verts) continue;
        double a[3], b[3];
        for (int j = 0; j < 3; ++j) {
            a[j] = (double)vert[9 * ix[1] + j] - (double)vert[9 * ix[0] + j];
            b[j] = (double)vert[9 * ix[2] + j] - (double)vert[9 * ix[0] + j];
        }
        const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) acc[3 * ix[j] + k] += c[k];
    }
    for (int64_t i = 0; i < n_verts; ++i) {
        const double* c = &acc[3 * i];
        const double len = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
        for (int k = 0; k < 3; ++k) vert[9 * i + 6 + k] = len > 0.0 && std::isfinite(len) ? (float)(c[k] / len) : 0.f;
    }
}

bool mesh_build(const MeshDescHost* meshes, int n, MeshSetHost* out, std::string* err) {
    *out = MeshSetHost();
    if (n < 0) return fail(err, "n must be >= 0");
    if (n > 0 && !meshes) return fail(err, "null meshes with n > 0");
    int64_t total = 0;
    for (int m = 0; m < n; ++m) {
        const MeshDescHost& d = meshes[m];
        const std::string at = "mesh " + std::to_string(m) + ": ";
        if (d.face_size < 1 || d.face_size > 3) return fail(err, at + "face_size must be 1, 2 or 3");
        if (d.n_verts < 0 || d.n_faces < 0) return fail(err, at + "negative n_verts or n_faces");
        if (d.n_verts > 0 && !d.vert) return fail(err, at + "null vert with n_verts > 0");
        if (!finite3(d.rotation) || !finite3(d.translation) || !std::isfinite(d.scale))
            return fail(err, at + "a non-finite rotation, translation or scale");
        const int64_t nf = d.faces ? d.n_faces : d.n_verts / d.face_size;
        total += nf;
        if (total > kMeshMaxPrims) return fail(err, "more than 2^30 primitives");
        if (d.faces)
            for (int64_t i = 0; i < nf * d.face_size; ++i)
                if ((int64_t)d.faces[i] >= d.n_verts) return fail(err, at + "a face index >= n_verts");
        for (int64_t i = 0; i < d.n_verts; ++i)
            if (!finite3(d.vert + 9 * i)) return fail(err, at + "a non-finite position");
    }
    std::vector<float> recs;
    recs.reserve((size_t)total * 32);
    std::vector<float> w;  // the mesh's vertices in world space: position, colour, normal
    for (int m = 0; m < n; ++m) {
        const MeshDescHost& d = meshes[m];
        w.assign(d.vert, d.vert + 9 * d.n_verts);
        if (d.estimate_normals && d.face_size == 3) mesh_estimate_normals(w.data(), d.n_verts, d.faces, d.n_faces);
        // Mesh::draw: M = rotation(axis-angle) * scale, then the translation; |r| < 1e-3 is the identity
        const double r[3] = {d.rotation[0], d.rotation[1], d.rotation[2]};
        const double ang = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
        double M[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        if (!(ang < 1e-3)) {
            const double a[3] = {r[0] / ang, r[1] / ang, r[2] / ang};
            const double c = cos(ang), s = sin(ang), k = 1.0 - c;
            const double X[3][3] = {{0, -a[2], a[1]}, {a[2], 0, -a[0]}, {-a[1], a[0], 0}};
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) M[i][j] = ((i == j ? c : 0.0) + k * (a[i] * a[j])) + s * X[i][j];
        }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) M[i][j] *= (double)d.scale;
        for (int64_t i = 0; i < d.n_verts; ++i) {
            float* v = w.data() + 9 * i;
            const double p[3] = {v[0], v[1], v[2]}, nn[3] = {v[6], v[7], v[8]};
            double q[3];
            for (int c = 0; c < 3; ++c) {
                v[c] = (float)(((M[c][0] * p[0] + M[c][1] * p[1]) + M[c][2] * p[2]) + (double)d.translation[c]);
                q[c] = (M[c][0] * nn[0] + M[c][1] * nn[1]) + M[c][2] * nn[2];
            }
            const double len = sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
            for (int c = 0; c < 3; ++c) v[6 + c] = len > 0.0 && std::isfinite(len) ? (float)(q[c] / len) : 0.f;
            if (!finite3(v)) return fail(err, "mesh " + std::to_string(m) + ": a position overflows in world space");
        }
        const int64_t nf = d.faces ? d.n_faces : d.n_verts / d.face_size;
        for (int64_t f = 0; f < nf; ++f) {
            float rec[32] = {0};
            for (int j = 0; j < d.face_size; ++j) {
                const int64_t ix = d.faces ? (int64_t)d.faces[d.face_size * f + j] : d.face_size * f + j;
                const float* v = w.data() + 9 * ix;
                for (int c = 0; c < 3; ++c) {
                    rec[3 * j + c] = v[c];
                    rec[9 + 3 * j + c] = v[3 + c];
                    rec[18 + 3 * j + c] = v[6 + c];
                }
            }
            const uint32_t kind = (uint32_t)d.face_size, unlit = d.unlit ? 1u : 0u, id = (uint32_t)(recs.size() / 32);
            memcpy(&rec[27], &kind, 4);
            memcpy(&rec[28], &unlit, 4);
            memcpy(&rec[29], &id, 4);
            recs.insert(recs.end(), rec, rec + 32);
            (d.face_size == 3 ? out->triangles : d.face_size == 2 ? out->segments : out->points) += 1;
        }
    }
    const int64_t np = (int64_t)recs.size() / 32;
    if (np == 0) return true;
    Builder b;
    b.recs = &recs;
    b.out = out;
    b.items.resize((size_t)np);
    for (int a = 0; a < 3; ++a) {
        out->lo[a] = INFINITY;
        out->hi[a] = -INFINITY;
    }
    for (int64_t i = 0; i < np; ++i) {
        const float* r = recs.data() + 32 * i;
        uint32_t kind;
        memcpy(&kind, &r[27], 4);
        Item& it = b.items[i];
        it.id = i;
        for (int a = 0; a < 3; ++a) {
            float lo = r[a], hi = r[a];
            for (uint32_t j = 1; j < kind; ++j) {
                lo = std::min(lo, r[3 * j + a]);
                hi = std::max(hi, r[3 * j + a]);
            }
            it.lo[a] = lo;
            it.hi[a] = hi;
            it.cen[a] = 0.5f * lo + 0.5f * hi;
            out->lo[a] = std::min(out->lo[a], lo);
            out->hi[a] = std::max(out->hi[a], hi);
        }
    }
    out->prims.reserve(recs.size());
    b.build(0, np);
    return true;
}

}  // namespace rto
