// host/mesh_io.cpp -- see mesh_io.h.
#include "mesh_io.h"

#include <ctype.h>
#include <math.h>
#include <string.h>

#include <cmath>

#include <algorithm>
#include <fstream>
#include <stdexcept>

namespace rto {
namespace {

const float kDefaultColor[3] = {1.f, 0.5f, 0.2f};
constexpr size_t kMaxPresetVerts = size_t(1) << 24;

[[noreturn]] void bad(const std::string& msg) { throw std::runtime_error(msg); }

void push_vert(std::vector<float>& v, const float* p, const float* c, const float* n) {
    v.insert(v.end(), p, p + 3);
    v.insert(v.end(), c, c + 3);
    v.insert(v.end(), n, n + 3);
}

// axis-angle -> matrix, |r| < 1e-3 the identity (Mesh::apply_transform)
void rotation_matrix(const float* r, double M[3][3]) {
    const double x = r[0], y = r[1], z = r[2];
    const double ang = sqrt((x * x + y * y) + z * z);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[i][j] = i == j ? 1.0 : 0.0;
    if (ang < 1e-3) return;
    const double a[3] = {x / ang, y / ang, z / ang};
    const double c = cos(ang), s = sin(ang), k = 1.0 - c;
    const double X[3][3] = {{0, -a[2], a[1]}, {a[2], 0, -a[0]}, {-a[1], a[0], 0}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[i][j] = ((i == j ? c : 0.0) + k * (a[i] * a[j])) + s * X[i][j];
}

float half_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 31u, man = h & 1023u;
    uint32_t u;
    if (exp == 0) {
        if (man == 0) {
            u = sign;
        } else {  // subnormal
            const float f = (float)man * (1.f / 16777216.f);
            memcpy(&u, &f, 4);
            u |= sign;
        }
    } else if (exp == 31) {
        u = sign | 0x7f800000u | (man << 13);
    } else {
        u = sign | ((exp + 112u) << 23) | (man << 13);
    }
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// ---- drawlist fields
using Fields = std::map<std::string, NpyArray>;

void check_payload(const NpyArray& a, const std::string& key) {
    if (!a.data || a.word_size == 0 || a.num_vals() > a.nbytes / a.word_size) bad("drawlist field '" + key + "' is truncated");
    if (a.fortran_order && a.shape.size() > 1) bad("drawlist field '" + key + "' is in Fortran order");
}

std::vector<float> get_floats(const Fields& f, const std::string& key) {
    std::vector<float> out;
    const auto it = f.find(key);
    if (it == f.end()) return out;
    const NpyArray& a = it->second;
    check_payload(a, key);
    const size_t n = a.num_vals();
    out.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* p = a.data + i * a.word_size;
        if (a.kind == 'f' && a.word_size == 2) {
            uint16_t h;
            memcpy(&h, p, 2);
            out[i] = half_to_float(h);
        } else if (a.kind == 'f' && a.word_size == 4) {
            memcpy(&out[i], p, 4);
        } else if (a.kind == 'f' && a.word_size == 8) {
            double d;
            memcpy(&d, p, 8);
            out[i] = (float)d;
        } else if ((a.kind == 'i' || a.kind == 'u') && a.word_size == 4) {
            int32_t v;
            memcpy(&v, p, 4);
            out[i] = a.kind == 'i' ? (float)v : (float)(uint32_t)v;
        } else if ((a.kind == 'i' || a.kind == 'u') && a.word_size == 8) {
            int64_t v;
            memcpy(&v, p, 8);
            out[i] = a.kind == 'i' ? (float)v : (float)(uint64_t)v;
        } else {
            bad("drawlist field '" + key + "' has dtype " + a.descr + ", not a float array");
        }
    }
    return out;
}

std::vector<int64_t> get_ints(const Fields& f, const std::string& key) {
    std::vector<int64_t> out;
    const auto it = f.find(key);
    if (it == f.end()) return out;
    const NpyArray& a = it->second;
    check_payload(a, key);
    if (a.kind != 'i' && a.kind != 'u' && a.kind != 'b') bad("drawlist field '" + key + "' has dtype " + a.descr + ", not an integer array");
    const size_t n = a.num_vals();
    out.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* p = a.data + i * a.word_size;
        const bool sg = a.kind == 'i';
        switch (a.word_size) {
            case 1: out[i] = sg ? (int64_t)(int8_t)p[0] : (int64_t)p[0]; break;
            case 2: { uint16_t v; memcpy(&v, p, 2); out[i] = sg ? (int64_t)(int16_t)v : (int64_t)v; } break;
            case 4: { uint32_t v; memcpy(&v, p, 4); out[i] = sg ? (int64_t)(int32_t)v : (int64_t)v; } break;
            case 8: { uint64_t v; memcpy(&v, p, 8); if (!sg && v > (uint64_t)INT64_MAX) bad("drawlist field '" + key + "' is out of range"); out[i] = (int64_t)v; } break;
            default: bad("drawlist field '" + key + "' has dtype " + a.descr);
        }
    }
    return out;
}

float get_float(const Fields& f, const std::string& key, float def) {
    if (!f.count(key)) return def;
    const std::vector<float> v = get_floats(f, key);
    if (v.size() != 1) bad("drawlist field '" + key + "' must be one number");
    return v[0];
}

int64_t get_int(const Fields& f, const std::string& key, int64_t def) {
    if (!f.count(key)) return def;
    const std::vector<int64_t> v = get_ints(f, key);
    if (v.size() != 1) bad("drawlist field '" + key + "' must be one integer");
    return v[0];
}

void get_vec3(const Fields& f, const std::string& key, const float* def, float* out) {
    for (int i = 0; i < 3; ++i) out[i] = def[i];
    if (!f.count(key)) return;
    const std::vector<float> v = get_floats(f, key);
    if (v.size() != 3) bad("drawlist field '" + key + "' must have shape (3,)");
    for (int i = 0; i < 3; ++i) out[i] = v[i];
}

MeshData from_points(const std::vector<float>& pts, const float* color, int face_size, bool unlit) {
    if (pts.size() % 3) bad("the number of elements of points must be divisible by 3");
    MeshData m;
    m.face_size = face_size;
    m.unlit = unlit;
    const float n[3] = {0.f, 0.f, 1.f};
    m.vert.reserve(pts.size() * 3);
    for (size_t i = 0; i < pts.size(); i += 3) push_vert(m.vert, &pts[i], color, n);
    return m;
}

void set_faces(MeshData& m, const std::vector<int64_t>& idx, const std::string& what) {
    const int64_t nv = (int64_t)m.vert.size() / 9;
    if (idx.size() % (size_t)m.face_size) bad(what + ": the number of indices is no multiple of the face size");
    m.faces.resize(idx.size());
    for (size_t i = 0; i < idx.size(); ++i) {
        if (idx[i] < 0 || idx[i] >= nv) bad(what + ": an index is out of range");
        m.faces[i] = (uint32_t)idx[i];
    }
}

std::string type_string(const NpyArray& a) {
    std::string s;
    if (!a.data || a.word_size == 0 || a.word_size > a.nbytes) bad("a drawlist type entry is truncated");
    if (a.kind == 'U') {
        for (size_t i = 0; i + 4 <= a.word_size; i += 4) {
            uint32_t cp;
            memcpy(&cp, a.data + i, 4);
            if (cp == 0) break;
            s.push_back(cp < 128 ? (char)tolower((int)cp) : '?');
        }
    } else if (a.kind == 'S' || a.kind == 'a') {
        for (size_t i = 0; i < a.word_size && a.data[i]; ++i) s.push_back((char)tolower(a.data[i]));
    } else {
        bad("a drawlist type entry is no string (dtype " + a.descr + ")");
    }
    return s;
}

}  // namespace

MeshDescHost MeshData::desc() const {
    MeshDescHost d;
    d.vert = vert.data();
    d.n_verts = (int64_t)vert.size() / 9;
    d.faces = faces.empty() ? nullptr : faces.data();
    d.n_faces = (int64_t)faces.size() / face_size;
    d.face_size = face_size;
    d.unlit = unlit;
    d.estimate_normals = estimate_normals;
    for (int i = 0; i < 3; ++i) {
        d.rotation[i] = rotation[i];
        d.translation[i] = translation[i];
    }
    d.scale = scale;
    return d;
}

MeshData mesh_cube(const float color[3]) {
    // from the six face normals -z, +z, -y, +y, -x, +x: two triangles per face over the two in-face axes (ascending)
    MeshData m;
    m.name = "Cube";
    static const int faces[6][2] = {{2, -1}, {2, 1}, {1, -1}, {1, 1}, {0, -1}, {0, 1}};
    static const float corner[6][2] = {{-0.5f, -0.5f}, {0.5f, 0.5f}, {0.5f, -0.5f}, {0.5f, 0.5f}, {-0.5f, -0.5f}, {-0.5f, 0.5f}};
    for (const auto& f : faces) {
        const int axis = f[0], a = axis == 0 ? 1 : 0, b = axis == 2 ? 1 : 2;
        float n[3] = {0, 0, 0};
        n[axis] = (float)f[1];
        for (const auto& c : corner) {
            float p[3];
            p[axis] = 0.5f * (float)f[1];
            p[a] = c[0];
            p[b] = c[1];
            push_vert(m.vert, p, color, n);
        }
    }
    return m;
}

MeshData mesh_sphere(int rings, int sectors, const float color[3]) {
    if (rings < 2 || sectors < 3 || (size_t)rings * (size_t)sectors > kMaxPresetVerts) bad("sphere: rings >= 2, sectors >= 3, at most 2^24 vertices");
    MeshData m;
    m.name = "Sphere";
    const double pi = 3.14159265358979323846;
    const double R = pi / (double)(rings - 1), S = 2.0 * pi / (double)sectors;
    for (int r = 0; r < rings; ++r)
        for (int s = 0; s < sectors; ++s) {
            const float p[3] = {(float)(cos(s * S) * sin(r * R)), (float)(sin(s * S) * sin(r * R)), (float)sin(r * R - 0.5 * pi)};
            push_vert(m.vert, p, color, p);
        }
    for (int r = 0; r + 1 < rings; ++r)
        for (int s = 0; s < sectors; ++s) {
            const uint32_t ns = (uint32_t)((s + 1) % sectors), a = (uint32_t)r * sectors, b = (uint32_t)(r + 1) * sectors;
            const uint32_t q[6] = {a + ns, a + (uint32_t)s, b + (uint32_t)s, b + (uint32_t)s, b + ns, a + ns};
            m.faces.insert(m.faces.end(), q, q + 6);
        }
    return m;
}

MeshData mesh_frustum(float focal, float width, float height, float z, const float color[3]) {
    MeshData m;
    m.name = "CameraFrustum";
    m.face_size = 2;
    m.unlit = true;
    const float inv = 1.f / focal, hw = 0.5f * width, hh = 0.5f * height, n[3] = {0.f, 0.f, 1.f};
    const float sx[4] = {-hw, -hw, hw, hw}, sy[4] = {-hh, hh, hh, -hh};
    const float apex[3] = {0.f, 0.f, 0.f};
    push_vert(m.vert, apex, color, n);
    for (int i = 0; i < 4; ++i) {
        const float p[3] = {z * sx[i] * inv, z * sy[i] * inv, z};
        push_vert(m.vert, p, color, n);
    }
    for (uint32_t i = 1; i <= 4; ++i) {
        m.faces.push_back(0);
        m.faces.push_back(i);
    }
    for (uint32_t i = 1; i <= 4; ++i) {
        m.faces.push_back(i);
        m.faces.push_back(i % 4 + 1);
    }
    return m;
}

void parse_obj(const char* text, size_t n, MeshData* out) {
    *out = MeshData();
    out->name = "OBJ";
    std::vector<float> pos, col, nrm;
    std::vector<uint32_t> faces;
    std::vector<int64_t> poly;
    size_t n_col = 0, line_no = 0;
    if (memchr(text, 0, n)) bad("OBJ: the file holds a NUL byte: not a text file");
    size_t i = 0;
    while (i < n) {
        size_t e = i;
        while (e < n && text[e] != '\n') ++e;
        std::string line(text + i, e - i);
        i = e + 1;
        ++line_no;
        const std::string at = "OBJ line " + std::to_string(line_no) + ": ";
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line.resize(hash);
        // tokens
        std::vector<std::string> tok;
        size_t p = 0;
        while (p < line.size()) {
            while (p < line.size() && isspace((unsigned char)line[p])) ++p;
            size_t q = p;
            while (q < line.size() && !isspace((unsigned char)line[q])) ++q;
            if (q > p) tok.push_back(line.substr(p, q - p));
            p = q;
        }
        if (tok.empty()) continue;
        auto numbers = [&](size_t most, std::vector<float>& dst) {
            size_t k = 0;
            for (size_t t = 1; t < tok.size() && k < most; ++t, ++k) {
                char* end = nullptr;
                const float v = strtof(tok[t].c_str(), &end);
                if (end == tok[t].c_str() || *end != 0 || !std::isfinite(v)) bad(at + "'" + tok[t] + "' is no finite number");
                dst.push_back(v);
            }
            return k;
        };
        if (tok[0] == "v") {
            std::vector<float> v;
            const size_t k = numbers(7, v);
            if (k < 3) bad(at + "a vertex needs three coordinates");
            pos.insert(pos.end(), v.begin(), v.begin() + 3);
            if (k >= 6) {
                col.insert(col.end(), v.begin() + 3, v.begin() + 6);
                ++n_col;
            } else {
                col.insert(col.end(), kDefaultColor, kDefaultColor + 3);
            }
        } else if (tok[0] == "vn") {
            std::vector<float> v;
            if (numbers(3, v) < 3) bad(at + "a normal needs three coordinates");
            nrm.insert(nrm.end(), v.begin(), v.end());
        } else if (tok[0] == "f") {
            poly.clear();
            const int64_t nv = (int64_t)pos.size() / 3;
            for (size_t t = 1; t < tok.size(); ++t) {
                const std::string a = tok[t].substr(0, tok[t].find('/'));  // a, a/b, a/b/c, a//c: the vertex index comes first
                char* end = nullptr;
                const long long v = strtoll(a.c_str(), &end, 10);
                if (end == a.c_str() || *end != 0) bad(at + "'" + tok[t] + "' is no face index");
                const int64_t ix = v > 0 ? (int64_t)v - 1 : (int64_t)v + nv;  // 1-based; negative: relative to the vertices so far
                if (v == 0 || ix < 0 || ix >= nv) bad(at + "face index " + a + " is out of range");
                poly.push_back(ix);
            }
            if (poly.size() == 3)
                for (int64_t ix : poly) faces.push_back((uint32_t)ix);
        }
        // anything else (vt, g, o, s, usemtl, mtllib, ...) is not parsed
    }
    const size_t nv = pos.size() / 3;
    if (nv == 0) bad("OBJ: no vertices");
    const bool use_col = n_col == nv, use_nrm = nrm.size() / 3 == nv;
    out->vert.resize(nv * 9);
    for (size_t v = 0; v < nv; ++v)
        for (int c = 0; c < 3; ++c) {
            out->vert[9 * v + c] = pos[3 * v + c];
            out->vert[9 * v + 3 + c] = use_col ? col[3 * v + c] : kDefaultColor[c];
            out->vert[9 * v + 6 + c] = use_nrm ? nrm[3 * v + c] : 0.f;
        }
    out->faces = faces;
    out->face_size = 3;
    out->estimate_normals = !use_nrm;
    if (faces.empty()) {  // (an empty index list would mean "consecutive vertices": a file without triangles draws none)
        out->vert.clear();
    }
}

void load_obj_file(const std::string& path, MeshData* out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) bad("cannot open " + path);
    const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    parse_obj(text.data(), text.size(), out);
    out->name = path;
}

void parse_drawlist(const std::map<std::string, NpyArray>& arrays, std::vector<MeshData>* out) {
    out->clear();
    std::map<std::string, std::pair<std::string, Fields>> parsed;  // name -> (type, fields): std::map keeps the reference's order
    for (const auto& kv : arrays) {
        const size_t sep = kv.first.find("__");
        if (sep == std::string::npos) {
            parsed[kv.first].first = type_string(kv.second);
        } else {
            const std::string name = kv.first.substr(0, sep), field = kv.first.substr(sep + 2);
            if (name.empty() || field.empty() || field.find("__") != std::string::npos) continue;  // (the reference warns and ignores)
            parsed[name].second[field] = kv.second;
        }
    }
    for (const auto& kv : parsed) {
        const std::string& type = kv.second.first;
        const Fields& f = kv.second.second;
        const std::string at = "drawlist mesh '" + kv.first + "': ";
        float color[3];
        get_vec3(f, "color", kDefaultColor, color);
        MeshData me;
        try {
            if (type == "cube") {
                me = mesh_cube(color);
            } else if (type == "sphere") {
                const int64_t rings = get_int(f, "rings", 15), sectors = get_int(f, "sectors", 30);
                if (rings < 2 || rings > 1 << 20 || sectors < 3 || sectors > 1 << 20) bad("rings or sectors out of range");
                me = mesh_sphere((int)rings, (int)sectors, color);
            } else if (type == "line") {
                const float da[3] = {0, 0, 0}, db[3] = {0, 0, 1};
                float a[3], b[3];
                get_vec3(f, "a", da, a);
                get_vec3(f, "b", db, b);
                me = from_points({a[0], a[1], a[2], b[0], b[1], b[2]}, color, 2, true);
                me.faces = {0, 1};
            } else if (type == "camerafrustum") {
                me = mesh_frustum(get_float(f, "focal_length", 1111.f), get_float(f, "image_width", 800.f),
                                  get_float(f, "image_height", 800.f), get_float(f, "z", -0.3f), color);
                if (f.count("t")) {
                    const std::vector<float> t = get_floats(f, "t"), r = get_floats(f, "r");
                    if (r.size() != t.size() || r.size() % 3) bad("r and t differ in size or are no multiple of 3");
                    const size_t reps = t.size() / 3;
                    if (reps * 5 > kMaxPresetVerts) bad("too many frusta");
                    const std::vector<float> v0 = me.vert;
                    const std::vector<uint32_t> f0 = me.faces;
                    me.vert.clear();
                    me.faces.clear();
                    for (size_t k = 0; k < reps; ++k) {
                        double M[3][3];
                        rotation_matrix(&r[3 * k], M);
                        for (size_t v = 0; v < 5; ++v) {
                            float p[3];
                            for (int c = 0; c < 3; ++c)
                                p[c] = (float)(((M[c][0] * v0[9 * v] + M[c][1] * v0[9 * v + 1]) + M[c][2] * v0[9 * v + 2]) + (double)t[3 * k + c]);
                            push_vert(me.vert, p, &v0[9 * v + 3], &v0[9 * v + 6]);
                        }
                        for (uint32_t ix : f0) me.faces.push_back(ix + (uint32_t)(5 * k));
                    }
                    if (get_int(f, "connect", 0) != 0)  // the camera centres joined into a trajectory
                        for (size_t k = 0; k + 1 < reps; ++k) {
                            me.faces.push_back((uint32_t)(5 * k));
                            me.faces.push_back((uint32_t)(5 * (k + 1)));
                        }
                }
            } else if (type == "lines") {
                me = from_points(get_floats(f, "points"), color, 2, true);
                if (f.count("segs")) {
                    set_faces(me, get_ints(f, "segs"), "segs");
                } else {
                    const uint32_t nv = (uint32_t)(me.vert.size() / 9);
                    for (uint32_t k = 0; k + 1 < nv; ++k) {
                        me.faces.push_back(k);
                        me.faces.push_back(k + 1);
                    }
                }
                if (me.faces.empty()) me.vert.clear();  // (fewer than two points: nothing to draw)
            } else if (type == "points") {
                me = from_points(get_floats(f, "points"), color, 1, true);
            } else if (type == "mesh") {
                const int64_t fs = get_int(f, "face_size", 3);
                if (fs < 1 || fs > 3) bad("face_size must be 1, 2 or 3");
                me = from_points(get_floats(f, "points"), color, (int)fs, false);
                if (f.count("faces")) {
                    set_faces(me, get_ints(f, "faces"), "faces");
                    if (me.faces.empty()) me.vert.clear();
                }
                me.estimate_normals = fs == 3;
            } else {
                bad("unsupported type '" + type + "'");
            }
            if (f.count("vert_color")) {
                const std::vector<float> vc = get_floats(f, "vert_color");
                if (vc.size() * 3 != me.vert.size()) bad("vert_color has the wrong size");
                for (size_t v = 0; v < vc.size() / 3; ++v)
                    for (int c = 0; c < 3; ++c) me.vert[9 * v + 3 + c] = vc[3 * v + c];
            }
            me.name = kv.first;
            const float zero[3] = {0, 0, 0};
            me.scale = get_float(f, "scale", 1.f);
            get_vec3(f, "translation", zero, me.translation);
            get_vec3(f, "rotation", zero, me.rotation);
            me.visible = get_int(f, "visible", 1) != 0;
            me.unlit = get_int(f, "unlit", 0) != 0 || me.face_size != 3;  // (lines and points are always unlit)
        } catch (const std::runtime_error& e) {
            bad(at + e.what());
        }
        for (float v : me.vert)
            if (!std::isfinite(v)) bad(at + "a non-finite vertex value");
        out->push_back(std::move(me));
    }
}

void load_drawlist_file(const std::string& path, std::vector<MeshData>* out) {
    NpzFile z;
    z.open(path);
    parse_drawlist(z.arrays(), out);
}

}  // namespace rto
