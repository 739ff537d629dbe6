// host_fuzz.cpp -- the host-side loaders under AddressSanitizer + UBSan (CPU only; GPU ASan is not available on this pool).
// Build + run: tools/sanitize/run.sh.  Input: a valid tree.npz, a transforms.json, a _poses_bounds.npy (written by run.sh through
// rt_octree_amd.synth).  For each: load it, then load `iters` mutations of it (truncations, byte flips in the header /
// central directory / payload, zeroed ranges, grown length fields).  Every mutation must either load or throw
// std::runtime_error -- anything else (a sanitizer report, a signal, another exception type) fails the run.
// The mesh loaders (OBJ parser, drawlist reader) and the BVH builder are targets too: their inputs are written by this program
// (an OBJ text, a drawlist npz as a stored zip), and whatever loads is built into a mesh set whose links and leaf ranges are
// then walked.  Their sources are included below, so that the build line of run.sh stays as it is.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../rt-octree_amd/csrc/cli/imwrite.h"
#include "../../rt-octree_amd/csrc/cli/poses.h"
#include "../../rt-octree_amd/csrc/host/n3tree_host.h"
#include "../../rt-octree_amd/csrc/host/npz.h"
#include "../../rt-octree_amd/csrc/host/mesh_build.cpp"
#include "../../rt-octree_amd/csrc/host/mesh_io.cpp"

#include <zlib.h>

namespace {

std::vector<uint8_t> slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    if (!f) {
        std::fprintf(stderr, "cannot read %s\n", p.c_str());
        std::exit(2);
    }
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

void spit(const std::string& p, const std::vector<uint8_t>& b) {
    std::ofstream f(p, std::ios::binary | std::ios::trunc);
    f.write(reinterpret_cast<const char*>(b.data()), (std::streamsize)b.size());
}

std::vector<uint8_t> mutate(const std::vector<uint8_t>& src, std::mt19937_64& rng) {
    std::vector<uint8_t> b = src;
    if (b.empty()) return b;
    auto pick = [&](size_t lo, size_t hi) { return lo + (size_t)(rng() % (hi - lo + 1)); };
    switch (rng() % 6) {
        case 0:  // truncate anywhere (favouring the tail: the zip central directory lives there)
            b.resize(rng() % 2 ? pick(0, b.size()) : b.size() - pick(0, std::min<size_t>(b.size(), 200)));
            break;
        case 1: {  // flip bytes near the end (central directory / end record)
            const size_t span = std::min<size_t>(b.size(), 400);
            for (int k = 0; k < 1 + (int)(rng() % 4); ++k) b[b.size() - 1 - pick(0, span - 1)] ^= (uint8_t)(1u << (rng() % 8));
        } break;
        case 2: {  // flip bytes near the start (first local header + npy header)
            const size_t span = std::min<size_t>(b.size(), 400);
            for (int k = 0; k < 1 + (int)(rng() % 4); ++k) b[pick(0, span - 1)] ^= (uint8_t)(1u << (rng() % 8));
        } break;
        case 3: {  // flip bytes anywhere
            for (int k = 0; k < 1 + (int)(rng() % 8); ++k) b[pick(0, b.size() - 1)] = (uint8_t)rng();
        } break;
        case 4: {  // zero a range
            const size_t a = pick(0, b.size() - 1), n = std::min<size_t>(b.size() - a, pick(1, 4096));
            std::memset(b.data() + a, 0, n);
        } break;
        default: {  // 0xff a short range (length fields become huge)
            const size_t a = pick(0, b.size() - 1), n = std::min<size_t>(b.size() - a, pick(1, 8));
            std::memset(b.data() + a, 0xff, n);
        } break;
    }
    return b;
}

template <typename F>
int fuzz(const char* what, const std::string& path, const std::string& tmp, int iters, uint64_t seed, F load) {
    const std::vector<uint8_t> src = slurp(path);
    load(path);  // the valid file must load (an exception here ends the run)
    std::mt19937_64 rng(seed);
    int ok = 0, refused = 0;
    for (int i = 0; i < iters; ++i) {
        spit(tmp, mutate(src, rng));
        try {
            load(tmp);
            ++ok;
        } catch (const std::runtime_error&) {
            ++refused;
        } catch (const std::exception& e) {  // bad_alloc on a grown length field, out_of_range, ...: not the documented error
            std::fprintf(stderr, "%s: mutation %d raised %s, not std::runtime_error\n", what, i, e.what());
            return 1;
        }
    }
    std::printf("%s: %d mutations: %d loaded, %d refused with std::runtime_error\n", what, iters, ok, refused);
    return 0;
}

// ---- mesh inputs
void put16(std::vector<uint8_t>& b, uint32_t v) {
    b.push_back((uint8_t)v);
    b.push_back((uint8_t)(v >> 8));
}
void put32(std::vector<uint8_t>& b, uint32_t v) {
    put16(b, v & 0xffffu);
    put16(b, v >> 16);
}

// one .npy image: descr like "<f4", shape, payload
std::vector<uint8_t> npy(const std::string& descr, const std::vector<size_t>& shape, const void* data, size_t nbytes) {
    std::string dict = "{'descr': '" + descr + "', 'fortran_order': False, 'shape': (";
    for (size_t i = 0; i < shape.size(); ++i) dict += std::to_string(shape[i]) + (shape.size() == 1 || i + 1 < shape.size() ? "," : "");
    dict += "), }";
    while ((10 + dict.size() + 1) % 64) dict += ' ';
    dict += '\n';
    std::vector<uint8_t> b = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0};
    put16(b, (uint32_t)dict.size());
    b.insert(b.end(), dict.begin(), dict.end());
    const uint8_t* p = static_cast<const uint8_t*>(data);
    b.insert(b.end(), p, p + nbytes);
    return b;
}

// a zip of STORED members, as numpy.savez writes it
std::vector<uint8_t> zip_stored(const std::vector<std::pair<std::string, std::vector<uint8_t>>>& members) {
    std::vector<uint8_t> out, dir;
    for (const auto& m : members) {
        const std::string name = m.first + ".npy";
        const uint32_t crc = (uint32_t)crc32(0L, m.second.data(), (uInt)m.second.size()), off = (uint32_t)out.size();
        put32(out, 0x04034b50u);
        put16(out, 20), put16(out, 0), put16(out, 0), put16(out, 0), put16(out, 0);
        put32(out, crc), put32(out, (uint32_t)m.second.size()), put32(out, (uint32_t)m.second.size());
        put16(out, (uint32_t)name.size()), put16(out, 0);
        out.insert(out.end(), name.begin(), name.end());
        out.insert(out.end(), m.second.begin(), m.second.end());
        put32(dir, 0x02014b50u);
        put16(dir, 20), put16(dir, 20), put16(dir, 0), put16(dir, 0), put16(dir, 0), put16(dir, 0);
        put32(dir, crc), put32(dir, (uint32_t)m.second.size()), put32(dir, (uint32_t)m.second.size());
        put16(dir, (uint32_t)name.size()), put16(dir, 0), put16(dir, 0), put16(dir, 0), put16(dir, 0);
        put32(dir, 0), put32(dir, off);
        dir.insert(dir.end(), name.begin(), name.end());
    }
    const uint32_t dir_off = (uint32_t)out.size();
    out.insert(out.end(), dir.begin(), dir.end());
    put32(out, 0x06054b50u);
    put16(out, 0), put16(out, 0), put16(out, (uint32_t)members.size()), put16(out, (uint32_t)members.size());
    put32(out, (uint32_t)dir.size()), put32(out, dir_off), put16(out, 0);
    return out;
}

std::vector<uint8_t> npy_str(const std::string& s) {
    std::vector<uint32_t> u(s.begin(), s.end());
    return npy("<U" + std::to_string(s.size()), {}, u.data(), u.size() * 4);
}
template <typename T>
std::vector<uint8_t> npy_of(const std::string& descr, const std::vector<size_t>& shape, const std::vector<T>& v) {
    return npy(descr, shape, v.data(), v.size() * sizeof(T));
}

std::vector<uint8_t> sample_drawlist() {
    const std::vector<double> pts = {0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0.5, 0.5, 2};
    const std::vector<float> rt = {0.1f, 0.2f, 0.3f, 1.f, -1.f, 0.5f, 0.f, 0.f, 0.f};
    return zip_stored({{"a", npy_str("mesh")},
                       {"a__points", npy_of<double>("<f8", {5, 3}, pts)},
                       {"a__faces", npy_of<int64_t>("<i8", {2, 3}, {0, 1, 2, 2, 3, 4})},
                       {"a__vert_color", npy_of<double>("<f8", {5, 3}, pts)},
                       {"b", npy_str("lines")},
                       {"b__points", npy_of<double>("<f8", {5, 3}, pts)},
                       {"b__segs", npy_of<int32_t>("<i4", {2, 2}, {0, 4, 1, 3})},
                       {"c", npy_str("camerafrustum")},
                       {"c__r", npy_of<float>("<f4", {3, 3}, rt)},
                       {"c__t", npy_of<float>("<f4", {3, 3}, rt)},
                       {"c__connect", npy_of<int64_t>("<i8", {}, {1})},
                       {"d", npy_str("sphere")},
                       {"d__rings", npy_of<int64_t>("<i8", {}, {5})},
                       {"d__sectors", npy_of<int32_t>("<i4", {}, {7})},
                       {"d__rotation", npy_of<double>("<f8", {3}, {0.5, 0.1, -0.3})},
                       {"e", npy_str("points")},
                       {"e__points", npy_of<double>("<f8", {5, 3}, pts)},
                       {"f", npy_str("cube")},
                       {"f__scale", npy_of<double>("<f8", {}, {2.0})}});
}

const char* kSampleObj =
    "# fuzz seed\nv 0 0 0 1 0 0\nv 1 0 0 0 1 0\nv 1 1 0 0 0 1\nv 0 1 0.5 1 1 1\nv 0.5 0.5 2 0 0 0\nvn 0 0 1\nvn 0 1 0\nvn 1 0 0\n"
    "vn 0 0 -1\nvn 0 -1 0\nvt 0.1 0.2\nf 1 2 3\nf 1/1 3/1 4/1\nf 1/1/1 2/1/2 5/1/5\nf -1//5 -2//4 -5//1\nf 1 2 3 4 5\nf 1 2\n";

// whatever loaded is built; the set's links and leaf ranges must stay inside it
void build_and_walk(const std::vector<rto::MeshData>& meshes) {
    std::vector<rto::MeshDescHost> descs;
    for (const rto::MeshData& m : meshes) descs.push_back(m.desc());
    rto::MeshSetHost set;
    std::string err;
    if (!rto::mesh_build(descs.data(), (int)descs.size(), &set, &err)) throw std::runtime_error(err);
    const int64_t nn = set.n_nodes(), np = set.n_prims();
    int64_t seen = 0;
    for (int64_t i = 0; i < nn; ++i) {
        uint32_t link, leaf;
        std::memcpy(&link, &set.nodes[8 * i + 3], 4);
        std::memcpy(&leaf, &set.nodes[8 * i + 7], 4);
        const int64_t miss = link & 0x3fffffffu;
        if (miss <= i || miss > nn) throw std::logic_error("BVH: a miss link does not point forward inside the node array");
        if (link & 0x80000000u) {
            const int64_t first = leaf >> 2, count = (leaf & 3u) + 1;
            if (first != seen || first + count > np) throw std::logic_error("BVH: a leaf range is out of order or out of bounds");
            seen += count;
        }
    }
    if (seen != np) throw std::logic_error("BVH: the leaves do not cover the records");
}

int fuzz_bvh(int iters) {
    std::mt19937_64 rng(7);
    for (int it = 0; it < iters; ++it) {
        std::vector<rto::MeshData> meshes(1 + rng() % 3);
        for (rto::MeshData& m : meshes) {
            m.face_size = 1 + (int)(rng() % 3);
            const size_t nv = rng() % 40;
            const int mode = (int)(rng() % 4);  // coincident vertices, a line of them, huge coordinates, random
            for (size_t v = 0; v < nv; ++v)
                for (int c = 0; c < 9; ++c) {
                    float x = (float)(rng() % 2001) / 1000.f - 1.f;
                    if (mode == 0) x = 0.25f;
                    if (mode == 1 && c != 0) x = 0.f;
                    if (mode == 2 && c < 3) x *= 1e30f;
                    m.vert.push_back(x);
                }
            if (nv && rng() % 2)
                for (size_t k = 0, nf = (rng() % 30) * (size_t)m.face_size; k < nf; ++k) m.faces.push_back((uint32_t)(rng() % nv));
            m.estimate_normals = rng() % 2;
            m.scale = mode == 2 ? 1e9f : 0.5f;
            m.rotation[0] = (float)(rng() % 7);
        }
        try {
            build_and_walk(meshes);
        } catch (const std::runtime_error&) {  // (a position that overflows in world space is refused)
        }
    }
    std::printf("BVH builder: %d random mesh sets built and walked\n", iters);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 6) {
        std::fprintf(stderr, "usage: host_fuzz tree.npz transforms.json poses_bounds.npy tmpdir iters\n");
        return 2;
    }
    const std::string tree = argv[1], json = argv[2], npy = argv[3], tmp = argv[4];
    const int iters = std::atoi(argv[5]);
    int rc = 0;
    rc |= fuzz("tree.npz", tree, tmp + "/m.npz", iters, 1, [](const std::string& p) {
        rto::HostTree t;
        if (t.open(p)) {
            (void)rto::tree_max_depth(t.child, t.capacity, t.N);  // walks every child offset (refuses one out of range)
            volatile uint16_t sink = t.data ? t.data[(size_t)t.capacity * t.N * t.N * t.N * t.data_dim - 1] : 0;  // the last element is mapped
            (void)sink;
        }
    });
    rc |= fuzz("transforms.json", json, tmp + "/transforms_m.json", iters, 2, [](const std::string& p) {
        rto::PoseSet ps;
        rto::load_poses("blender", p, false, ps);
    });
    rc |= fuzz("poses_bounds.npy", npy, tmp + "/poses_bounds_m.npy", iters, 3, [](const std::string& p) {
        rto::PoseSet ps;
        rto::load_poses("llff", p, false, ps);
    });
    spit(tmp + "/seed.obj", std::vector<uint8_t>(kSampleObj, kSampleObj + std::strlen(kSampleObj)));
    rc |= fuzz("mesh.obj", tmp + "/seed.obj", tmp + "/m.obj", iters, 4, [](const std::string& p) {
        std::vector<rto::MeshData> m(1);
        rto::load_obj_file(p, &m[0]);
        build_and_walk(m);
    });
    spit(tmp + "/seed_drawlist.npz", sample_drawlist());
    rc |= fuzz("drawlist.npz", tmp + "/seed_drawlist.npz", tmp + "/m_drawlist.npz", iters, 5, [](const std::string& p) {
        std::vector<rto::MeshData> m;
        rto::load_drawlist_file(p, &m);
        build_and_walk(m);
    });
    rc |= fuzz_bvh(iters);
    {  // a hostile nesting depth must be refused, not recursed into
        spit(tmp + "/transforms_deep.json", std::vector<uint8_t>(2000000, (uint8_t)'['));
        try {
            rto::PoseSet ps;
            rto::load_poses("blender", tmp + "/transforms_deep.json", false, ps);
            rc |= 1;
        } catch (const std::runtime_error& e) {
            std::printf("deeply nested json: refused (%s)\n", e.what());
        }
    }
    {  // PNG writer on odd sizes
        std::vector<uint8_t> px(37 * 19 * 4);
        for (size_t i = 0; i < px.size(); ++i) px[i] = (uint8_t)(i * 7);
        if (!rto::write_png_rgba8(tmp + "/o.png", px.data(), 37, 19) || !rto::write_png_rgba8(tmp + "/o1.png", px.data(), 1, 1)) rc |= 1;
    }
    std::printf(rc ? "FAILED\n" : "host loaders: clean under ASan + UBSan\n");
    return rc;
}
