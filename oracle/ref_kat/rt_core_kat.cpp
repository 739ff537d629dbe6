// Known-answer generator for the reference's ray core, compiled against the REFERENCE's own headers where they lie
// (rt_core.cuh, n3tree_query.hpp, lumisphere.hpp, data_spec.hpp, cuda/common.cuh, pcg32.h; src/n3tree.cpp and cnpy are
// linked) behind the stand-in CUDA headers of shim/.  This file is the harness only: it reads one case (an .npz: a tree,
// points, directions, rays, options), calls the reference's functions and writes what they return.
//
//   rt_core_kat case.npz out.bin        the four tables (query, basis, dst, trace) of one case
//   rt_core_kat --n3tree tree.npz out.json   what the reference's N3Tree(path) holds after loading (decode included)
//   rt_core_kat --half out.bin          the stand-in __half: all 65536 widenings, and a narrowing sweep
//
// log / exp: __logf / __expf (rt_core.cuh:74,95,314) and the expf of the SG / ASG lobes (lumisphere.hpp:24,33) are this
// project's orc_det_logf / orc_det_expf (DESIGN.md "Math definitions", section 7a); everything else is the reference's code
// over IEEE float / double arithmetic (-O2 -ffp-contract=off, SSE).
// Authoring container only.
#include <cuda_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pcg32.h"

// the lobes' expf: found by unqualified lookup from volrend::internal before the C library's
namespace volrend {
namespace internal {
static inline float expf(float x) { return orc_det_expf(x); }
}  // namespace internal
}  // namespace volrend

#include "volrend/cuda/rt_core.cuh"

namespace volrend {
// n3tree.cpp calls these three; the device side does not exist here
void N3Tree::load_cuda() {}
void N3Tree::free_cuda() {}
cudaError_t cuda_assert(const cudaError_t code, const char* const, const int, const bool) { return code; }
}  // namespace volrend

using volrend::N3Tree;
using volrend::RenderOptions;
using volrend::internal::TreeSpec;

static FILE* g_out;

static void emit(const std::string& name, const char* dtype, const void* p, size_t count, size_t word) {
    fprintf(g_out, "%s %s %zu\n", name.c_str(), dtype, count);
    if (count) fwrite(p, word, count, g_out);
}
static void emit_f32(const std::string& n, const std::vector<float>& v) { emit(n, "f4", v.data(), v.size(), 4); }
static void emit_u64(const std::string& n, const std::vector<uint64_t>& v) { emit(n, "u8", v.data(), v.size(), 8); }
static void emit_i64(const std::string& n, const std::vector<int64_t>& v) { emit(n, "i8", v.data(), v.size(), 8); }

struct Rays {
    size_t n = 0;
    std::vector<float> dir, cen;  // what trace_ray is handed
    const float* tmax = nullptr;
};

template <int SPP>
static void dst_table(int ndst) {
    std::vector<float> dst((size_t)ndst * (SPP + 1));
    std::vector<uint64_t> state(ndst);
    for (int i = 0; i < ndst; ++i) {
        pcg32 rng(20230418);   // render_context.hpp:16
        rng.advance(i * SPP);  // volrend.cu:157
        volrend::device::sample_dst<SPP>(&dst[(size_t)i * (SPP + 1)], rng);
        state[i] = rng.state;
    }
    emit_f32("dst" + std::to_string(SPP), dst);
    emit_u64("dst" + std::to_string(SPP) + "_state", state);
}

template <int SPP>
static void trace_table(const TreeSpec& spec, const RenderOptions& opt, const Rays& rays) {
    std::vector<float> out(rays.n * 4, 0.f);
    std::vector<uint64_t> state(rays.n);
    for (size_t i = 0; i < rays.n; ++i) {
        float dir[3], vdir[3], cen[3];
        for (int k = 0; k < 3; ++k) {
            dir[k] = vdir[k] = rays.dir[i * 3 + k];
            cen[k] = rays.cen[i * 3 + k];
        }
        pcg32 rng(20230418);
        rng.advance((int)i * SPP);
        volrend::device::trace_ray<float, SPP>(spec, dir, vdir, cen, opt, rays.tmax[i], &out[i * 4], rng);
        state[i] = rng.state;
    }
    emit_f32("trace" + std::to_string(SPP) + "_out", out);
    emit_u64("trace" + std::to_string(SPP) + "_state", state);
}

static uint64_t fnv1a(const unsigned char* p, size_t n) {
    uint64_t h = 1469598103934665603ULL;
    for (size_t i = 0; i < n; ++i) {
        h ^= p[i];
        h *= 1099511628211ULL;
    }
    return h;
}

static int n3tree_mode(const char* path, const char* out_path) {
    N3Tree tree{std::string(path)};
    if (!tree.is_data_loaded()) return 3;
    FILE* f = fopen(out_path, "w");
    if (!f) return 2;
    auto shape = [&](const cnpy::NpyArray& a) {
        fprintf(f, "[");
        for (size_t i = 0; i < a.shape.size(); ++i) fprintf(f, "%s%zu", i ? ", " : "", a.shape[i]);
        fprintf(f, "]");
    };
    fprintf(f, "{\"N\": %d, \"data_dim\": %d, \"data_format\": \"%s\", \"capacity\": %d, ", tree.N, tree.data_dim,
            tree.data_format.to_string().c_str(), tree.capacity);
    uint32_t sb[6];
    memcpy(sb, tree.scale.data(), 12);
    memcpy(sb + 3, tree.offset.data(), 12);
    fprintf(f, "\"scale_bits\": [%u, %u, %u], \"offset_bits\": [%u, %u, %u], ", sb[0], sb[1], sb[2], sb[3], sb[4], sb[5]);
    fprintf(f, "\"child_shape\": ");
    shape(tree.child_);
    fprintf(f, ", \"child_fnv1a64\": \"%016llx\", \"data_shape\": ",
            (unsigned long long)fnv1a((const unsigned char*)tree.child_.data<char>(), tree.child_.num_bytes()));
    shape(tree.data_);
    fprintf(f, ", \"data_word_size\": %zu, \"data_fnv1a64\": \"%016llx\"}\n", tree.data_.word_size,
            (unsigned long long)fnv1a((const unsigned char*)tree.data_.data<char>(), tree.data_.num_bytes()));
    fclose(f);
    return 0;
}

static int half_mode(const char* out_path) {
    g_out = fopen(out_path, "wb");
    if (!g_out) return 2;
    std::vector<float> wide(65536);
    for (uint32_t h = 0; h < 65536; ++h) {
        __half v;
        v.bits = (uint16_t)h;
        wide[h] = __half2float(v);
    }
    emit_f32("widen", wide);
    // narrowing: every 4099th binary32 pattern
    std::vector<float> src;
    std::vector<uint64_t> narrow;
    for (uint64_t u = 0; u < (1ull << 32); u += 4099) {
        uint32_t b = (uint32_t)u;
        float f;
        memcpy(&f, &b, 4);
        src.push_back(f);
        narrow.push_back(__half(f).bits);
    }
    emit_f32("narrow_src", src);
    emit_u64("narrow", narrow);
    fclose(g_out);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "--n3tree")) return n3tree_mode(argv[2], argv[3]);
    if (argc == 3 && !strcmp(argv[1], "--half")) return half_mode(argv[2]);
    if (argc != 3) {
        fprintf(stderr, "usage: rt_core_kat case.npz out.bin | --n3tree tree.npz out.json | --half out.bin\n");
        return 2;
    }
    cnpy::npz_t z = cnpy::npz_load(argv[1]);
    auto count = [&](const char* k) -> size_t { return z.count(k) ? z[k].num_vals : 0; };
    for (const char* k : {"child", "data", "scale", "offset", "fmt", "optf", "opti"})
        if (!z.count(k)) {
            fprintf(stderr, "case lacks %s\n", k);
            return 2;
        }

    // the tree, filled as N3Tree::load_npz would (n3tree.cpp:228-362) from arrays that are already decoded
    N3Tree tree;
    const cnpy::NpyArray& child = z["child"];
    const cnpy::NpyArray& data = z["data"];
    if (child.word_size != 4 || data.word_size != 2 || data.shape.size() != 5) return 2;
    tree.N = (int)child.shape[1];
    tree.capacity = (int)child.shape[0];
    tree.data_dim = (int)data.shape[4];
    const int32_t* fmt = z["fmt"].data<int32_t>();
    tree.data_format.format = (decltype(tree.data_format.format))fmt[0];
    tree.data_format.basis_dim = fmt[1];
    for (int k = 0; k < 3; ++k) {
        tree.scale[k] = z["scale"].data<float>()[k];
        tree.offset[k] = z["offset"].data<float>()[k];
    }
    tree.use_ndc = false;
    tree.ndc_width = tree.ndc_height = tree.ndc_focal = 0.f;
    tree.child_ = child;
    tree.data_ = data;
    if (count("extra")) {
        tree.extra_ = z["extra"];
    } else {
        tree.extra_.reinit({1}, 4, false);  // (never read; TreeSpec takes the address of its first element)
    }
    const TreeSpec spec(tree, /*cpu=*/true);

    RenderOptions opt;
    const float* optf = z["optf"].data<float>();
    const int32_t* opti = z["opti"].data<int32_t>();
    opt.step_size = optf[0];
    opt.sigma_thresh = optf[1];
    for (int k = 0; k < 6; ++k) opt.render_bbox[k] = optf[2 + k];
    opt.basis_minmax[0] = opti[0];
    opt.basis_minmax[1] = opti[1];
    const int ndst = opti[2];

    g_out = fopen(argv[2], "wb");
    if (!g_out) return 2;

    // ---- query: internal::query_single_from_root at xyz = offset + scale * p
    {
        const size_t nq = count("qpts") / 3;
        std::vector<float> xyz_in(nq * 3), local(nq * 3), cube(nq), sigma(nq);
        std::vector<int64_t> leaf(nq);
        for (size_t i = 0; i < nq; ++i) {
            float xyz[3];
            for (int k = 0; k < 3; ++k) {
                const float scaled = tree.scale[k] * z["qpts"].data<float>()[i * 3 + k];
                xyz[k] = tree.offset[k] + scaled;
                xyz_in[i * 3 + k] = xyz[k];
            }
            const half* val = nullptr;
            volrend::internal::query_single_from_root(spec, xyz, &val, &cube[i]);
            leaf[i] = (int64_t)(val - spec.data) / spec.data_dim;
            sigma[i] = __half2float(val[spec.data_dim - 1]);
            for (int k = 0; k < 3; ++k) local[i * 3 + k] = xyz[k];
        }
        emit_f32("q_xyz", xyz_in);
        emit_i64("q_leaf", leaf);
        emit_f32("q_cube_sz", cube);
        emit_f32("q_sigma", sigma);
        emit_f32("q_local", local);
    }

    // ---- basis: internal::maybe_precalc_basis, 25 floats per direction (entries it does not write stay 0)
    {
        const size_t nb = count("bdirs") / 3;
        std::vector<float> basis(nb * VOLREND_GLOBAL_BASIS_MAX, 0.f);
        for (size_t i = 0; i < nb; ++i)
            volrend::internal::maybe_precalc_basis(spec, z["bdirs"].data<float>() + i * 3, &basis[i * VOLREND_GLOBAL_BASIS_MAX]);
        emit_f32("basis", basis);
    }

    // ---- dst: device::sample_dst<SPP>
    if (ndst > 0) {
        dst_table<1>(ndst);
        dst_table<2>(ndst);
        dst_table<3>(ndst);
        dst_table<4>(ndst);
        dst_table<6>(ndst);
        dst_table<8>(ndst);
        dst_table<16>(ndst);
        dst_table<32>(ndst);
    }

    // ---- trace: device::trace_ray<float, SPP>
    {
        Rays rays;
        rays.n = count("origins") / 3;
        if (rays.n) {
            if (count("dirs") != rays.n * 3 || count("tmax") != rays.n) return 2;
            rays.dir.resize(rays.n * 3);
            rays.cen.resize(rays.n * 3);
            rays.tmax = z["tmax"].data<float>();
            for (size_t i = 0; i < rays.n; ++i) {
                float dir[3];
                for (int k = 0; k < 3; ++k) dir[k] = z["dirs"].data<float>()[i * 3 + k];
                _normalize(dir);  // cuda/common.cuh:22-27
                for (int k = 0; k < 3; ++k) {
                    rays.dir[i * 3 + k] = dir[k];
                    const float scaled = tree.scale[k] * z["origins"].data<float>()[i * 3 + k];
                    rays.cen[i * 3 + k] = tree.offset[k] + scaled;  // volrend.cu:142-144
                }
            }
            emit_f32("ray_dir", rays.dir);
            emit_f32("ray_cen", rays.cen);
            trace_table<1>(spec, opt, rays);
            trace_table<2>(spec, opt, rays);
            trace_table<3>(spec, opt, rays);
            trace_table<4>(spec, opt, rays);
            trace_table<6>(spec, opt, rays);
            trace_table<8>(spec, opt, rays);
            trace_table<16>(spec, opt, rays);
            trace_table<32>(spec, opt, rays);
        }
    }
    fclose(g_out);
    return 0;
}
