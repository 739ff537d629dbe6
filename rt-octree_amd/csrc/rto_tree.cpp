// rto_tree.cpp -- the rto_tree_* half of the C ABI (include/rto.h): a tree's upload in stages, its lazily rebuilt reference
// arrays, point queries and the basis probe.  The layouts themselves are computed in host/tree_layout.cpp.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "host/n3tree_host.h"
#include "host/tree_layout.h"
#include "rto_internal.h"

namespace {

// Device memory of a tree: allocate / free one of its arrays and keep the tally that rto_tree_info::device_bytes reports
bool tree_alloc(rto_tree* t, void** p, size_t bytes) {
    if (hipMalloc(p, bytes) != hipSuccess) return false;
    t->info.device_bytes += (int64_t)bytes;
    return true;
}
void tree_release(rto_tree* t, void** p, size_t bytes) {
    if (!*p) return;
    (void)hipFree(*p);
    *p = nullptr;
    t->info.device_bytes -= (int64_t)bytes;
}

// The host arrays of an upload as its stages take them (breadth-first after relay_breadth_first)
struct HostArrays {
    const int32_t* child;
    const uint16_t* data;          // nullptr: a quantised tree
    const rto::HostTree* quant;    // nullptr: a dense tree
    const uint16_t* sigma;         // the fp16 density of slot sl is sigma[sl * sigma_stride]
    size_t sigma_stride;
    int64_t capacity, n_slots;
    int N, data_dim, max_depth;
    size_t child_bytes() const { return (size_t)n_slots * sizeof(int32_t); }
    size_t data_bytes() const { return (size_t)n_slots * data_dim * sizeof(uint16_t) + 16; }  // (+16: see upload_dense)
};

int hip_fail(const char* what, hipError_t e) { return set_err(RTO_E_HIP, std::string(what) + hipGetErrorString(e)); }

// ---- the stages of an upload, in the order upload_tree runs them ----

int validate_upload(const int32_t* child, const uint16_t* data, int64_t capacity, int N, int data_dim, const rto::DataFormat& fmt,
                    const rto::HostTree* quant, const float* extra, int64_t extra_floats, rto_tree** out, int* max_depth) {
    if (!child || (!data && !quant) || capacity <= 0 || N < 1 || data_dim < 1 || !out)
        return set_err(RTO_E_INVALID, "rto_tree: null array or non-positive size");
    if (quant && (N != 2 || fmt.format != RTO_FMT_SH ||
                  !(fmt.basis_dim == 4 || fmt.basis_dim == 9 || fmt.basis_dim == 16 || fmt.basis_dim == 25) ||
                  quant->n_basis != fmt.basis_dim))
        return set_err(RTO_E_UNSUPPORTED, "direct rendering of quantised trees needs N == 2 and SH4/9/16/25 with matching codebooks");
    if (fmt.format == RTO_FMT_SH || fmt.format == RTO_FMT_SG || fmt.format == RTO_FMT_ASG) {
        if (fmt.basis_dim < 1 || data_dim != 3 * fmt.basis_dim + 1)
            return set_err(RTO_E_FORMAT, "rto_tree: data_dim " + std::to_string(data_dim) + " does not match format " +
                                             fmt.to_string());
        if (fmt.basis_dim > RTO_BASIS_MAX)
            return set_err(RTO_E_FORMAT, "rto_tree: basis_dim above " + std::to_string(RTO_BASIS_MAX));
    } else if (data_dim < 4) {
        return set_err(RTO_E_FORMAT, "rto_tree: RGBA trees need data_dim >= 4");
    }
    if (extra) {
        const std::string bad = rto::check_lobes(fmt, extra, extra_floats);
        if (!bad.empty()) return set_err(RTO_E_FORMAT, "rto_tree: " + bad);
    }
    try {
        *max_depth = rto::tree_max_depth(child, capacity, N);
    } catch (const std::exception& e) {
        return set_err(RTO_E_FORMAT, e.what());
    }
    return RTO_OK;
}

// Re-lay the tree breadth-first unless the file already is (derived layout: every query returns the same
// leaf values, so no pixel can change -- tests/test_render_parity.py::test_node_order_never_changes_pixels)
// -> order[new] = old, empty when the file's order stays
std::vector<int64_t> relay_breadth_first(HostArrays& h, rto::Relaid& relaid, rto::HostTree& quant_relaid) {
    const int64_t N3 = h.n_slots / h.capacity;
    const std::vector<int64_t> order = rto::bfs_order(h.child, h.capacity, N3);
    bool identity = true;
    for (int64_t n = 0; n < h.capacity && identity; ++n) identity = order[(size_t)n] == n;
    if (identity) return {};
    rto::relay_tree(order, h.child, h.data, h.capacity, N3, h.data_dim, h.quant, relaid);
    h.child = relaid.child.data();
    if (h.data) h.data = relaid.data.data();
    if (h.quant) {
        quant_relaid = *h.quant;
        quant_relaid.q_map = relaid.q_map.data();
        quant_relaid.q_sigma = relaid.q_sigma.data();
        quant_relaid.q_retained = relaid.q_retained.empty() ? nullptr : relaid.q_retained.data();
        h.quant = &quant_relaid;
    }
    return order;
}

// child[] first, for either kind of tree
bool upload_child(rto_tree* t, const HostArrays& h) {
    return tree_alloc(t, &t->d_child, h.child_bytes()) && hipMemcpy(t->d_child, h.child, h.child_bytes(), hipMemcpyHostToDevice) == hipSuccess;
}

int upload_dense(rto_tree* t, const HostArrays& h) {
    // +16 B: shade_leaf_packed reads whole dwords around a record and may touch up to 4 B past it
    const size_t bytes = h.data_bytes() - 16;
    if (!upload_child(t, h)) return set_err(RTO_E_HIP, "tree upload failed");
    if (!tree_alloc(t, &t->d_data, h.data_bytes())) return set_err(RTO_E_HIP, "hipMalloc(tree.data) failed");
    if (hipMemcpy(t->d_data, h.data, bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset((char*)t->d_data + bytes, 0, 16) != hipSuccess)
        return set_err(RTO_E_HIP, "tree upload failed");
    return RTO_OK;
}

int upload_quant(rto_tree* t, const HostArrays& h) {
    const rto::HostTree* quant = h.quant;
    const int64_t n_slots = h.n_slots;
    const int nq = quant->n_basis - quant->n_retain, nr = quant->n_retain;
    const int q_rec = (3 * nr + nq + 1) & ~1;  // u16 per slot record, dword aligned
    const size_t map_b = (size_t)nq * n_slots * 2, ret_b = (size_t)nr * n_slots * 3 * 2, sig_b = (size_t)n_slots * 2;
    const size_t rec_b = (size_t)n_slots * q_rec * 2, col_b = (size_t)nq * 65536 * 8;
    // codebooks: {r,g,b} fp16 -> {r,g,b,0} so that one 8 B load fetches an entry
    std::vector<uint16_t> cb((size_t)nq * 65536 * 4, 0);
    for (size_t i = 0; i < (size_t)nq * 65536; ++i)
        for (int c = 0; c < 3; ++c) cb[i * 4 + c] = quant->q_colors[i * 3 + c];
    void *tmp_map = nullptr, *tmp_ret = nullptr;
    auto up = [&](void** dst, const void* src, size_t bytes, bool staging) {  // (staging arrays are not the tree's: no tally)
        if (bytes == 0) return true;
        const bool got = staging ? hipMalloc(dst, bytes) == hipSuccess : tree_alloc(t, dst, bytes);
        return got && hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
    };
    // file layout up, re-laid slot-major on the device, staging freed (peak = 2x the quantised arrays)
    const bool ok = upload_child(t, h) && up(&tmp_map, quant->q_map, map_b, true) && up(&tmp_ret, quant->q_retained, ret_b, true) &&
                    up(&t->d_qcolors, cb.data(), col_b, false) && up(&t->d_qsigma, quant->q_sigma, sig_b, false) &&
                    tree_alloc(t, &t->d_qrec, rec_b) &&
                    rto::launch_pack_quant((const uint16_t*)tmp_map, (const uint16_t*)tmp_ret, n_slots, nr, nq, q_rec,
                                           (uint16_t*)t->d_qrec, nullptr) == hipSuccess &&
                    hipDeviceSynchronize() == hipSuccess;
    if (tmp_map) (void)hipFree(tmp_map);
    if (tmp_ret) (void)hipFree(tmp_ret);
    if (!ok) return set_err(RTO_E_HIP, "quantised tree upload failed");
    t->quant = true;
    t->dev.q_retain = nr;
    t->dev.q_rec = q_rec;
    return RTO_OK;
}

// traversal image for the fast kernel: N == 2, depth within the 24 fixed-point bits, slot index within the 29
// bits of a top-grid entry (the hit-list budget depends on the SPP and is checked per launch: slots_fit_spp)
int build_nodew(rto_tree* t, const HostArrays& h) {
    if (!(h.N == 2 && h.max_depth <= 24 && h.n_slots < (int64_t(1) << rto::kGridSlotBits))) return RTO_OK;
    int* d_bad = nullptr;
    if (!tree_alloc(t, &t->d_nodew, (size_t)h.n_slots * 4) || hipMalloc((void**)&d_bad, 4) != hipSuccess ||
        hipMemset(d_bad, 0, 4) != hipSuccess)
        return set_err(RTO_E_HIP, "hipMalloc(nodew) failed");
    // sigma source: the last value of each dense record, or the quantised set's own sigma array
    const uint16_t* d_sigma = h.quant ? (const uint16_t*)t->d_qsigma : (const uint16_t*)t->d_data;
    hipError_t e = rto::launch_build_nodew((const int32_t*)t->d_child, d_sigma, h.n_slots, h.quant ? 1 : h.data_dim,
                                           (uint32_t*)t->d_nodew, d_bad, nullptr);
    int bad = 0;
    if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost);
    (void)hipFree(d_bad);
    if (e != hipSuccess) return hip_fail("build_nodew failed: ", e);
    t->fast_ok = !bad;
    if (bad) tree_release(t, &t->d_nodew, (size_t)h.n_slots * 4);
    return RTO_OK;
}

// culling cells for the batched path (see TreeDev::occ_cells)
int upload_culling_cells(rto_tree* t, const HostArrays& h, const float scale[3], const float offset[3]) {
    if (!t->fast_ok || (t->flags & RTO_TREE_NO_CULLING)) return RTO_OK;
    std::vector<float> cells, cubes;  // (cubes: the same cells as whole cubes, for tuning "cull_cubes")
    if (!rto::culling_cells(h.child, h.capacity, scale, offset, h.sigma, h.sigma_stride, cells, &cubes)) return RTO_OK;
    const size_t bytes = cells.empty() ? 32 : cells.size() * sizeof(float);
    auto up = [&](void** dst, const std::vector<float>& src) {
        return tree_alloc(t, dst, bytes) && (src.empty() || hipMemcpy(*dst, src.data(), bytes, hipMemcpyHostToDevice) == hipSuccess);
    };
    if (!up(&t->d_occ, cells) || !up(&t->d_occ_cubes, cubes)) return set_err(RTO_E_HIP, "hipMalloc(culling cells) failed");
    t->dev.occ_cells = (const float4*)t->d_occ;
    t->dev.n_occ_cells = (int)(cells.size() / 8);
    return RTO_OK;
}

// shortcut grid over the top levels: 2^(3G) x 8 B (2 MB at G = 6: L2-resident)
// (6 levels: measured again in round 3 with 7 waves per SIMD -- 5 levels 7.1-7.25 ms per 100 frames, 6: 6.88-7.0,
//  7 (16 MB): 6.85-6.96, 8 (134 MB): 6.93-6.99)
int build_top_grid(rto_tree* t, const HostArrays& h) {
    if (!t->fast_ok || h.max_depth < 3) return RTO_OK;
    int top_levels = h.max_depth - 1 < 6 ? h.max_depth - 1 : 6;
    if (const char* ev = getenv("RTO_TOP_LEVELS")) {  // (A/B hook: levels the top grid covers, 3..8; same pixels for every value)
        const int g = atoi(ev);
        if (g >= 3 && g <= 8 && g <= h.max_depth - 1) top_levels = g;
    }
    if (!tree_alloc(t, &t->d_topgrid, (size_t)8 << (3 * top_levels))) return set_err(RTO_E_HIP, "hipMalloc(topgrid) failed");
    hipError_t e = rto::launch_build_topgrid((const uint32_t*)t->d_nodew, top_levels, (uint2*)t->d_topgrid, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail("build_topgrid failed: ", e);
    t->dev.top_levels = top_levels;
    return RTO_OK;
}

// the two-level traversal image of the batched kernel (build_wide_image).  Not enough memory for it is no error: the kernel
// then walks the one-level image
void upload_wide_image(rto_tree* t, const HostArrays& h) {
    if (!t->fast_ok || getenv("RTO_NO_WIDE")) return;
    rto::WideImage wi;
    if (!rto::build_wide_image(h.child, h.capacity, t->dev.top_levels, h.sigma, h.sigma_stride, wi)) return;
    const size_t wb = wi.widew.size() * 4, ob = wi.worig.size() * 4, gb = wi.gslot.size() * 4;
    const bool up = tree_alloc(t, &t->d_widew, wb) && tree_alloc(t, &t->d_worig, ob) && tree_alloc(t, &t->d_grid2, gb) &&
                    hipMemcpy(t->d_widew, wi.widew.data(), wb, hipMemcpyHostToDevice) == hipSuccess &&
                    hipMemcpy(t->d_worig, wi.worig.data(), ob, hipMemcpyHostToDevice) == hipSuccess &&
                    hipMemcpy(t->d_grid2, wi.gslot.data(), gb, hipMemcpyHostToDevice) == hipSuccess;
    if (!up) {
        (void)hipGetLastError();
        tree_release(t, &t->d_widew, wb);
        tree_release(t, &t->d_worig, ob);
        tree_release(t, &t->d_grid2, gb);
        return;
    }
    t->dev.widew = (const uint32_t*)t->d_widew;
    t->dev.worig = (const uint32_t*)t->d_worig;
    t->dev.wgslot = (const uint32_t*)t->d_grid2;
    t->dev.wide_entries = wi.n_wide * 64u;
    t->dev.wide_grid_nodes = wi.grid_nodes;
}

int upload_lobes(rto_tree* t, const float* extra, int64_t extra_floats) {
    if (!extra) return RTO_OK;
    const size_t eb = (size_t)extra_floats * sizeof(float);
    if (!tree_alloc(t, &t->d_extra, eb) || hipMemcpy(t->d_extra, extra, eb, hipMemcpyHostToDevice) != hipSuccess)
        return set_err(RTO_E_HIP, "lobe (extra_data) upload failed");
    return RTO_OK;
}

// aligned copy of the coefficients for the shading kernels (+ 64 / 128 B per slot): compact, by entry of the two-level image or
// by slot.  Not enough memory for it is no error: the kernels then shade from data[]
// (SG / ASG records have the layout of SH records of the same basis size: only the basis the coefficients meet differs)
int build_records(rto_tree* t, const HostArrays& h, const rto::DataFormat& fmt) {
    const bool sh_like = fmt.format == RTO_FMT_SH || rto::lobe_floats(fmt.format) != 0;
    if (!t->fast_ok || h.quant || !sh_like || !(fmt.basis_dim == 9 || fmt.basis_dim == 16) || (t->flags & RTO_TREE_COMPACT))
        return RTO_OK;
    const int64_t n_slots = h.n_slots;
    const int rec = 3 * fmt.basis_dim * 2 <= 64 ? 32 : 64;  // = shrec_halves()
    int64_t n_rec = n_slots;
    if (t->flags & RTO_TREE_COMPACT_RECORDS) {
        // records only for the leaf slots a ray can hit -- density > 0 (a hit needs sigma > sigma_thresh >= 0,
        // rt_core.cuh:252; launches with a negative threshold are refused for such a tree) -- in slot order
        std::vector<uint32_t> idx((size_t)n_slots, rto::kNoRecord);
        uint32_t n = 0;
        for (int64_t sl = 0; sl < n_slots; ++sl)
            if (h.child[sl] == 0 && rto::half_to_float(h.sigma[(size_t)sl * h.sigma_stride]) > 0.f) idx[(size_t)sl] = n++;
        n_rec = n > 0 ? n : 1;
        if (!tree_alloc(t, &t->d_recidx, (size_t)n_slots * 4) ||
            hipMemcpy(t->d_recidx, idx.data(), (size_t)n_slots * 4, hipMemcpyHostToDevice) != hipSuccess)
            return set_err(RTO_E_HIP, "hipMalloc(record index) failed");
    }
    // Round 5: with a two-level traversal image the records follow ITS entries (TreeDev::rec_by_entry), so that a hit entry
    // names its record and nothing translates between traversal and shading.  Not with compact records (their index is
    // per slot), not when the entries would not fit the hit-entry budget of every SPP (2^26 at SPP 32: such a tree must
    // stay able to fall back to the one-level walk, whose hits name slots), not with RTO_TREE_SLOT_RECORDS (A/B, tests).
    const int64_t n_entries = t->dev.widew ? (int64_t)t->dev.wide_entries + (int64_t)t->dev.wide_grid_nodes * 64 : 0;
    // (the gate is fast_path_for_spp's own test at the largest supported SPP: a by-entry tree has no one-level fallback)
    bool by_entry = n_entries > 0 && !(t->flags & RTO_TREE_COMPACT_RECORDS) && slots_fit_spp(n_entries, kMaxSpp) &&
                    !getenv("RTO_TREE_SLOT_RECORDS");
    size_t rb = (size_t)(by_entry ? n_entries : n_rec) * rec * 2;
    bool got = tree_alloc(t, &t->d_shrec, rb) && !(by_entry && getenv("RTO_TEST_FAIL_ENTRY_RECORDS"));
    if (!got && by_entry) {  //  the entry-ordered copy (up to ~8x the slots) does not fit: the slot-ordered one may
        (void)hipGetLastError();
        tree_release(t, &t->d_shrec, rb);
        by_entry = false;
        rb = (size_t)n_rec * rec * 2;
        got = tree_alloc(t, &t->d_shrec, rb);
    }
    if (!got) {  // not enough memory for the copy: shade from data[]
        (void)hipGetLastError();
        tree_release(t, &t->d_recidx, (size_t)n_slots * 4);
        return RTO_OK;
    }
    hipError_t e;
    if (by_entry) {
        rto::TreeDev td = t->dev;  // (the look-up tables of the two-level image are set; the rest of it as far as the kernel reads it)
        td.nodew = (const uint32_t*)t->d_nodew;
        td.data_dim = h.data_dim;
        e = rto::launch_build_shrec_wide(td, (const uint16_t*)t->d_data, n_entries, rec, (uint16_t*)t->d_shrec, nullptr);
        t->dev.rec_by_entry = 1;
    } else
        e = rto::launch_build_shrec((const uint16_t*)t->d_data, n_slots, h.data_dim, rec, (const uint32_t*)t->d_recidx,
                                    (uint16_t*)t->d_shrec, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail("build_shrec failed: ", e);
    t->shrec_halves = rec;
    return RTO_OK;
}

// what the kernels of this tree never read goes: child[] / data[] of a tree with coefficient records (rebuilt on demand:
// ensure_reference_arrays), and the quantised set's sigma array, which now lives in the traversal image
void release_upload_only_arrays(rto_tree* t, const HostArrays& h) {
    if (t->d_shrec && !(t->flags & RTO_TREE_KEEP_REFERENCE)) {
        tree_release(t, &t->d_data, h.data_bytes());
        tree_release(t, &t->d_child, h.child_bytes());
        t->reference_dropped = true;
    }
    tree_release(t, &t->d_qsigma, (size_t)h.n_slots * 2);
}

void fill_tree_dev_and_info(rto_tree* t, const HostArrays& h, const rto::DataFormat& fmt, const float scale[3], const float offset[3]) {
    rto::TreeDev& d = t->dev;  // (the stages set what they built: occ_cells, top_levels, the two-level image, rec_by_entry, q_*)
    d.topgrid = (const uint2*)t->d_topgrid;
    d.shrec = (const uint16_t*)t->d_shrec;
    d.recidx = (const uint32_t*)t->d_recidx;
    d.qrec = (const uint16_t*)t->d_qrec;
    if (h.quant)
        d.qcolors = (const uint2*)t->d_qcolors;
    else
        d.extra = (const float*)t->d_extra;  // (shares qcolors' place in TreeDev)
    d.data = (const uint16_t*)t->d_data;
    d.child = (const int32_t*)t->d_child;
    d.nodew = (const uint32_t*)t->d_nodew;
    d.N = h.N;
    d.N3 = (int)(h.n_slots / h.capacity);
    d.data_dim = h.data_dim;
    d.format = fmt.format;
    d.basis_dim = fmt.basis_dim;
    d.ndc_width = -1.f;  // data_spec.hpp:49
    d.ndc_height = 0.f;
    d.ndc_focal = 0.f;
    d.max_depth = h.max_depth;

    rto_tree_info& inf = t->info;  // (device_bytes: the tally of tree_alloc / tree_release)
    inf.capacity = h.capacity;
    inf.N = h.N;
    inf.data_dim = h.data_dim;
    inf.format = fmt.format;
    inf.basis_dim = fmt.basis_dim;
    for (int i = 0; i < 3; ++i) {
        d.offset[i] = inf.offset[i] = offset[i];
        d.scale[i] = inf.scale[i] = scale[i];
    }
    inf.use_ndc = 0;
    inf.ndc_width = inf.ndc_height = inf.ndc_focal = 0.f;
    inf.max_depth = h.max_depth;
    inf.wide_nodes = d.widew ? (int64_t)(d.wide_entries / 64u) : 0;
}

// extra / extra_floats: the lobes of an SG / ASG tree (nullptr: none -- the tree loads, its launches are refused); ignored
// for SH and RGBA trees, as by the reference
int upload_tree(const int32_t* child, const uint16_t* data, int64_t capacity, int N, int data_dim,
                const rto::DataFormat& fmt, const float scale[3], const float offset[3], int device,
                rto_tree** out, const rto::HostTree* quant = nullptr, int flags = 0, const float* extra = nullptr,
                int64_t extra_floats = 0) {
    if (rto::lobe_floats(fmt.format) == 0) extra = nullptr;
    int max_depth = 0;
    int rc = validate_upload(child, data, capacity, N, data_dim, fmt, quant, extra, extra_floats, out, &max_depth);
    if (rc != RTO_OK) return rc;

    rc = check_device_index(device, kNoDeviceMsg);
    if (rc != RTO_OK) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");

    HostArrays h = {child, data, quant, nullptr, 0, capacity, capacity * N * N * N, N, data_dim, max_depth};
    rto::Relaid relaid;
    rto::HostTree quant_relaid;
    const std::vector<int64_t> node_old = relay_breadth_first(h, relaid, quant_relaid);
    h.sigma = h.quant ? h.quant->q_sigma : h.data + data_dim - 1;
    h.sigma_stride = h.quant ? 1 : (size_t)data_dim;

    auto t = new rto_tree();
    t->device = device;
    t->flags = flags;
    rc = h.quant ? upload_quant(t, h) : upload_dense(t, h);
    if (rc == RTO_OK) rc = build_nodew(t, h);
    if (rc == RTO_OK) rc = upload_culling_cells(t, h, scale, offset);
    if (rc == RTO_OK) rc = build_top_grid(t, h);
    if (rc == RTO_OK) upload_wide_image(t, h);
    if (rc == RTO_OK) rc = upload_lobes(t, extra, extra_floats);
    if (rc == RTO_OK) rc = build_records(t, h, fmt);
    if (rc == RTO_OK) release_upload_only_arrays(t, h);
    if (rc == RTO_OK && !node_old.empty()) {  // the caller's node numbering, for per-slot outputs (rto_tree_leaf_weights)
        const std::vector<uint32_t> old32(node_old.begin(), node_old.end());
        if (!tree_alloc(t, &t->d_node_old, old32.size() * sizeof(uint32_t)) ||
            hipMemcpy(t->d_node_old, old32.data(), old32.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
            rc = set_err(RTO_E_HIP, "tree upload failed");
    }
    if (rc == RTO_OK && h.quant && !t->fast_ok)
        rc = set_err(RTO_E_UNSUPPORTED, "direct rendering of quantised trees needs the N == 2 traversal image");
    if (rc != RTO_OK) {
        rto_tree_free(t);
        return rc;
    }
    fill_tree_dev_and_info(t, h, fmt, scale, offset);
    *out = t;
    return RTO_OK;
}

}  // namespace

bool missing_lobes(const rto_tree* tree) { return rto::lobe_floats(tree->dev.format) != 0 && !tree->d_extra; }
const char* const missing_lobes_msg = "an SG / ASG tree needs its lobes: the tree has no extra_data (npz key) / extra (rto_tree_from_arrays_extra)";

int fast_path_for_spp(const rto_tree* tree, int spp, int wide_bits, rto::TreeDev* td) {
    if (td) *td = tree->dev;
    if (!tree->fast_ok) return 0;
    const int64_t n_slots = tree->info.capacity * tree->dev.N3;
    const int64_t wide = tree->dev.widew ? (int64_t)tree->dev.wide_entries + (int64_t)tree->dev.wide_grid_nodes * 64 : 0;
    const bool wide_fits = wide_bits > 0 ? wide < (int64_t(1) << wide_bits) : slots_fit_spp(wide, spp);
    if (tree->dev.rec_by_entry) return wide_fits ? 1 : 0;  // (its records are indexed by the entries: no one-level fallback; the
                                                           //  upload only chooses that layout when the entries fit every SPP)
    if (!slots_fit_spp(n_slots, spp)) return 0;
    if (wide_fits) return 1;
    // the entry count of the two-level image can be ~8x the slot count of the deepest level (odd number of levels
    // below the grid), so it can exceed the budget where the slots do not -- such a launch walks the one-level image
    // (nodew + topgrid, the WIDE = false instantiations) instead of dropping to the generic kernel
    if (td) {
        td->widew = nullptr;
        td->wgslot = nullptr;
        td->worig = nullptr;
        td->wide_entries = 0;
        td->wide_grid_nodes = 0;
    }
    return 2;
}

int ensure_reference_arrays(const rto_tree* tree) {
    if (!tree->reference_dropped) return RTO_OK;
    rto_tree* t = const_cast<rto_tree*>(tree);  // derived, lazily materialised state of a logically const tree
    std::lock_guard<std::mutex> lock(t->rebuild_mutex);
    if (!t->reference_dropped) return RTO_OK;
    DeviceGuard guard(t->device);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    const int64_t n_slots = t->info.capacity * t->dev.N3;
    const size_t data_bytes = (size_t)n_slots * t->dev.data_dim * sizeof(uint16_t), child_bytes = (size_t)n_slots * sizeof(int32_t);
    // (the handle's pointers and tally move while the rebuild runs; readers go by reference_dropped and dev.data / dev.child, set last)
    if (!tree_alloc(t, &t->d_data, data_bytes + 16) || !tree_alloc(t, &t->d_child, child_bytes)) {
        tree_release(t, &t->d_data, data_bytes + 16);
        (void)hipGetLastError();
        return set_err(RTO_E_HIP, "the generic kernel needs the tree's child[] / data[] arrays back on the device: hipMalloc failed");
    }
    hipError_t e = hipMemset((char*)t->d_data + data_bytes, 0, 16);
    if (e == hipSuccess)
        e = rto::launch_rebuild_reference(t->dev.rec_by_entry ? nullptr : (const uint16_t*)t->d_shrec, (const uint32_t*)t->d_nodew,
                                          (const uint32_t*)t->d_recidx, n_slots, t->dev.data_dim, t->shrec_halves, (uint16_t*)t->d_data,
                                          (int32_t*)t->d_child, nullptr);
    if (e == hipSuccess && t->dev.rec_by_entry)  // entry-ordered records: the coefficients in a second pass, entry by entry
        e = rto::launch_rebuild_reference_wide(t->dev, (int64_t)t->dev.wide_entries + (int64_t)t->dev.wide_grid_nodes * 64, t->shrec_halves,
                                               (uint16_t*)t->d_data, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        tree_release(t, &t->d_data, data_bytes + 16);
        tree_release(t, &t->d_child, child_bytes);
        return hip_fail("rebuilding child[] / data[] failed: ", e);
    }
    t->dev.data = (const uint16_t*)t->d_data;
    t->dev.child = (const int32_t*)t->d_child;
    t->reference_dropped = false;
    return RTO_OK;
}

int query_plan(const rto_tree* tree, bool values, int* walk, rto::ValuesSrc* vs) {
    const rto::TreeDev& d = tree->dev;
    *walk = d.widew ? rto::kWalkWide : d.nodew ? rto::kWalkNodew : rto::kWalkChild;
    *vs = rto::ValuesSrc{nullptr, 0u, 0};
    if (!values) return RTO_OK;
    if (tree->quant)
        return set_err(RTO_E_UNSUPPORTED, "the values of a quantised tree loaded with RTO_TREE_QUANT_DIRECT live in its codebooks: sigma, level "
                                          "and cube can be queried, values need an expanded tree");
    // compact records exist for leaves of positive density only, and the upload released data[]: the coefficients of the other
    // leaves are gone (ensure_reference_arrays rebuilds them as zeros, which no ray can see)
    if (tree->d_recidx && !(tree->flags & RTO_TREE_KEEP_REFERENCE))
        return set_err(RTO_E_UNSUPPORTED, "a tree loaded with RTO_TREE_COMPACT_RECORDS keeps the coefficients of leaves of positive density "
                                          "only: load it with RTO_TREE_KEEP_REFERENCE as well to query values (sigma, level and cube work)");
    if (d.shrec && d.rec_by_entry && d.widew)
        *vs = rto::ValuesSrc{d.shrec, (uint32_t)tree->shrec_halves, 1};
    else if (d.shrec && !d.rec_by_entry && !d.recidx)
        *vs = rto::ValuesSrc{d.shrec, (uint32_t)tree->shrec_halves, 0};
    else if (d.data)  // (the uploaded array: only a tree with records ever releases it)
        *vs = rto::ValuesSrc{d.data, (uint32_t)d.data_dim, 0};
    else
        return set_err(RTO_E_UNSUPPORTED, "the tree holds neither coefficient records nor data[] to answer values from");
    return RTO_OK;
}

extern "C" {

int rto_tree_load_npz(const char* path, int device, rto_tree** out) { return rto_tree_load_npz_ex(path, device, 0, out); }

int rto_tree_load_npz_ex(const char* path, int device, int flags, rto_tree** out) {
    if (!path || !out) return set_err(RTO_E_INVALID, "rto_tree_load_npz: null argument");
    rto::HostTree h;
    try {
        if (!h.open(path, (flags & RTO_TREE_QUANT_DIRECT) != 0))
            return set_err(RTO_E_IO, std::string("file does not exist: ") + path);
    } catch (const std::exception& e) {
        return set_err(RTO_E_FORMAT, e.what());
    }
    std::fprintf(stdout, "INFO: Scale %f %f %f\n", h.scale[0], h.scale[1], h.scale[2]);  // n3tree.cpp:264
    int rc = upload_tree(h.child, h.data, h.capacity, h.N, h.data_dim, h.data_format, h.scale, h.offset, device, out,
                         h.quantized ? &h : nullptr, flags, h.extra, h.extra_floats);
    if (rc != RTO_OK) return rc;
    if (h.use_ndc) rto_tree_set_ndc(*out, h.ndc_width, h.ndc_height, h.ndc_focal);
    return RTO_OK;
}

int rto_tree_probe_npz(const char* path, char* json_out, size_t cap) {
    if (!path || !json_out || cap == 0) return set_err(RTO_E_INVALID, "rto_tree_probe_npz: null argument");
    rto::HostTree h;
    try {
        if (!h.open(path)) return set_err(RTO_E_IO, std::string("file does not exist: ") + path);
    } catch (const std::exception& e) {
        return set_err(RTO_E_FORMAT, e.what());
    }
    auto fnv = [](const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        uint64_t x = 1469598103934665603ULL;
        for (size_t i = 0; i < n; ++i) {
            x ^= b[i];
            x *= 1099511628211ULL;
        }
        return x;
    };
    const size_t n_slots = (size_t)h.capacity * h.N * h.N * h.N;
    int max_depth = 0;
    try {
        max_depth = rto::tree_max_depth(h.child, h.capacity, h.N);
    } catch (const std::exception& e) {
        return set_err(RTO_E_FORMAT, e.what());
    }
    // the lobes of an SG / ASG tree as the file stores them (null: none, or an SH / RGBA tree, whose extra_data is ignored)
    std::string extra_shape = "null", extra_fnv = "null";
    if (h.extra) {
        extra_shape = "[";
        for (size_t i = 0; i < h.extra_shape.size(); ++i) extra_shape += (i ? ", " : "") + std::to_string(h.extra_shape[i]);
        extra_shape += "]";
        char hex[24];
        std::snprintf(hex, sizeof(hex), "\"%016llx\"", (unsigned long long)fnv(h.extra, (size_t)h.extra_floats * 4));
        extra_fnv = hex;
    }
    char buf[1024];
    const int n = std::snprintf(
        buf, sizeof(buf),
        "{\"capacity\": %lld, \"N\": %d, \"data_dim\": %d, \"data_format\": \"%s\", \"basis_dim\": %d, "
        "\"scale\": [%.9g, %.9g, %.9g], \"offset\": [%.9g, %.9g, %.9g], \"use_ndc\": %d, \"max_depth\": %d, "
        "\"quantized\": %d, \"child_fnv1a64\": \"%016llx\", \"data_fnv1a64\": \"%016llx\", \"extra_shape\": %s, "
        "\"extra_fnv1a64\": %s}",
        (long long)h.capacity, h.N, h.data_dim, h.data_format.to_string().c_str(), h.data_format.basis_dim,
        h.scale[0], h.scale[1], h.scale[2], h.offset[0], h.offset[1], h.offset[2], (int)h.use_ndc, max_depth,
        (int)!h.decoded.empty(), (unsigned long long)fnv(h.child, n_slots * 4),
        (unsigned long long)fnv(h.data, n_slots * (size_t)h.data_dim * 2), extra_shape.c_str(), extra_fnv.c_str());
    if (n < 0 || (size_t)n + 1 > cap) return set_err(RTO_E_INVALID, "rto_tree_probe_npz: output buffer too small");
    std::memcpy(json_out, buf, (size_t)n + 1);
    return RTO_OK;
}

int rto_tree_from_arrays(const int32_t* child, const uint16_t* data, int64_t capacity, int N, int data_dim,
                         const char* data_format, const float scale[3], const float offset[3], int device,
                         rto_tree** out) {
    return rto_tree_from_arrays_ex(child, data, capacity, N, data_dim, data_format, scale, offset, device, 0, out);
}

int rto_tree_from_arrays_ex(const int32_t* child, const uint16_t* data, int64_t capacity, int N, int data_dim,
                            const char* data_format, const float scale[3], const float offset[3], int device, int flags,
                            rto_tree** out) {
    return rto_tree_from_arrays_extra(child, data, capacity, N, data_dim, data_format, scale, offset, device, flags, nullptr, 0, out);
}

int rto_tree_from_arrays_extra(const int32_t* child, const uint16_t* data, int64_t capacity, int N, int data_dim,
                               const char* data_format, const float scale[3], const float offset[3], int device, int flags,
                               const float* extra, int64_t extra_floats, rto_tree** out) {
    if (!scale || !offset) return set_err(RTO_E_INVALID, "rto_tree_from_arrays: null scale/offset");
    if (!extra && extra_floats != 0) return set_err(RTO_E_INVALID, "rto_tree_from_arrays_extra: null extra with extra_floats != 0");
    rto::DataFormat fmt;
    if (data_format && data_format[0]) {
        fmt.parse(data_format);
    } else if (data_dim == 4) {  // n3tree.cpp:241-254 legacy autodetect
        fmt.format = RTO_FMT_RGBA;
        fmt.basis_dim = -1;
    } else {
        fmt.format = RTO_FMT_SH;
        fmt.basis_dim = (data_dim - 1) / 3;
    }
    return upload_tree(child, data, capacity, N, data_dim, fmt, scale, offset, device, out, nullptr, flags & ~RTO_TREE_QUANT_DIRECT,
                       extra, extra_floats);
}

int rto_tree_set_ndc(rto_tree* t, float w, float h, float focal) {
    if (!t) return set_err(RTO_E_INVALID, "rto_tree_set_ndc: null tree");
    t->info.use_ndc = w > 0;
    t->info.ndc_width = w;
    t->info.ndc_height = h;
    t->info.ndc_focal = focal;
    t->dev.ndc_width = w > 0 ? w : -1.f;
    t->dev.ndc_height = h;
    t->dev.ndc_focal = focal;
    return RTO_OK;
}

int rto_tree_get_info(const rto_tree* t, rto_tree_info* info) {
    if (!t || !info) return set_err(RTO_E_INVALID, "rto_tree_get_info: null argument");
    *info = t->info;
    return RTO_OK;
}

void rto_tree_free(rto_tree* t) {
    if (!t) return;
    DeviceGuard guard(t->device);
    for (void* p : {t->d_data, t->d_child, t->d_nodew, t->d_topgrid, t->d_widew, t->d_worig, t->d_grid2, t->d_shrec, t->d_recidx, t->d_occ,
                    t->d_occ_cubes, t->d_qrec, t->d_qcolors, t->d_qsigma, t->d_extra, t->d_node_old})
        if (p) (void)hipFree(p);
    delete t;
}

int rto_probe_basis(const rto_tree* tree, const rto_options* o, const float* dirs, int64_t n, int path, float* host_out) {
    if (!tree || !o || !dirs || !host_out || n <= 0 || (path != 0 && path != 1))
        return set_err(RTO_E_INVALID, "rto_probe_basis: null argument, n <= 0 or path not 0 / 1");
    if (missing_lobes(tree)) return set_err(RTO_E_FORMAT, missing_lobes_msg);
    if (n > (int64_t(1) << 31) - 256) return set_err(RTO_E_INVALID, "rto_probe_basis: n above 2^31 - 256");
    DeviceGuard guard(tree->device);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    const rto::OptDev od = make_opt_dev(o);
    const size_t in_b = (size_t)n * 3 * sizeof(float), out_b = (size_t)n * RTO_BASIS_MAX * sizeof(float);
    float *d_dirs = nullptr, *d_out = nullptr;
    hipError_t e = hipMalloc((void**)&d_dirs, in_b);
    if (e == hipSuccess) e = hipMalloc((void**)&d_out, out_b);
    if (e == hipSuccess) e = hipMemcpy(d_dirs, dirs, in_b, hipMemcpyHostToDevice);
    bool no_form = false;
    if (e == hipSuccess) {
        e = rto::launch_probe_basis(tree->dev, od, d_dirs, n, path, d_out, nullptr);
        no_form = e == hipErrorInvalidValue;
    }
    if (e == hipSuccess) e = hipMemcpy(host_out, d_out, out_b, hipMemcpyDeviceToHost);
    if (d_dirs) (void)hipFree(d_dirs);
    if (d_out) (void)hipFree(d_out);
    if (no_form) {
        rto::DataFormat fmt;
        fmt.format = tree->dev.format;
        fmt.basis_dim = tree->dev.basis_dim;
        return set_err(RTO_E_UNSUPPORTED, "rto_probe_basis: the shading kernel has no per-B form for " + fmt.to_string());
    }
    if (e != hipSuccess) return set_err(RTO_E_HIP, std::string("rto_probe_basis: ") + hipGetErrorString(e));
    return RTO_OK;
}

int rto_tree_query(const rto_tree* tree, const float* points, int64_t n, const rto_query_out* out, void* stream_) {
    if (!tree || !out) return set_err(RTO_E_INVALID, "rto_tree_query: null tree or out");
    if (n < 0) return set_err(RTO_E_INVALID, "rto_tree_query: n must be >= 0");
    if (n > 0 && !points) return set_err(RTO_E_INVALID, "rto_tree_query: null points with n > 0");
    if ((uintptr_t)out->cube % 16 != 0) return set_err(RTO_E_INVALID, "rto_tree_query: out->cube must be 16-byte aligned");
    int walk;
    rto::ValuesSrc vs;
    int rc = query_plan(tree, out->values != nullptr, &walk, &vs);
    if (rc != RTO_OK) return rc;
    if (n == 0 || (!out->values && !out->sigma && !out->level && !out->cube)) return RTO_OK;
    DeviceGuard guard(tree->device);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    const int64_t per_launch = int64_t(1) << 38;  // (2^30 workgroups of 256 points: inside the grid's 2^31 - 1)
    for (int64_t i0 = 0; i0 < n; i0 += per_launch) {
        rto::QueryOut qo;
        qo.values = out->values ? out->values + i0 * tree->dev.data_dim : nullptr;
        qo.sigma = out->sigma ? out->sigma + i0 : nullptr;
        qo.level = out->level ? out->level + i0 : nullptr;
        qo.cube = out->cube ? out->cube + 4 * i0 : nullptr;
        const hipError_t e = rto::launch_query(tree->dev, walk, vs, points + 3 * i0, std::min(per_launch, n - i0), qo, (hipStream_t)stream_);
        if (e != hipSuccess) return set_err(RTO_E_HIP, std::string("query launch failed: ") + hipGetErrorString(e));
    }
    return RTO_OK;
}

void rto_grid_params_default(rto_grid_params* p, const rto_options* o) {
    if (!p) return;
    rto_options def;
    if (!o) {
        rto_options_default(&def);
        o = &def;
    }
    p->max_depth = o->grid_max_depth;
    p->line_px = 1.f;
    p->color[0] = p->color[1] = p->color[2] = 0.f;  // black lines
    p->background = o->background_brightness;
    p->flags = 0;
}

int rto_draw_grid_layers(const rto_tree* tree, const rto_camera* cams, int n, const rto_grid_params* p, float* depth, float* color,
                         void* stream_) {
    static_assert(RTO_GRID_MERGE == 1, "check_layer_call takes bit 0 of the flags for the merge flag");
    const int rc = check_layer_call("rto_draw_grid_layers", "tree", "RTO_GRID_MERGE", tree, cams, n, p, depth, color, [&]() -> const char* {
        if (!(std::isfinite(p->line_px) && p->line_px > 0.f)) return "line_px must be finite and > 0";
        if (p->max_depth < 0) return "max_depth must be >= 0";
        if (!(std::isfinite(p->color[0]) && std::isfinite(p->color[1]) && std::isfinite(p->color[2]) && std::isfinite(p->background)))
            return "the line colour and the background must be finite";
        return nullptr;
    });
    if (rc != RTO_OK) return rc;
    if (tree->dev.ndc_width > 0)
        return set_err(RTO_E_UNSUPPORTED, "rto_draw_grid_layers: the line width is defined in unwarped space: NDC trees are not drawn");
    if (tree->dev.N != 2) return set_err(RTO_E_UNSUPPORTED, "rto_draw_grid_layers: N != 2");
    int walk;
    rto::ValuesSrc vs;
    (void)query_plan(tree, false, &walk, &vs);
    if (walk == rto::kWalkChild && !tree->dev.child)
        return set_err(RTO_E_UNSUPPORTED, "rto_draw_grid_layers: the tree has neither a traversal image nor child[] resident");
    if (n == 0) return RTO_OK;
    DeviceGuard guard(tree->device);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    rto::GridDraw gd;
    gd.max_depth = std::min(p->max_depth, 22);
    gd.line_px = p->line_px;
    for (int i = 0; i < 3; ++i) gd.color_rgb[i] = p->color[i];
    gd.background = p->background;
    return launch_layer_chunks("grid", cams, n, p->flags, depth, color, [&](const rto::LayerTarget& lt, const rto::LayerCams& lc, int k) {
        gd.target = lt;
        return rto::launch_grid_layers(tree->dev, walk, gd, lc, k, (hipStream_t)stream_);
    });
}

// Host-only check of the two-level traversal image (no device needed): builds it for child[] (breadth-first node order) and
// walks it for n points.  out_level / out_slot / out_sigma: the leaf each point lies in.  tests/test_wide_image.py compares
// them with the plain walk over child[].
int rto_wide_image_probe(const int32_t* child, const uint16_t* sigma_bits, int64_t capacity, int max_depth, int top_levels,
                         const uint32_t* points, int64_t n, int32_t* out_level, int64_t* out_slot, uint16_t* out_sigma,
                         int64_t* out_wide_nodes) {
    if (!child || !sigma_bits || !points || !out_level || !out_slot || !out_sigma || capacity < 1 || n < 0)
        return set_err(RTO_E_INVALID, "rto_wide_image_probe: null argument");
    (void)max_depth;
    rto::WideImage wi;
    if (!rto::build_wide_image(child, capacity, top_levels, sigma_bits, 1, wi))
        return set_err(RTO_E_UNSUPPORTED, "rto_wide_image_probe: the tree has no two-level image (not breadth-first, too deep or too large)");
    if (out_wide_nodes) *out_wide_nodes = wi.n_wide;
    rto::wide_image_lookup(wi, child, top_levels, points, n, out_level, out_slot, out_sigma);
    return RTO_OK;
}

}  // extern "C"
