// rto_internal.h -- what the translation units of the render side of the C ABI (rto_abi.cpp, rto_tree.cpp, rto_render_abi.cpp,
// rto_mesh.cpp) share: the two handle types and a few helpers, on top of rto_abi_common.h (error plumbing, device scope, shared
// checks, scratch buffers).  Not installed; nothing here is an exported symbol.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "rto.h"
#include "rto_abi_common.h"
#include "rto_launch.h"

#pragma GCC visibility push(hidden)

// check_device_index of the contexts and trees (the side handles say it without the parenthesis)
constexpr const char* kNoDeviceMsg = "no HIP device available (librto has no CPU fallback)";
constexpr int kKtRing = 256;
constexpr int kProbeFloats = 128;  // >= 3 * RTO_BASIS_MAX: what the probe's disc reads of a leaf's data_dim - 1 coefficients
#pragma GCC visibility pop

struct rto_tree {
    int device = 0;
    rto::TreeDev dev{};
    rto_tree_info info{};  // (device_bytes: kept by tree_alloc / tree_release, rto_tree.cpp)
    void* d_data = nullptr;
    void* d_child = nullptr;
    void* d_nodew = nullptr;
    void* d_topgrid = nullptr;
    void *d_widew = nullptr, *d_worig = nullptr, *d_grid2 = nullptr;  // two-level traversal image (build_wide_image)
    void* d_shrec = nullptr;  // aligned copy of the SH coefficients (shading)
    void* d_recidx = nullptr; // RTO_TREE_COMPACT_RECORDS: slot -> record of d_shrec
    void* d_occ = nullptr;    // culling cells (TreeDev::occ_cells)
    void* d_occ_cubes = nullptr;  // the same cells as whole cubes (tuning "cull_cubes" renders with these for occ_cells)
    void* d_qrec = nullptr;
    void* d_qcolors = nullptr;
    void* d_qsigma = nullptr;
    void* d_extra = nullptr;  // SG / ASG lobes (TreeDev::extra)
    // the upload re-laid the nodes breadth-first: node_old[n] (uint32) = the index node n has in the arrays the tree was uploaded
    // from, which per-slot outputs of the caller's numbering go by (rto_tree_leaf_weights); nullptr: the order is the same
    void* d_node_old = nullptr;
    bool quant = false;  // rendered from the codebooks; only the batched path can shade it
    int flags = 0;       // the RTO_TREE_* flags of the upload
    bool fast_ok = false;
    // Footprint (VERDICT r2 task 8): a dense SH9 / SH16 tree that renders through the fast / batched kernels reads only
    // nodew + topgrid + shrec, so child[] / data[] are released after the upload and rebuilt from those two on the first
    // launch that selects the generic kernel (ensure_reference_arrays).  RTO_TREE_KEEP_REFERENCE keeps them resident.
    std::atomic<bool> reference_dropped{false};  // (read outside rebuild_mutex: the usual double-checked test)
    int shrec_halves = 0;
    std::mutex rebuild_mutex;
};

// tile rows per band of the XCD ray queues (build_tile_tables; 0: angular wedges, rounds 3-5).  Per 100 C2 frames: wedges 3.84 ms,
// bands of 1 / 2 / 4 / 8 tile rows 3.73 / 3.70 / 3.72 / 3.75; through bench.py 3.92 -> 3.78 (2) / 3.75 (3); C5 2.48 -> 2.37, C3 shape
// 3.30 -> 3.15, C4 unchanged (profiles/r6_y_ab_queue_bands*.txt)
#ifndef RTO_QUEUE_BANDS_DEFAULT
#define RTO_QUEUE_BANDS_DEFAULT 3
#endif
// rto_launch_rays: which rays a workgroup takes (RayBatch::per_xcd); see DESIGN.md "Rays from the caller"
#ifndef RTO_RAY_ORDER_DEFAULT
#define RTO_RAY_ORDER_DEFAULT 0
#endif
struct rto_ctx {
    int device = 0;
    int width = 0, height = 0;
    int frames = 1;  // frame slots (batched launches render slots 0..n-1)
    int sel = 0;     // slot the single-frame entry points and accessors refer to
    int num_cus = 256;
    unsigned long long* queue = nullptr;  // persistent-kernel ray queues (kQueueWords u64)
    rto::FrameDesc* d_frames = nullptr;   // frame table of the batch in flight (kMaxBatch descriptors)
    rto::OccupancyCache occ;              // of the persistent kernel instantiation last launched
    uint32_t* tile_order = nullptr;       // centre-out order of the 8x8 ray tiles (persistent kernel)
    uint32_t* wedge_order = nullptr;      // the same tiles grouped into 8 angular wedges (one ray queue per XCD)
    int wedge_start[rto::kMaxQueues + 1] = {0};
    bool xcd_queues = true;
    bool tile_major = true;
    int tile_block = 4;  // tiles per side of the blocks the wedge queues are ordered by
    int queue_bands = RTO_QUEUE_BANDS_DEFAULT;  // > 0: the XCD queues take BANDS of this many tile rows (band j -> queue j % 8) instead of angular wedges
    uint32_t* hits = nullptr;             // [frames][hits_spp][H*W] traversal -> shading hand-off
    int hits_spp = 0;
    // empty-space culling + ray-queue lists of the batched path (ensure_tile_buffers: allocated with the first launch that culls)
    uint32_t* tile_mask = nullptr;        // [frames][mask_words]
    uint32_t* qlist = nullptr;            // [tiles * frames] live tile slots, queue after queue
    uint32_t* qscratch = nullptr;         // chunk_count | chunk_base | qcount
    int mask_words = 0, q_chunks_cap = 0;
    bool cull_on = true;
    bool cull_cubes = false;              // tuning "cull_cubes": mark from the cells' whole cubes (rto_tree::d_occ_cubes), the rule before the bounds
    bool frame_via_batch = false;
    int last_n_queues = 0;                // of the last batched launch (rto_ctx_queue_stats)
    int64_t last_slots = 0;
    int batch_fallback = 0;               // tuning / test hook, see rto_ctx_set_tuning
    int lean = 0;                         // rto_ctx_set_lean_outputs: 0 full, 1 lean, 2 lean + sparse
    std::vector<uint8_t> lean_slot;       // per frame slot: the level of its last writer (1: no aux planes, noisy.a = alpha; 2: and
                                          // nothing stored for the pixels of unmarked tiles)
    int test_wide_bits = 0;               // test hook "wide_bits": pretend a hit entry has this many bits for an entry of the two-level image
    bool cull_single = false;             // tuning "cull_single": the single-frame kernel culls too.  Off by default: a LONE frame waits
                                          // for its longest rays (marked tiles), and the two extra launches cost it 14 us (0.375 ->
                                          // 0.389 ms); with several frames in flight the skipped work is throughput (+6 %)
    int marks_n = 0, marks_slot0 = 0;     // frames whose tile marks the last launch left in tile_mask (0: none), their first slot
    float marks_bg = 0.f;                 // ... and the background brightness of that launch
    // per-kernel event timing of the batched path (off by default)
    bool kt_on = false;
    std::vector<hipEvent_t> kt_ev;  // kKtRing quadruples
    int kt_count = 0;               // launches recorded since the last read
    float* aux = nullptr;
    float* noisy = nullptr;
    float* image = nullptr;
    // rto_ctx_set_layers (RenderContext::offscreen = false): borrowed device planes, one per frame slot; both null = offscreen
    const float* layer_depth = nullptr;  // [frames][H][W]
    const float* layer_color = nullptr;  // [frames][H][W][4]
    // rto_ctx_enable_depth: the depth outputs of the frame slots, [frames][H][W] each; both null = disabled
    float* depth = nullptr;
    float* t_near = nullptr;
    int depth_mode = 0;  // 0 disabled, 1 batches frame by frame, RTO_DEPTH_BATCHED batches through render_persist_depth
    float* probe_coeffs = nullptr;       // kProbeFloats: the probe point's leaf coefficients of the launch in flight (enable_probe)
    uint8_t* rgba8 = nullptr;
    rto::Pcg32 rng{};
    rto::PcgJumpEntry* jump = nullptr;
    uint64_t jump_inc = 0;
    bool jump_valid = false;
    int kernel = RTO_KERNEL_AUTO;
    int strip_rows = 1;
    int ray_order = RTO_RAY_ORDER_DEFAULT;  // tuning "ray_order" (rto_launch_rays): 0 = block b takes rays 256 b .., 1 = a contiguous range per XCD
    int refill = 0;  // 0 = the default instantiation; 100 * waves/SIMD + idle-lane threshold picks an A/B one
    bool tile_order_on = true;
    bool stats_on = false;
    bool stats_marks = false;             // rto_ctx_enable_stats(2): count against the tile marks of the last batched launch
    unsigned long long* stats = nullptr;  // device, rto::kStatsWords counters
    // Timer (render_context.hpp:122-213)
    hipStream_t t_stream = nullptr;
    hipEvent_t t_start[3] = {nullptr, nullptr, nullptr}, t_stop[3] = {nullptr, nullptr, nullptr};
    bool t_used[3] = {false, false, false};
    float t_sum[3] = {0, 0, 0};
    int t_cnt = 0;
};

#pragma GCC visibility push(hidden)
inline size_t frame_px(const rto_ctx* c) { return (size_t)c->width * c->height; }

constexpr int kMaxSpp = 32;  // the largest of the supported set below: a hit entry's slot field is narrowest there
inline bool spp_supported(int spp) {  // volrend.cu:266-278
    return spp == 1 || spp == 2 || spp == 3 || spp == 4 || spp == 6 || spp == 8 || spp == 16 || spp == 32;
}
// a hit-list entry packs {slot, count - 1}: at this SPP the tree's leaf slots must fit hit_slot_bits(spp) bits
// (strictly: the all-ones entry terminates a list)
inline bool slots_fit_spp(int64_t n_slots, int spp) { return n_slots < (int64_t(1) << rto::hit_slot_bits(spp)); }

// (mult, plus) of the affine map "advance by delta" for increment `inc` (pcg32.h:145-166)
inline rto::PcgJumpEntry pcg_jump(uint64_t inc, uint64_t delta) {
    uint64_t cur_mult = rto::kPcgMult, cur_plus = inc, acc_mult = 1u, acc_plus = 0u;
    while (delta > 0) {
        if (delta & 1) {
            acc_mult *= cur_mult;
            acc_plus = acc_plus * cur_mult + cur_plus;
        }
        cur_plus = (cur_mult + 1) * cur_plus;
        cur_mult *= cur_mult;
        delta /= 2;
    }
    return {acc_mult, acc_plus};
}

rto::OptDev make_opt_dev(const rto_options* o);  // (rto_abi.cpp) RenderOptions -> the fields the kernels read

inline rto::CamDev cam_dev(const rto_camera& cam) {
    rto::CamDev cd;
    cd.width = cam.width;
    cd.height = cam.height;
    cd.fx = cam.fx;
    cd.fy = cam.fy;
    std::memcpy(cd.transform, cam.transform, sizeof(cd.transform));
    return cd;
}

// ---- the host half of a layer pass (rto_layer_pass.h): rto_draw_grid_layers, rto_draw_mesh_layers ----
// The argument checks of every pass, in one order; none reads `handle`, whose own checks follow in the caller (then n == 0).
// fn: the message prefix; merge_name: the pass's merge flag (bit 0 of p->flags, the only one); own() -> nullptr or a message.
template <class Params, class Own>
int check_layer_call(const char* fn, const char* handle_noun, const char* merge_name, const void* handle, const rto_camera* cams, int n,
                     const Params* p, const float* depth, const float* color, Own own) {
    const std::string at = std::string(fn) + ": ";
    if (!handle || !cams || !p) return set_err(RTO_E_INVALID, at + "null " + handle_noun + ", cams or params");
    if (!depth && !color) return set_err(RTO_E_INVALID, at + "depth and color are both null");
    if (n < 0) return set_err(RTO_E_INVALID, at + "n must be >= 0");
    if (const char* msg = own()) return set_err(RTO_E_INVALID, at + msg);
    if (p->flags & ~1) return set_err(RTO_E_INVALID, at + "unknown flag");
    if ((p->flags & 1) && !depth) return set_err(RTO_E_INVALID, at + merge_name + " tests against the depth buffer, which is null");
    if ((uintptr_t)color % 16 != 0) return set_err(RTO_E_INVALID, at + "color must be 16-byte aligned");
    for (int f = 0; f < n; ++f) {
        const rto_camera& c = cams[f];
        if (c.width != cams[0].width || c.height != cams[0].height)
            return set_err(RTO_E_INVALID, at + "the cameras of one call share width and height");
        if (c.width <= 0 || c.height <= 0 || c.height > 65535 * 16 || !std::isfinite(c.fx) || !std::isfinite(c.fy) || c.fx == 0.f || c.fy == 0.f)
            return set_err(RTO_E_INVALID, at + "a camera's width, height (<= 1048560), fx or fy is out of range");
    }
    return RTO_OK;
}

// The launches of a checked call (n > 0): launch(target, cams, k) -> hipError_t for each chunk of k <= kLayerCamChunk cameras
// (the unused slots hold the chunk's first) and the planes of its first frame.  what: "grid" / "mesh", for the error message.
template <class Launch>
int launch_layer_chunks(const char* what, const rto_camera* cams, int n, int flags, float* depth, float* color, Launch launch) {
    rto::LayerTarget lt;
    lt.width = cams[0].width;
    lt.height = cams[0].height;
    lt.merge = flags & 1;
    const size_t px = (size_t)lt.width * lt.height;
    for (int f0 = 0; f0 < n; f0 += rto::kLayerCamChunk) {
        const int k = std::min(rto::kLayerCamChunk, n - f0);
        rto::LayerCams lc;
        for (int f = 0; f < rto::kLayerCamChunk; ++f) lc.c[f] = cam_dev(cams[f0 + (f < k ? f : 0)]);
        lt.depth = depth ? depth + (size_t)f0 * px : nullptr;
        lt.color = color ? reinterpret_cast<float4*>(color) + (size_t)f0 * px : nullptr;
        const hipError_t e = launch(lt, lc, k);
        if (e != hipSuccess) return set_err(RTO_E_HIP, std::string(what) + " launch failed: " + hipGetErrorString(e));
    }
    return RTO_OK;
}

// ---- rto_tree.cpp ----
// How the fast / batched kernels render `tree` at this SPP: 0 = not at all (generic kernel), 1 = with tree->dev as it is,
// 2 = with *td = tree->dev minus the two-level image (its entries do not fit a hit entry at this SPP, the leaf slots do:
// the one-level walk, whose hits name slots).  wide_bits > 0: test hook, pretend a hit entry leaves that many bits for an
// entry of the two-level image.
int fast_path_for_spp(const rto_tree* tree, int spp, int wide_bits, rto::TreeDev* td);
// child[] / data[] of a tree that dropped them at upload, back on the device for the generic kernel (same leaf values:
// tests/test_render_parity.py::test_generic_kernel_on_a_tree_without_reference_arrays)
int ensure_reference_arrays(const rto_tree* tree);
// an SG / ASG tree loaded without its lobes: the reference would read a null device pointer (data_spec.hpp:44)
bool missing_lobes(const rto_tree* tree);
extern const char* const missing_lobes_msg;
// How a point query walks `tree` (whatever image is resident) and where `values` are read (rto_launch.h).  Needs no device.
int query_plan(const rto_tree* tree, bool values, int* walk, rto::ValuesSrc* vs);

#pragma GCC visibility pop
