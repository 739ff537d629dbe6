// rto_launch.h -- host-callable launchers of the gfx950 kernels (defined in *.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"
#include "rto_layer_pass.h"

namespace rto {

// traversal image for N == 2 trees; *bad_flag (device int, pre-zeroed) is set if an offset cannot
// be encoded
hipError_t launch_build_nodew(const int32_t* child, const uint16_t* data, int64_t n_slots, int data_dim,
                              uint32_t* nodew, int* bad_flag, hipStream_t stream);

// aligned copy of the SH coefficients (TreeDev::shrec): `rec` halves per slot = shrec_halves(basis_dim)
hipError_t launch_build_shrec(const uint16_t* data, int64_t n_slots, int data_dim, int rec, const uint32_t* recidx, uint16_t* out,
                              hipStream_t stream);
// child[] / data[] (reference layout) rebuilt from the traversal image and the aligned coefficient copy
hipError_t launch_rebuild_reference(const uint16_t* shrec, const uint32_t* nodew, const uint32_t* recidx, int64_t n_slots, int data_dim,
                                    int rec, uint16_t* data, int32_t* child, hipStream_t stream);

// entry-ordered records (TreeDev::rec_by_entry): built from data[] through the tree's two-level image (tree.widew / wgslot /
// worig / nodew must be set), and data[]'s coefficients back from them (after launch_rebuild_reference with shrec = nullptr)
hipError_t launch_build_shrec_wide(const TreeDev& tree, const uint16_t* data, int64_t n_entries, int rec, uint16_t* out, hipStream_t stream);
hipError_t launch_rebuild_reference_wide(const TreeDev& tree, int64_t n_entries, int rec, uint16_t* data, hipStream_t stream);

// top-of-tree shortcut grid: 2^(3G) entries (TreeDev::topgrid)
hipError_t launch_build_topgrid(const uint32_t* nodew, int G, uint2* grid, hipStream_t stream);

TileMap make_tile_map(int width, int height, int strip_rows);

// kernel: 1 = generic, 2 = fast.  spp must be one of {1,2,3,4,6,8,16,32} (hipErrorInvalidValue otherwise)
// layers != nullptr (rto_ctx_set_layers; never with fo.stats): the layered kernels -- pixel (x, y) stops at layers->depth[y W + x]
// and is composited over layers->color[y W + x] (the caller has offset both to the frame's plane)
// depth != nullptr (rto_ctx_enable_depth; never with fo.stats): the depth-carrying layered kernels, over `layers` or none -- the
// same pixels, and pixel (x, y)'s depth / t_near at index y W + x of depth's planes (offset to the frame's by the caller)
hipError_t launch_render(int kernel, int spp, const TreeDev& tree, const CamDev& cam, const OptDev& opt,
                         const Pcg32& rng, const PcgJumpEntry* jump, const FrameOut& fo, int strip_rows, const LayerDev* layers,
                         const DepthOut* depth, hipStream_t stream);

// rto_launch_rays: the rb.n rays of rb (rb.n * spp < 2^32, else hipErrorInvalidValue) with the fast (2: render_rays) or the generic
// (1: render_rays_generic) kernel; ray i draws its samples from rng advanced by i * spp.  xcd_order: each XCD takes one contiguous
// range of the rays (RayBatch::per_xcd) instead of every eighth block of 256.  depth != nullptr (rto_launch_rays_ex with depth or
// t_near): render_rays_depth / render_rays_generic_depth, which also store ray i's depth / t_near at index i (either pointer may
// be nullptr, and rb.out may then be nullptr too: no colour is computed); nullptr: the kernels of rto_launch_rays
hipError_t launch_rays(int kernel, int spp, const TreeDev& tree, const OptDev& opt, const Pcg32& rng, const PcgJumpEntry* jump,
                       const RayBatch& rb, const DepthOut* depth, bool xcd_order, hipStream_t stream);

// tile marks of ONE frame for the single-frame kernel's culling (FrameOut::cull_marks): zeroes `mask` ((tiles + 31) / 32 + 1
// words) on the stream and projects the tree's culling cells into the camera
hipError_t launch_mark_tiles_one(const TreeDev& tree, const CamDev& cam, uint32_t* mask, int mask_words, hipStream_t stream);

// writes n frame descriptors (host memory, read before the call returns) into a device table on `stream`
hipError_t launch_write_frames(const FrameDesc* host, int n, FrameDesc* dev_table, hipStream_t stream);

// occupancy of the persistent kernel, cached per render context (which is per device and per thread): the
// answer depends on the instantiation and on its dynamic LDS size (deeper trees need more)
struct OccupancyCache {
    const void* fn = nullptr;
    size_t lds = 0;
    int blocks_per_cu = 0;
    int cap = 0;  // tuning ("blocks_per_cu"): launch at most this many workgroups per CU (0 = what fits)
    // out: the device refused the dynamic LDS this launch needs (hipFuncSetAttribute failed); NOTHING was launched and
    // launch_render_batch returned hipSuccess -- the caller renders the frames with the generic kernel instead
    bool lds_refused = false;
    bool force_lds_refusal = false;  // test hook
};

// persistent batched renderer (N == 2 trees): fb.n frames in one launch (traversal kernel, then the
// shading kernel); layers != nullptr (rto_ctx_set_layers): frame f stops at plane f of layers->depth and is composited over plane
// f of layers->color, by the layered kernels of the default tuning (the A/B part of `refill` is then ignored); `queue` = kQueueWords u64 (zeroed by queue_scan_kernel on the stream before every traversal launch); ev = nullptr or 4 events recorded before the thresholds kernel, before / after the traversal, after the shading
// depth != nullptr (rto_ctx_enable_depth(RTO_DEPTH_BATCHED)): the traversal is render_persist_depth (depth_kernels.hip; default tuning,
// over `layers` or none), which also stores pixel p of frame f's depth / t_near at index f * W * H + p of depth's planes; the
// launch first fills those fb.n planes with (0, +inf) on the stream, for the pixels whose ray has no hit
hipError_t launch_render_batch(int spp, const TreeDev& tree, const OptDev& opt, const FrameBatch& fb,
                               const PcgJumpEntry* jump, unsigned long long* queue, uint32_t* hits, int num_cus,
                               int refill, bool cull, OccupancyCache* occ, hipEvent_t* ev, const LayerDev* layers, const DepthOut* depth,
                               hipStream_t stream);

// quant_map [nq][ns] + data_retained [nr][ns][3] -> slot-major records of `rec` u16 (TreeDev::qrec)
hipError_t launch_pack_quant(const uint16_t* qmap, const uint16_t* retained, int64_t ns, int nr, int nq, int rec,
                             uint16_t* out, hipStream_t stream);

hipError_t launch_rgba8(const float* rgba, uint8_t* out, int64_t n_pixels, hipStream_t stream);

// rto_probe_basis: out[n][RTO_BASIS_MAX_DEV] = the basis of the view directions dirs[n][3] (device pointers) as the kernels
// compute it; path 0 the run-time ray_basis, 1 the per-B forms of the shading kernel (hipErrorInvalidValue where none exists)
hipError_t launch_probe_basis(const TreeDev& tree, const OptDev& opt, const float* dirs, int64_t n, int path, float* out, hipStream_t stream);

// ---- query_kernels.hip: rto_tree_query and the probe ----
// which structure a point's walk descends: child[] with the reference's float descent (a tree without traversal image), the
// one-level image (top grid + nodew), the two-level image
constexpr int kWalkChild = 0, kWalkNodew = 1, kWalkWide = 2;
// where the `values` of a leaf are read: half k of row r is src[r * stride + k], r = the leaf's entry of the two-level image
// (by_entry: TreeDev::rec_by_entry records) or its slot (slot-ordered records, data[]).  src == nullptr: no values asked for
struct ValuesSrc {
    const uint16_t* src;
    uint32_t stride;
    int by_entry;
};
struct QueryOut {  // rto_query_out
    float* values;
    float* sigma;
    int32_t* level;
    float* cube;
};
// n points [n][3] (device) -> out; one thread per point, 256 per workgroup
hipError_t launch_query(const TreeDev& tree, int walk, const ValuesSrc& vs, const float* points, int64_t n, const QueryOut& out,
                        hipStream_t stream);
// the probe point's leaf coefficients -> coeffs[0 .. min(data_dim - 1, cap) - 1] (retrieve_cursor_lumisphere_kernel)
hipError_t launch_probe_fetch(const TreeDev& tree, int walk, const ValuesSrc& vs, const float point[3], float* coeffs, int cap,
                              hipStream_t stream);
// The probe's disc drawn over `frames` frames a launch wrote: frame f = table[f] (device memory), or the one descriptor `one`
// (table == nullptr, frames = 1); only transform, aux and image of a descriptor are read.  lean: no aux planes.
struct ProbeDraw {
    int width, height;
    int disp;  // options.probe_disp_size (> 0)
    int lean;
    int x0, y1;  // (set by the launcher: the probe's square clipped to the image is x >= x0, y < y1)
    const FrameDesc* table;
    FrameDesc one;
};
hipError_t launch_probe_overlay(const TreeDev& tree, const OptDev& opt, ProbeDraw pd, int frames, const float* coeffs, hipStream_t stream);

// ---- grid_kernels.hip: rto_draw_grid_layers, a layer pass (rto_layer_pass.h) ----
struct GridDraw {
    LayerTarget target;
    int max_depth;  // cells: the leaves cut off at level max_depth + 1 (<= 22)
    float line_px;
    float color_rgb[3];
    float background;
};
// frames <= kLayerCamChunk; walk: as launch_query's (kWalkChild needs tree.child)
hipError_t launch_grid_layers(const TreeDev& tree, int walk, const GridDraw& gd, const LayerCams& cams, int frames, hipStream_t stream);

#ifdef RTO_DBG_COUNTERS
hipError_t debug_shade_phases(unsigned long long* out16, bool reset);  // tools/dbg_shade_phases.py
#endif
}  // namespace rto
