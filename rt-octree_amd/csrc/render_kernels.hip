// render_kernels.hip -- batched-regular-tracking octree renderer for gfx950 (MI355X).
//
// What the reference computes (relative to /root/reference):
//   render_kernel<SPP>      renderer/src/cuda/volrend.cu:84-213   pixel -> ray, RNG jump, trace, bg
//                                                                  composite, aux + image writes
//   trace_ray<float,SPP>    renderer/include/volrend/cuda/rt_core.cuh:195-332
//   query_single_from_root  renderer/include/volrend/internal/n3tree_query.hpp:13-48
//   maybe_precalc_basis     renderer/include/volrend/internal/lumisphere.hpp:38-80 (SH)
//   sample_dst<SPP>         rt_core.cuh:67-193
//
// Three traversal kernels with bit-identical results (tests/test_render_parity.py):
//   render_generic<SPP>  any N, root-restart float descent -- the plain statement of the algorithm.
//   render_fast<SPP>     N == 2, one frame per launch (the latency path): integer descent over a
//                        4-byte-per-slot traversal image (child offset or leaf sigma in one word),
//                        restart from the deepest ancestor shared with the previous step (per-lane
//                        ancestor stack in LDS), 8x8-pixel wave tiles in an XCD-interleaved strip
//                        order, register-resident thresholds/hit lists with static indexing only,
//                        table-driven RNG jump.
//   render_persist<SPP>  N == 2, up to 128 frames per launch (the throughput path): persistent waves,
//                        ray compaction, one ray queue per XCD; sample_kernel before it (thresholds)
//                        and shade_kernel after it (SH colour + pixel epilogue).
// Since round 4 render_fast and render_persist walk the TWO-LEVEL traversal image when the tree has one
// (TreeDev::widew, host/tree_layout.cpp build_wide_image): top-grid cells and nodes merged with their eight children in
// ONE array, so that a node visit is one uniform 4-byte load resolving two levels; a ray's hit entries name
// entries of that image, wait in LDS while it marches and are translated to leaf slots and written once, when
// it has ended (flush_hits).  The one-level image (nodew + topgrid) serves the counting instantiation and trees
// whose two-level image would not fit; both give the same pixels.
//
// Why the descent can be done on integers (SURVEY.md section 7 "hard parts"): after the clamp to
// [0, 1-1e-6] every operation of the reference descent (x*=2; floor; x-=floor) is exact in fp32,
// so the child digit at level l is bit (23-l) of floor(pos*2^24) and the leaf-local coordinate is
// frac(pos * 2^(l+1)) exactly.
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"
#include "rto_tree_device.h"

#pragma clang fp contract(off)

// ray set-up, pixel / ray outputs, tiles, hit entries, packed shading, RTO_FAST_WPS: shared with depth_kernels.hip
#include "rto_render_shared.h"
#include "rto_depth_launch.h"  // the launchers of depth_kernels.hip, which launch_render / launch_rays forward to

namespace rto {

// ------------------------------------------------------------------ generic kernel (any N)

template <int SPP>
__global__ void __launch_bounds__(256) render_generic(const TreeDev tree, const CamDev cam, const OptDev opt,
                                                       const Pcg32 rng_base, const FrameOut fo) {
#include "rto_render_generic.inc"
}

// rto_launch_rays on any tree the fast kernel does not take (N != 2, hit entries too wide) and RTO_KERNEL_GENERIC
template <int SPP>
__global__ void __launch_bounds__(256) render_rays_generic(const TreeDev tree, const OptDev opt, const Pcg32 rng_base,
                                                            const RayBatch rays) {
#define RTO_GENERIC_RAYS 1
#include "rto_render_generic.inc"
#undef RTO_GENERIC_RAYS
}

// rto_launch_renderer over the context's layers (rto_ctx_set_layers) on any tree the fast kernel does not take and RTO_KERNEL_GENERIC
template <int SPP>
__global__ void __launch_bounds__(256) render_generic_layers(const TreeDev tree, const CamDev cam, const OptDev opt, const Pcg32 rng_base,
                                                              const FrameOut fo, const LayerDev layers) {
#define RTO_GENERIC_LAYERS 1
#include "rto_render_generic.inc"
#undef RTO_GENERIC_LAYERS
}

// ------------------------------------------------------------------ traversal image

// One word per child slot: internal -> child[] value, leaf -> kLeafTag | sigma fp16 bits.
// Derived data (like the reference's commented-out occupancy LUT, n3tree.cpp:206-225): it only
// re-packs what child[]/data[] already say, so traversal decisions cannot change.
__global__ void build_nodew_kernel(const int32_t* __restrict__ child, const uint16_t* __restrict__ data,
                                   int64_t n_slots, int data_dim, uint32_t* __restrict__ nodew,
                                   int* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots) return;
    const int32_t c = child[i];
    if (c == 0) {
        nodew[i] = kLeafTag | (uint32_t)data[i * data_dim + data_dim - 1];
    } else {
        if (nodew_is_leaf((uint32_t)c)) atomicExch(bad, 1);  // |offset| >= 2^30: not encodable
        nodew[i] = (uint32_t)c;
    }
}

// Aligned copy of the SH coefficients for the shading kernels (TreeDev::shrec): per slot the 3 B coefficients of
// data[] in the same order, zero-padded to shrec_halves(B).  Derived data: the same fp16 values.
__global__ void build_shrec_kernel(const uint16_t* __restrict__ data, int64_t n_slots, int data_dim, int rec,
                                   const uint32_t* __restrict__ recidx, uint16_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // one thread per half of a slot's record
    if (i >= n_slots * rec) return;
    const int64_t slot = i / rec;
    const int k = (int)(i - slot * rec);
    int64_t dst = slot;
    if (recidx) {  // compact records (RTO_TREE_COMPACT_RECORDS): only the slots that own one
        const uint32_t r = recidx[slot];
        if (r == kNoRecord) return;
        dst = r;
    }
    out[dst * rec + k] = k < data_dim - 1 ? data[slot * data_dim + k] : (uint16_t)0;
}

// The reference-layout arrays back from the derived ones (rto_tree.cpp ensure_reference_arrays): a tree that renders through
// the fast / batched kernels keeps only nodew + shrec resident; the generic kernel's child[] / data[] are rebuilt on
// first use.  Leaf slots get their exact fp16 values back (coefficients from shrec, sigma from the leaf word); an
// internal slot's sigma -- which no query ever returns -- becomes 0.
__global__ void rebuild_reference_kernel(const uint16_t* __restrict__ shrec, const uint32_t* __restrict__ nodew,
                                         const uint32_t* __restrict__ recidx, int64_t n_slots, int data_dim, int rec,
                                         uint16_t* __restrict__ data, int32_t* __restrict__ child) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // one thread per half of data[]
    if (i >= n_slots * data_dim) return;
    const int64_t slot = i / data_dim;
    const int k = (int)(i - slot * data_dim);
    const uint32_t w = nodew[slot];
    const bool leaf = nodew_is_leaf(w);
    int64_t src = slot;
    bool has = true;
    if (recidx) {  // compact records: a slot without one (internal, or a leaf of zero density) reads as zeros
        const uint32_t r = recidx[slot];
        has = r != kNoRecord;
        src = r;
    }
    // (shrec == nullptr: entry-ordered records -- rebuild_reference_wide_kernel fills the coefficients in afterwards)
    data[i] = k < data_dim - 1 ? (has && shrec ? shrec[src * rec + k] : (uint16_t)0) : (leaf ? (uint16_t)(w & 0xffffu) : (uint16_t)0);
    if (k == 0) child[slot] = leaf ? 0 : (int32_t)w;
}

// Top-of-tree shortcut (TreeDev::topgrid): one thread per cell of the 2^G-per-axis grid walks its
// root path over node levels 0..G-1 and records where it ends: {slot | level << kGridSlotBits, nodew[slot]}.
__global__ void build_topgrid_kernel(const uint32_t* __restrict__ nodew, int G, uint2* __restrict__ grid) {
    const uint32_t key = blockIdx.x * blockDim.x + threadIdx.x;
    if (key >= (1u << (3 * G))) return;
    const uint32_t mask = (1u << G) - 1u;
    const uint32_t cx = key >> (2 * G), cy = (key >> G) & mask, cz = key & mask;
    uint32_t node = 0, slot = 0, w = 0;
    int lvl = 0;
    for (;;) {
        const int sh = G - 1 - lvl;
        const uint32_t ci = (((cx >> sh) & 1u) << 2) | (((cy >> sh) & 1u) << 1) | ((cz >> sh) & 1u);
        slot = node * 8u + ci;
        w = nodew[slot];
        if (nodew_is_leaf(w) || lvl == G - 1) break;
        node += w;
        ++lvl;
    }
    grid[key] = make_uint2(slot | ((uint32_t)lvl << kGridSlotBits), w);
}

// ------------------------------------------------------------------ fast kernel (N == 2)

// the aligned coefficient records in the order of the two-level image's entries (TreeDev::rec_by_entry): record e = the 3 B
// coefficients of the leaf that entry e of widew names, zero-padded to `rec` halves; entries that are internal nodes (or
// padding) keep zeros.  One thread per half.  Derived data: the same fp16 values.
__global__ void build_shrec_wide_kernel(const TreeDev tree, const uint16_t* __restrict__ data, int64_t n_entries, int rec,
                                        uint16_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_entries * rec) return;
    const uint32_t e = (uint32_t)(i / rec);
    const int k = (int)(i - (int64_t)e * rec);
    uint16_t v = 0;
    if (nodew_is_leaf(tree.widew[e]) && k < tree.data_dim - 1) {
        const uint32_t pad = tree.wide_grid_nodes * 64u, cells = 1u << (3 * tree.top_levels);
        if (e >= pad || e < cells) v = data[(uint64_t)wide_to_slot(tree, e) * tree.data_dim + k];
    }
    out[i] = v;
}

// ... and back: the coefficients of data[] from entry-ordered records (rebuild_reference_kernel wrote child[], sigma and
// zeros before).  A first-level leaf's 8 entries write the same values to the same place.
__global__ void rebuild_reference_wide_kernel(const TreeDev tree, int64_t n_entries, int rec, uint16_t* __restrict__ data) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_entries * rec) return;
    const uint32_t e = (uint32_t)(i / rec);
    const int k = (int)(i - (int64_t)e * rec);
    if (k >= tree.data_dim - 1 || !nodew_is_leaf(tree.widew[e])) return;
    const uint32_t pad = tree.wide_grid_nodes * 64u, cells = 1u << (3 * tree.top_levels);
    if (e < pad && e >= cells) return;  // padding behind the grid cells
    data[(uint64_t)wide_to_slot(tree, e) * tree.data_dim + k] = tree.shrec[(uint64_t)e * rec + k];
}

// STATS: also count the units of SURVEY 8(d)'s algorithmic-byte formula (march steps, descent
// levels a root-restart walk would visit, distinct hit leaves, ...) into fo.stats.  Separate
// instantiation; the timed kernel carries none of it.
// STACK == 1 (two-level image, at most two pairs of levels below the grid; the launcher decides): the restart of render_persist's
// register-stack form -- the node a step starts from is chosen by where the ray is and which coordinate bits changed
// (rto_march_leaf.inc), positions are kept scaled by 2^24 (kPos24), the step's power-of-two factors come from the level bits of
// the leaf word -- seven dependent instructions fewer on the chain a lone frame's longest rays wait for
// The body (rto_render_fast.inc) serves two kernels: render_fast for SH and RGBA trees and render_fast_lobes for SG / ASG trees
// (LOBES = kFmtSG / kFmtASG, see ray_basis), so that the SH kernels keep their names and their code.
template <int SPP, bool STATS, bool WIDE, int STACK = 0>
__global__ void __launch_bounds__(256, SPP <= 8 ? RTO_FAST_WPS : 4) render_fast(const TreeDev tree, const CamDev cam, const OptDev opt,
                                                    const Pcg32 rng_base, const PcgJumpEntry* __restrict__ jump,
                                                    const TileMap tm, const FrameOut fo) {
    constexpr int LOBES = 0;
#include "rto_render_fast.inc"
}

// the single-frame kernel of an SG / ASG tree (LOBES = kFmtSG / kFmtASG): the same body under its own name
template <int SPP, bool STATS, bool WIDE, int STACK, int LOBES>
__global__ void __launch_bounds__(256, SPP <= 8 ? RTO_FAST_WPS : 4) render_fast_lobes(const TreeDev tree, const CamDev cam, const OptDev opt,
                                                          const Pcg32 rng_base, const PcgJumpEntry* __restrict__ jump,
                                                          const TileMap tm, const FrameOut fo) {
#include "rto_render_fast.inc"
}

// rto_launch_rays on an N == 2 tree: the same body with the rays of the batch for the camera's pixels -- one thread per ray, no
// tile map and no culling marks (both are per camera tile), each ray's own depth limit and backdrop, a float4 per ray
template <int SPP, bool WIDE, int STACK, int LOBES>
__global__ void __launch_bounds__(256, SPP <= 8 ? RTO_FAST_WPS : 4) render_rays(const TreeDev tree, const OptDev opt, const Pcg32 rng_base,
                                                    const PcgJumpEntry* __restrict__ jump, const RayBatch rays) {
    constexpr bool STATS = false;
#define RTO_FAST_RAYS 1
#include "rto_render_fast.inc"
#undef RTO_FAST_RAYS
}

// rto_launch_renderer over the context's layers (rto_ctx_set_layers) on an N == 2 tree: the same body, each pixel's ray stopped at
// its depth and composited over its colour; the tiles culled by fo.cull_marks get their backdrop.  No counting instantiation
// (layers and rto_ctx_enable_stats are refused together).
template <int SPP, bool WIDE, int STACK, int LOBES>
__global__ void __launch_bounds__(256, SPP <= 8 ? RTO_FAST_WPS : 4) render_fast_layers(const TreeDev tree, const CamDev cam, const OptDev opt,
                                                           const Pcg32 rng_base, const PcgJumpEntry* __restrict__ jump,
                                                           const TileMap tm, const FrameOut fo, const LayerDev layers) {
    constexpr bool STATS = false;
#define RTO_FAST_LAYERS 1
#include "rto_render_fast.inc"
#undef RTO_FAST_LAYERS
}

// ------------------------------------------------------------------ persistent kernel (N == 2)
//
// render_persist: the throughput form of render_fast.  One launch renders a BATCH of frames
// (independent poses of the same tree): a frame is only ~10 k waves of very uneven length, so a
// one-frame launch spends most of its time waiting for its longest rays on a nearly empty chip
// (profiles/r1_a_*: mean residency 1.7 k of 8 k wave slots).  Here a fixed grid of persistent
// waves pulls rays from queues that span every frame of the batch:
//   * ray compaction: a lane whose ray ended (all SPP thresholds crossed, left the box, missed)
//     idles only until the wave has REFILL such lanes; then a ballot / mbcnt prefix sum hands each
//     idle lane the next ray of the wave's reservoir (one atomicAdd per 64-256 rays);
//   * rays are queued in 8x8-pixel tile order, so a wave's 64 rays stay spatially coherent; one
//     queue per XCD over interleaved bands of tile rows (rounds 3-5: an angular image wedge each), tile-major across the frames (FrameBatch::qstart);
//   * the end-of-queue drain happens once per batch instead of once per frame.
// Per-ray arithmetic is exactly render_fast's; results are bit-identical.

// (RayState, kGridNext, kCamFloats: rto_render_shared.h -- depth_kernels.hip's render_persist_depth is the same body)

// ------------------------------------------------------------------ empty-space culling + ray queues (round 3)
// A ray that never meets a leaf of positive density composites nothing: its pixel is the background, its hit list empty
// (rt_core.cuh:252-262 only ever accumulates in leaves with sigma > sigma_thresh).  73 % of the bench scene's rays are such
// rays and a third of all march steps are theirs.  mark_tiles_kernel decides it per 8x8-pixel tile, conservatively and
// without marching: every culling cell of the tree (TreeDev::occ_cells: the cubes that hold the leaves of positive density,
// as world-space boxes padded far above the float error of a sample point) is projected into every frame of the batch; the
// tiles its projection can touch are marked.  An unmarked tile holds no ray that passes through a box, hence no ray that
// visits a dense leaf: its rays are never queued, its pixels get no threshold draws.
// The ball bound (rounds 3-6 applied it to the box's bounding sphere): with a ball's centre at camera coordinates (a, b, -d),
// d > 2 r, every point of the ball lands within f r / (d - r) (1 + |a| / d) pixels of the centre's pixel along x (same with b
// along y) -- from |a'/d' - a/d| <= (r d + |a| r) / (d (d - r)).
// The box rule: a box whose 8 corners all lie in front of the camera is convex and in front of it, so its projection lies
// in the hull of the projected corners, hence in their bounding rectangle; the tiles of that rectangle are marked.  The
// corners are centre +- hw[i] e_i through the same Cramer inverse (M need not be orthonormal, nor the tree's scale isotropic).
// Two pads:
//   * relative: a corner is taken as a ball of radius e = 1e-5 (|p|_1 |M^-1|_F + r) around its computed position and the ball
//     bound widens the rectangle by it.  The float error of p, of Cramer's sums and of the corner offsets is a few ulp of
//     those magnitudes (~1e-6 of them for a camera matrix that is not close to singular); e is 10 times that.  The
//     rectangle is used only while every corner's depth exceeds 100 e (the ball bound needs > 2 e; the rest keeps 1 / depth tame).
//   * absolute, 1.5 pixels, as before: the ray of pixel x leaves through image-plane point (x - W / 2) / fx exactly, so the
//     pad is pure slack for the float error of the pixel coordinates here (0.5 W + fx x: ~1e-4 pixel) and of the ray's own
//     direction (ray_setup: the same size).
// A box with a corner nearer than that marks the whole frame; one with every corner behind the camera nothing.
// The sphere rule stays as an upper clamp: where it yields a rectangle the tiles are the intersection of the two (each is a
// bound by itself, and a box lies inside its bounding sphere: in exact arithmetic the box rectangle is the smaller one
// already -- |M^-1|_F alone overstates an orthonormal camera's sphere by sqrt 3), where it marks nothing so does this, so
// the marks are a subset of rounds 3-6's for every cell and camera whatever the rounding.  (Pixels are bit-identical with
// and without: tests/test_culling.py, tests/test_culling_cubes.py, and every parity test against the oracle, which marches
// every ray, runs with it.)
// One workgroup = kMarkCells cells of one frame, marked into a private copy of the frame's mask in LDS (LDS_MASK; a frame
// of more than kMarkLdsWords * 32 tiles marks straight into memory) that is OR-ed into the frame's mask once at the end:
// tens of thousands of cells land on a few hundred mask words, and device-scope atomics on one address serialise
// (the first version, one global atomic per cell and tile, took 2.5 ms per 100 frames; this one 0.1).
constexpr int kMarkCells = 2048, kMarkLdsWords = 8192;
template <class MarkFn>
RTO_DEV void mark_cell(const float4 cell, const TreeDev& tree, const FrameDesc& fd, const FrameBatch& fb, MarkFn mark);
template <bool LDS_MASK>
__global__ void __launch_bounds__(256) mark_tiles_kernel(const TreeDev tree, const FrameBatch fb, uint32_t* __restrict__ mask) {
    extern __shared__ uint32_t s_mask[];
    const FrameDesc& fd = fb.f[blockIdx.y];
    uint32_t* const gm = mask + (size_t)blockIdx.y * fb.mask_words;
    if (LDS_MASK) {
        for (int i = threadIdx.x; i < fb.mask_words; i += 256) s_mask[i] = 0u;
        __syncthreads();
    }
    // (round 6: a thread takes a RUN of kMarkCells / 256 consecutive cells, not every 256th: the cells come in Morton order, so the
    //  64 lanes of a wave then mark 64 different neighbourhoods instead of one -- their ds_or_b32 land on different words instead
    //  of serialising on a few: 0.104 -> 0.07 ms per 100 C2 frames, profiles/r6_zz_ab_mark_cells.txt)
    static_assert(kMarkCells % 256 == 0, "a run per thread");
    for (int i = 0; i < kMarkCells / 256; ++i) {
        const int c = (int)blockIdx.x * kMarkCells + (int)threadIdx.x * (kMarkCells / 256) + i;
        if (c >= tree.n_occ_cells) break;
        if (LDS_MASK)
            mark_cell(tree.occ_cells[c], tree, fd, fb, [&](uint32_t w, uint32_t bits) { atomicOr(&s_mask[w], bits); });  // ds_or_b32
        else
            mark_cell(tree.occ_cells[c], tree, fd, fb, [&](uint32_t w, uint32_t bits) { atomicOr(gm + w, bits); });
    }
    if (LDS_MASK) {
        __syncthreads();
        for (int i = threadIdx.x; i < fb.mask_words; i += 256)
            if (s_mask[i]) atomicOr(gm + i, s_mask[i]);
    }
}

template <class MarkFn>
RTO_DEV void mark_cell(const float4 cell, const TreeDev& tree, const FrameDesc& fd, const FrameBatch& fb, MarkFn mark) {
    {
    const float* m = fd.transform;  // columns 0..2: camera axes, column 3: centre (common.cuh:29-44)
    const float p[3] = {cell.x - m[9], cell.y - m[10], cell.z - m[11]};
    // camera coordinates (a, b, cc) of the cell centre: M (a, b, cc)^T = p (Cramer; M need not be orthonormal)
    const float c12[3] = {m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6]};
    const float c20[3] = {m[7] * m[2] - m[8] * m[1], m[8] * m[0] - m[6] * m[2], m[6] * m[1] - m[7] * m[0]};
    const float c01[3] = {m[1] * m[5] - m[2] * m[4], m[2] * m[3] - m[0] * m[5], m[0] * m[4] - m[1] * m[3]};
    const float det = m[0] * c12[0] + m[1] * c12[1] + m[2] * c12[2];
    const float inv = 1.f / det;
    const float a = (p[0] * c12[0] + p[1] * c12[1] + p[2] * c12[2]) * inv;
    const float b = (p[0] * c20[0] + p[1] * c20[1] + p[2] * c20[2]) * inv;
    const float d = -(p[0] * c01[0] + p[1] * c01[1] + p[2] * c01[2]) * inv;  // depth along the viewing direction (0, 0, -1)
    // |M^-1| <= its Frobenius norm: the sphere's radius in camera coordinates
    const float frob = sqrtf(c12[0] * c12[0] + c12[1] * c12[1] + c12[2] * c12[2] + c20[0] * c20[0] + c20[1] * c20[1] + c20[2] * c20[2] +
                             c01[0] * c01[0] + c01[1] * c01[1] + c01[2] * c01[2]) * fabsf(inv);
    // world half-widths of the box, and the radius of its bounding sphere (0.1 % above the half diagonal)
    const float hw[3] = {cell.w / fabsf(tree.scale[0]), cell.w / fabsf(tree.scale[1]), cell.w / fabsf(tree.scale[2])};
    const float r = sqrtf(hw[0] * hw[0] + hw[1] * hw[1] + hw[2] * hw[2]) * 1.001f * frob * 1.0001f;
    if (d <= -r) return;    // wholly behind the camera (a NaN pose falls through to "keep everything")
    const float fx = fabsf(fd.fx), fy = fabsf(fd.fy);
    // ---- the sphere rule (rounds 3-6): a rectangle while d > 2 r, else every tile.  Kept as an upper clamp of the box rule.
    const bool sphere = d > 2.f * r;
    float x0f = 0.f, x1f = 0.f, y0f = 0.f, y1f = 0.f;
    if (sphere) {
        const float xs = a / d, ys = b / d;
        const float k = r / (d - r);
        const float pxc = 0.5f * fb.width + fd.fx * xs, pyc = 0.5f * fb.height - fd.fy * ys;  // volrend.cu:139-141 inverted
        const float rx = fx * k * (1.f + fabsf(xs)) + 1.5f, ry = fy * k * (1.f + fabsf(ys)) + 1.5f;
        x0f = floorf((pxc - rx) * 0.125f), x1f = floorf((pxc + rx) * 0.125f);
        y0f = floorf((pyc - ry) * 0.125f), y1f = floorf((pyc + ry) * 0.125f);
    }
    // ---- the box rule: the 8 corners centre +- hw[i] e_i in camera coordinates, each taken as a ball of radius e
    const float ua[3] = {hw[0] * c12[0] * inv, hw[1] * c12[1] * inv, hw[2] * c12[2] * inv};   // M^-1 (hw[i] e_i): its a,
    const float ub[3] = {hw[0] * c20[0] * inv, hw[1] * c20[1] * inv, hw[2] * c20[2] * inv};   // b
    const float ud[3] = {-hw[0] * c01[0] * inv, -hw[1] * c01[1] * inv, -hw[2] * c01[2] * inv};  // and depth component
    const float e = 1e-5f * ((fabsf(p[0]) + fabsf(p[1]) + fabsf(p[2])) * frob + r);
    const float dmin = 100.f * e;
    bool front = true, behind = true;
    float xlo = 3e38f, xhi = -3e38f, ylo = 3e38f, yhi = -3e38f;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const float sx = (s & 4) ? 1.f : -1.f, sy = (s & 2) ? 1.f : -1.f, sz = (s & 1) ? 1.f : -1.f;
        const float A = a + sx * ua[0] + sy * ua[1] + sz * ua[2];
        const float B = b + sx * ub[0] + sy * ub[1] + sz * ub[2];
        const float D = d + sx * ud[0] + sy * ud[1] + sz * ud[2];
        const float x = A / D, y = B / D, k = e / (D - e);
        const float kx = k * (1.f + fabsf(x)), ky = k * (1.f + fabsf(y));
        front = front && D > dmin && fabsf(x) + fabsf(y) < 3e38f;  // (false for a NaN anywhere)
        behind = behind && D < -e;
        xlo = fminf(xlo, x - kx), xhi = fmaxf(xhi, x + kx);
        ylo = fminf(ylo, y - ky), yhi = fmaxf(yhi, y + ky);
    }
    if (behind) return;  // every corner behind the camera: so is the box
    const float px0 = 0.5f * fb.width + fd.fx * xlo, px1 = 0.5f * fb.width + fd.fx * xhi;    // (fx, fy may be negative)
    const float py0 = 0.5f * fb.height - fd.fy * ylo, py1 = 0.5f * fb.height - fd.fy * yhi;
    const bool box = front && fabsf(px0) + fabsf(px1) + fabsf(py0) + fabsf(py1) < 3e38f;
    if (!box && !sphere) {  // a corner too close to the camera plane (or a NaN pose): keep every tile of this frame
        mark((uint32_t)fb.mask_words - 1u, 1u);
        return;
    }
    if (box) {
        const float bx0 = floorf((fminf(px0, px1) - 1.5f) * 0.125f), bx1 = floorf((fmaxf(px0, px1) + 1.5f) * 0.125f);
        const float by0 = floorf((fminf(py0, py1) - 1.5f) * 0.125f), by1 = floorf((fmaxf(py0, py1) + 1.5f) * 0.125f);
        // with both rules in hand the tiles are the intersection of the two rectangles (each alone is a valid bound)
        x0f = sphere ? fmaxf(x0f, bx0) : bx0, x1f = sphere ? fminf(x1f, bx1) : bx1;
        y0f = sphere ? fmaxf(y0f, by0) : by0, y1f = sphere ? fminf(y1f, by1) : by1;
    }
    const int tiles_x = (fb.width + 7) >> 3, tiles_y = (fb.height + 7) >> 3;
    if (!(x1f >= 0.f && y1f >= 0.f && x0f < (float)tiles_x && y0f < (float)tiles_y)) {
        if (!(x0f == x0f && y0f == y0f)) mark((uint32_t)fb.mask_words - 1u, 1u);  // NaN: keep everything
        return;
    }
    const int x0 = x0f < 0.f ? 0 : (int)x0f, x1 = x1f >= (float)tiles_x ? tiles_x - 1 : (int)x1f;
    const int y0 = y0f < 0.f ? 0 : (int)y0f, y1 = y1f >= (float)tiles_y ? tiles_y - 1 : (int)y1f;
    for (int ty = y0; ty <= y1; ++ty)
        for (int tx = x0; tx <= x1; ++tx) {
            const uint32_t t = (uint32_t)(ty * tiles_x + tx);
            mark(t >> 5, 1u << (t & 31u));
        }
    }
}

// the same for ONE frame whose camera arrives as a kernel argument (rto_launch_renderer: no frame table): one workgroup =
// kMarkCells cells, marks OR-ed into `mask` (zeroed on the stream before)
__global__ void __launch_bounds__(256) mark_tiles_one_kernel(const TreeDev tree, const FrameDesc fd, const int width, const int height,
                                                             const int mask_words, uint32_t* __restrict__ mask) {
    extern __shared__ uint32_t s_mask[];
    FrameBatch fb;
    fb.width = width;
    fb.height = height;
    fb.mask_words = mask_words;
    const bool lds = mask_words <= kMarkLdsWords;
    if (lds) {
        for (int i = threadIdx.x; i < mask_words; i += 256) s_mask[i] = 0u;
        __syncthreads();
    }
    for (int i = 0; i < kMarkCells / 256; ++i) {  // (runs of consecutive cells per thread, as in mark_tiles_kernel)
        const int c = (int)blockIdx.x * kMarkCells + (int)threadIdx.x * (kMarkCells / 256) + i;
        if (c >= tree.n_occ_cells) break;
        if (lds)
            mark_cell(tree.occ_cells[c], tree, fd, fb, [&](uint32_t w, uint32_t bits) { atomicOr(&s_mask[w], bits); });
        else
            mark_cell(tree.occ_cells[c], tree, fd, fb, [&](uint32_t w, uint32_t bits) { atomicOr(mask + w, bits); });
    }
    if (lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < mask_words; i += 256)
            if (s_mask[i]) atomicOr(mask + i, s_mask[i]);
    }
}

RTO_DEV bool tile_marked(const FrameBatch& fb, int frame, uint32_t tile_index) {
    const uint32_t* fm = fb.tile_mask + (size_t)frame * fb.mask_words;
    return ((fm[tile_index >> 5] >> (tile_index & 31u)) | fm[fb.mask_words - 1]) & 1u;
}

// Tile slot `pt` of queue k -> is it live, and its list entry {frame << 20 | ty << 10 | tx}.  The queue order: the tiles
// tile_order[qstart[k] .. qstart[k+1]) (ty << 16 | tx; row-major tiles without a table), tile after tile -- the same tile of
// every frame of the batch in turn (neighbouring poses see nearly the same rays through a tile) -- or frame after frame.
RTO_DEV bool queue_slot(const FrameBatch& fb, int k, uint32_t pt, uint32_t& entry) {
    const uint32_t qt0 = (uint32_t)fb.qstart[k], qtiles = (uint32_t)fb.qstart[k + 1] - qt0, n = (uint32_t)fb.n;
    if (pt >= qtiles * n) return false;
    uint32_t tile, frame;
    if (fb.tile_major) {
        const uint32_t t = pt / n;
        frame = pt - t * n;
        tile = qt0 + t;
    } else {
        frame = pt / qtiles;
        tile = qt0 + (pt - frame * qtiles);
    }
    const uint32_t tiles_x = (uint32_t)(fb.width + 7) >> 3;
    uint32_t tx, ty;
    if (fb.tile_order) {
        const uint32_t code = fb.tile_order[tile];
        ty = code >> 16;
        tx = code & 0xffffu;
    } else {
        ty = tile / tiles_x;
        tx = tile - ty * tiles_x;
    }
    entry = frame << 20 | ty << 10 | tx;
    return tile_marked(fb, (int)frame, ty * tiles_x + tx);
}

// queue k of a compaction chunk (the chunks of a queue are consecutive: fb.qchunk)
RTO_DEV int chunk_queue(const FrameBatch& fb, uint32_t chunk) {
    int k = 0;
    while (k + 1 < fb.n_queues && chunk >= (uint32_t)fb.qchunk[k + 1]) ++k;
    return k;
}

__global__ void __launch_bounds__(kQueueChunk) queue_count_kernel(const FrameBatch fb) {
    __shared__ uint32_t s_w[kQueueChunk / 64];
    const int k = chunk_queue(fb, blockIdx.x);
    uint32_t entry;
    const bool live = queue_slot(fb, k, (blockIdx.x - (uint32_t)fb.qchunk[k]) * kQueueChunk + threadIdx.x, entry);
    const unsigned long long m = __builtin_amdgcn_ballot_w64(live);
    if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kQueueChunk / 64; ++w) t += s_w[w];
        fb.chunk_count[blockIdx.x] = t;
    }
}

// exclusive scan of the chunk counts (a few thousand chunks): one WAVE per queue, lane shuffles, no barrier (round 6: the
// one-workgroup Hillis-Steele scan, queue after queue, was ~320 barrier rounds = 22 us on the launch chain in front of the
// traversal).  The kernel also arms the ray queues (kQueueWords u64: a launch never depends on how the previous one on its
// context ended) -- one fill launch less on that chain.
static_assert(kQueueWords <= 64 * kMaxQueues, "queue words zeroed by the scan's threads");
__global__ void __launch_bounds__(64 * kMaxQueues) queue_scan_kernel(const FrameBatch fb, unsigned long long* __restrict__ queue) {
    if (threadIdx.x < (unsigned)kQueueWords) queue[threadIdx.x] = 0ULL;
    const int k = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    if (k >= fb.n_queues) return;
    const int c1 = fb.qchunk[k + 1];
    uint32_t carry = 0;
    for (int c0 = fb.qchunk[k]; c0 < c1; c0 += 64) {
        const int c = c0 + lane;
        const uint32_t v = c < c1 ? fb.chunk_count[c] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (c < c1) fb.chunk_base[c] = carry + incl - v;
        carry += (uint32_t)__shfl((int)incl, 63, 64);
    }
    if (lane == 0) fb.qcount[k] = carry;
}

__global__ void __launch_bounds__(kQueueChunk) queue_write_kernel(const FrameBatch fb) {
    __shared__ uint32_t s_w[kQueueChunk / 64];
    const int k = chunk_queue(fb, blockIdx.x);
    uint32_t entry = 0;
    const bool live = queue_slot(fb, k, (blockIdx.x - (uint32_t)fb.qchunk[k]) * kQueueChunk + threadIdx.x, entry);
    const unsigned long long m = __builtin_amdgcn_ballot_w64(live);
    if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!live) return;
    uint32_t before = 0;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) before += s_w[w];
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    fb.qlist[(size_t)fb.qstart[k] * (uint32_t)fb.n + fb.chunk_base[blockIdx.x] + before + rank] = entry;
}

// sample_dst (rt_core.cuh:67-193) for every pixel of the batch, at full lane utilisation: the RNG
// jump (volrend.cu:157), SPP draws of -log(1-u) and their sort.  The thresholds go to the hand-off
// buffer slots [i][pixel] that the traversal later overwrites with the pixel's hit list.
// Tiles (waves) per workgroup: ONE, as in the shading kernel and for the same reason -- two thirds of the waves find their tile
// unmarked and leave after one load, the others draw for ~400 instructions, and a workgroup frees its slots when its last wave ends
// (4 waves: 0.438 ms per 100 C2 frames for marks + lists + thresholds, 2: 0.436, 1: 0.427; profiles/r6_w_ab_sample_waves.txt)
#ifndef RTO_SAMPLE_WG_WAVES
#define RTO_SAMPLE_WG_WAVES 1
#endif
constexpr int kSampleWaves = RTO_SAMPLE_WG_WAVES;
// tiles per wave of sample_kernel (round 6): with one 8x8 tile per single-wave workgroup a 100-frame launch is a million
// workgroups, two thirds of which leave after their mark load -- the kernel then runs at the rate workgroups are DISPATCHED
// (~2 per clock chip-wide: 0.24 ms before a single draw), not at any arithmetic rate.  A wave takes a strip of consecutive
// tiles, reads their marks in one round trip (lane i: tile i of the strip, ballot) and walks the marked ones.
#ifndef RTO_SAMPLE_TILES
#define RTO_SAMPLE_TILES 8
#endif
constexpr int kSampleTiles = RTO_SAMPLE_TILES;
static_assert(kSampleTiles >= 1 && kSampleTiles <= 64, "a strip's marks come from one ballot");
template <int SPP>
__global__ void __launch_bounds__(64 * kSampleWaves) sample_kernel(const FrameBatch fb, const PcgJumpEntry* __restrict__ jump) {
    // one wave = a strip of 8x8 tiles (row-major tiles): a culled tile costs its wave one bit of a ballot --
    // with one thread per pixel of a scanline nearly every wave held some marched pixel and paid for all the draws
    const uint32_t SIZE = (uint32_t)fb.width * (uint32_t)fb.height;
    const uint32_t tiles_x = (uint32_t)(fb.width + 7) >> 3, tiles_y = (uint32_t)(fb.height + 7) >> 3, n_tiles = tiles_x * tiles_y;
    const uint32_t tile0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * (uint32_t)kSampleWaves + (threadIdx.x >> 6)) * (uint32_t)kSampleTiles));
    if (tile0 >= n_tiles) return;
    const uint32_t lane = threadIdx.x & 63u;
    // a pixel of a culled tile: an empty hit list, no draws (its RNG stream is its own: nobody observes the skipped ones;
    // shade_kernel reads the marks, not a list)
    bool marked = lane < (uint32_t)kSampleTiles && tile0 + lane < n_tiles;
    if (marked && fb.tile_mask) marked = tile_marked(fb, (int)blockIdx.y, tile0 + lane);
    unsigned long long todo = __builtin_amdgcn_ballot_w64(marked);
    if (todo == 0ULL) return;
    const FrameDesc& fd = fb.f[blockIdx.y];
    RTO_GLOBAL uint32_t* const fhits = as_global(fd.hits);
    while (todo) {
        const uint32_t tile = tile0 + (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1ULL;
        const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const uint32_t x = tx * 8u + (lane & 7u), y = ty * 8u + (lane >> 3);
        if (x >= (uint32_t)fb.width || y >= (uint32_t)fb.height) continue;
        const uint32_t idx = y * (uint32_t)fb.width + x;
        Pcg32 rng;
        rng.state = fd.rng_state;
        rng.inc = fd.rng_inc;
        pcg_advance_tab(rng, idx * (uint32_t)SPP, jump);
        float dst[SPP];
#pragma unroll
        for (int n = 0; n < SPP; ++n) {
            float tv = -det_log_one_minus(pcg_next_float(rng));
#pragma unroll
            for (int i = 0; i < n; ++i) {  // static-index insertion: same sorted array
                // (v_min_f32 / v_max_f32: the draws are never NaN, and the only zero a draw can be is -0.0 = -log(1 - 0), so
                //  these return what the reference's `a < b ? a : b` forms do -- in half the instructions)
                const float lo = __builtin_fminf(dst[i], tv), hi = __builtin_fmaxf(dst[i], tv);
                dst[i] = lo;
                tv = hi;
            }
            dst[n] = tv;
        }
        // (-log(1 - 0) = -0.0: the thresholds are only ever compared, so +0.0 serves; its clear top bit is what the
        //  shading kernel ends a hit list on)
#pragma unroll
        for (int i = 0; i < SPP; ++i) fhits[hit_index<SPP>(idx, (uint32_t)i, SIZE)] = __float_as_uint(dst[i]) & ~kHitValid;
    }
}

// (flush_hits, the staged hit lists of a ray: rto_render_shared.h)

// REFILL = idle lanes that trigger a retire + refill round
// Flat traversal: one node visit (one load) per lane per loop iteration -- a lane either descends one level or,
// at a leaf, takes its march step and picks the restart node of the next one -- instead of a nested
// "descend until leaf" loop whose trip count is the maximum over the wave (measured: 1.4 loads per
// lane-step on average, but ~4 per wave-step for the slowest lane).
// STACK: where the ancestor stack lives -- 1: two registers (WIDE and at most two pairs of levels below the grid: decided by the
// launcher, so the loop body holds no wave-uniform "which stack?" dispatch: that was 11 scalar instructions per iteration of ~135
// issue slots), 0: the LDS rows
template <int SPP, int REFILL, int WPS, bool WIDE, int STACK>
__global__ void __launch_bounds__(256, WPS) render_persist(const TreeDev tree, const OptDev opt, const FrameBatch fb,
                                                       unsigned long long* __restrict__ queue,
                                                       uint32_t* __restrict__ hits, const uint32_t chunk) {
#include "rto_render_persist.inc"
}

// the batched traversal over the context's depth layer (rto_ctx_set_layers): the same body, the ray set-up reads the depth of its
// tile's pixels.  Instantiated for the default tuning only (REFILL 32, RTO_WPS_DEFAULT waves per SIMD).
template <int SPP, int REFILL, int WPS, bool WIDE, int STACK>
__global__ void __launch_bounds__(256, WPS) render_persist_layers(const TreeDev tree, const OptDev opt, const FrameBatch fb,
                                                              unsigned long long* __restrict__ queue,
                                                              uint32_t* __restrict__ hits, const uint32_t chunk, const LayerDev layers) {
#define RTO_PERSIST_LAYERS 1
#include "rto_render_persist.inc"
#undef RTO_PERSIST_LAYERS
}


// One hit leaf of a quantised tree, shaded straight from the codebooks (TreeDev::qrec / qcolors): the
// coefficients are the very fp16 values N3Tree::load_npz would have expanded (n3tree.cpp:310-339),
// summed in shade_leaf's order, so the pixel is bit-identical to rendering the decoded tree.
template <int B>
RTO_DEV void shade_leaf_quant(const TreeDev& tree, uint32_t slot, const float* basis_fn, float cnt, float* out) {
    const int nr = tree.q_retain;
    const uint16_t* __restrict__ rec = tree.qrec + (uint64_t)slot * (uint32_t)tree.q_rec;
    float v[B][3];
#pragma unroll
    for (int k = 0; k < B; ++k) {
        if (k < nr) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[k][c] = half_bits_to_float(rec[k * 3 + c]);
        } else {
            const uint32_t id = rec[2 * nr + k];  // 3 * nr + (k - nr)
            const uint2 e = tree.qcolors[(uint32_t)(k - nr) * 65536u + id];
            v[k][0] = half_bits_to_float((uint16_t)(e.x & 0xffffu));
            v[k][1] = half_bits_to_float((uint16_t)(e.x >> 16));
            v[k][2] = half_bits_to_float((uint16_t)(e.y & 0xffffu));
        }
    }
    float t3[3], o3[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float tmp = basis_fn[0] * v[0][c];
        if constexpr (B >= 25) {
            tmp += basis_fn[16] * v[16][c] + basis_fn[17] * v[17][c] + basis_fn[18] * v[18][c] +
                   basis_fn[19] * v[19][c] + basis_fn[20] * v[20][c] + basis_fn[21] * v[21][c] +
                   basis_fn[22] * v[22][c] + basis_fn[23] * v[23][c] + basis_fn[24] * v[24][c];
        }
        if constexpr (B >= 16) {
            tmp += basis_fn[9] * v[9][c] + basis_fn[10] * v[10][c] + basis_fn[11] * v[11][c] +
                   basis_fn[12] * v[12][c] + basis_fn[13] * v[13][c] + basis_fn[14] * v[14][c] +
                   basis_fn[15] * v[15][c];
        }
        if constexpr (B >= 9) {
            tmp += basis_fn[4] * v[4][c] + basis_fn[5] * v[5][c] + basis_fn[6] * v[6][c] + basis_fn[7] * v[7][c] +
                   basis_fn[8] * v[8][c];
        }
        if constexpr (B >= 4) {
            tmp += basis_fn[1] * v[1][c] + basis_fn[2] * v[2][c] + basis_fn[3] * v[3][c];
        }
        t3[c] = tmp;
    }
    sigmoid_cnt3(t3, cnt, o3);  // out[c] += cnt / (1.f + det_expf(-tmp)), rt_core.cuh:314-318
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] += o3[c];
    out[3] += cnt;
}

// quant_map [nq][ns] + data_retained [nr][ns][3]  ->  slot-major records (TreeDev::qrec)
__global__ void pack_quant_kernel(const uint16_t* __restrict__ qmap, const uint16_t* __restrict__ retained,
                                  int64_t ns, int nr, int nq, int rec, uint16_t* __restrict__ out) {
    const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= ns) return;
    uint16_t* o = out + slot * rec;
    for (int k = 0; k < nr; ++k)
        for (int c = 0; c < 3; ++c) o[k * 3 + c] = retained[((int64_t)k * ns + slot) * 3 + c];
    for (int j = 0; j < nq; ++j) o[3 * nr + j] = qmap[(int64_t)j * ns + slot];
    if (rec > 3 * nr + nq) o[rec - 1] = 0;
}

hipError_t launch_pack_quant(const uint16_t* qmap, const uint16_t* retained, int64_t ns, int nr, int nq, int rec,
                             uint16_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(pack_quant_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, stream, qmap, retained, ns, nr,
                       nq, rec, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------ shading kernel
// Second half of trace_ray (rt_core.cuh:272-331) + the pixel epilogue (volrend.cu:174-212) for the
// batched path.  hits: packed entries per frame, ended by the first word without kHitValid (layout: hit_index).
//
// Only about a quarter of the pixels hit anything and those that do hold 1..SPP leaves, so a
// thread-per-pixel loop leaves most lanes idle while the gathers of a few run.  Instead each wave
// owns 64 * P consecutive pixels, compacts their hit entries into an LDS list (wave prefix sum),
// shades the entries one per lane -- every lane busy, all of an entry's loads independent -- and
// the pixel lanes then add their entries' contributions up in hit order, which keeps the float sums
// those of the reference's loop.  The list is processed in windows of kShadeCap entries so LDS use
// does not depend on SPP.
#ifndef RTO_SHADE_CAP
#define RTO_SHADE_CAP 320
#endif
constexpr int kShadeCap = RTO_SHADE_CAP;

// contribution of one hit leaf: rgb[c] = cnt * sigmoid(<basis, coeffs_c>) (or cnt * rgb for RGBA trees)
// MODE (host-chosen, so that each instantiation carries one leaf layout's registers only):
// 0 any dense tree; 28 / 49 / 76 dense SH9 / SH16 / SH25 records (or SG / ASG records of the same data_dim: the layout does
// not depend on the basis); -B quantised SH<B>, not expanded
template <int MODE>
RTO_DEV void leaf_contrib(const TreeDev& tree, uint32_t slot, const float* basis_fn, float cnt, float* o) {
    o[0] = o[1] = o[2] = o[3] = 0.f;  // 0 + x == x: the helpers' "+=" yields the bare term
    if constexpr (MODE < 0) {
        shade_leaf_quant<-MODE>(tree, slot, basis_fn, cnt, o);
    } else if constexpr (MODE == 0) {
        shade_leaf(tree, tree.data + (uint64_t)slot * tree.data_dim, basis_fn, cnt, o);
    } else {
        shade_leaf_packed<MODE>(tree, slot, basis_fn, cnt, o);
    }
}

#ifndef RTO_SHADE_WPS
#define RTO_SHADE_WPS 4
#endif
// workgroups per CU the kernel is built for: the SH25 layouts (76 coefficients in registers) and the quantised SH16 one need
// more than the 128 VGPRs that 4 leave them (they spilled 10-50 registers to scratch: SH25 shading 9.6 -> 8.7 ms per 100
// frames of 1920x1080 without the spills, at 3)
#ifndef RTO_SHADE_WPS_SH25
#define RTO_SHADE_WPS_SH25 3
#endif
constexpr int shade_wps(int mode) { return (mode == 76 || mode == -25 || mode == -16) ? RTO_SHADE_WPS_SH25 : RTO_SHADE_WPS; }
#ifdef RTO_DBG_COUNTERS
// where a shading wave's lifetime goes (tools/dbg_shade_phases.py): per wave (blockIdx.x * 4 + wave, up to 2^19 of them) the s_memtime
// stamps 0..5 and its number of hit entries; plain stores, reduced on the host (atomics would slow the very kernel they time)
constexpr int kShadeStampWaves = 1 << 19;
__device__ unsigned long long g_shade_phase[kShadeStampWaves * 8];
#define RTO_SHADE_STAMP(i) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); ph[i] = __builtin_amdgcn_s_memtime(); }
#else
#define RTO_SHADE_STAMP(i) {}
#endif
// Waves per workgroup: ONE (round 6).  The waves of this kernel never talk to each other (wave-level barriers only), and their
// lifetimes differ by a factor of eight -- a wave over culled tiles ends after ~7 k clocks, one with 500 hit entries after ~58 k
// (tools/dbg_shade_phases.py, profiles/r6_d_shade_phases.txt) -- but a workgroup's LDS and wave slots are released only when its
// LAST wave ends: with 4 waves per workgroup the SIMDs held 2.9 waves of the 4 they have room for.
#ifndef RTO_SHADE_WG_WAVES
#define RTO_SHADE_WG_WAVES 1
#endif
constexpr int kShadeWaves = RTO_SHADE_WG_WAVES;
#ifndef RTO_SHADE_BAND_ROWS
#define RTO_SHADE_BAND_ROWS 8
#endif
// pixel blocks (of block_px consecutive pixels, scanline order) per band of RTO_SHADE_BAND_ROWS rows
__host__ __device__ constexpr uint32_t shade_blocks_per_band(int W, int block_px) {
    return (uint32_t)((RTO_SHADE_BAND_ROWS > 0 ? RTO_SHADE_BAND_ROWS : 1) * W + block_px - 1) / (uint32_t)block_px;
}
// LOBES: 0 for SH and RGBA trees, kFmtSG / kFmtASG for a tree of that format (with MODE 0 / 28 / 49 / 76)
template <int SPP, int P, int MODE, int LOBES = 0>
__global__ void __launch_bounds__(64 * kShadeWaves, shade_wps(MODE)) shade_kernel(const TreeDev tree, const OptDev opt, const FrameBatch fb,
                                                                              const uint32_t* __restrict__ hits0) {
#include "rto_shade.inc"
}

// the shading kernel over the context's colour layer (rto_ctx_set_layers): the same body, the epilogue composites every pixel --
// hit, missed or culled -- over its pixel of the colour plane of its frame
template <int SPP, int P, int MODE, int LOBES = 0>
__global__ void __launch_bounds__(64 * kShadeWaves, shade_wps(MODE)) shade_kernel_layers(const TreeDev tree, const OptDev opt, const FrameBatch fb,
                                                                                     const uint32_t* __restrict__ hits0, const LayerDev layers) {
#define RTO_SHADE_LAYERS 1
#include "rto_shade.inc"
#undef RTO_SHADE_LAYERS
}

// ------------------------------------------------------------------ frame table
// The frame descriptors of a batch reach the device as kernel arguments of this one-wave kernel, at most kFrameChunk
// per launch (a kernarg segment holds 4 KB; 64 descriptors are 6 KB), and are written to the context's table on the
// launch stream: no host staging buffer whose lifetime would have to outlast an asynchronous copy.
__global__ void write_frames_kernel(const FrameChunk c, FrameDesc* __restrict__ dst, int n) {
    const int i = threadIdx.x;
    if (i < n) dst[i] = c.f[i];
}

// ------------------------------------------------------------------ u8 conversion
// main_headless.cpp:535-538: (uint8_t)(f * 255), truncation, all four channels
__global__ void rgba8_kernel(const float4* __restrict__ in, uchar4* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 v = in[i];
    uchar4 o;
    o.x = (unsigned char)(v.x * 255);
    o.y = (unsigned char)(v.y * 255);
    o.z = (unsigned char)(v.z * 255);
    o.w = (unsigned char)(v.w * 255);
    out[i] = o;
}

}  // namespace rto

// ------------------------------------------------------------------ host launchers (C++ linkage,
// declared in rto_launch.h)
#include "rto_dispatch.h"
#include "rto_launch.h"

namespace rto {

hipError_t launch_build_nodew(const int32_t* child, const uint16_t* data, int64_t n_slots, int data_dim,
                              uint32_t* nodew, int* bad_flag, hipStream_t stream) {
    const int threads = 256;
    const int64_t blocks = (n_slots + threads - 1) / threads;
    hipLaunchKernelGGL(build_nodew_kernel, dim3((unsigned)blocks), dim3(threads), 0, stream, child, data, n_slots,
                       data_dim, nodew, bad_flag);
    return hipGetLastError();
}

hipError_t launch_build_shrec(const uint16_t* data, int64_t n_slots, int data_dim, int rec, const uint32_t* recidx, uint16_t* out,
                              hipStream_t stream) {
    const int64_t n = n_slots * rec;
    hipLaunchKernelGGL(build_shrec_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, data, n_slots, data_dim, rec, recidx, out);
    return hipGetLastError();
}

hipError_t launch_build_shrec_wide(const TreeDev& tree, const uint16_t* data, int64_t n_entries, int rec, uint16_t* out, hipStream_t stream) {
    const int64_t n = n_entries * rec;
    hipLaunchKernelGGL(build_shrec_wide_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, tree, data, n_entries, rec, out);
    return hipGetLastError();
}

hipError_t launch_rebuild_reference_wide(const TreeDev& tree, int64_t n_entries, int rec, uint16_t* data, hipStream_t stream) {
    const int64_t n = n_entries * rec;
    hipLaunchKernelGGL(rebuild_reference_wide_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, tree, n_entries, rec, data);
    return hipGetLastError();
}

hipError_t launch_rebuild_reference(const uint16_t* shrec, const uint32_t* nodew, const uint32_t* recidx, int64_t n_slots, int data_dim,
                                    int rec, uint16_t* data, int32_t* child, hipStream_t stream) {
    const int64_t n = n_slots * data_dim;
    hipLaunchKernelGGL(rebuild_reference_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, shrec, nodew, recidx, n_slots,
                       data_dim, rec, data, child);
    return hipGetLastError();
}

hipError_t launch_build_topgrid(const uint32_t* nodew, int G, uint2* grid, hipStream_t stream) {
    const unsigned n = 1u << (3 * G);
    hipLaunchKernelGGL(build_topgrid_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, nodew, G, grid);
    return hipGetLastError();
}

TileMap make_tile_map(int width, int height, int strip_rows) {
    TileMap tm;
    tm.tiles_x = (width + kTileW - 1) / kTileW;
    tm.tiles_y = (height + kTileH - 1) / kTileH;
    tm.strip_rows = strip_rows < 1 ? 1 : strip_rows;
    const int strips = (tm.tiles_y + tm.strip_rows - 1) / tm.strip_rows;
    const int strips_per_xcd = (strips + 7) / 8;
    tm.per_xcd = strips_per_xcd * tm.strip_rows * tm.tiles_x;
    return tm;
}

template <int SPP, int LOBES>
static void launch_fast(const TreeDev& tree, const CamDev& cam, const OptDev& opt, const Pcg32& rng, const PcgJumpEntry* jump,
                        const FrameOut& fo, int strip_rows, const LayerDev* layers, hipStream_t stream) {
    const TileMap tm = make_tile_map(cam.width, cam.height, strip_rows);
    const size_t lds = fast_lds_bytes(tree);
    const dim3 grid(8 * tm.per_xcd), block(256);
    const auto offscreen = [&](auto stats, auto wide, auto stack) {
        if constexpr (LOBES == 0)
            hipLaunchKernelGGL((render_fast<SPP, stats, wide, stack>), grid, block, lds, stream, tree, cam, opt, rng, jump, tm, fo);
        else
            hipLaunchKernelGGL((render_fast_lobes<SPP, stats, wide, stack, LOBES>), grid, block, lds, stream, tree, cam, opt, rng, jump, tm, fo);
    };
    if (fo.stats && !layers) {  // (the counting instantiation walks the one-level image: its units are defined on that walk)
        offscreen(std::true_type{}, std::false_type{}, int_c<0>{});
        return;
    }
    with_image(tree, [&](auto wide, auto stack) {
        if (layers)  // (the host refuses layers with work counters)
            hipLaunchKernelGGL((render_fast_layers<SPP, wide, stack, LOBES>), grid, block, lds, stream, tree, cam, opt, rng, jump, tm, fo, *layers);
        else
            offscreen(std::false_type{}, wide, stack);
    });
}

hipError_t launch_rays(int kernel, int spp, const TreeDev& tree, const OptDev& opt, const Pcg32& rng, const PcgJumpEntry* jump,
                       const RayBatch& rb_in, const DepthOut* depth, bool xcd_order, hipStream_t stream) {
    if (rb_in.n == 0) return hipSuccess;
    if ((uint64_t)rb_in.n * (uint64_t)spp >= (uint64_t(1) << 32)) return hipErrorInvalidValue;  // (the RNG offset of a ray is 32-bit)
    RayBatch rb = rb_in;
    const uint32_t blocks = (uint32_t)(((uint64_t)rb.n + 255) / 256);
    rb.per_xcd = xcd_order ? (blocks + 7) / 8 : 0u;
    const dim3 grid(xcd_order ? 8 * rb.per_xcd : blocks);
    if (depth)  // the depth-carrying kernels (depth_kernels.hip)
        return kernel == 2 ? launch_rays_depth_fast(spp, tree, opt, rng, jump, rb, *depth, grid, stream)
                           : launch_rays_depth_generic(spp, tree, opt, rng, rb, *depth, grid, stream);
    return with_spp(spp, [&](auto SPP) {
        if (kernel == 2)
            with_lobes(tree, [&](auto LOBES) {
                with_image(tree, [&](auto wide, auto stack) {
                    hipLaunchKernelGGL((render_rays<SPP, wide, stack, LOBES>), grid, dim3(256), fast_lds_bytes(tree), stream, tree, opt, rng, jump, rb);
                });
            });
        else
            hipLaunchKernelGGL(render_rays_generic<SPP>, grid, dim3(256), 0, stream, tree, opt, rng, rb);
        return hipGetLastError();
    });
}

hipError_t launch_mark_tiles_one(const TreeDev& tree, const CamDev& cam, uint32_t* mask, int mask_words, hipStream_t stream) {
    FrameDesc fd = {};
    fd.fx = cam.fx;
    fd.fy = cam.fy;
    for (int i = 0; i < 12; ++i) fd.transform[i] = cam.transform[i];
    if (hipMemsetAsync(mask, 0, (size_t)mask_words * sizeof(uint32_t), stream) != hipSuccess) return hipErrorLaunchFailure;
    if (tree.n_occ_cells > 0) {
        const dim3 grid((unsigned)((tree.n_occ_cells + kMarkCells - 1) / kMarkCells));
        const size_t lds = mask_words <= kMarkLdsWords ? (size_t)mask_words * sizeof(uint32_t) : 0;
        hipLaunchKernelGGL(mark_tiles_one_kernel, grid, dim3(256), lds, stream, tree, fd, cam.width, cam.height, mask_words, mask);
    }
    return hipGetLastError();
}

hipError_t launch_render(int kernel, int spp, const TreeDev& tree, const CamDev& cam, const OptDev& opt,
                         const Pcg32& rng, const PcgJumpEntry* jump, const FrameOut& fo, int strip_rows,
                         const LayerDev* layers, const DepthOut* depth, hipStream_t stream) {
    if (depth) {  // the depth-carrying layered kernels (depth_kernels.hip), over the context's layers or none
        const LayerDev ld = layers ? *layers : LayerDev{nullptr, nullptr};
        return kernel == 2 ? launch_fast_depth(spp, tree, cam, opt, rng, jump, fo, strip_rows, ld, *depth, stream)
                           : launch_generic_depth(spp, tree, cam, opt, rng, fo, ld, *depth, stream);
    }
    return with_spp(spp, [&](auto SPP) {
        const dim3 ggrid((unsigned)(((int64_t)cam.width * cam.height + 255) / 256));
        if (kernel == 2)
            with_lobes(tree, [&](auto LOBES) { launch_fast<SPP, LOBES>(tree, cam, opt, rng, jump, fo, strip_rows, layers, stream); });
        else if (layers)
            hipLaunchKernelGGL(render_generic_layers<SPP>, ggrid, dim3(256), 0, stream, tree, cam, opt, rng, fo, *layers);
        else
            hipLaunchKernelGGL(render_generic<SPP>, ggrid, dim3(256), 0, stream, tree, cam, opt, rng, fo);
        return hipGetLastError();
    });
}

// (RTO_WPS_DEFAULT, the waves per SIMD the default instantiation is built for: rto_render_shared.h)
// LAYERS: the launch may carry layers (`layers` != nullptr: rto_ctx_set_layers) -- a depth layer takes render_persist_layers, a
// colour layer shade_kernel_layers; instantiated for the default tuning only
// depth != nullptr (LAYERS only; rto_ctx_enable_depth(RTO_DEPTH_BATCHED)): the traversal is render_persist_depth, over the layers or
// none, through the launcher of depth_kernels.hip; its planes are filled with (0, +inf) on the stream first.  Marks, queues,
// thresholds and shading are what they are without
// WIDE, STACK: the traversal image (with_image, chosen by launch_batch_spp)
template <int SPP, int REFILL, int WPS, bool WIDE, int STACK, bool LAYERS = false>
static hipError_t launch_batch_impl(const TreeDev& tree, const OptDev& opt, const FrameBatch& fb,
                                    const PcgJumpEntry* jump, unsigned long long* queue, uint32_t* hits, int num_cus,
                                    int chunk_override, bool cull, OccupancyCache* occ, hipEvent_t* ev, hipStream_t stream,
                                    const LayerDev* layers = nullptr, const DepthOut* depth = nullptr) {
    // dynamic LDS: ancestor stack + thresholds per lane, then the frame table of THIS batch (96 B per frame: a batch of
    // one does not pay for 128)
    constexpr bool regstack = STACK == 1;  // (the LDS rows of the register-stack form only park a ray's two hand-off offsets)
    bool with_depth = false;  // (two more rows, the ray's hit distances; without the register stack four: rto_render_persist.inc)
    if constexpr (LAYERS) with_depth = depth != nullptr;
    const size_t lds = (size_t)((regstack ? 2 : tree.max_depth + 1 - tree.top_levels) + SPP + 1 + (with_depth ? (regstack ? 2 : 4) : 0)) * 256 * sizeof(uint32_t) + sizeof(float) * kCamFloats * (size_t)fb.n;
    // the traversal kernel of this launch: the key of the occupancy cache, of the occupancy query and of the LDS request below
    const void* fn = reinterpret_cast<const void*>(&render_persist<SPP, REFILL, WPS, WIDE, STACK>);
    bool depth_layer = false, color_layer = false;
    if constexpr (LAYERS) {
        depth_layer = layers && layers->depth;
        color_layer = layers && layers->color;
        if (depth_layer) fn = reinterpret_cast<const void*>(&render_persist_layers<SPP, REFILL, WPS, WIDE, STACK>);
        if (with_depth) fn = persist_depth_kernel(SPP, tree);
    }
    OccupancyCache local;
    if (!occ) occ = &local;
    occ->lds_refused = false;
    if (occ->force_lds_refusal) {
        occ->lds_refused = true;
        return hipSuccess;
    }
    if (occ->blocks_per_cu == 0 || occ->fn != fn || occ->lds != lds) {
        if (lds > 64 * 1024) {  // beyond the default dynamic-LDS window: ask for it (the CU has 160 KB)
            if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
                (void)hipGetLastError();
                occ->lds_refused = true;  // (deep tree x SPP 32 x many frames) nothing launched: the caller takes the generic kernel
                return hipSuccess;
            }
        }
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, 256, lds) != hipSuccess || nb < 1)
            nb = 2;
        occ->blocks_per_cu = nb > 8 ? 8 : nb;
        occ->fn = fn;
        occ->lds = lds;
    }
    const int blocks_per_cu = occ->cap > 0 && occ->cap < occ->blocks_per_cu ? occ->cap : occ->blocks_per_cu;
    const int tiles = ((fb.width + 7) / 8) * ((fb.height + 7) / 8) * fb.n;
    int grid = num_cus * blocks_per_cu;
    if (grid > (tiles + 3) / 4) grid = (tiles + 3) / 4;  // never more waves than 8x8 tiles
    if (grid < 1) grid = 1;
    // dequeue granularity: big enough to keep the single counter far below its ~90 dequeues/us,
    // small enough that every wave draws several times (a wave that draws twice while its
    // neighbour draws three times is a 33 % imbalance)
    const int64_t rays_per_wave = (int64_t)tiles * 64 / ((int64_t)grid * 4);
    // (round 6, with the band queues: two tiles per dequeue beat four on every configuration -- C2 3.83 -> 3.74 ms per 100 frames,
    //  C5 2.44 -> 2.41, C4 11.85 -> 11.71, 8 scenes 3.26 -> 3.13; one tile 3.74 / 2.48 / 11.73 / 3.14, eight 3.90 on C2:
    //  profiles/r6_zz_ab_chunk_*.txt)
    const uint32_t chunk = chunk_override > 0 ? (uint32_t)chunk_override : (rays_per_wave >= 512 ? 128u : 64u);
    const int64_t size = (int64_t)fb.width * fb.height;
    if (ev) (void)hipEventRecord(ev[0], stream);
    // tile marks (empty-space culling; all ones when it is off), then the ray queues as lists of the marked tile slots
    uint32_t* mask = const_cast<uint32_t*>(fb.tile_mask);
    const size_t mask_bytes = (size_t)fb.n * fb.mask_words * sizeof(uint32_t);
    if (hipMemsetAsync(mask, cull ? 0 : 0xff, mask_bytes, stream) != hipSuccess) return hipErrorLaunchFailure;
    if constexpr (LAYERS) {
        // a pixel whose ray never flushes -- culled tile, box miss, dead depth-layer pixel, no hit -- reads (0, +inf): the planes of
        // the launch's slots are filled on the stream before the traversal stores the others (0x7f800000 = +inf)
        if (with_depth) {
            const size_t n_px = (size_t)fb.n * (size_t)fb.width * (size_t)fb.height;
            if (hipMemsetAsync(depth->depth, 0, n_px * sizeof(float), stream) != hipSuccess ||
                hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(depth->t_near), 0x7f800000, n_px, stream) != hipSuccess)
                return hipErrorLaunchFailure;
        }
    }
    if (cull && tree.n_occ_cells > 0) {
        const dim3 mgrid((unsigned)((tree.n_occ_cells + kMarkCells - 1) / kMarkCells), fb.n);
        if (fb.mask_words <= kMarkLdsWords)
            hipLaunchKernelGGL(mark_tiles_kernel<true>, mgrid, dim3(256), (size_t)fb.mask_words * sizeof(uint32_t), stream, tree, fb, mask);
        else
            hipLaunchKernelGGL(mark_tiles_kernel<false>, mgrid, dim3(256), 0, stream, tree, fb, mask);
    }
    const unsigned n_chunks = (unsigned)fb.qchunk[fb.n_queues];
    hipLaunchKernelGGL(queue_count_kernel, dim3(n_chunks), dim3(kQueueChunk), 0, stream, fb);
    hipLaunchKernelGGL(queue_scan_kernel, dim3(1), dim3(64 * kMaxQueues), 0, stream, fb, queue);  // (+ arms the ray queues)
    hipLaunchKernelGGL(queue_write_kernel, dim3(n_chunks), dim3(kQueueChunk), 0, stream, fb);
    hipLaunchKernelGGL(sample_kernel<SPP>, dim3((unsigned)(((tiles / fb.n + kSampleTiles - 1) / kSampleTiles + kSampleWaves - 1) / kSampleWaves), fb.n), dim3(64 * kSampleWaves), 0, stream, fb, jump);
    if (ev) (void)hipEventRecord(ev[1], stream);
    if constexpr (LAYERS) {
        if (with_depth) {
            if (launch_persist_depth(SPP, tree, grid, lds, stream, opt, fb, queue, hits, chunk, layers ? *layers : LayerDev{nullptr, nullptr},
                                     *depth) != hipSuccess)
                return hipErrorLaunchFailure;
        } else if (depth_layer)
            hipLaunchKernelGGL((render_persist_layers<SPP, REFILL, WPS, WIDE, STACK>), dim3(grid), dim3(256), lds, stream, tree, opt, fb, queue,
                               hits, chunk, *layers);
    }
    if (!depth_layer && !with_depth)
        hipLaunchKernelGGL((render_persist<SPP, REFILL, WPS, WIDE, STACK>), dim3(grid), dim3(256), lds, stream, tree, opt, fb, queue, hits, chunk);
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    if (ev) (void)hipEventRecord(ev[2], stream);
#ifndef RTO_SHADE_P
#define RTO_SHADE_P 2
#endif
    constexpr int SP = SPP <= 8 ? RTO_SHADE_P : 1;  // pixels per lane of the shading kernel (its hit lists live in registers)
    const unsigned pblocks = (unsigned)((size + 64 * kShadeWaves * SP - 1) / (64 * kShadeWaves * SP));
#if RTO_SHADE_BAND_ROWS > 0
    const unsigned cpb = shade_blocks_per_band(fb.width, 64 * kShadeWaves * SP), bands = (pblocks + cpb - 1u) / cpb;
    const dim3 sgrid(((bands + 7u) / 8u) * 8u * cpb * (unsigned)fb.n);  // see shade_kernel: (band, frame, pixel block of the band) <- block id
#else
    const dim3 sgrid(((pblocks + 7u) / 8u) * 8u * (unsigned)fb.n);  // see shade_kernel: (pixel block, frame) <- block id
#endif
    const dim3 sblock(64 * kShadeWaves);
    if (tree.qrec && !color_layer) {  // (the host admits SH4/9/16/25 only, and refuses a quantised-direct tree layers)
        const auto quant = [&](auto mode) { hipLaunchKernelGGL((shade_kernel<SPP, SP, mode>), sgrid, sblock, 0, stream, tree, opt, fb, (const uint32_t*)hits); };
        if (tree.basis_dim == 4)
            quant(int_c<-4>{});
        else if (tree.basis_dim == 9)
            quant(int_c<-9>{});
        else if (tree.basis_dim == 16)
            quant(int_c<-16>{});
        else
            quant(int_c<-25>{});
    } else {  // an expanded tree: the record modes for SH, SG and ASG trees, over the colour layer or not
        with_lobes(tree, [&](auto lobes) {
            with_record_mode(tree, lobes != 0 || tree.format == kFmtSH, [&](auto mode) {
                if (!color_layer)
                    hipLaunchKernelGGL((shade_kernel<SPP, SP, mode, lobes>), sgrid, sblock, 0, stream, tree, opt, fb, (const uint32_t*)hits);
                else if constexpr (LAYERS)
                    hipLaunchKernelGGL((shade_kernel_layers<SPP, SP, mode, lobes>), sgrid, sblock, 0, stream, tree, opt, fb, (const uint32_t*)hits, *layers);
            });
        });
    }
    if (ev) (void)hipEventRecord(ev[3], stream);
    return hipGetLastError();
}

template <int SPP>
static hipError_t launch_batch_spp(const TreeDev& tree, const OptDev& opt, const FrameBatch& fb,
                                   const PcgJumpEntry* jump, unsigned long long* queue, uint32_t* hits, int num_cus,
                                   int refill, bool cull, OccupancyCache* occ, hipEvent_t* ev, const LayerDev* layers, const DepthOut* depth,
                                   hipStream_t stream) {
    // tuning: refill = 1000 * tiles_per_dequeue + 100 * waves/SIMD + threshold
    refill %= 100000;
    const int chunk_override = (refill / 1000) * 64;
    refill %= 1000;
    if constexpr (SPP == 6) {  // tuning instantiations only for the benchmark configuration (and its usual two-level image)
#define RTO_F(R, O)                                                                                                                     \
    return with_wide_image(tree, [&](auto wide, auto stack) {                                                                           \
        return launch_batch_impl<SPP, R, O, wide, stack>(tree, opt, fb, jump, queue, hits, num_cus, chunk_override, cull, occ, ev, stream); \
    })
        // A/B set kept for tools/ab_tuning.py: 100 * waves/SIMD + refill threshold
        // (a layered launch: the default instantiation whatever the key's A/B part says)
        if (tree.widew && !layers && !depth) switch (refill) {
            case 808: RTO_F(8, 8);
            case 816: RTO_F(16, 8);
            case 824: RTO_F(24, 8);
            case 832: RTO_F(32, 8);
            case 840: RTO_F(40, 8);
            case 724: RTO_F(24, 7);
            case 732: RTO_F(32, 7);
            case 740: RTO_F(40, 7);
            case 632: RTO_F(32, 6);
            case 432: RTO_F(32, 4);
            case 232: RTO_F(32, 2);
            case 132: RTO_F(32, 1);
            default: break;
        }
#undef RTO_F
    }
    // Refill once half the lanes are idle (larger refill rounds waste fewer issue slots on the partially filled ray set-up:
    // 32 idle lanes beat 16 by 4 %); registers budgeted for RTO_WPS_DEFAULT waves per SIMD.  Occupancy matters (round 3,
    // measured with the real knob, tuning key blocks_per_cu: 1 / 2 / 3 / 4 / 5 / 6 workgroups per CU take 26.2 / 14.4 /
    // 10.6 / 8.8 / 7.8 / 7.35 ms per 100 frames -- round 2's "4 to 8 waves within 2 %" compared __launch_bounds__ hints,
    // which change the register budget, not the number of resident waves).
    // (Round 5's reservoir kernel -- whole-tile set-up, rays parked in LDS, refill rounds at 8-24 idle lanes -- lost its same-box
    //  A/B, 4.27-4.32 against 4.11-4.20 ms per 100 C2 frames, and lives in tools/experiments/r5_lab_switches.patch.)
    return with_image(tree, [&](auto wide, auto stack) {
        if (layers || depth)  // (depth outputs: the default instantiation too, render_persist_depth has no other)
            return launch_batch_impl<SPP, 32, RTO_WPS_DEFAULT, wide, stack, true>(tree, opt, fb, jump, queue, hits, num_cus, chunk_override, cull, occ,
                                                                                  ev, stream, layers, depth);
        return launch_batch_impl<SPP, 32, RTO_WPS_DEFAULT, wide, stack>(tree, opt, fb, jump, queue, hits, num_cus, chunk_override, cull, occ, ev, stream);
    });
}

hipError_t launch_render_batch(int spp, const TreeDev& tree, const OptDev& opt, const FrameBatch& fb,
                               const PcgJumpEntry* jump, unsigned long long* queue, uint32_t* hits, int num_cus,
                               int refill, bool cull, OccupancyCache* occ, hipEvent_t* ev, const LayerDev* layers, const DepthOut* depth,
                               hipStream_t stream) {
    return with_spp(spp, [&](auto SPP) {
        return launch_batch_spp<SPP>(tree, opt, fb, jump, queue, hits, num_cus, refill, cull, occ, ev, layers, depth, stream);
    });
}

#ifdef RTO_DBG_COUNTERS
hipError_t debug_shade_phases(unsigned long long* out, bool reset) {  // out: kShadeStampWaves * 8 words
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_shade_phase), sizeof(unsigned long long) * kShadeStampWaves * 8);
    if (e == hipSuccess && reset) {
        void* p = nullptr;
        e = hipGetSymbolAddress(&p, HIP_SYMBOL(g_shade_phase));
        if (e == hipSuccess) e = hipMemset(p, 0, sizeof(unsigned long long) * kShadeStampWaves * 8);
    }
    return e;
}
#endif

// ------------------------------------------------------------------ basis probe (rto_probe_basis)
// out[i][0..24] = the basis the kernels compute for the view direction dirs[i] (before the rot_dirs rotation): PATH 0 the run-time
// ray_basis of the generic / fast kernels and shade_kernel<..., 0>, PATH 1 the per-B forms of the shading kernel's record modes
// (ray_basis_sh<B> / ray_basis_lobes<LOBES, B>; entries from B on are 0)
template <int PATH, int LOBES, int B>
__global__ void __launch_bounds__(256) basis_probe_kernel(const TreeDev tree, const OptDev opt, const float* __restrict__ dirs, int64_t n,
                                                          float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float vdir[3] = {dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]};
    float basis_fn[RTO_BASIS_MAX_DEV];
#pragma unroll
    for (int k = 0; k < RTO_BASIS_MAX_DEV; ++k) basis_fn[k] = 0.f;
    if constexpr (PATH == 0)
        ray_basis_any(tree, opt, vdir, basis_fn);
    else if constexpr (LOBES == 0)
        ray_basis_sh<B>(opt, vdir, basis_fn);
    else
        ray_basis_lobes<LOBES, B>(tree, opt, vdir, basis_fn);
#pragma unroll
    for (int k = 0; k < RTO_BASIS_MAX_DEV; ++k) out[i * RTO_BASIS_MAX_DEV + k] = basis_fn[k];
}

template <int LOBES, int B = 1>
static hipError_t launch_probe_lobes(const TreeDev& tree, const OptDev& opt, const float* dirs, int64_t n, float* out, hipStream_t stream) {
    if (tree.basis_dim == B) {
        hipLaunchKernelGGL((basis_probe_kernel<1, LOBES, B>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, tree, opt, dirs, n, out);
        return hipGetLastError();
    }
    if constexpr (B < RTO_BASIS_MAX_DEV)
        return launch_probe_lobes<LOBES, B + 1>(tree, opt, dirs, n, out, stream);
    else
        return hipErrorInvalidValue;
}

hipError_t launch_probe_basis(const TreeDev& tree, const OptDev& opt, const float* dirs, int64_t n, int path, float* out, hipStream_t stream) {
    const dim3 grid((unsigned)((n + 255) / 256));
#define RTO_PROBE(P, L, B) hipLaunchKernelGGL((basis_probe_kernel<P, L, B>), grid, dim3(256), 0, stream, tree, opt, dirs, n, out)
    if (path == 0) {
        RTO_PROBE(0, 0, 0);
    } else if (tree.format == kFmtSG) {
        return launch_probe_lobes<kFmtSG>(tree, opt, dirs, n, out, stream);
    } else if (tree.format == kFmtASG) {
        return launch_probe_lobes<kFmtASG>(tree, opt, dirs, n, out, stream);
    } else if (tree.format == kFmtSH) {  // (the basis sizes the shading kernel has per-B forms for)
        switch (tree.basis_dim) {
            case 4: RTO_PROBE(1, 0, 4); break;
            case 9: RTO_PROBE(1, 0, 9); break;
            case 16: RTO_PROBE(1, 0, 16); break;
            case 25: RTO_PROBE(1, 0, 25); break;
            default: return hipErrorInvalidValue;
        }
    } else {
        return hipErrorInvalidValue;
    }
#undef RTO_PROBE
    return hipGetLastError();
}

hipError_t launch_write_frames(const FrameDesc* host, int n, FrameDesc* dev_table, hipStream_t stream) {
    for (int f0 = 0; f0 < n; f0 += kFrameChunk) {
        FrameChunk c;
        const int m = n - f0 < kFrameChunk ? n - f0 : kFrameChunk;
        for (int i = 0; i < m; ++i) c.f[i] = host[f0 + i];
        hipLaunchKernelGGL(write_frames_kernel, dim3(1), dim3(64), 0, stream, c, dev_table + f0, m);
    }
    return hipGetLastError();
}

hipError_t launch_rgba8(const float* rgba, uint8_t* out, int64_t n_pixels, hipStream_t stream) {
    const int threads = 256;
    hipLaunchKernelGGL(rgba8_kernel, dim3((unsigned)((n_pixels + threads - 1) / threads)), dim3(threads), 0, stream,
                       reinterpret_cast<const float4*>(rgba), reinterpret_cast<uchar4*>(out), n_pixels);
    return hipGetLastError();
}

}  // namespace rto
