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
//
// The render stage is one translation unit per group of kernels, each with the launchers of its kernels, so that they
// compile side by side; the launchers the units call in each other are rto_render_internal.h:
//   tree_image_kernels.hip  the builders of a tree's derived arrays (nodew, shrec, topgrid, qrec), the rebuild of the reference
//                           layout, the frame table and the u8 conversion
//   frame_kernels.hip       render_generic and render_fast, offscreen and over layers: launch_render
//   ray_kernels.hip         the same bodies over a batch of rays, render_rays_generic and render_rays: launch_rays
//   render_kernels.hip      (this unit) the batched traversal stage -- tile marks, ray queues, sample_kernel, render_persist --
//                           and the batched launch itself, launch_render_batch
//   shade_kernels.hip       shade_kernel and its knobs behind launch_shade; the basis probe
//   depth_kernels.hip       the depth-carrying forms of the frame, ray and batched traversal kernels
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"
#include "rto_tree_device.h"

#pragma clang fp contract(off)

// ray set-up, pixel / ray outputs, tiles, hit entries, packed shading, RTO_FAST_WPS: shared with the other render units
#include "rto_render_shared.h"
#include "rto_render_internal.h"  // launch_shade (shade_kernels.hip) and the batched depth traversal (depth_kernels.hip)

namespace rto {

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
// without marching: every culling cell of the tree (TreeDev::occ_cells: boxes that hold the leaves of positive density -- per
// node of level kOccLevel the bounds of its subtree's dense leaves, not its cube: a shell a few leaves thick fills a fraction
// of most cubes -- as world-space boxes padded far above the float error of a sample point) is projected into every frame of the batch; the
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
//   * absolute, kMarkPad = 0.5 pixels (1.5 while the cells were cubes).  ray_setup sends the ray of pixel (x, y), x and y integers,
//     through the camera-space point ((x - 0.5 W) / fx, -(y - 0.5 H) / fy, -1): the inverse of px = 0.5 W + fx a / d below AT
//     the integer, with no half-pixel offset, and every sample of a pixel shares that ray.  So a ray can meet the box only if
//     px0 <= x <= px1 up to float error, and the tiles floor(px0 / 8) .. floor(px1 / 8) would do.  The errors: of 0.5 W + fx x
//     here two roundings at the magnitude of a pixel coordinate (~1e-4 pixel at W ~ 1000); of the ray's direction
//     (a division, M xyz, normalize3) a few 1e-7 relative, ~1e-4 pixel at fx ~ 1000.  Both grow with the frame as fx does,
//     and so does the relative pad above (1e-5 fx (1 + |x|) or more: 100 times either at any frame size); the absolute pad
//     is 5000 times them at W ~ 1000 and never the one that is needed.  The sphere clamp keeps its 1.5.
// A box with a corner nearer than that marks the whole frame; one with every corner behind the camera nothing.
// The sphere rule stays as an upper clamp: where it yields a rectangle the tiles are the intersection of the two (each is a
// bound by itself, and a box lies inside its bounding sphere: in exact arithmetic the box rectangle is the smaller one
// already -- |M^-1|_F alone overstates an orthonormal camera's sphere by sqrt 3), where it marks nothing so does this, so
// the marks are a subset of the sphere rule's for every box and camera whatever the rounding.  (The sphere is the box's own:
// a cell's bounds lie inside its cube, so their box rectangle lies inside the cube's and inside the cube's sphere rectangle
// in exact arithmetic, and the sphere's 0.1 % and |M^-1|_F are far more than the rounding.)  (Pixels are bit-identical with
// and without: tests/test_culling.py, tests/test_culling_cubes.py, and every parity test against the oracle, which marches
// every ray, runs with it.)
// One workgroup = kMarkCells cells of one frame, marked into a private copy of the frame's mask in LDS (LDS_MASK; a frame
// of more than kMarkLdsWords * 32 tiles marks straight into memory) that is OR-ed into the frame's mask once at the end:
// tens of thousands of cells land on a few hundred mask words, and device-scope atomics on one address serialise
// (the first version, one global atomic per cell and tile, took 2.5 ms per 100 frames; this one 0.1).
constexpr int kMarkCells = 2048, kMarkLdsWords = 8192;
#ifndef RTO_MARK_PAD  // (A/B hook: the absolute pad in pixels; same pixels for every value >= 0.5)
#define RTO_MARK_PAD 0.5f
#endif
constexpr float kMarkPad = RTO_MARK_PAD;
template <class MarkFn>
RTO_DEV void mark_cell(const float4 cell, const float4 half, const TreeDev& tree, const FrameDesc& fd, const FrameBatch& fb, MarkFn mark);
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
            mark_cell(tree.occ_cells[2 * c], tree.occ_cells[2 * c + 1], tree, fd, fb, [&](uint32_t w, uint32_t bits) { atomicOr(&s_mask[w], bits); });  // ds_or_b32
        else
            mark_cell(tree.occ_cells[2 * c], tree.occ_cells[2 * c + 1], tree, fd, fb, [&](uint32_t w, uint32_t bits) { atomicOr(gm + w, bits); });
    }
    if (LDS_MASK) {
        __syncthreads();
        for (int i = threadIdx.x; i < fb.mask_words; i += 256)
            if (s_mask[i]) atomicOr(gm + i, s_mask[i]);
    }
}

template <class MarkFn>
RTO_DEV void mark_cell(const float4 cell, const float4 half, const TreeDev& tree, const FrameDesc& fd, const FrameBatch& fb, MarkFn mark) {
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
    const float hw[3] = {half.x / fabsf(tree.scale[0]), half.y / fabsf(tree.scale[1]), half.z / fabsf(tree.scale[2])};
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
        const float bx0 = floorf((fminf(px0, px1) - kMarkPad) * 0.125f), bx1 = floorf((fmaxf(px0, px1) + kMarkPad) * 0.125f);
        const float by0 = floorf((fminf(py0, py1) - kMarkPad) * 0.125f), by1 = floorf((fmaxf(py0, py1) + kMarkPad) * 0.125f);
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
            mark_cell(tree.occ_cells[2 * c], tree.occ_cells[2 * c + 1], tree, fd, fb, [&](uint32_t w, uint32_t bits) { atomicOr(&s_mask[w], bits); });
        else
            mark_cell(tree.occ_cells[2 * c], tree.occ_cells[2 * c + 1], tree, fd, fb, [&](uint32_t w, uint32_t bits) { atomicOr(mask + w, bits); });
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

}  // namespace rto

// ------------------------------------------------------------------ host launchers (C++ linkage,
// declared in rto_launch.h)
#include "rto_dispatch.h"
#include "rto_launch.h"

namespace rto {

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
    bool depth_layer = false;
    if constexpr (LAYERS) {
        depth_layer = layers && layers->depth;
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
    // the shading stage (shade_kernels.hip): over the colour layer where the launch carries one
    const hipError_t shaded = launch_shade(SPP, tree, opt, fb, hits, layers, stream);
    if (ev) (void)hipEventRecord(ev[3], stream);
    return shaded;
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

}  // namespace rto
