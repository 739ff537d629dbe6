// rto_render_abi.cpp -- the launch entries of the C ABI (include/rto.h): rto_launch_renderer (one frame),
// rto_launch_renderer_batch (n frames in one launch of the persistent kernels) and rto_launch_rays / rto_launch_rays_ex, built
// from one set of refusals and one set-up.  Every refusal for a call's arguments comes before the first change to the context.
#include <algorithm>
#include <cstring>

#include "rto_internal.h"

namespace {

int ensure_jump_table(rto_ctx* c) {
    if (c->jump_valid && c->jump_inc == c->rng.inc) return RTO_OK;
    std::vector<rto::PcgJumpEntry> tab(4 * 256);
    for (int ch = 0; ch < 4; ++ch)
        for (int j = 0; j < 256; ++j) tab[ch * 256 + j] = pcg_jump(c->rng.inc, (uint64_t)j << (8 * ch));
    if (!c->jump) HIP_TRY(hipMalloc((void**)&c->jump, tab.size() * sizeof(rto::PcgJumpEntry)));
    // synchronous copy from a stack-lifetime vector; happens once per `inc`
    HIP_TRY(hipMemcpy(c->jump, tab.data(), tab.size() * sizeof(rto::PcgJumpEntry), hipMemcpyHostToDevice));
    c->jump_inc = c->rng.inc;
    c->jump_valid = true;
    return RTO_OK;
}

// ---- refusals ----

// what every launch asks of (tree, options, context)
int check_tree_options(const rto_tree* tree, const rto_options* o, const rto_ctx* ctx) {
    if (!spp_supported(o->spp))  // volrend.cu:275-277
        return set_err(RTO_E_SPP, "spp == " + std::to_string(o->spp) + " not supported. (supported: 1,2,3,4,6,8,16,32)");
    if (tree->device != ctx->device) return set_err(RTO_E_INVALID, "tree and context live on different devices");
    if (tree->d_recidx && !(o->sigma_thresh >= 0.f))
        return set_err(RTO_E_UNSUPPORTED, "a tree loaded with RTO_TREE_COMPACT_RECORDS keeps coefficient records for leaves of positive "
                                          "density only: sigma_thresh must be >= 0");
    if (missing_lobes(tree)) return set_err(RTO_E_FORMAT, missing_lobes_msg);
    return RTO_OK;
}

int check_camera(const rto_camera& cam, const rto_ctx* ctx) {
    if (cam.width != ctx->width || cam.height != ctx->height)
        return set_err(RTO_E_INVALID, "camera size does not match the render context");
    if (!(cam.fx != 0.f) || !(cam.fy != 0.f)) return set_err(RTO_E_INVALID, "camera focal length is zero");
    return RTO_OK;
}

// the layers of a launch whose first frame is context slot `slot0`, as the kernels take them; false: the context has none
bool ctx_layers_at(const rto_ctx* c, int slot0, rto::LayerDev* out) {
    if (!c->layer_depth && !c->layer_color) return false;
    const size_t off = (size_t)slot0 * frame_px(c);
    out->depth = c->layer_depth ? c->layer_depth + off : nullptr;
    out->color = c->layer_color ? reinterpret_cast<const float4*>(c->layer_color) + off : nullptr;
    return true;
}
int check_layers(const rto_tree* tree, const rto_ctx* ctx, bool layered) {
    if (layered && ctx->stats_on)
        return set_err(RTO_E_UNSUPPORTED, "layers (rto_ctx_set_layers) and work counters (rto_ctx_enable_stats) do not combine");
    if (layered && tree->quant)
        return set_err(RTO_E_UNSUPPORTED, "a quantised tree loaded with RTO_TREE_QUANT_DIRECT takes no layers (rto_ctx_set_layers): expand it");
    return RTO_OK;
}

// the depth outputs of a launch into context slot `slot` (rto_ctx_enable_depth); false: the context keeps none
bool ctx_depth_at(const rto_ctx* c, int slot, rto::DepthOut* out) {
    if (!c->depth) return false;
    out->depth = c->depth + (size_t)slot * frame_px(c);
    out->t_near = c->t_near + (size_t)slot * frame_px(c);
    return true;
}
// what a context with depth outputs refuses: the set the layers refuse (the depth kernels are layered kernels)
int check_depth(const rto_tree* tree, const rto_options* o, const rto_ctx* ctx) {
    if (!ctx->depth) return RTO_OK;
    if (ctx->stats_on)
        return set_err(RTO_E_UNSUPPORTED, "depth outputs (rto_ctx_enable_depth) and work counters (rto_ctx_enable_stats) do not combine");
    if (tree->quant)
        return set_err(RTO_E_UNSUPPORTED, "a quantised tree loaded with RTO_TREE_QUANT_DIRECT renders no depth outputs (rto_ctx_enable_depth): expand it");
    if (o->enable_probe) return set_err(RTO_E_UNSUPPORTED, "enable_probe on a context with depth outputs (rto_ctx_enable_depth) is not built");
    return RTO_OK;
}

// enable_probe (volrend.cu:100-134, 244-251): what a frame launch checks before it renders ...
int probe_check(const rto_tree* tree, const rto_options* o, const rto_ctx* ctx, bool layered) {
    // (pinned by the suite rather than principled: the overlay would work over layers too)
    if (layered) return set_err(RTO_E_UNSUPPORTED, "enable_probe over a context with layers (rto_ctx_set_layers) is not built");
    if (ctx->stats_on) return set_err(RTO_E_UNSUPPORTED, "enable_probe and work counters (rto_ctx_enable_stats) do not combine");
    if (tree->quant)
        return set_err(RTO_E_UNSUPPORTED, "enable_probe reads a leaf's coefficients: not with a quantised tree loaded with RTO_TREE_QUANT_DIRECT");
    if (o->probe_disp_size <= 0) return set_err(RTO_E_INVALID, "enable_probe: probe_disp_size must be > 0");
    int walk;
    rto::ValuesSrc vs;
    return query_plan(tree, true, &walk, &vs);
}

// ... and what it launches behind its render kernels: the probe point's coefficients into the context's buffer, then the disc
// over every output the launch wrote -- frame f = table[f] (device), or the one descriptor `one`
int draw_probe(const rto_tree* tree, const rto_options* o, rto_ctx* ctx, hipStream_t stream, const rto::FrameDesc* table,
               const rto::FrameDesc* one, int frames, int lean) {
    int walk;
    rto::ValuesSrc vs;
    int rc = query_plan(tree, true, &walk, &vs);
    if (rc != RTO_OK) return rc;
    hipError_t e = rto::launch_probe_fetch(tree->dev, walk, vs, o->probe, ctx->probe_coeffs, kProbeFloats, stream);
    if (e == hipSuccess) {
        rto::OptDev od = make_opt_dev(o);
        od.rot_on = 0;  // the probe's basis is evaluated at the unrotated direction (volrend.cu:114-116)
        rto::ProbeDraw pd;
        std::memset(&pd, 0, sizeof(pd));
        pd.width = ctx->width;
        pd.height = ctx->height;
        pd.disp = o->probe_disp_size;
        pd.lean = lean;
        pd.table = table;
        if (one) pd.one = *one;
        e = rto::launch_probe_overlay(tree->dev, od, pd, frames, ctx->probe_coeffs, stream);
    }
    if (e != hipSuccess) return set_err(RTO_E_HIP, std::string("probe launch failed: ") + hipGetErrorString(e));
    return RTO_OK;
}

// ---- set-up ----

// AUTO / FAST / GENERIC for a frame or ray launch; *tdev = the tree as the fast kernel takes it at this SPP (fast_path_for_spp)
int choose_kernel(const rto_tree* tree, const rto_options* o, const rto_ctx* ctx, int* kernel, rto::TreeDev* tdev) {
    const bool fast_here = fast_path_for_spp(tree, o->spp, ctx->test_wide_bits, tdev) != 0;
    *kernel = ctx->kernel != RTO_KERNEL_AUTO ? ctx->kernel : fast_here ? RTO_KERNEL_FAST : RTO_KERNEL_GENERIC;
    if (*kernel == RTO_KERNEL_FAST && !fast_here)
        return set_err(RTO_E_UNSUPPORTED, "fast kernel needs an N == 2 tree of depth <= 24 whose leaf slots fit 31 - ceil(log2 spp) bits "
                                          "(2^28 slots at spp <= 8, 2^26 at spp 32: a hit entry is {valid bit, count - 1, slot})");
    return RTO_OK;
}

// ctx.rng advanced by delta draws: frame f of a batch starts at (its jump count) << 32, as after that many ctx.rng.advance()
// of the reference's frame loop (main_headless.cpp:494-506); a ray at (its index) * spp
rto::Pcg32 rng_after(const rto_ctx* ctx, uint64_t delta) {
    const rto::PcgJumpEntry j = pcg_jump(ctx->rng.inc, delta);
    return {j.mult * ctx->rng.state + j.plus, ctx->rng.inc};
}
uint64_t frame_jump(const int64_t* rng_jumps, int f) { return (uint64_t)(rng_jumps ? rng_jumps[f] : (int64_t)f) << 32; }

// where frame slot `slot` goes (volrend.cu:206: the noisy image when the denoiser runs behind); no counters, no marks
rto::FrameOut frame_out(const rto_ctx* ctx, int slot, bool denoise) {
    rto::FrameOut fo = {};
    fo.aux = ctx->aux + (size_t)slot * RTO_AUX_CHANNELS * frame_px(ctx);
    fo.image = (denoise ? ctx->noisy : ctx->image) + (size_t)slot * 4 * frame_px(ctx);
    return fo;
}

int tiles_of(const rto_ctx* ctx) { return ((ctx->width + 7) / 8) * ((ctx->height + 7) / 8); }  // 8x8-pixel ray tiles of a frame
int mask_words_of(const rto_ctx* ctx) { return (tiles_of(ctx) + 31) / 32 + 1; }                // (+1: the keep-all word)

// The context's tile marks ([frames][mask_words]) and, with chunks_cap > 0, the queue lists of a batched launch.  A single
// frame that culls asks for marks only (chunks_cap 0) and leaves q_chunks_cap at 0: a later batched launch sizes its lists.
int ensure_tile_buffers(rto_ctx* ctx, int mask_words, int chunks_cap) {
    if (ctx->tile_mask && ctx->mask_words == mask_words && ctx->q_chunks_cap >= chunks_cap) return RTO_OK;
    if (ctx->tile_mask) {
        HIP_TRY(hipDeviceSynchronize());
        for (void* p : {(void*)ctx->tile_mask, (void*)ctx->qlist, (void*)ctx->qscratch}) HIP_TRY(hipFree(p));
        ctx->tile_mask = ctx->qlist = ctx->qscratch = nullptr;
    }
    ctx->q_chunks_cap = 0;
    HIP_TRY(hipMalloc((void**)&ctx->tile_mask, (size_t)ctx->frames * mask_words * sizeof(uint32_t)));
    ctx->mask_words = mask_words;
    if (chunks_cap > 0) {
        HIP_TRY(hipMalloc((void**)&ctx->qlist, (size_t)tiles_of(ctx) * ctx->frames * sizeof(uint32_t)));
        HIP_TRY(hipMalloc((void**)&ctx->qscratch, ((size_t)2 * chunks_cap + rto::kMaxQueues) * sizeof(uint32_t)));
        ctx->q_chunks_cap = chunks_cap;
    }
    return RTO_OK;
}

// One frame through `kernel` to where fo says, over `layers` (nullptr: none), its depth outputs to `depth` (nullptr: none kept),
// the probe's disc on top when the options ask.
// tree_dev: the tree as that kernel takes it (choose_kernel's for the fast kernel, tree->dev itself for the generic one, whose
// child[] / data[] ensure_reference_arrays may just have rebuilt)
int render_frame(const rto_tree* tree, const rto::TreeDev& tree_dev, int kernel, const rto::CamDev& cd, const rto_options* o,
                 const rto::OptDev& od, const rto::Pcg32& rng, const rto::FrameOut& fo, const rto::LayerDev* layers,
                 const rto::DepthOut* depth, rto_ctx* ctx, hipStream_t stream) {
    const hipError_t e = rto::launch_render(kernel, o->spp, tree_dev, cd, od, rng, ctx->jump, fo, ctx->strip_rows, layers, depth, stream);
    if (e != hipSuccess) return set_err(RTO_E_HIP, std::string("render launch failed: ") + hipGetErrorString(e));
    if (!o->enable_probe) return RTO_OK;
    rto::FrameDesc one = {};
    std::memcpy(one.transform, cd.transform, sizeof(one.transform));
    one.aux = fo.aux;
    one.image = fo.image;
    return draw_probe(tree, o, ctx, stream, nullptr, &one, 1, 0);
}

// The frames of a batched call rendered one by one with the generic kernel (render_generic: any N, any depth, any slot
// count): what rto_launch_renderer_batch does for a tree the batched kernels cannot take.  The generic kernel reads the
// reference arrays child[] / data[], which a dense SH9 / SH16 upload released: they are rebuilt first.
// No tile marks exist afterwards (marks_n stays 0: the denoise stage must not fill "culled" tiles from an older launch),
// and the slots hold full outputs.  The caller has checked the cameras.
int generic_frames(const rto_tree* tree, const rto_camera* cams, const int64_t* rng_jumps, int n, const rto_options* o,
                   rto_ctx* ctx, hipStream_t stream, int slot0) {
    if (tree->quant)
        return set_err(RTO_E_UNSUPPORTED, "a quantised tree kept quantised cannot take the generic kernel (too many leaf slots for the "
                                          "batched kernels at this spp, or the traversal kernel's LDS was refused)");
    ctx->marks_n = 0;
    for (int f = 0; f < n; ++f) ctx->lean_slot[(size_t)(slot0 + f)] = 0;
    int rc = ensure_reference_arrays(tree);
    if (rc != RTO_OK) return rc;
    const rto::OptDev od = make_opt_dev(o);
    for (int f = 0; f < n; ++f) {
        rto::LayerDev layers;
        const bool layered = ctx_layers_at(ctx, slot0 + f, &layers);
        rc = render_frame(tree, tree->dev, RTO_KERNEL_GENERIC, cam_dev(cams[f]), o, od, rng_after(ctx, frame_jump(rng_jumps, f)),
                          frame_out(ctx, slot0 + f, o->denoise), layered ? &layers : nullptr, nullptr, ctx, stream);
        if (rc != RTO_OK) return rc;
    }
    return RTO_OK;
}

// The frames of a batched call on a context with depth outputs, one by one through the single-frame depth kernels: frame f into
// slot slot0 + f with the RNG of a batch's frame f -- the bytes of n single launches.  The route of rto_ctx_enable_depth(1), and of
// RTO_DEPTH_BATCHED for a launch the persistent kernels cannot take.  As after generic_frames: no tile marks, full outputs.  The
// caller has checked the cameras and the lean level.
int depth_frames(const rto_tree* tree, const rto_camera* cams, const int64_t* rng_jumps, int n, const rto_options* o, rto_ctx* ctx,
                 hipStream_t stream, int slot0) {
    int kernel;
    rto::TreeDev tdev;
    int rc = choose_kernel(tree, o, ctx, &kernel, &tdev);
    if (rc != RTO_OK) return rc;
    const bool fast = kernel == RTO_KERNEL_FAST;
    ctx->marks_n = 0;
    for (int f = 0; f < n; ++f) ctx->lean_slot[(size_t)(slot0 + f)] = 0;
    rc = fast ? ensure_jump_table(ctx) : ensure_reference_arrays(tree);
    if (rc != RTO_OK) return rc;
    const rto::OptDev od = make_opt_dev(o);
    for (int f = 0; f < n; ++f) {
        rto::LayerDev layers;
        const bool layered = ctx_layers_at(ctx, slot0 + f, &layers);
        rto::DepthOut depth;
        ctx_depth_at(ctx, slot0 + f, &depth);
        rc = render_frame(tree, fast ? tdev : tree->dev, kernel, cam_dev(cams[f]), o, od, rng_after(ctx, frame_jump(rng_jumps, f)),
                          frame_out(ctx, slot0 + f, o->denoise), layered ? &layers : nullptr, &depth, ctx, stream);
        if (rc != RTO_OK) return rc;
    }
    return RTO_OK;
}

// every refusal of a batched call for its arguments (frames 0..n-1 -> slots slot0..); batched: the persistent kernels take it
int check_batch(const rto_tree* tree, const rto_camera* cams, int n, const rto_options* o, const rto_ctx* ctx, int slot0,
                bool batched) {
    if (n < 1 || slot0 < 0 || slot0 + n > ctx->frames)
        return set_err(RTO_E_INVALID, "rto_launch_renderer_batch: n exceeds the context's frame slots");
    int rc = check_tree_options(tree, o, ctx);
    if (rc != RTO_OK) return rc;
    rto::LayerDev layers;
    const bool layered = ctx_layers_at(ctx, slot0, &layers);
    if (o->enable_probe) {
        rc = probe_check(tree, o, ctx, layered);
        if (rc != RTO_OK) return rc;
        // sparse lean outputs store nothing for unmarked tiles because those are the constant background -- the disc is not
        if (o->denoise && ctx->lean == 2)
            return set_err(RTO_E_UNSUPPORTED, "sparse lean outputs (rto_ctx_set_lean_outputs level 2) need a constant backdrop: not with enable_probe");
    }
    rc = check_layers(tree, ctx, layered);
    if (rc != RTO_OK) return rc;
    rc = check_depth(tree, o, ctx);
    if (rc != RTO_OK) return rc;
    if (ctx->depth && ctx->lean != 0 && ctx->depth_mode != RTO_DEPTH_BATCHED)  // (the single-frame kernels the frames go through store full outputs)
        return set_err(RTO_E_UNSUPPORTED, "a context with depth outputs (rto_ctx_enable_depth) renders its batches frame by frame: lean "
                                          "outputs (rto_ctx_set_lean_outputs) must be off");
    if (ctx->depth && ctx->lean != 0 && !batched)  // (RTO_DEPTH_BATCHED, and the launch is known to go frame by frame all the same)
        return set_err(RTO_E_UNSUPPORTED, "the persistent kernels cannot take this launch (no traversal image, too many leaf slots at this "
                                          "spp, or tuning key batch_fallback): a context with depth outputs renders it frame by frame, and "
                                          "lean outputs (rto_ctx_set_lean_outputs) must be off");
    // sparse lean outputs store nothing for unmarked tiles because those are the constant background -- not over a colour layer
    if (layered && layers.color && o->denoise && ctx->lean == 2)
        return set_err(RTO_E_UNSUPPORTED, "sparse lean outputs (rto_ctx_set_lean_outputs level 2) need a constant backdrop: not with a colour "
                                          "layer (rto_ctx_set_layers)");
    for (int f = 0; f < n; ++f) {
        rc = check_camera(cams[f], ctx);
        if (rc != RTO_OK) return rc;
    }
    if (!batched) return RTO_OK;
    // the traversal kernel addresses the hand-off buffer with 32-bit offsets (frame * spp * pixels + pixel)
    if ((uint64_t)(slot0 + n) * (uint64_t)o->spp * (uint64_t)frame_px(ctx) > 0xffffffffULL)
        return set_err(RTO_E_UNSUPPORTED, "frames x spp x pixels exceeds 2^32 hit-list entries: render fewer frames per launch");
    if ((ctx->width + 7) / 8 > 1023 || (ctx->height + 7) / 8 > 1023)
        return set_err(RTO_E_UNSUPPORTED, "the batched path packs tile coordinates into 10 bits: frames up to 8184 x 8184 pixels");
    return RTO_OK;
}

// the ray queues of a batch of n frames (FrameBatch): tile order, queue starts, the chunks of the queue compaction and, from the
// context's buffers (ensure_tile_buffers), tile marks and lists
int queue_layout(rto_ctx* ctx, int n, rto::FrameBatch* fb) {
    const int tiles = tiles_of(ctx);
    fb->tile_major = ctx->tile_major ? 1 : 0;
    if (ctx->tile_order_on && ctx->xcd_queues) {  // one queue per XCD over an image wedge each
        fb->tile_order = ctx->wedge_order;
        fb->n_queues = rto::kMaxQueues;
        for (int k = 0; k <= rto::kMaxQueues; ++k) fb->qstart[k] = ctx->wedge_start[k];
    } else {  // one queue over whole frames (centre-out or row-major tiles)
        fb->tile_order = ctx->tile_order_on ? ctx->tile_order : nullptr;
        fb->n_queues = 1;
        fb->qstart[0] = 0;
        for (int k = 1; k <= rto::kMaxQueues; ++k) fb->qstart[k] = tiles;
    }
    fb->qchunk[0] = 0;
    for (int k = 0; k < rto::kMaxQueues; ++k) {
        const int64_t slots = k < fb->n_queues ? (int64_t)(fb->qstart[k + 1] - fb->qstart[k]) * n : 0;
        fb->qchunk[k + 1] = fb->qchunk[k] + (int)((slots + rto::kQueueChunk - 1) / rto::kQueueChunk);
    }
    const int chunks_cap = (int)(((int64_t)tiles * ctx->frames + rto::kQueueChunk - 1) / rto::kQueueChunk) + rto::kMaxQueues;
    const int rc = ensure_tile_buffers(ctx, mask_words_of(ctx), chunks_cap);
    if (rc != RTO_OK) return rc;
    fb->tile_mask = ctx->tile_mask;
    fb->mask_words = ctx->mask_words;
    fb->qlist = ctx->qlist;
    fb->chunk_count = ctx->qscratch;
    fb->chunk_base = ctx->qscratch + ctx->q_chunks_cap;
    fb->qcount = ctx->qscratch + 2 * (size_t)ctx->q_chunks_cap;
    return RTO_OK;
}

// frames 0..n-1 of the batch land in context slots slot0..slot0+n-1
int launch_batch_at(const rto_tree* tree, const rto_camera* cams, const int64_t* rng_jumps, int n, const rto_options* o,
                    rto_ctx* ctx, void* stream_, int slot0) {
    if (!tree || !cams || !o || !ctx) return set_err(RTO_E_INVALID, "rto_launch_renderer_batch: null argument");
    // No traversal image (N != 2, depth > 24, >= 2^29 leaf slots: the top-grid entry's budget) or more slots than a
    // hit-list entry can name at this SPP (2^28 at spp <= 8, 2^26 at spp 32): the same frames, one launch of the
    // generic kernel each -- same images, without the batching gain.
    rto::TreeDev tdev;
    // A context with depth outputs: frame by frame through the single-frame depth kernels (depth_frames) -- unless it was enabled
    // with RTO_DEPTH_BATCHED, whose batches take the persistent kernels like any other (render_persist_depth for the traversal)
    // and depth_frames, not generic_frames, where those cannot take the launch.
    const bool depth_batched = ctx->depth && ctx->depth_mode == RTO_DEPTH_BATCHED;
    const bool batched = spp_supported(o->spp) && fast_path_for_spp(tree, o->spp, ctx->test_wide_bits, &tdev) != 0 &&
                         ctx->batch_fallback != 1 && (!ctx->depth || depth_batched);
    int rc = check_batch(tree, cams, n, o, ctx, slot0, batched);
    if (rc != RTO_OK) return rc;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    hipStream_t stream = (hipStream_t)stream_;
    if (ctx->depth && !batched) return depth_frames(tree, cams, rng_jumps, n, o, ctx, stream, slot0);
    if (!batched) return generic_frames(tree, cams, rng_jumps, n, o, ctx, stream, slot0);

    ctx->marks_n = 0;  // whatever happens below, the tile marks of an earlier launch no longer describe this context's frames
    for (int f = 0; f < n; ++f) ctx->lean_slot[(size_t)(slot0 + f)] = 0;  // (set again below if this launch stores lean)
    const size_t px = frame_px(ctx);
    if (ctx->hits_spp < o->spp) {  // grow the hit-list buffer (first use, or a larger spp); stream-ordered free
        if (ctx->hits) {
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(hipFree(ctx->hits));
            ctx->hits = nullptr;
        }
        HIP_TRY(hipMalloc((void**)&ctx->hits, (size_t)ctx->frames * o->spp * px * sizeof(uint32_t)));
        ctx->hits_spp = o->spp;
    }
    rto::FrameBatch fb;
    std::memset(&fb, 0, sizeof(fb));
    fb.n = n;
    fb.width = ctx->width;
    fb.height = ctx->height;
    rc = queue_layout(ctx, n, &fb);
    if (rc != RTO_OK) return rc;
    ctx->last_n_queues = fb.n_queues;
    ctx->last_slots = (int64_t)tiles_of(ctx) * n;
    // Rays that provably never meet density are not marched (see mark_tiles_kernel): needs the tree's culling cells, a
    // non-negative density threshold (a hit needs sigma > sigma_thresh, rt_core.cuh:252) and straight world-space rays
    // (the NDC warp of LLFF scenes bends them: maybe_world2ndc, volrend.cu:35-56)
    const bool cull = ctx->cull_on && tree->dev.occ_cells && o->sigma_thresh >= 0.f && !(tree->dev.ndc_width > 0.f);
    if (ctx->cull_cubes && tree->d_occ_cubes) tdev.occ_cells = (const float4*)tree->d_occ_cubes;
    rto::FrameDesc frames[rto::kMaxBatch];
    fb.f = ctx->d_frames;
    fb.lean = o->denoise ? ctx->lean : 0;
    for (int f = 0; f < n; ++f) {
        rto::FrameDesc& d = frames[f];
        d.fx = cams[f].fx;
        d.fy = cams[f].fy;
        std::memcpy(d.transform, cams[f].transform, sizeof(d.transform));
        const rto::Pcg32 rng = rng_after(ctx, frame_jump(rng_jumps, f));
        d.rng_state = rng.state;
        d.rng_inc = rng.inc;
        const rto::FrameOut fo = frame_out(ctx, slot0 + f, o->denoise);
        d.aux = fo.aux;
        d.image = fo.image;
        d.hits = ctx->hits + (size_t)(slot0 + f) * o->spp * px;
    }
    rc = ensure_jump_table(ctx);
    if (rc != RTO_OK) return rc;
    const rto::OptDev od = make_opt_dev(o);
    HIP_TRY(rto::launch_write_frames(frames, n, ctx->d_frames, stream));
    hipEvent_t* ev = nullptr;
    if (ctx->kt_on && ctx->kt_count < kKtRing) ev = &ctx->kt_ev[(size_t)ctx->kt_count++ * 4];
    ctx->occ.force_lds_refusal = ctx->batch_fallback == 2;
    rto::LayerDev layers;
    const bool layered = ctx_layers_at(ctx, slot0, &layers);  // (batch frame f = slot slot0 + f reads plane slot0 + f)
    rto::DepthOut dout;  // (batch frame f = slot slot0 + f writes plane slot0 + f)
    const bool with_depth = ctx_depth_at(ctx, slot0, &dout);
    hipError_t e = rto::launch_render_batch(o->spp, tdev, od, fb, ctx->jump, ctx->queue,
                                            frames[0].hits,  // the kernel indexes frames from here
                                            ctx->num_cus, ctx->refill, cull, &ctx->occ, ev, layered ? &layers : nullptr,
                                            with_depth ? &dout : nullptr, stream);
    if (ctx->occ.lds_refused) {
        if (ev) --ctx->kt_count;  //  nothing was launched, nothing recorded the slot's events: give it back
        if (with_depth) {  // (RTO_DEPTH_BATCHED) frame by frame through the single-frame depth kernels, which store full outputs
            if (ctx->lean != 0)
                return set_err(RTO_E_UNSUPPORTED, "the device refused the LDS the batched traversal kernel needs: a context with depth outputs "
                                                  "renders this launch frame by frame, and lean outputs (rto_ctx_set_lean_outputs) must be off");
            return depth_frames(tree, cams, rng_jumps, n, o, ctx, stream, slot0);
        }
        // the device does not grant a workgroup the LDS the traversal kernel needs for this depth x SPP x frame count
        // ((max_depth + 1 - top_levels + spp + 1) KB for the ancestor stack and thresholds + 56 B per frame); nothing but
        // the frame table was written so far: the same frames through the generic kernel, frame by frame
        return generic_frames(tree, cams, rng_jumps, n, o, ctx, stream, slot0);
    }
    if (e != hipSuccess) return set_err(RTO_E_HIP, std::string("batched render launch failed: ") + hipGetErrorString(e));
    if (o->enable_probe) {
        rc = draw_probe(tree, o, ctx, stream, ctx->d_frames, nullptr, n, fb.lean);
        if (rc != RTO_OK) return rc;
    }
    // Over a colour layer an unmarked tile's pixels are not the constant background the marks' consumers take them for (the
    // launch culled its marching with them, and rto_ctx_tile_marks / rto_denoise then see none), nor are the disc's pixels: a
    // launch with the probe leaves no marks either
    ctx->marks_n = (layered && layers.color) || o->enable_probe ? 0 : n;
    ctx->marks_slot0 = slot0;
    ctx->marks_bg = o->background_brightness;
    if (fb.lean)
        for (int f = 0; f < n; ++f) ctx->lean_slot[(size_t)(slot0 + f)] = (uint8_t)fb.lean;
    return RTO_OK;
}

}  // namespace

extern "C" {

int rto_launch_renderer(const rto_tree* tree, const rto_camera* cam, const rto_options* o, rto_ctx* ctx, void* stream_) {
    if (!tree || !cam || !o || !ctx) return set_err(RTO_E_INVALID, "rto_launch_renderer: null argument");
    rto::LayerDev layers;
    const bool layered = ctx_layers_at(ctx, ctx->sel, &layers);  // (a single-frame launch reads the selected slot's planes)
    int rc = check_layers(tree, ctx, layered);
    if (rc == RTO_OK) rc = check_depth(tree, o, ctx);
    if (rc != RTO_OK) return rc;
    if (tree->quant) {  // codebook shading lives in the batched kernels: a batch of one into the selected slot
        if (ctx->kernel == RTO_KERNEL_GENERIC || ctx->stats_on)
            return set_err(RTO_E_UNSUPPORTED, "a quantised tree loaded with RTO_TREE_QUANT_DIRECT has no generic kernel / work counters");
        return launch_batch_at(tree, cam, nullptr, 1, o, ctx, stream_, ctx->sel);
    }
    rc = check_tree_options(tree, o, ctx);
    if (rc == RTO_OK) rc = check_camera(*cam, ctx);
    if (rc == RTO_OK && o->enable_probe) rc = probe_check(tree, o, ctx, layered);
    int kernel;
    rto::TreeDev tdev;
    if (rc == RTO_OK) rc = choose_kernel(tree, o, ctx, &kernel, &tdev);
    if (rc != RTO_OK) return rc;
    const bool fast = kernel == RTO_KERNEL_FAST;
    if (fast && ctx->frame_via_batch && ctx->kernel == RTO_KERNEL_AUTO && !ctx->stats_on && !ctx->depth)
        return launch_batch_at(tree, cam, nullptr, 1, o, ctx, stream_, ctx->sel);

    DeviceGuard guard(ctx->device);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    hipStream_t stream = (hipStream_t)stream_;
    rc = fast ? ensure_jump_table(ctx) : ensure_reference_arrays(tree);  // (the latter a no-op unless the upload released them)
    if (rc != RTO_OK) return rc;
    const rto::CamDev cd = cam_dev(*cam);
    rto::FrameOut fo = frame_out(ctx, ctx->sel, o->denoise);
    // Empty-space culling for the single-frame kernel as well (round 4, VERDICT r3 task 6): one small kernel projects the
    // tree's culling cells into this camera (same bound and premises as the batched path, see launch_batch_at), and the
    // waves of unmarked 8x8 tiles write the background without ray set-up, threshold draws or marching.  The marks stay
    // on the context for the denoise stage (rto_ctx_tile_marks), like after a batched launch.
    // (not with the probe: its disc is no background, so the launch would leave marks nobody may use)
    const bool cull_one = fast && !ctx->stats_on && ctx->cull_on && ctx->cull_single && tree->dev.occ_cells &&
                          o->sigma_thresh >= 0.f && !(tree->dev.ndc_width > 0.f) && !o->enable_probe;
    if (cull_one) {
        rc = ensure_tile_buffers(ctx, mask_words_of(ctx), 0);
        if (rc != RTO_OK) return rc;
        if (ctx->cull_cubes && tree->d_occ_cubes) tdev.occ_cells = (const float4*)tree->d_occ_cubes;
        HIP_TRY(rto::launch_mark_tiles_one(tdev, cd, ctx->tile_mask, ctx->mask_words, stream));
        fo.cull_marks = ctx->tile_mask;
        fo.cull_mask_words = ctx->mask_words;
    }
    bool keep_marks = false;
    if (ctx->stats_on) {
        if (!fast) return set_err(RTO_E_UNSUPPORTED, "work counters need the fast kernel");
        fo.stats = ctx->stats;
        if (ctx->stats_marks) {  // the selected slot's marks of the last batched launch (the caller re-renders that frame)
            if (ctx->marks_n < 1 || !ctx->tile_mask || ctx->sel < ctx->marks_slot0 || ctx->sel >= ctx->marks_slot0 + ctx->marks_n)
                return set_err(RTO_E_INVALID, "rto_ctx_enable_stats(2): the selected frame slot holds no tile marks of a batched launch");
            fo.stat_marks = ctx->tile_mask + (size_t)(ctx->sel - ctx->marks_slot0) * ctx->mask_words;
            fo.stat_mask_words = ctx->mask_words;
            keep_marks = true;  // (the counting launch re-renders the frame the marks describe)
        }
    }
    if (!keep_marks) ctx->marks_n = 0;  // (the generic kernel and the counting instantiation mark no tiles)
    ctx->lean_slot[(size_t)ctx->sel] = 0;  // (a single frame has full outputs; the other slots keep what they hold)
    rto::DepthOut depth;
    const bool with_depth = ctx_depth_at(ctx, ctx->sel, &depth);
    rc = render_frame(tree, fast ? tdev : tree->dev, kernel, cd, o, make_opt_dev(o), ctx->rng, fo, layered ? &layers : nullptr,
                      with_depth ? &depth : nullptr, ctx, stream);
    if (rc != RTO_OK) return rc;
    // (over a colour layer an unmarked tile is not the constant background: the marks are kept from the denoise stage)
    if (cull_one && !(layered && layers.color)) {  // the selected slot's marks, for rto_ctx_tile_marks / the culled denoise stage
        ctx->marks_n = 1;
        ctx->marks_slot0 = ctx->sel;
        ctx->marks_bg = o->background_brightness;
    }
    return RTO_OK;
}

int rto_launch_renderer_batch(const rto_tree* tree, const rto_camera* cams, const int64_t* rng_jumps, int n,
                              const rto_options* o, rto_ctx* ctx, void* stream_) {
    return launch_batch_at(tree, cams, rng_jumps, n, o, ctx, stream_, 0);
}

int rto_launch_rays(const rto_tree* tree, const rto_rays* rays, const rto_options* o, rto_ctx* ctx, float* out, void* stream_) {
    if (!out) return set_err(RTO_E_INVALID, "rto_launch_rays: null argument");
    const rto_rays_out ro = {out, nullptr, nullptr};
    return rto_launch_rays_ex(tree, rays, o, ctx, &ro, stream_);
}

// (with only rgba asked for, the launches below are rto_launch_rays': the same kernels with the same arguments)
int rto_launch_rays_ex(const rto_tree* tree, const rto_rays* rays, const rto_options* o, rto_ctx* ctx, const rto_rays_out* ro,
                       void* stream_) {
    if (!tree || !rays || !o || !ctx || !ro) return set_err(RTO_E_INVALID, "rto_launch_rays: null argument");
    if (!ro->rgba && !ro->depth && !ro->t_near) return set_err(RTO_E_INVALID, "rto_launch_rays_ex: no output asked for");
    if (rays->n < 0 || rays->first_ray < 0) return set_err(RTO_E_INVALID, "rto_launch_rays: n and first_ray must be >= 0");
    if (rays->n > 0 && (!rays->origins || !rays->dirs)) return set_err(RTO_E_INVALID, "rto_launch_rays: null origins / dirs");
    if ((uintptr_t)ro->rgba % 16 != 0) return set_err(RTO_E_INVALID, "rto_launch_rays: out must be 16-byte aligned");
    if ((uintptr_t)ro->depth % 4 != 0 || (uintptr_t)ro->t_near % 4 != 0)
        return set_err(RTO_E_INVALID, "rto_launch_rays_ex: depth and t_near must be 4-byte aligned");
    float* const out = ro->rgba;
    const bool with_depth = ro->depth || ro->t_near;
    if (tree->quant)
        return set_err(RTO_E_UNSUPPORTED, "a quantised tree loaded with RTO_TREE_QUANT_DIRECT is shaded by the batched kernels only: "
                                          "rto_launch_rays needs an expanded tree");
    int rc = check_tree_options(tree, o, ctx);
    if (rc != RTO_OK) return rc;
    if (o->enable_probe) return set_err(RTO_E_UNSUPPORTED, "enable_probe draws into a frame's corner: caller-supplied rays have no frame");
    int kernel;
    rto::TreeDev tdev;
    rc = choose_kernel(tree, o, ctx, &kernel, &tdev);
    if (rc != RTO_OK) return rc;
    if (rays->n == 0) return RTO_OK;

    DeviceGuard guard(ctx->device);
    if (!guard.ok) return set_err(RTO_E_HIP, "hipSetDevice failed");
    hipStream_t stream = (hipStream_t)stream_;
    const bool fast = kernel == RTO_KERNEL_FAST;
    rc = fast ? ensure_jump_table(ctx) : ensure_reference_arrays(tree);  // (once per RNG stream / tree)
    if (rc != RTO_OK) return rc;
    const rto::OptDev od = make_opt_dev(o);
    // a launch takes fewer than 2^32 / spp rays (the kernels' RNG offset i * spp is 32-bit; the grid's last blocks stay below 2^32 too)
    const int64_t per_launch = (int64_t)((0xffffffffull / (uint64_t)o->spp - 4096) & ~255ull);
    for (int64_t i0 = 0; i0 < rays->n; i0 += per_launch) {
        rto::RayBatch rb;
        rb.origins = rays->origins + 3 * i0;
        rb.dirs = rays->dirs + 3 * i0;
        rb.t_max = rays->t_max ? rays->t_max + i0 : nullptr;
        rb.background = rays->background ? rays->background + 3 * i0 : nullptr;
        rb.out = out ? reinterpret_cast<float4*>(out) + i0 : nullptr;
        const rto::DepthOut depth = {ro->depth ? ro->depth + i0 : nullptr, ro->t_near ? ro->t_near + i0 : nullptr};
        rb.n = (uint32_t)std::min(per_launch, rays->n - i0);
        rb.per_xcd = 0;
        // ray i0 + i draws from ctx.rng advanced by (first_ray + i0 + i) * spp: the host takes (first_ray + i0) * spp (mod 2^64,
        // the generator's period), the kernel i * spp
        const rto::Pcg32 rng = rng_after(ctx, (uint64_t)(rays->first_ray + i0) * (uint64_t)o->spp);
        // (the generic kernel reads tree->dev itself: child[] / data[] may just have been rebuilt by ensure_reference_arrays)
        const hipError_t e = rto::launch_rays(kernel, o->spp, fast ? tdev : tree->dev, od, rng, ctx->jump, rb, with_depth ? &depth : nullptr,
                                              ctx->ray_order != 0, stream);
        if (e != hipSuccess) return set_err(RTO_E_HIP, std::string("ray launch failed: ") + hipGetErrorString(e));
    }
    return RTO_OK;
}

}  // extern "C"
