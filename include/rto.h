/*
 * rto.h -- C ABI of the MI355X-native RT-Octree render path (librto.so).
 *
 * Drop-in boundary for the reference's operator `volrend::launch_renderer` and the objects it
 * takes (reference paths are relative to /root/reference):
 *
 *   rto_tree      <- volrend::N3Tree            renderer/include/volrend/n3tree.hpp, src/n3tree.cpp:111-362,
 *                                               src/cuda/n3tree.cu:9-49   (tree.npz -> device arrays)
 *   rto_camera    <- internal::CameraSpec       renderer/include/volrend/internal/data_spec.hpp:11-24
 *   rto_options   <- volrend::RenderOptions     renderer/include/volrend/render_options.hpp:13-78
 *   rto_ctx       <- volrend::RenderContext     renderer/include/volrend/render_context.hpp:14-214
 *   rto_launch_renderer <- launch_renderer      renderer/include/volrend/cuda/renderer_kernel.hpp:11-16,
 *                                               src/cuda/volrend.cu:236-285
 *   rto_filtering <- denoiser::filtering        denoiser/extension/filtering.h:7-13, filtering.cu:701-717
 *   rto_ctx_download_rgba8 <- the u8 conversion renderer/main_headless.cpp:521-538
 *
 * Plain pointers and sizes only; no torch / HIP types in the signatures (streams are passed as
 * `void*` = hipStream_t, NULL = the default stream).  All device pointers returned by the
 * accessors are plain linear hipMalloc memory (the reference's cudaArray/surface/texture objects
 * are replaced by linear buffers with the same logical layout).
 *
 * Threading: handles are thread-compatible, not thread-safe -- one rto_ctx (and one rto_guidance_net) per host thread
 * and per stream at a time: a context owns the hand-off buffers, ray queues and frame table of the launch in flight,
 * and two batched launches of one context on different streams would share them.  Two more places hold lazily built,
 * shared state: (1) a tree whose upload released child[] / data[] (dense SH9 / SH16, the default) rebuilds them under a lock
 * at the FIRST launch that selects the generic kernel (rto_ctx_set_kernel(RTO_KERNEL_GENERIC), N != 2, the per-frame
 * fallback of a batched launch) -- make that first launch before other threads render the same tree, or load the tree with
 * RTO_TREE_KEEP_REFERENCE; (2) the *_culled denoise entry points measure the network's background tile once per background
 * brightness, synchronising the stream and rewriting the handle's copy of it -- work queued on ANOTHER stream with the
 * previous brightness must have finished (one network handle per stream, as above, makes that automatic).
 *
 * Error convention: every function returning int returns RTO_OK (0) or a negative RTO_E_* code;
 * rto_last_error() gives the message for the calling thread.  The library never calls exit()
 * (the reference does: src/cuda/common.cu:8-21) and never falls back to a CPU path: without a
 * usable HIP device every entry point that needs one fails with RTO_E_HIP.
 */
#ifndef RTO_H
#define RTO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTO_OK 0
#define RTO_E_INVALID -1     /* bad argument */
#define RTO_E_SPP -2         /* spp not in {1,2,3,4,6,8,16,32} (volrend.cu:266-278) */
#define RTO_E_UNSUPPORTED -3 /* a combination not built (e.g. SG/ASG + QUANT_DIRECT, enable_probe over layers) */
#define RTO_E_HIP -4         /* HIP runtime error / no device */
#define RTO_E_IO -5          /* file missing / malformed */
#define RTO_E_FORMAT -6      /* npz content violates the tree schema (n3tree.cpp:283-291,345) */

#define RTO_AUX_CHANNELS 8   /* render_context.hpp:23 */
#define RTO_BASIS_MAX 25     /* render_options.hpp:7 */

/* data_format.hpp:8-14 */
enum { RTO_FMT_RGBA = 0, RTO_FMT_SH = 1, RTO_FMT_SG = 2, RTO_FMT_ASG = 3 };

/* RenderOptions, field for field (render_options.hpp:13-78).  bools are ints. */
typedef struct rto_options {
    float step_size;              /* 1e-4 */
    float sigma_thresh;           /* 1e-2 */
    float stop_thresh;            /* 1e-2; parsed, unused by regular tracking */
    float background_brightness;  /* 1.0 */
    float render_bbox[6];         /* {0,0,0,1,1,1} */
    int basis_minmax[2];          /* {0,24} */
    float rot_dirs[3];            /* {0,0,0} */
    int show_grid;                /* false; no launch reads it: rto_draw_grid_layers draws the grid into layers (rto_ctx_set_layers) */
    int grid_max_depth;           /* 4; rto_grid_params_default takes it as the grid's max_depth */
    int render_depth;             /* false; unused by the kernel */
    int enable_probe;             /* false; draws the lumisphere of the leaf at `probe` into the frame's top right corner (see rto_launch_renderer) */
    float probe[3];               /* {0,0,1} */
    int probe_disp_size;          /* 100 */
    int denoise;                  /* true: kernel writes the noisy image, else the final image */
    int spp;                      /* 1 */
} rto_options;

/* CameraSpec (data_spec.hpp:11-24).  transform = 4x3 column-major camera-to-world
 * (camera.hpp: glm::mat4x3): [0..8] rotation columns, [9..11] centre.  Passed to the kernel by
 * value: no per-frame H2D copy (camera.cpp:67-75 in the reference). */
typedef struct rto_camera {
    int width, height;
    float fx, fy;
    float transform[12];
} rto_camera;

typedef struct rto_tree_info {
    int64_t capacity;   /* nodes */
    int N;              /* branching per axis (2) */
    int data_dim;       /* 3*basis_dim+1, or 4 for RGBA */
    int format;         /* RTO_FMT_* */
    int basis_dim;      /* -1 for RGBA */
    float scale[3];     /* invradius3 */
    float offset[3];
    int use_ndc;
    float ndc_width, ndc_height, ndc_focal;
    int max_depth;      /* deepest leaf level (levels of child[] visited to reach it) */
    int64_t device_bytes;
    int64_t wide_nodes; /* nodes of the two-level traversal image the batched kernel walks (0: it walks the one-level image) */
} rto_tree_info;

typedef struct rto_tree rto_tree; /* opaque */
typedef struct rto_ctx rto_ctx;   /* opaque */

/* Which traversal kernel rto_launch_renderer uses.  Results are bit-identical. */
enum {
    RTO_KERNEL_AUTO = 0,    /* fast path when the tree allows it (N == 2), else generic */
    RTO_KERNEL_GENERIC = 1, /* root-restart descent, one thread per pixel (any N) */
    RTO_KERNEL_FAST = 2     /* integer descent + ancestor stack (N == 2) */
};

const char* rto_version(void);
const char* rto_last_error(void);
/* number of HIP devices visible, or RTO_E_HIP */
int rto_device_count(void);

/* ---- options (render_options.hpp) ---- */
void rto_options_default(rto_options* o);
/* Parses the reference's options JSON (options/opt.json).  Like NLOHMANN_DEFINE_TYPE_INTRUSIVE
 * (render_options.hpp:61-77) all 11 keys are required; render_bbox/basis_minmax/rot_dirs keep
 * their defaults. */
int rto_options_from_json_file(const char* path, rto_options* o);
int rto_options_from_json(const char* text, rto_options* o);

/* ---- tree (N3Tree) ---- */
/* N3Tree::open (n3tree.cpp:111-154) + load_cuda (n3tree.cu:9-41).  Reads `tree.npz` (dense fp16
 * `data`, or the quantised set quant_colors/quant_map/sigma[/data_retained]) and uploads it. */
int rto_tree_load_npz(const char* path, int device, rto_tree** out);
/* flags: RTO_TREE_QUANT_DIRECT keeps a quantised tree (quant_colors / quant_map / sigma
 * [/ data_retained]) as stored and renders straight from the codebooks instead of expanding it to
 * the dense fp16 layout: same pixels, a fraction of the footprint.  N == 2,
 * SH4/9/16/25 only; such a tree renders through the batched kernels (also for single frames).
 * Ignored for dense files. */
#define RTO_TREE_QUANT_DIRECT 1
/* RTO_TREE_COMPACT: do not build the aligned copy of the SH coefficients the shading kernels otherwise read (dense SH9 /
 * SH16 trees: + 64 / 128 B per leaf slot, i.e. the device footprint roughly doubles, for ~11 % faster shading = ~2 % more
 * frames/s on the benchmark scene).  Same pixels either way. */
#define RTO_TREE_COMPACT 2
/* RTO_TREE_KEEP_REFERENCE: a dense SH9 / SH16 tree that has the aligned copy renders through the fast and the batched
 * kernels from the traversal image + that copy alone, so by default the upload RELEASES the reference-layout child[] and
 * data[] arrays once the derived ones exist (device footprint of the benchmark tree: 2.2 GB instead of 4.0 GB for a
 * 1.7 GB file) and rebuilds them -- the same leaf values -- on the first launch that selects the generic kernel
 * (rto_ctx_set_kernel(RTO_KERNEL_GENERIC)), which then pays one pass over the tree.  This flag keeps them resident. */
#define RTO_TREE_KEEP_REFERENCE 4
/* RTO_TREE_COMPACT_RECORDS: the aligned coefficient copy holds a record only for the leaf slots a ray can hit -- density
 * > 0: a hit needs sigma > sigma_thresh (rt_core.cuh:252) -- found through a 4-byte-per-slot index (8.6 M of 17 M slots of
 * the benchmark tree: 1.3 instead of 2.2 GB resident, 0.75x the file).  Same pixels; the shading kernels pay one more
 * dependent gather per hit leaf (measured: DESIGN_HISTORY.md section 3).  Launches with sigma_thresh < 0 are refused for such a
 * tree (RTO_E_UNSUPPORTED).  Ignored where no aligned copy is built (RTO_TREE_COMPACT, SH25, RGBA, quantised-direct). */
#define RTO_TREE_COMPACT_RECORDS 8
/* RTO_TREE_NO_CULLING: do not build the empty-space culling cells (the batched path then marches every ray, as rounds 1-2
 * did).  By default an N == 2 tree carries the cubes (no finer than 1/128 of the volume) that contain its leaves of
 * positive density; every batched launch projects them into its frames and skips the 8x8-pixel tiles none of them
 * touches -- rays that provably never meet density are background pixels.  Same pixels either way. */
#define RTO_TREE_NO_CULLING 16
int rto_tree_load_npz_ex(const char* path, int device, int flags, rto_tree** out);
/* Same upload from host arrays: child int32 [capacity*N^3], data fp16 bits
 * [capacity*N^3*data_dim], data_format like "SH9"/"SH16"/"RGBA" (DataFormat::parse,
 * n3tree.cpp:55-78). */
int rto_tree_from_arrays(const int32_t* child, const uint16_t* data, int64_t capacity, int N,
                         int data_dim, const char* data_format, const float scale[3],
                         const float offset[3], int device, rto_tree** out);
/* the same with the RTO_TREE_* flags of rto_tree_load_npz_ex (RTO_TREE_QUANT_DIRECT does not apply to arrays) */
int rto_tree_from_arrays_ex(const int32_t* child, const uint16_t* data, int64_t capacity, int N,
                            int data_dim, const char* data_format, const float scale[3],
                            const float offset[3], int device, int flags, rto_tree** out);
/* the same with the lobes of an SG / ASG tree (the npz's extra_data, n3tree.cpp:350-353; TreeSpec::extra,
 * data_spec.hpp:30): extra_floats = basis_dim * 4 floats {lambda, mu_x, mu_y, mu_z} per lobe (SG) or basis_dim * 11
 * {lambda_x, lambda_y, mu_x[3], mu_y[3], mu_z[3]} (ASG), all finite, else RTO_E_FORMAT.  Ignored for SH and RGBA trees.
 * An SG / ASG tree uploaded without lobes (extra = NULL) loads, and every launch of it returns RTO_E_FORMAT. */
int rto_tree_from_arrays_extra(const int32_t* child, const uint16_t* data, int64_t capacity, int N,
                               int data_dim, const char* data_format, const float scale[3],
                               const float offset[3], int device, int flags, const float* extra,
                               int64_t extra_floats, rto_tree** out);
/* main_headless.cpp:400-405 (llff): switch the NDC warp on. width <= 0 turns it off. */
int rto_tree_set_ndc(rto_tree* t, float ndc_width, float ndc_height, float ndc_focal);
int rto_tree_get_info(const rto_tree* t, rto_tree_info* info);
/* Host-only: runs the same npz parsing + N3Tree::load_npz decode as rto_tree_load_npz (no device
 * needed) and writes a JSON description into json_out: schema fields plus FNV-1a-64 checksums of
 * the child[] and (decoded) data[] arrays, and for an SG / ASG tree "extra_shape" / "extra_fnv1a64" of its
 * lobes (null without lobes, and for SH / RGBA trees, whose extra_data is ignored).  Malformed lobes -- not
 * float32, not basis_dim * 4 (SG) / * 11 (ASG) values shaped [basis_dim, 4 / 11] or flat, not finite -- give
 * RTO_E_FORMAT here and in rto_tree_load_npz.  Returns RTO_E_INVALID if `cap` is too small. */
int rto_tree_probe_npz(const char* path, char* json_out, size_t cap);
void rto_tree_free(rto_tree* t);

/* ---- render context (RenderContext) ---- */
/* RenderContext::update (render_context.hpp:70-91): aux [8][H][W] f32, noisy and final images
 * [H][W][4] f32, rng = pcg32(20230418) (:16).  offscreen is true until rto_ctx_set_layers hands the context a depth / colour layer. */
int rto_ctx_create(int width, int height, int device, rto_ctx** out);
/* The same with `frames` (1..128) frame slots: aux [frames][8][H][W], noisy / image [frames][H][W][4],
 * contiguous.  Single-frame entry points and accessors act on the slot chosen with
 * rto_ctx_select_frame (default 0); rto_launch_renderer_batch fills slots 0..n-1. */
int rto_ctx_create_batch(int width, int height, int frames, int device, rto_ctx** out);
int rto_ctx_frames(const rto_ctx* c);
int rto_ctx_select_frame(rto_ctx* c, int frame);
int rto_ctx_selected_frame(const rto_ctx* c);
void rto_ctx_free(rto_ctx* c);
int rto_ctx_width(const rto_ctx* c);
int rto_ctx_height(const rto_ctx* c);
float* rto_ctx_aux(rto_ctx* c);    /* device, planar [8][H][W]: r,g,b,a,r^2,g^2,b^2,a^2 */
float* rto_ctx_noisy(rto_ctx* c);  /* device, [H][W][4] (reference: noisy_image_arr) */
float* rto_ctx_image(rto_ctx* c);  /* device, [H][W][4] (reference: image_arr / surf_obj) */
/* ctx.rng (pcg32): seed(initstate, initseq) pcg32.h:53-59; advance(delta) :145-166 (the
 * reference's per-frame `ctx.rng.advance()` is delta = 1<<32) */
void rto_ctx_rng_seed(rto_ctx* c, uint64_t initstate, uint64_t initseq);
void rto_ctx_rng_advance(rto_ctx* c, int64_t delta);
void rto_ctx_rng_set(rto_ctx* c, uint64_t state, uint64_t inc);
void rto_ctx_rng_get(const rto_ctx* c, uint64_t* state, uint64_t* inc);
/* RenderContext::offscreen = false with surf_obj_depth / surf_obj (render_context.hpp; volrend.cu:146-153,162-184; the viewer's
 * frame, cuda_renderer.cpp:96-156): every pixel's ray stops at a depth surface and the volume is composited over a colour surface
 * instead of the constant background -- a PlenOctree shown together with rasterised geometry.
 *   depth: device memory [frames][H][W] float32, the world distance along the pixel's unit ray direction (as rto_rays.t_max);
 *          +inf = no limit; a value <= 0 or NaN = the pixel is not traced (its backdrop, alpha 0).
 *   color: device memory [frames][H][W][4] float32, 16-byte aligned; only r, g, b are read.
 * frames, H, W are the context's.  Frame slot k reads plane k: a single-frame launch the selected slot's plane, frame f of a
 * batched launch plane f.  Either pointer may be NULL: no depth = 1e9f, no colour = options->background_brightness; both NULL
 * restores the offscreen behaviour.  The pointers are BORROWED: they must stay valid until the launches that read them have
 * finished, and live on the context's device.  They must not overlap the context's aux / noisy / image buffers -- the reference
 * reads and overwrites surf_obj in place; here the batched path stores a pixel from another kernel than the one that would
 * have to read it, so a binding keeps its mesh pass in a buffer of its own.
 * Semantics: pixel (x, y) of a layered frame is, bit for bit, ray y * W + x of rto_launch_rays on that camera's rays (origin =
 * the camera centre, direction = M xyz) with t_max = its depth, background = its colour's rgb, first_ray = 0 and the frame's RNG
 * base (batch frame f: ctx.rng advanced by rng_jumps[f] * 2^32) -- (r, g, b, alpha).  The outputs are the reference's
 * (volrend.cu:186-212): aux planes 0..3 those four values, planes 4..7 their squares, the noisy / final image (r, g, b, 1); a
 * lean level-1 launch stores (r, g, b, alpha).
 * Affects rto_launch_renderer and rto_launch_renderer_batch only (all kernels; empty-space culling stays on: a tile no culling
 * cell projects into meets no density whatever the depth, its pixels are their backdrop).  rto_launch_rays ignores it.
 * The layered batched kernels exist for the default tuning: the A/B part of the tuning key "refill" (100 * waves/SIMD +
 * threshold) is ignored by a layered launch; its tiles-per-dequeue part and every other key apply.
 * The tile marks promise "an unmarked tile's pixels are the constant background".  With a depth layer only that holds: lean
 * level 2, rto_ctx_tile_marks and rto_denoise's culled routes work unchanged.  With a colour layer it does not: the launch still
 * culls its marching, but rto_ctx_tile_marks returns RTO_E_INVALID after it, rto_denoise takes its plain kernels, and a lean
 * level-2 launch returns RTO_E_UNSUPPORTED.
 * RTO_E_INVALID: color not 16-byte aligned, a layer that overlaps the context's buffers or is not memory of the context's device
 * (the context keeps the layers it had).  Launches return RTO_E_UNSUPPORTED for layers combined with rto_ctx_enable_stats or
 * with a tree loaded with RTO_TREE_QUANT_DIRECT.  enable_probe on a context with layers stays RTO_E_UNSUPPORTED: the suite pins that
 * refusal, it is not principled -- the probe's overlay (rto_launch_renderer) would work over layers as it does offscreen. */
int rto_ctx_set_layers(rto_ctx* c, const float* depth, const float* color);
/* the layers the context holds (NULL: none); either out pointer may be NULL */
int rto_ctx_layers(const rto_ctx* c, const float** depth, const float** color);
/* choose the traversal kernel (RTO_KERNEL_*); default AUTO */
int rto_ctx_set_kernel(rto_ctx* c, int kernel);
/* Performance knobs; never change results.  key: "strip_rows" (single-frame kernel: tile rows per XCD
 * strip, >= 1); batched kernel: "refill" (0 = default; 100 * waves/SIMD + idle-lane threshold selects one of the A/B instantiations), "tile_order"
 * (0 = row-major tiles, 1 = centre-out), "xcd_queues" (1 = one ray queue per XCD over its share of the image,
 * with stealing; 0 = a single queue), "tile_major" / "tile_block" (queue order), "queue_bands" (the XCD queues take bands of this many
 * 8-pixel tile rows, band j -> queue j % 8; 0 = angular wedges around the image centre; default 3), "cull" (1 = skip the tiles whose rays provably meet no density, the default; 0 = march every ray), "blocks_per_cu" (0 = as many
 * workgroups of the persistent traversal kernel per CU as fit, else a cap 1..8: the kernel's true occupancy knob --
 * `refill`'s waves/SIMD only sets the register budget); rto_launch_rays: "ray_order" (0 = workgroup b takes rays 256 b .. 256 b + 255,
 * 1 = each XCD takes one contiguous range of the rays). */
int rto_ctx_set_tuning(rto_ctx* c, const char* key, int value);
/* Lean outputs of the batched render -> denoise route (round 5; off by default).  The reference's kernel stores, per pixel,
 * 8 aux planes and an RGBA32F image (volrend.cu:187-212: 48 bytes) -- of which its own denoise stage reads aux planes 0..3
 * (planes 4..7 are their squares) and the image's rgb, which duplicates planes 0..2.  With lean outputs on, a
 * rto_launch_renderer_batch with options.denoise = 1 stores 16 bytes per pixel instead: the noisy image as (r, g, b, ALPHA)
 * -- alpha = aux plane 3 where the reference writes 1.0 -- and NO aux planes (the context's aux buffer keeps whatever it
 * held).  Consumers: rto_denoise (picks the route by itself), or rto_guidance_net_forward*(..., flags = RTO_NET_INPUT_RGBA)
 * on rto_ctx_noisy + rto_filtering* on the same image (the filter never reads the image's alpha, filtering.cu:186-199).
 * The denoised image is bit-identical to the full-output route's.  Single-frame launches, launches with denoise = 0 and
 * everything that reads the aux buffer (--write_buffer, rto_ctx_download_aux) need the full outputs: leave it off there.
 * The state is kept PER FRAME SLOT: a launch changes it only for the slots it writes (a single-frame launch into slot k of a
 * lean batch leaves the other slots lean).  rto_ctx_frames_are_lean: 1 when slots [first_slot, first_slot + n) were all
 * written by a lean launch last, 0 when none was, -1 for a mixed range -- which rto_denoise refuses (RTO_E_INVALID): denoise
 * each run of slots by itself. */
int rto_ctx_set_lean_outputs(rto_ctx* c, int level);
int rto_ctx_frames_are_lean(const rto_ctx* c, int first_slot, int n);
/* Level 2 (round 6), SPARSE lean outputs: as level 1, and the launch stores NOTHING for the pixels of the 8x8 tiles its
 * empty-space culling left unmarked (two thirds of the bench scene's pixels; they are the background: colour =
 * background_brightness, alpha 0).  The noisy image is then valid inside marked tiles only; its consumers need the launch's
 * tile marks (rto_ctx_tile_marks): rto_denoise with RTO_FILTER_FACTORISED does it by itself, the two-call form passes
 * RTO_NET_INPUT_RGBA | RTO_NET_INPUT_SPARSE and the marks to rto_guidance_net_forward_packed_culled + rto_filtering_packed_culled.
 * rto_ctx_download_image / _rgba8 of the noisy image fill the unmarked tiles in on the host.  The denoised image is complete and
 * bit-identical to the other levels'.  rto_ctx_frames_lean_level: 0 / 1 / 2 when all of the slots agree, -1 otherwise. */
int rto_ctx_frames_lean_level(const rto_ctx* c, int first_slot, int n);
/* Per-kernel HIP-event timing of the batched path: when enabled, every rto_launch_renderer_batch
 * records events before the traversal kernel, between it and the shading kernel, and after (on the
 * launch stream; up to 256 launches between reads).  _read synchronises on the recorded events and
 * returns the mean milliseconds per launch of each kernel, then resets the ring. */
/* Diagnostic (synchronises the device): of the last rto_launch_renderer_batch on this context, how many 8x8-pixel tile
 * slots (tile x frame) were marched and how many there were -- the rest were culled as provably empty (see
 * RTO_TREE_NO_CULLING; tuning key "cull" = 0 switches the culling off per context). */
int rto_ctx_queue_stats(rto_ctx* c, int64_t* live_tile_slots, int64_t* all_tile_slots);
/* The tile marks the last rto_launch_renderer_batch left on the device: frames x words_per_frame uint32 (bit t of a frame's
 * words = 8x8 tile t, row-major, may hold a ray that meets density; bit 0 of the frame's last word = treat every tile as
 * marked).  An unmarked tile's pixels are exactly the background: colour = *background, alpha 0.  Valid (stream-ordered
 * after that launch) until the next launch on the context; RTO_E_INVALID when the last launch was a single-frame one.
 * Frame f of the marks is context slot first_slot + f.  For rto_filtering_packed_culled. */
int rto_ctx_tile_marks(const rto_ctx* c, const uint32_t** marks, int* words_per_frame, int* first_slot, int* frames, float* background);
int rto_ctx_kernel_timing(rto_ctx* c, int enable);
int rto_ctx_kernel_timing_read(rto_ctx* c, float* traverse_ms, float* shade_ms, int* launches);
/* the same with the thresholds kernel (sample_kernel: RNG jump, SPP draws, sort for every pixel of the batch) reported too,
 * as raygen_ms */
int rto_ctx_kernel_timing_read3(rto_ctx* c, float* raygen_ms, float* traverse_ms, float* shade_ms, int* launches);
/* Work counters for the roofline's ALGORITHMIC byte count.  When enabled, the fast
 * kernel's counting instantiation runs instead of the timed one and accumulates, over the launches
 * since the last rto_ctx_get_stats(reset=1): {rays, rays_in_box, march steps, descent levels a
 * root-restart walk visits, distinct hit leaves, rays with a hit}.  Never enable it in a timed run. */
int rto_ctx_enable_stats(rto_ctx* c, int enable);
int rto_ctx_get_stats(rto_ctx* c, void* stream, uint64_t out[6], int reset);
/* enable = 2: additionally count the frame as the BATCHED path works through it (round 4: the figure above prices a
 * root-restart walk of every ray, rt_core.cuh:241-270 + n3tree_query.hpp:22-47, which the batched kernels do not perform).
 * The caller renders frames with rto_launch_renderer_batch, selects a slot and re-renders that slot's pose (same RNG) with
 * rto_launch_renderer: rays of tiles the batched launch culled are left out, and a node visit counts as the one load
 * render_persist issues for it.  out = {rays of marked tiles, their march steps, top-grid entries loaded (8 B each),
 * traversal-image words loaded (4 B each), hit entries written (4 B each), rays of marked tiles that entered the volume,
 * entries of the two-level traversal image loaded (4 B each: render_persist loads these INSTEAD of the traversal-image words
 * when the tree has that image, rto_tree_info.wide_image), 0}. */
int rto_ctx_get_march_stats(rto_ctx* c, void* stream, uint64_t out[8], int reset);

/* Diagnostics, host only (no device): the two-level traversal image the batched kernel walks (a node of level G + 2p merged
 * with its eight children: one load per two levels; derived from child[], n3tree.hpp / n3tree_query.hpp:22-47 is what it
 * must answer like) built for a breadth-first child[] and walked for n points (24-bit fixed-point x, y, z each) exactly as
 * the kernel walks it; out: the leaf's level, its slot in child[] / data[], its sigma bits, the number of wide nodes. */
int rto_wide_image_probe(const int32_t* child, const uint16_t* sigma_bits, int64_t capacity, int max_depth, int top_levels,
                         const uint32_t* points, int64_t n, int32_t* out_level, int64_t* out_slot, uint16_t* out_sigma,
                         int64_t* out_wide_nodes);

/* ---- point queries (svox's tree(points); the reference's query_single_from_root, n3tree_query.hpp:13-48) ---- */
/* What the tree holds at n points.  All pointers are device memory on the tree's device; any member of rto_query_out may be NULL
 * (that output is not computed; sigma, level and cube come from the walk alone and read neither data[] nor a coefficient record). */
typedef struct rto_query_out {
    float*   values; /* [n][data_dim]: half -> float of the leaf's data[], in data[]'s order (last = sigma) */
    float*   sigma;  /* [n] */
    int32_t* level;  /* [n]: levels of child[] visited to reach the leaf (rto_tree_info.max_depth's convention); -1 = not answered */
    float*   cube;   /* [n][4], 16-byte aligned: the leaf's min corner in tree coordinates and its side, 1 / cube_sz */
} rto_query_out;
/* Point p (world space) maps to xyz[i] = offset[i] + scale[i] * p[i] in float arithmetic, the product rounded before the add
 * (volrend.cu:220-222); NO NDC warp is applied, also for an NDC tree (the reference's probe applies none): pass points of the
 * tree's own space there.  Then the reference's clamp to [0, 1 - 1e-6f] and its descent: the answer names the leaf
 * query_single_from_root reaches, for every finite float, whichever traversal image the kernel walks.  A point with a non-finite
 * coordinate is not answered: level -1, zeros elsewhere (the convention of rto_launch_rays' degenerate rays).
 * Asynchronous on `stream`: no host synchronisation, no allocation and no host-to-device copy per call; n == 0 launches nothing.
 * Splitting a call gives the same bytes.  Reads the tree as it is resident: child[] / data[] of a tree that released them are
 * not brought back.
 * RTO_E_INVALID (checked before any device use): null tree or out, n < 0, null points with n > 0, cube not 16-byte aligned.
 * RTO_E_UNSUPPORTED, for `values` only (sigma, level and cube still work): a tree loaded with RTO_TREE_QUANT_DIRECT (its values
 * live in codebooks, as for rto_launch_rays); a tree loaded with RTO_TREE_COMPACT_RECORDS, which keeps the coefficients of leaves
 * with sigma > 0 only -- load it with RTO_TREE_KEEP_REFERENCE as well. */
int rto_tree_query(const rto_tree* tree, const float* points /* device [n][3] world space */, int64_t n,
                   const rto_query_out* out, void* stream);

/* The octree grid of RenderOptions::show_grid (the reference's GL wireframe pass, cuda_renderer.cpp:112-124 over
 * N3Tree::gen_wireframe, n3tree.cpp:390-434) ray-traced into a depth and a colour layer, the inputs of rto_ctx_set_layers.
 * Cells: the tree's leaves cut off at level max_depth + 1 (levels of child[] visited; max_depth = 0: the root's eight children,
 * gen_wireframe's `child == 0 || depth >= max_depth`), empty leaves included.  A pixel is a line pixel when its ray -- the
 * pixel's ray of rto_launch_renderer -- passes within 0.5 * line_px pixels (perpendicular distance r = 0.5 * line_px / fx times
 * the distance along the ray) of a cell edge at a cell face it crosses inside the volume; DESIGN.md section 7f has the exact
 * float32 rule, tests/grid_ref.py restates it bit for bit.  No antialiasing; a ray that misses the volume's box is never a line
 * pixel, however close it passes to the box's silhouette.
 *   depth: device [n][H][W] float32 or NULL: the world distance along the pixel's unit ray to the line (the measure of
 *          rto_rays.t_max and of the depth layer); +inf where there is none.
 *   color: device [n][H][W][4] float32, 16-byte aligned, or NULL: (params->color, 1) on a line pixel, (background x 3, 1) elsewhere.
 * RTO_GRID_MERGE: the GL depth test against what the buffers already hold (a mesh pass of the caller's): a line pixel replaces
 * depth and colour only where the existing depth is greater than the line's; a pixel whose existing depth is <= 0 or NaN (not
 * traced, see rto_ctx_set_layers) is left alone; nothing else is written.  It needs `depth`.
 * All n cameras share width and height; frame f goes to plane f.  The cameras are read before the call returns and travel to the
 * kernel BY VALUE, 32 per launch: the call does no allocation, no host synchronisation and no host-to-device copy, and is
 * asynchronous on `stream`.  n == 0 launches nothing; n calls of one frame give the same bytes as one call of n frames.
 * RTO_E_INVALID (checked before any device use; the buffers are untouched): a null tree / cams / params, both outputs NULL,
 * n < 0, line_px not finite or <= 0, max_depth < 0 (above 22 it is clamped to 22), a non-finite colour or background, an
 * unknown flag, RTO_GRID_MERGE without depth, color not 16-byte aligned, cameras of differing size, a camera whose width or
 * height is <= 0 or whose fx / fy is zero or not finite.  RTO_E_UNSUPPORTED: a tree with NDC set (the line width is defined in
 * unwarped space), N != 2, a tree with neither a traversal image nor child[] resident.  Trees loaded with
 * RTO_TREE_QUANT_DIRECT work: the walk reads no values. */
#define RTO_GRID_MERGE 1
typedef struct rto_grid_params {
    int max_depth;     /* >= 0 */
    float line_px;     /* line width in pixels, > 0 */
    float color[3];    /* the lines' rgb */
    float background;  /* rgb of every other pixel of `color` */
    int flags;         /* 0 or RTO_GRID_MERGE */
} rto_grid_params;
/* max_depth = o->grid_max_depth, line_px = 1, black lines, background = o->background_brightness, flags = 0 (o == NULL: the
 * default options) */
void rto_grid_params_default(rto_grid_params* p, const rto_options* o);
int rto_draw_grid_layers(const rto_tree* tree, const rto_camera* cams /* host [n] */, int n, const rto_grid_params* p,
                         float* depth, float* color, void* stream);

/* ---- meshes: triangles, lines and points as depth and colour layers ----
 * The reference's mesh pass (Mesh::draw and its shaders, mesh.cpp:100-161, 366-397; cuda_renderer.cpp:96-111) without a
 * rasteriser: a pixel is a ray, and the answer is the nearest primitive along it.  DESIGN.md section 7g has the float32 rule
 * operation by operation, tests/mesh_ref.py restates it bit for bit.  In short, for the ray o + t d (d unit; t is the world
 * distance, the measure of rto_rays.t_max and of the depth layer, the reference's Depth = length(FragPos.xyz)):
 *   triangle: Moeller-Trumbore, two-sided (the reference culls no faces); hit when det != 0, u >= 0, v >= 0, u + v <= 1, t > 0.
 *     Colour: the vertex colours interpolated with (1 - u - v, u, v); a lit mesh multiplies by ambient + diffuse + diffuse2 +
 *     specular of the fragment shader with the interpolated, NOT renormalised, normal and pow(x, 32) as five squarings.
 *     DEVIATION: viewDir = -d.  The shader subtracts a view-space position from a world-space camera position
 *     (normalize(camPos - vec3(FragPos)), FragPos = MV * pos); here the view direction is the one from the hit point to the eye.
 *     No clamp: the reference's colour surface is RGBA32F.
 *   segment, point (a segment with a == b): the closest approach of the ray's line to the segment, the segment's parameter s
 *     clamped to [0, 1]; tc = the ray parameter of the point nearest to it, dist = their distance; hit when tc > 0 and
 *     dist <= spread * tc.  Depth tc, colour (1 - s) c0 + s c1, always unlit.  For a camera pixel spread = 0.5 * line_px / fx
 *     (point_px for points): lines are cones of line_px pixels, as the grid's are.
 *   nearest wins: the smallest depth, among equal depths the lowest primitive index (GL_LESS in draw order: mesh order, then
 *     face order).  No hit: depth +inf, colour (background x 3, 1).
 * A mesh set holds world-space primitives only: the model transform (Mesh::draw: rotation(axis-angle) * scale, then translation;
 * |rotation| < 1e-3 is the identity) is applied on the host at creation, in double precision rounded to float once, and normals
 * are stored as normalize(mat3(M) n).  An invisible mesh is simply not passed in.  One threaded BVH (host-built, deterministic)
 * covers all primitives. */
typedef struct rto_mesh_desc {
    const float* vert;       /* host [n_verts][9]: position, rgb, normal -- the reference's VERT_SZ layout */
    int64_t n_verts;
    const uint32_t* faces;   /* host [n_faces][face_size], or NULL: consecutive vertices form the n_verts / face_size faces */
    int64_t n_faces;
    int face_size;           /* 3 triangles, 2 lines, 1 points */
    int unlit;
    int estimate_normals;    /* triangles only: overwrite the normals as mesh.cpp estimate_normals does */
    float rotation[3];       /* axis-angle; |r| < 1e-3 = identity (Mesh::draw) */
    float translation[3];
    float scale;
} rto_mesh_desc;
typedef struct rto_meshes rto_meshes; /* opaque */
typedef struct rto_meshes_info {
    int64_t triangles, segments, points;
    int64_t nodes;           /* of the BVH */
    int64_t device_bytes;
    float lo[3], hi[3];      /* world bounds of the positions (zeros for an empty set) */
    int device;
} rto_meshes_info;
/* device >= 0: the set is uploaded to that GPU.  device < 0: a host-only set, for rto_meshes_trace_rays_host and the queries --
 * no device is touched.  n == 0 or zero primitives give a valid, empty set.
 * RTO_E_INVALID (before any device use): null meshes with n > 0 or null out, n < 0, face_size outside 1..3, negative counts, a
 * face index >= n_verts, a non-finite position, rotation, translation or scale (or a position that overflows in world space),
 * more than 2^30 primitives. */
int rto_meshes_create(const rto_mesh_desc* meshes, int n, int device, rto_meshes** out);
/* A set from files: an .obj (Mesh::load_basic_obj: `v x y z [r g b]`, `vn`, `f` with a, a/b, a/b/c, a//c and negative indices;
 * polygons that are no triangles are dropped; colours and normals are taken only when there is one per vertex, else (1, 0.5, 0.2)
 * and estimated normals; nothing else is parsed) or a drawlist .npz (Mesh::open_drawlist, mesh.cpp:770-938: entries `<name>` =
 * type string, `<name>__<field>`; types cube, sphere (rings, sectors), line (a, b), lines (points, segs), points, camerafrustum
 * (focal_length, image_width, image_height, z, r, t, connect), mesh (points, faces, face_size); common fields color, vert_color,
 * scale, translation, rotation, visible, unlit, with the reference's defaults; meshes in the order of their names, invisible ones
 * left out), chosen by the extension.  rto_meshes_load_files concatenates the meshes of n files in order.
 * RTO_E_IO: a file that cannot be opened.  RTO_E_FORMAT, with a message: another extension, malformed or truncated content, an
 * index out of range, a non-finite value. */
int rto_meshes_load(const char* path, int device, rto_meshes** out);
int rto_meshes_load_files(const char* const* paths, int n, int device, rto_meshes** out);
int rto_meshes_get_info(const rto_meshes* m, rto_meshes_info* info);
/* What the set holds, for tests and tools: prims = host [triangles + segments + points][32] floats or NULL, nodes = host
 * [nodes][8] floats or NULL -- the records (in leaf order; word 29 is the primitive's index in draw order) and the BVH nodes
 * in the layouts of csrc/rto_mesh_trace.h. */
int rto_meshes_download(const rto_meshes* m, float* prims, float* nodes);
void rto_meshes_free(rto_meshes* m);

#define RTO_MESH_MERGE 1
typedef struct rto_mesh_params {
    float line_px, point_px; /* widths in pixels, > 0 */
    float background;        /* rgb of a pixel without a hit */
    int flags;               /* 0 or RTO_MESH_MERGE */
} rto_mesh_params;
/* line_px = point_px = 1, background = o->background_brightness, flags = 0 (o == NULL: the default options) */
void rto_mesh_params_default(rto_mesh_params* p, const rto_options* o);
/* The set drawn for n cameras of one size into depth (device [n][H][W] float32 or NULL) and color (device [n][H][W][4] float32,
 * 16-byte aligned, or NULL), the inputs of rto_ctx_set_layers; the pixel's ray is the one of rto_launch_renderer.
 * RTO_MESH_MERGE has exactly RTO_GRID_MERGE's semantics: a hit replaces depth and colour only where the existing depth is
 * greater than its own; a pixel whose existing depth is <= 0 or NaN is left alone and not traced; nothing else is written; it
 * needs `depth`.  The reference's draw order is rto_draw_mesh_layers, then rto_draw_grid_layers(... RTO_GRID_MERGE).
 * The cameras travel to the kernel BY VALUE, 32 per launch: no allocation, no host synchronisation and no host-to-device copy
 * per call; asynchronous on `stream`; n == 0 launches nothing; n calls of one frame give the bytes of one call of n frames.
 * RTO_E_INVALID (checked before any device use; the buffers are untouched): a null set / cams / params, a host-only set, both
 * outputs NULL, n < 0, line_px or point_px not finite or <= 0, a non-finite background, an unknown flag, RTO_MESH_MERGE without
 * depth, color not 16-byte aligned, cameras of differing size, a camera whose width or height is <= 0 or whose fx / fy is zero
 * or not finite. */
int rto_draw_mesh_layers(const rto_meshes* m, const rto_camera* cams /* host [n] */, int n, const rto_mesh_params* p,
                         float* depth, float* color, void* stream);
/* n arbitrary rays against the set.  The direction is normalised as rto_launch_rays does; a degenerate ray (a direction that
 * cannot be normalised, a non-finite origin) is a miss: (+inf, background).  A pixel of rto_draw_mesh_layers equals the ray
 * camera_rays(cam)[y W + x] with line_spread = 0.5f * line_px / fx (point_spread likewise), bit for bit; t_hit can be passed
 * to rto_launch_rays as t_max and rgb as background.  Splitting a batch gives the same bytes. */
typedef struct rto_mesh_rays {
    const float* origins;    /* [n][3] */
    const float* dirs;       /* [n][3], any length */
    int64_t n;
    float line_spread, point_spread; /* >= 0: a line is hit within line_spread * (distance along the ray) of it */
    float background;
} rto_mesh_rays;
/* device pointers; t_hit [n] or NULL, rgb [n][3] or NULL.  Asynchronous on `stream`.  RTO_E_INVALID (before any device use):
 * null set / rays, a host-only set, both outputs NULL, n < 0, null origins / dirs with n > 0, a spread that is negative or not
 * finite, a non-finite background. */
int rto_meshes_trace_rays(const rto_meshes* m, const rto_mesh_rays* rays, float* t_hit, float* rgb, void* stream);
/* The same on the CPU, with HOST pointers: the same code as the kernels' (csrc/rto_mesh_trace.h) compiled for the host. */
int rto_meshes_trace_rays_host(const rto_meshes* m, const rto_mesh_rays* rays, float* t_hit, float* rgb);

/* ---- the operator ---- */
/* launch_renderer(tree, cam, options, ctx, stream, offscreen) (volrend.cu:236-285); offscreen = false is a context with
 * layers (rto_ctx_set_layers).  Asynchronous on `stream`.  Writes ctx aux + (options->denoise ? noisy : image).
 * cam->width/height must equal the ctx size.
 * options->enable_probe (volrend.cu:100-134, 215-231, 244-251; offscreen contexts, both launch forms): one query of the point
 * options->probe -- as rto_tree_query maps, clamps and answers it -- fetches that leaf's coefficients into a buffer the context
 * owns (stream-ordered; the reference allocates and frees one per launch), and behind the render kernels one overlay kernel
 * overwrites the pixels of the probe's disc in every output the launch wrote, for each frame with its camera.  A disc pixel never
 * depended on the trace (enable_draw = false), a pixel outside the disc is traced as always: the overlay is exact.  Pixel (x, y)
 * with y < probe_disp_size + 5 and x >= width - probe_disp_size - 5 is in the disc when c = cen0^2 + cen1^2 <= 1.f, cen0 =
 * -(xx / (0.5f * probe_disp_size) - 1.f), cen1 = yy / (0.5f * probe_disp_size) - 1.f, xx = x - (width - probe_disp_size) + 5,
 * yy = y - 5 (float arithmetic, every operation rounded).  Its colour: dir = M (cen0, cen1, -sqrtf(1 - c)) with the camera's
 * rotation columns (not normalised, no rot_dirs rotation), the tree's basis at dir, per channel tmp = the left-to-right sum of
 * basis[i] * coeff[channel * basis_dim + i] and 1.f / (1.f + expf(-tmp)) in the library's deterministic expf; an RGBA tree's first
 * three coefficients as they are.  Outputs as volrend.cu:174-212 with nalpha = 0: aux planes 0..3 = (r, g, b, 1), 4..7 their
 * squares, the noisy / final image (r, g, b, 1); a lean level-1 launch stores (r, g, b, 1).  The disc is clipped to the image.
 * Deviation: the reference sums i = basis_minmax[0] .. basis_minmax[1] whatever the tree's basis_dim (with the default {0, 24} on
 * an SH9 tree it reads uninitialised basis entries and the next channel's coefficients); here i runs over max(lo, 0) ..
 * min(hi, basis_dim - 1).
 * With the probe on a launch still culls its marching but leaves no tile marks (the disc is no background: the colour layer's
 * precedent) -- rto_ctx_tile_marks returns RTO_E_INVALID after it, rto_denoise takes its plain kernels, a lean level-2 launch
 * returns RTO_E_UNSUPPORTED, the tuning key "cull_single" is ignored.  RTO_E_INVALID: probe_disp_size <= 0.  RTO_E_UNSUPPORTED:
 * a context with layers, rto_ctx_enable_stats, a tree whose `values` rto_tree_query refuses. */
int rto_launch_renderer(const rto_tree* tree, const rto_camera* cam, const rto_options* options,
                        rto_ctx* ctx, void* stream);

/* Throughput form of the operator: n frames (poses of the same tree) in ONE launch of the
 * persistent ray-queue kernel (n <= 128).  Frame f is rendered with cams[f] into frame slot f with the RNG
 * ctx.rng advanced by rng_jumps[f] * 2^32 (NULL: f jumps) -- bit-identical to n sequential
 * rto_launch_renderer calls separated by rto_ctx_rng_advance(ctx, 1<<32), the reference's frame
 * loop (main_headless.cpp:485-506).  ctx.rng itself is not modified.  Needs an N == 2 tree. */
int rto_launch_renderer_batch(const rto_tree* tree, const rto_camera* cams, const int64_t* rng_jumps, int n,
                              const rto_options* options, rto_ctx* ctx, void* stream);

/* ---- rays from the caller (no reference counterpart) ---- */
/* A batch of arbitrary rays.  All pointers are device memory on the tree's device, float32, contiguous. */
typedef struct rto_rays {
    const float* origins;    /* [n][3] world space */
    const float* dirs;       /* [n][3] world space; need not be unit length */
    const float* t_max;      /* [n] or NULL (= 1e9f): world distance along the unit direction where the ray stops (a depth
                                surface, volrend.cu:146-152 with offscreen = false); +inf = no limit */
    const float* background; /* [n][3] or NULL (= options->background_brightness): the colour composited behind the ray
                                (volrend.cu:161-185 with offscreen = false) */
    int64_t n;               /* >= 0 */
    int64_t first_ray;       /* >= 0: RNG index of ray 0 */
} rto_rays;

/* out[i] = (r, g, b, alpha) of ray i: its colour composited over its backdrop, alpha = accumulated opacity (aux plane 3 of a
 * frame).  `out` is [n][4] float32 device memory, 16-byte aligned.  Asynchronous on `stream`: no host sync and no host-to-device
 * copy per call.  Uses ctx for the RNG (ctx.rng advanced by (first_ray + i) * spp; ctx.rng itself is not modified), the jump
 * table, the device and the kernel choice (rto_ctx_set_kernel); ctx's frame buffers and size play no part.
 * Ray i is traced as the frame kernels trace a pixel whose ray_setup produced normalize3(dirs[i]) and centre origins[i] (the NDC
 * warp of an NDC tree included), with tmax_bg = t_max[i]: a ray built as a camera pixel's (rto_launch_renderer) gives that
 * pixel's aux planes 0..3 bit for bit.  Splitting a batch into calls with matching first_ray gives the same results.
 * A degenerate ray -- non-finite origin, a direction that is zero, NaN, infinite or whose squared length under- / overflows,
 * t_max <= 0 or NaN -- returns its backdrop with alpha 0.
 * RTO_E_INVALID: a null argument, n < 0, first_ray < 0, null origins / dirs with n > 0, out not 16-byte aligned, tree and ctx
 * on different devices; RTO_E_SPP; RTO_E_UNSUPPORTED: enable_probe (the probe is drawn into a frame; rays have none), or a tree loaded with RTO_TREE_QUANT_DIRECT (its codebook
 * shading lives only in the batched kernels); RTO_E_FORMAT: an SG / ASG tree without lobes.  n == 0 launches nothing. */
int rto_launch_rays(const rto_tree* tree, const rto_rays* rays, const rto_options* options, rto_ctx* ctx, float* out,
                    void* stream);

/* ---- depth outputs: how far along a ray the volume was hit (no reference counterpart: render_options.hpp:48-49 carries a
 * render_depth option no kernel reads; options->render_depth stays parsed and ignored -- depth is an output beside the colour) ----
 * Definitions.  A HIT of a ray is an iteration of the march loop (rt_core.cuh:241-270) in which src + delta >= dst[spp] holds
 * (:254).  For hit k, in hit order:
 *   cnt_k = the number of thresholds crossed there (the do ... while);
 *   t_k   = the value of t at the top of that iteration, in tree units;
 *   d_k   = t_k * delta_scale, one float product, rounded; delta_scale is the value trace_ray divides tmax_bg by (:206-208), so
 *           d_k is a distance along the unit ray in the measure of rto_rays.t_max and of the depth layer of rto_ctx_set_layers
 *           (for an NDC tree that is the warped space, as for t_max).
 * Two float32 outputs per ray or pixel:
 *   depth  = (sum_k (float)cnt_k * d_k) * (1.f / SPP): every product and every add rounded (no FMA contraction), the sum left to
 *            right in hit order from 0.f.  The hit distance summed over the samples that collided, premultiplied as aux planes
 *            0..2 are: depth / alpha is the mean hit distance, depth + (1 - alpha) * far the expected depth against a far plane.
 *   t_near = d_0, or +inf when the ray has no hit.
 * A ray that is not traced or has no hit -- a degenerate ray, a ray that misses the box, t_max <= 0, a pixel of a tile the
 * single-frame culling (tuning key "cull_single") skips -- gives depth = 0 and t_near = +inf.  A hit at t = 0 is legal (the origin
 * lies inside a dense leaf): d = 0.  With a t_max or a depth layer only hits with t_k < tmax exist: the loop's own condition.
 * The generic kernel's loop is the reference's own arithmetic and defines the values; the fast kernel returns the same bits. */
typedef struct rto_rays_out {
    float* rgba;   /* [n][4], 16-byte aligned: what rto_launch_rays writes */
    float* depth;  /* [n] */
    float* t_near; /* [n] */
} rto_rays_out;
/* rto_launch_rays with the depth outputs.  Any member of `out` may be NULL (that output is not stored; without rgba no colour is
 * computed); all NULL is RTO_E_INVALID, as a null `out`.  With only rgba set this IS rto_launch_rays: the same kernel, the same
 * bytes.  With depth or t_near set the depth-carrying kernels run (render_rays_depth, render_rays_generic_depth) and rgba, when
 * asked for, is still bit for bit what rto_launch_rays returns.  Contract, refusals, the splitting rule (matching first_ray gives
 * the same bytes) and the per-launch split above 2^32 draws are rto_launch_rays'; every argument check comes before any device
 * use. */
int rto_launch_rays_ex(const rto_tree* tree, const rto_rays* rays, const rto_options* options, rto_ctx* ctx,
                       const rto_rays_out* out, void* stream);
/* Depth outputs of a context's frames: allocates (enable != 0) / releases (0; synchronises the device) two planes [frames][H][W]
 * float32 on the context's device, depth and t_near of every frame slot; a slot no launch has written yet reads (0, +inf).
 * While enabled:
 *   rto_launch_renderer (all kernels, offscreen and over layers, "cull_single" too) writes the selected slot's two planes with
 *     the rest of its outputs, through the depth-carrying single-frame kernels (render_fast_layers_depth,
 *     render_generic_layers_depth).  Pixel (x, y) equals, bit for bit, ray y * W + x of rto_launch_rays_ex on the camera's rays
 *     (origin = the camera centre, direction = M xyz) with t_max = the depth layer's value there, as rto_ctx_set_layers states
 *     for the colour.
 *   rto_launch_renderer_batch, enable == 1 (or any non-zero value but RTO_DEPTH_BATCHED), renders its frames ONE BY ONE through
 *     those kernels: frame f into slot f with the RNG advanced by rng_jumps[f] * 2^32, the same bytes as n single launches.  Like
 *     any single-frame launch it leaves no tile marks (rto_ctx_tile_marks: RTO_E_INVALID) and writes full outputs; a lean level
 *     other than 0 is RTO_E_UNSUPPORTED.
 *   rto_launch_renderer_batch, enable == RTO_DEPTH_BATCHED, sends the batch through the persistent kernels like a batch of a context
 *     without depth outputs; the traversal kernel (render_persist_depth, the default tuning's) also accumulates the two outputs.
 *     Frame f's aux, image, depth and t_near in slot f are bit for bit what enable == 1 writes, and the planes of the launch's
 *     slots are first filled with (0, +inf) on the stream (no synchronisation; other slots keep their contents).  The launch
 *     leaves tile marks, takes lean levels 1 and 2 and lets rto_denoise take its culled routes under the rules of an ordinary
 *     batch (no marks and no level 2 over a colour layer).  A launch the persistent kernels cannot take -- a tree without
 *     traversal image, more leaf slots than a hit entry names at this spp, tuning key "batch_fallback" 1, or the device refusing the
 *     traversal kernel's LDS ("batch_fallback" 2) -- goes frame by frame as with enable == 1: no marks, and with a lean level
 *     other than 0 RTO_E_UNSUPPORTED before anything is rendered (a caller that set one turns it off and launches again:
 *     volrend_headless --write_depth does, and keeps full outputs from then on).
 *   rto_launch_renderer behaves the same in both modes.
 *   RTO_E_UNSUPPORTED in both modes: options->enable_probe, rto_ctx_enable_stats, a tree loaded with RTO_TREE_QUANT_DIRECT (what
 *     the layers refuse).
 * Calling it on an enabled context with the other non-zero value changes the mode only: no allocation, no synchronisation, the
 * planes keep their contents.  rto_ctx_depth_enabled returns the mode: 0, 1 or RTO_DEPTH_BATCHED.
 * While disabled nothing on the context behaves differently.  rto_launch_rays / _ex do not touch the context's planes. */
#define RTO_DEPTH_BATCHED 2
int rto_ctx_enable_depth(rto_ctx* c, int enable);
int rto_ctx_depth_enabled(const rto_ctx* c);
float* rto_ctx_depth(rto_ctx* c);  /* device, the selected slot's plane [H][W]; NULL while disabled */
float* rto_ctx_t_near(rto_ctx* c); /* device, the selected slot's plane [H][W]; NULL while disabled */
/* the selected slot's planes -> host [H][W] f32 each (either may be NULL); synchronises `stream`.  RTO_E_INVALID while disabled */
int rto_ctx_download_depth(rto_ctx* c, void* stream, float* host_depth, float* host_t_near);

/* denoiser::filtering(stream, weight_map[L,H,W], guidance_map[L,H,W], img_in, img_out)
 * (filtering.cu:701-717).  All pointers are device pointers; img_in/img_out are [H][W][4] f32
 * (the reference passes ctx.noisy_tex_obj / ctx.surf_obj, denoiser.cpp:56-57).  L in 1..6. */
int rto_filtering(void* stream, const float* weight_map, const float* guidance_map, int L, int H,
                  int W, const float* img_in, float* img_out);
/* n images per launch: weight_map / guidance_map [n][L][H][W], img_in / img_out [n][H][W][4] */
int rto_filtering_batch(void* stream, const float* weight_map, const float* guidance_map, int L, int H,
                        int W, int n, const float* img_in, float* img_out);
/* The same filter in one of two arithmetic forms.  RTO_FILTER_EXACT = rto_filtering_batch: every tap's
 * exp(g(q) - max_p) evaluated as the reference does, bit-identical to the CPU oracle.  RTO_FILTER_FACTORISED:
 * exp(g(q) - c) once per pixel with a per-tile constant c (the factor cancels in sum k rgb / sum k) and the
 * window sums as box filters -- 4 exps per pixel instead of 164 at L = 4; results agree with the exact form
 * to ~1e-6 relative (> 120 dB), inside the 1e-4 dB tolerance of the float paths, not bit for bit. */
enum { RTO_FILTER_EXACT = 0, RTO_FILTER_FACTORISED = 1 };
int rto_filtering_batch_mode(void* stream, const float* weight_map, const float* guidance_map, int L, int H,
                             int W, int n, const float* img_in, float* img_out, int mode);
/* Training side -- Filtering::forward with requires_grad and Filtering::backward
 * (filtering.cu:596-707; grad_weight_accumulate :230-248, grad_guidance_accumulate :250-301), what
 * `_denoiser.filtering_autograd` (bindings.cpp) runs under autograd.  All device pointers, fp32:
 *   forward : as rto_filtering_batch, also writing rgb_filtered [n][L][H][W][4] (alpha 0), max_map and
 *             inv_kernel_sum [n][L][H][W] (the reference keeps one [B,H,W,*] tensor per level);
 *   backward: grad_output, img_in [n][H][W][4] + the forward's inputs and saves ->
 *             grad_weight, grad_guidance [n][L][H][W] (fully overwritten).
 * The guidance gradient is gathered per pixel in a fixed order (no atomics): results are run-to-run
 * identical, which the reference's atomicAdd scatter is not. */
int rto_filtering_train_forward(void* stream, const float* weight_map, const float* guidance_map, int L, int H,
                                int W, int n, const float* img_in, float* img_out, float* rgb_filtered,
                                float* max_map, float* inv_kernel_sum);
int rto_filtering_backward(void* stream, const float* grad_output, const float* img_in, const float* weight_map,
                           const float* guidance_map, const float* rgb_filtered, const float* max_map,
                           const float* inv_kernel_sum, int L, int H, int W, int n, float* grad_weight,
                           float* grad_guidance);
/* convenience: filtering from ctx noisy -> ctx image */
int rto_ctx_filtering(rto_ctx* c, void* stream, const float* weight_map, const float* guidance_map, int L);

/* ---- outputs (main_headless.cpp:508-540) ---- */
/* final image -> RGBA8 on the device ((uint8_t)(f*255), truncation) -> host [H][W][4];
 * synchronises `stream`.  which: 0 = final image, 1 = noisy image */
int rto_ctx_download_rgba8(rto_ctx* c, void* stream, int which, uint8_t* host_out);
int rto_ctx_download_image(rto_ctx* c, void* stream, int which, float* host_out); /* [H][W][4] f32 */
int rto_ctx_download_aux(rto_ctx* c, void* stream, float* host_out);              /* [8][H][W] f32 */

/* ---- event timer (RenderContext::Timer, render_context.hpp:122-213) ---- */
enum { RTO_T_RENDER = 0, RTO_T_TORCH = 1, RTO_T_FILTER = 2 };
int rto_timer_reset(rto_ctx* c, void* stream);
int rto_timer_start(rto_ctx* c, int which);
int rto_timer_stop(rto_ctx* c, int which);
/* Timer::record(denoise): synchronise on the last stop event and accumulate */
int rto_timer_record(rto_ctx* c, int denoise);
/* Timer::report: mean ms per bucket and FPS = 1000/(render+torch+filter) */
int rto_timer_report(const rto_ctx* c, float ms_out[3], float* fps_out, int* frames_out);

/* ---- GuidanceNet forward as one fused kernel ---- */
/* The compact network of denoiser/network.py:156-168 (what compact_and_compile exports and
 * Denoiser::denoise runs, denoiser.cpp:46): relu6(conv3x3(8 -> c1)) -> relu6(conv3x3(c1 -> 2*levels))
 * -> softmax over the first `levels` channels.  Weights in PyTorch layout, fp32:
 * w1 [c1][8][3][3], b1 [c1], w2 [2*levels][c1][3][3], b2 [2*levels]; they are rounded to fp16 like the
 * reference's `.half()` module.  Supported: c1 in 1..64, levels in 1..6 (the trainer's --mid_channels / --kernel_levels,
 * denoiser/main.py:101-110); anything else returns RTO_E_UNSUPPORTED.  This is rto_guidance_net_create_layers for two layers. */
typedef struct rto_guidance_net rto_guidance_net;
int rto_guidance_net_create(const float* w1, const float* b1, const float* w2, const float* b2, int c1, int levels,
                            int device, rto_guidance_net** out);
/* Any compact stack the trainer can produce: 8 -> c1 [-> c1] -> 2*levels, i.e. num_layers 2 or 3, c1 in 1..64, levels in 1..6;
 * every layer conv3x3 "same" + ReLU6 with fp16 rounding after it, softmax over the first `levels` channels of the last.
 * RTO_E_INVALID (checked before any device is touched): a null pointer, layers[0].cin != 8, layers[i].cin != layers[i-1].cout,
 * last cout != 2*levels, a non-finite weight or bias.  RTO_E_UNSUPPORTED: num_layers outside 2..3, c1 outside 1..64, a middle
 * layer that is not c1 -> c1, levels outside 1..6.
 * c1 = 32, levels = 4, two layers (denoiser/configs/blender.txt:21-25) is the reference shape: it runs the kernel tuned for it
 * and has every route below.  Every other shape is a GENERAL net: one fused kernel as well (guidance_general.inc), on fp32
 * planes -- rto_guidance_net_forward / _forward_ex / _forward_culled, rto_filtering_culled and rto_denoise (both modes; lean
 * level-1 frames included) work with the net's own `levels`; the packed fp16 maps and sparse frames do not exist for it:
 * rto_guidance_net_forward_packed[_culled], rto_filtering_packed[_culled], rto_guidance_net_reserve, RTO_NET_INPUT_SPARSE and
 * rto_denoise on sparse (lean level 2) frames return RTO_E_UNSUPPORTED and leave the handle usable. */
typedef struct rto_guidance_layer {
    const float* weight; /* host, [cout][cin][3][3] */
    const float* bias;   /* host, [cout] */
    int cin, cout;
} rto_guidance_layer;
int rto_guidance_net_create_layers(const rto_guidance_layer* layers, int num_layers, int levels, int device, rto_guidance_net** out);
/* halo = pixels of aux around a map value that it depends on (= num_layers); packed_route = 1 for the reference shape */
typedef struct rto_guidance_net_info {
    int c1, levels, num_layers, halo, packed_route;
} rto_guidance_net_info;
int rto_guidance_net_get_info(const rto_guidance_net* net, rto_guidance_net_info* info);
/* aux: device [n][8][H][W] fp32; outputs: device [n][levels][H][W] fp32 (weight_map, guidance_map) */
int rto_guidance_net_forward(const rto_guidance_net* net, void* stream, const float* aux, int n, int H, int W,
                             float* weight_map, float* guidance_map);
/* flags: RTO_NET_AUX_SQUARES_IMPLIED -- the caller guarantees that aux planes 4..7 are the fp32 squares of planes
 * 0..3, which is how the renderer fills them (volrend.cu:195-202); the kernel then reads planes 0..3 only and
 * squares them itself: the same values from half the bytes.  Results are bit-identical to flags = 0 on such input. */
#define RTO_NET_AUX_SQUARES_IMPLIED 1
/* RTO_NET_INPUT_RGBA (round 5) -- `aux` is not an aux buffer but an interleaved image, device [n][H][W][4] fp32 = (r, g, b,
 * alpha): the values of aux planes 0..3 (volrend.cu:187-194), as a LEAN batched launch leaves them in the context's noisy
 * buffer (rto_ctx_set_lean_outputs).  Squares implied.  Bit-identical maps to the aux-buffer input. */
#define RTO_NET_INPUT_RGBA 2
/* RTO_NET_INPUT_SPARSE (round 6; with RTO_NET_INPUT_RGBA, tile marks and the packed route only) -- the image is that of a SPARSE
 * lean launch (rto_ctx_set_lean_outputs level 2): it holds nothing for the pixels of unmarked (culled) render tiles, which are
 * the background by construction; the network takes (background x 3, alpha 0) for them and stores no maps for the tiles it
 * skips -- rto_filtering_packed_culled with the same marks substitutes both.  Same denoised images, bit for bit. */
#define RTO_NET_INPUT_SPARSE 4
int rto_guidance_net_forward_ex(const rto_guidance_net* net, void* stream, const float* aux, int n, int H, int W,
                                float* weight_map, float* guidance_map, int flags);
/* The denoise stage (Denoiser::denoise, denoiser.cpp:31-61) as two launches that keep the maps in their native
 * precision: _forward_packed runs the network and leaves its 8 output channels as fp16 (4 softmax logits + 4
 * guidance values per pixel, [n][H][W][8], in a scratch buffer the handle owns) -- the reference's `.float()` only
 * widens those values; rto_filtering_packed then runs the factorised filter (RTO_FILTER_FACTORISED) on them, taking
 * the softmax itself: img_in / img_out [n][H][W][4] fp32.  Output = rto_guidance_net_forward_ex +
 * rto_filtering_batch_mode(FACTORISED) bit for bit, from half the map bytes.  Same stream for both calls; one
 * handle per stream at a time.
 * rto_filtering_packed is told the extent of the images it is handed and refuses (RTO_E_INVALID) one that differs from
 * the maps' -- a handle shared between contexts of different batch sizes cannot overrun the smaller one.  The scratch
 * grows on demand, which synchronises the device once; rto_guidance_net_reserve sizes it up front so that a timed or
 * captured region never does. */
int rto_guidance_net_forward_packed(rto_guidance_net* net, void* stream, const float* aux, int n, int H, int W, int flags);
int rto_guidance_net_reserve(rto_guidance_net* net, int n, int H, int W);
int rto_filtering_packed(const rto_guidance_net* net, void* stream, const float* img_in, float* img_out, int n, int H, int W);
/* rto_filtering_packed that does not filter where there is nothing to filter: a 32x32 output tile whose inputs (its 40x40
 * staged pixels and the 5x5 aux neighbourhood behind each of their map values) all lie inside the frame and in unmarked tiles
 * of `tile_marks` (rto_ctx_tile_marks of the launch that rendered img_in and the network's aux; frame f of the marks = image
 * f) reads only background pixels and the network's background maps.  Every such tile computes the same 32x32 values; the
 * handle measures them once per `background` by running the two kernels on a synthetic background frame (the first call
 * with a new brightness synchronises `stream`) and copies them instead.  Output = rto_filtering_packed bit for bit.
 * tile_marks == NULL: rto_filtering_packed.
 * rto_guidance_net_forward_packed_culled is the same idea one stage earlier: a 32x8 tile of the network whose 36x12 input
 * pixels all lie inside the frame and in unmarked tiles is filled with the network's background output (8 fp16 values,
 * measured on the same synthetic frame) instead of being computed.  Maps = rto_guidance_net_forward_packed's bit for bit. */
/* The two stages on fp32 weight / guidance planes (the reference's tensors; RTO_FILTER_EXACT = the bit-exact route) with the
 * same tile skipping: the maps must be this network's output for the aux of the launch the marks belong to.  Outputs =
 * rto_guidance_net_forward_ex / rto_filtering_batch_mode bit for bit.  tile_marks == NULL: those functions. */
int rto_guidance_net_forward_culled(rto_guidance_net* net, void* stream, const float* aux, int n, int H, int W, float* weight_map,
                                    float* guidance_map, int flags, const uint32_t* tile_marks, int words_per_frame, float background);
int rto_filtering_culled(rto_guidance_net* net, void* stream, const float* weight_map, const float* guidance_map, int H, int W, int n,
                         const float* img_in, float* img_out, int mode, const uint32_t* tile_marks, int words_per_frame, float background);
int rto_guidance_net_forward_packed_culled(rto_guidance_net* net, void* stream, const float* aux, int n, int H, int W, int flags,
                                           const uint32_t* tile_marks, int words_per_frame, float background);
int rto_filtering_packed_culled(rto_guidance_net* net, void* stream, const float* img_in, float* img_out, int n, int H, int W,
                                const uint32_t* tile_marks, int words_per_frame, float background);
/* Denoiser::denoise (denoiser.cpp:31-61) in one call, for the n frames of `ctx` from its selected slot on: the network on the
 * context's aux buffer, the filter from its noisy buffer into its image buffer.  mode RTO_FILTER_FACTORISED: packed fp16
 * maps + factorised filter (the throughput route; a general net: fp32 planes + the factorised filter); RTO_FILTER_EXACT: fp32
 * planes (a scratch the handle owns, 8 * levels B per pixel) + the bit-exact filter.  A three-layer net culls its network
 * tiles only: the filter kernels' tile test covers the receptive field of two layers.  When the frames are those of the last rto_launch_renderer_batch on `ctx` its tile marks
 * are used (the *_culled calls above); after a single-frame launch the plain kernels run.  Same results either way.
 * Like the packed scratch, the plane scratch grows on demand and growing synchronises the device once: call it once at the
 * largest extent before a timed or captured region. */
int rto_denoise(rto_guidance_net* net, rto_ctx* ctx, int n, int mode, void* stream);
/* The launch shape of the denoise kernels for n frames of H x W.  In the factorised filter (filter_fast, tiles 32 x 16) and in
 * the GuidanceNet kernels (tiles 32 x 8) a workgroup walks a STRIP of tiles along x, the next tile's loads in flight while the
 * current one computes; the launchers choose the strip from the launch size: s = 5 (filter) / 13 (network), and while s > 1 and
 * ceil(tiles_x / s) * tiles_y * n < 2048 one less -- a batch gets full strips, a lone frame short ones.  This call reports what
 * a launch of that extent uses, computed by the functions the launchers call (the filter kernel derives its strip from the
 * grid, ceil(tiles_x / ceil(tiles_x / s)): the same number unless tiles_x splits evenly into shorter strips).  No result
 * depends on the strip; the tests use the query to prove which strips they reach.
 * Touches no device.  RTO_E_INVALID: a non-positive extent or a null output. */
int rto_denoise_launch_strips(int n, int H, int W, int* filter_strip, int* net_strip);
void rto_guidance_net_free(rto_guidance_net* net);

/* ---- image metrics (denoiser/metrics.py:7-9, 61-79; denoiser/runner.py:126-160) ----
 * Per frame, of a predicted against a true image, [n][H][W][4] each, r, g, b only:
 *   mse   = mean of (p - t)^2 over the 3 H W values;  psnr = -10 log10(mse), +inf when mse is 0
 *   smape = mean of |p - t| / (|p| + |t| + 1e-5)
 *   ssim  = pytorch_msssim.ssim(X, Y, data_range = 1): 11-tap Gaussian window (sigma 1.5, normalised), separable, no padding --
 *           the map is (H - 10) x (W - 10); per channel mu = G(x), var = G(x^2) - mu^2, cov = G(xy) - mu_x mu_y, C1 = 1e-4,
 *           C2 = 9e-4, map = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1) * (2 cov + C2) / (var_x + var_y + C2); the mean of the
 *           map over positions and channels.  NaN when H < 11 or W < 11 (the other three are still computed).
 * All arithmetic after the input conversion is float64 on the device, compiled without FMA contraction: identical inputs give
 * ssim == 1.0, mse == 0 and smape == 0 exactly.  Sums are taken in a fixed order without atomics: a frame's result depends on
 * neither n, its position in the batch nor the run.  A non-finite r, g or b makes that frame's four values NaN and leaves
 * the other frames untouched.
 * Formats, each side on its own: RTO_IMAGE_RGBA32F (the context's image layout; 16-byte aligned) or RTO_IMAGE_RGBA8 (value / 255.0f
 * in float32; 4-byte aligned).  RTO_METRICS_TRUTH_OVER_BACKGROUND: the true image's rgb becomes rgb * a + background * (1 - a),
 * in float32 with separate multiplies and adds (denoiser/dataset.py:82-84, where the background is 1), before the promotion
 * to double.
 * RTO_E_INVALID, decided before anything is enqueued: a null argument; n, H or W < 1; an unknown format or unknown flag bits; a
 * non-finite background with the flag set; pred, truth or device_out misaligned or not memory of the handle's device; n H W >
 * 2^31 - 1.  The handle owns the partial-sum scratch ([frame][workgroup][4] doubles) and, for rto_metrics_compute, the device
 * results; both grow on demand, and growing synchronises the device once (as rto_guidance_net_reserve's scratch does): call once
 * at the largest extent before a timed or captured region.  One handle serves one stream at a time. */
#define RTO_IMAGE_RGBA32F 0
#define RTO_IMAGE_RGBA8 1
#define RTO_METRICS_TRUTH_OVER_BACKGROUND 1
typedef struct {
    double mse, psnr, smape, ssim;
} rto_frame_metrics;
typedef struct rto_metrics rto_metrics;
int rto_metrics_create(int device, rto_metrics** out);
void rto_metrics_free(rto_metrics* m);
/* asynchronous on `stream`; device_out: device memory [n][4] doubles = mse, psnr, smape, ssim */
int rto_metrics_compute_async(rto_metrics* m, void* stream, const void* pred, int pred_format, const void* truth, int truth_format,
                              int n, int H, int W, int flags, float background, double* device_out);
/* the same, results copied to host_out[n]; synchronises `stream` before it returns */
int rto_metrics_compute(rto_metrics* m, void* stream, const void* pred, int pred_format, const void* truth, int truth_format, int n,
                        int H, int W, int flags, float background, rto_frame_metrics* host_out);
/* Host only, no device: an 8-bit RGB or RGBA, non-interlaced PNG -> RGBA8 [height][width][4] (alpha 255 for RGB).  rgba == NULL
 * or cap < width * height * 4: sizes only (signature and IHDR are validated), returns RTO_OK with *width / *height set.
 * The signature, every chunk's length against the file size and every chunk's CRC are checked.  RTO_E_INVALID: a null path /
 * width / height.  RTO_E_IO, with a message that names the file: a file that cannot be opened, and everything this reader does
 * not take -- 16-bit, palette, grey or interlaced images, a truncated file, inflated data shorter or longer than the image, a
 * bad CRC, a filter type above 4. */
int rto_image_read_png(const char* path, int* width, int* height, uint8_t* rgba, size_t cap);
/* Host only: RGBA8 [height][width][4] -> an 8-bit RGBA PNG, the writer of the headless renderer (renderer/src/imwrite.cpp:14-86:
 * filter 0, stored deflate blocks).  RTO_E_INVALID: a null argument or a non-positive extent; RTO_E_IO: the file cannot be written. */
int rto_image_write_png(const char* path, const uint8_t* rgba, int width, int height);

/* ---- quantiser (renderer/scripts/compress_octree.py:68-119; the median cut that script takes from svox) ----
 * A deterministic median cut of m rows of three fp16 values into 2^bits boxes: ids[m] (uint16) = the box of every row,
 * palette[2^bits][3] (fp16) = the mean of every box.  All 16-bit arrays are bit patterns.  1 <= m <= 2^31 - 1, bits in 1..16.
 *   key      of a value with bit pattern h: the order-preserving uint16 (h & 0x8000 ? ~h : h | 0x8000); the order of values IS the
 *            order of keys, so -0 sorts before +0.
 *   a round  All rows start in box 0.  Round l = 0 .. bits - 1, for every box b < 2^l holding cnt rows: lo[c], hi[c] = the
 *            minimum and maximum of the box on axis c, converted to float32; the extent hi[c] - lo[c] is one IEEE float32
 *            subtraction; the split axis is the lowest c with the largest extent.  Order the box's rows by (key on that axis,
 *            original row index): the first (cnt + 1) / 2 rows (integer division) go to box 2b, the rest to box 2b + 1.  An
 *            empty box yields two empty boxes; a one-row box sends its row to 2b.
 *   ids      after `bits` rounds, ids[row] = the row's box.
 *   palette  for box b and channel c, S = the exact integer sum of value * 2^24 (every fp16 value is an integer in those units);
 *            mean = (double)S / (double)cnt * 2^-24, converted to float32 and then to fp16, round to nearest even both times;
 *            cnt = 0 gives +0.  Integer sums: the palette does not depend on any order of summation.
 * Nothing is left to the implementation: the device entry, the host twin and the numpy model of the tests give the same bits.
 * RTO_E_INVALID, with a text: a NaN or an infinity in any row; m * max|value| * 2^24 >= 2^63 (a box sum could leave an int64;
 * decided on the actual maximum, out of reach of real SH coefficients); a null argument, m < 1 or above 2^31 - 1, bits outside
 * 1..16; on the device entry also pointers that are misaligned or not memory of the handle's device.  The argument refusals are
 * decided before anything is enqueued; the two that depend on the values are found by the kernels and reported after the run,
 * with palette and ids unspecified.
 * rto_quantize_median_cut is a TOOL path, not a frame path: it enqueues its kernels on `stream`, reads the refusal flags back and
 * returns after the stream has drained.  Kernel boundaries are its only grid-wide synchronisation and integer atomics its only
 * atomics: two runs give the same bits.  The handle owns all scratch (about 24 m bytes), which grows on demand and is reused
 * across calls; growing synchronises the device once.  One handle serves one stream at a time.
 * rto_quantize_median_cut_host is the host twin: host pointers, no device, the definition followed literally. */
typedef struct rto_quantizer rto_quantizer;
int rto_quantizer_create(int device, rto_quantizer** out);
void rto_quantizer_free(rto_quantizer* q);
int rto_quantize_median_cut(rto_quantizer* q, void* stream, const uint16_t* rows /* device [m][3] */, int64_t m, int bits,
                            uint16_t* palette /* device [2^bits][3] */, uint16_t* ids /* device [m] */);
int rto_quantize_median_cut_host(const uint16_t* rows /* [m][3] */, int64_t m, int bits, uint16_t* palette /* [2^bits][3] */,
                                 uint16_t* ids /* [m] */);

/* ---- simplifier (what svox's shrink_to_fit and the pruning of PlenOctree extraction do; the reference holds no counterpart) ----
 * Makes a tree smaller AS A TREE without changing the field it stores: every point query of the result returns the bits the
 * input returns (+0 in all D halves where a leaf was killed).
 *   input    child[cap][N^3] (int32): relative node offsets, 0 = leaf, as svox writes them; data[cap][N^3][D]: fp16 bit patterns,
 *            the density is the last of the D; kill_thresh: a float, NaN = no kill.  1 <= cap, cap * N^3 < 2^31, N >= 2, D >= 1.
 *   links    Node 0 is the root.  Slot s of node n with c = child[n][s] != 0 refers to node n + c -- for EVERY n < cap, whether
 *            the walk reaches it or not.  RTO_E_FORMAT, with a text and the outputs unspecified: an n + c outside [1, cap); a
 *            node referred to by more than one slot; a node at level 32 (the root is level 0, a node referred to by a node of
 *            level l is level l + 1).  With those excluded the walk from the root is a tree; a node it does not reach (never
 *            referred to, below such a node, or on a cycle apart from the root) is UNREACHABLE and is dropped.  Every read that
 *            decides this is bounds-checked before the dereference it guards: a malformed array is refused, it never faults.
 *   kill     (kill_thresh not NaN) th = kill_thresh rounded to fp16 (to nearest even, beyond 65504 an infinity).  A leaf slot of
 *            a reachable node whose density half d is not IEEE d > th is DEAD (a NaN density is dead; -0 == +0): its record
 *            becomes D halves +0.
 *   merge    Deepest level first, a parent after all its children: a reachable node other than the root is UNIFORM when its N^3
 *            slots are all leaves and their N^3 records (after the kill) are equal bit for bit.  The slot that refers to it
 *            becomes a leaf holding that record and the node is dropped; cascades finish within the call; the root stays.
 *   compact  The survivors keep their order; a node's new index is its rank among them; an offset becomes
 *            new[target] - new[node]; records move unchanged.  child_out and data_out have room for cap nodes and hold
 *            *out_capacity nodes afterwards (what lies behind is unspecified); node_map[i] (optional, int64, room for cap) = the
 *            old index of new node i.
 *   stats    reachable: nodes the walk reaches; unreachable = cap - reachable; killed: dead leaf slots of reachable nodes,
 *            whatever their record held; merged: uniform nodes dropped; levels: 1 + the deepest level of a surviving node.
 * Nothing is left to the implementation: the device entry, the host twin and the numpy model of the tests give the same bits.
 * RTO_E_INVALID, decided before anything is enqueued: a null pointer (node_map and stats may be NULL), cap < 1, cap * N^3 >= 2^31,
 * N < 2, D < 1, an output that overlaps an input or another output, a pointer not aligned to its element; on the device entry
 * also child, data, child_out, data_out or node_map not memory of the handle's device (out_capacity and stats are host memory).
 * rto_tree_simplify is a TOOL path like rto_quantize_median_cut: it enqueues on `stream`, reads the link flags and the level
 * counts back once before the merge passes (one per level) and the result words once at the end, and returns after the stream
 * has drained.  Kernel boundaries are its only grid-wide synchronisation, integer atomics its only atomics, the scan of the keep
 * flags is reduce-then-scan: two runs give the same bytes.  The handle owns all scratch (about 8 N^3 + 16 bytes per node), which
 * grows on demand and is reused; one handle serves one stream at a time.  data and data_out aligned to 16 bytes with N^3 * D a
 * multiple of 8 (always for N = 2 or 4) take the 16-byte scatter, anything else a half-by-half one.
 * rto_tree_simplify_host is the host twin: host pointers, no handle, no device. */
typedef struct rto_simplify_stats {
    int64_t reachable, unreachable, killed, merged, levels;
} rto_simplify_stats;
typedef struct rto_simplifier rto_simplifier;
int rto_simplifier_create(int device, rto_simplifier** out);
void rto_simplifier_free(rto_simplifier* s);
int rto_tree_simplify(rto_simplifier* s, void* stream, const int32_t* child, const uint16_t* data, int64_t cap, int N, int D,
                      float kill_thresh, int32_t* child_out, uint16_t* data_out, int64_t* out_capacity /* host */,
                      int64_t* node_map /* device, or NULL */, rto_simplify_stats* stats /* host, or NULL */);
int rto_tree_simplify_host(const int32_t* child, const uint16_t* data, int64_t cap, int N, int D, float kill_thresh,
                           int32_t* child_out, uint16_t* data_out, int64_t* out_capacity, int64_t* node_map,
                           rto_simplify_stats* stats);

/* ---- leaf weights (the pruning criterion of PlenOctree extraction: render every training view, record for every leaf the largest
 * compositing weight any ray gives it, drop the leaves that stay under a threshold; the reference holds no counterpart) ----
 * A dense leaf buried behind an opaque surface has a large sigma and weight 0: no density threshold finds it, this does.
 *   weights  one word per slot of child[]: indexed like child[capacity][N][N][N], flattened, in the numbering of the arrays the
 *            tree was uploaded from (the slot query_single_from_root names) -- whichever traversal image is resident, and also
 *            when child[] has been released.  A word is the bit pattern of a float in [0, 1].  The call ACCUMULATES into what
 *            weights holds (max); the caller zeroes it.
 *   rays     For every camera k of the call and every pixel 0 <= x < width, 0 <= y < height the renderer's own ray: set up as
 *            the frame kernels set it up (volrend.cu:23-56,138-144, the NDC warp of an NDC tree included), entered as they enter
 *            the volume with tmax_bg = 1e9f (rt_core.cuh:206-222: double sub-expressions, render_bbox +- 1e-6, delta_scale).  A
 *            ray is not marched when a component of dir or cen is not finite after the set-up, or when it misses the box.
 *   march    float32, every operation rounded once, no contraction:
 *                T = 1.f;  t = tmin
 *                while (t < tmax):
 *                    pos   = cen + t * dir
 *                    leaf, cube_sz, local = query_single_from_root(pos)          (its clamp to [0, 1 - 1e-6f] included)
 *                    dt    = _dda_unit(local, invdir) / cube_sz + step_size
 *                    sigma = (float)(the density half of leaf)
 *                    if (sigma > sigma_thresh):                                   (a NaN density is skipped)
 *                        att = fminf(expf(-((dt * delta_scale) * sigma)), 1.f)    (expf: the library's deterministic one, full range)
 *                        w   = T * (1.f - att)
 *                        weights[leaf] = max(weights[leaf], w)
 *                        T   = T * att
 *                        if (T < stop_thresh) break
 *                    tn = t + dt
 *                    if (!(tn > t)) break         (a step that does not advance ends the ray: no input makes the loop endless)
 *                    t = tn
 *            -- the bookkeeping of the shader backend's trace (rt.frag:244-321) without its colour, on the CUDA backend's ray.
 *            Of rto_options only step_size, sigma_thresh, stop_thresh and render_bbox are read (spp is not validated);
 *            stop_thresh = 0 never stops a ray.
 *   max      w is never NaN and never negative (att lies in [0, 1], T >= 0; an infinite sigma gives att = 0), so the words are
 *            compared as unsigned integers: the result does not depend on the order of the rays, on how the cameras are split
 *            over calls, or on the thread count.  The device entry, the host twin and the numpy restatement of the tests give
 *            the same bits.
 * rto_tree_leaf_weights: asynchronous on `stream`; no allocation, no host synchronisation, no host-to-device copy (the cameras
 * travel in the kernel arguments, 32 per launch; a launch takes a run of consecutive cameras of one size, so mixed sizes are
 * accepted); n == 0 launches nothing.  Only sigma is read: quantised-direct and compact-records trees work.  The kernel walks what
 * the tree has resident (the two-level image, the one-level image, or child[] with the float descent); a tree that has neither an
 * image nor child[] / data[] resident is RTO_E_UNSUPPORTED.
 * RTO_E_INVALID, decided before anything is enqueued: a null pointer; n < 0; a camera with width or height < 1 (height at most
 * 1048560), fx or fy not finite or zero; weights not 4-byte aligned; on the device entry weights not memory of the tree's device.
 * rto_leaf_weights_host is the host twin: host pointers, no device; the root-restart float descent over child[] (links are checked
 * first: RTO_E_FORMAT for an offset outside [1, capacity) or a node reached twice); threads <= 0 means one thread, and the result
 * does not depend on threads. */
int rto_tree_leaf_weights(const rto_tree* tree, const rto_camera* cams /* host [n] */, int n, const rto_options* opt,
                          uint32_t* weights /* device [capacity * N^3] */, void* stream);
int rto_leaf_weights_host(const int32_t* child, const uint16_t* data, int64_t capacity, int N, int data_dim,
                          const float scale[3], const float offset[3], const float* ndc /* {w,h,focal} or NULL */,
                          const rto_camera* cams, int n, const rto_options* opt, int threads, uint32_t* weights);

/* ---- tree fit (the last step of PlenOctree extraction: the leaf values are optimised against the training images by gradient
 * descent on a fixed structure, PlenOctrees' octree/optimization.py; the reference renderer holds no counterpart) ----
 * The images are rendered by deterministic compositing (a transmittance T, no RNG), the loss is 1/2 sum over rays |out - target|^2,
 * and its gradient with respect to the leaf values is accumulated in 64-bit FIXED POINT, so that no order can change a bit.
 *   params   float32 [capacity][N][N][N][D], D = data_dim, in the numbering of the arrays the tree was uploaded from: indexed like
 *            weights[] of the leaf weights, times D.  The tree handle gives the TOPOLOGY and the SUPPORT, params the field.
 *   support  A leaf is DENSE when its uploaded density half is > sigma_thresh AND params[slot][D-1] > sigma_thresh (a NaN fails
 *            either test).  A leaf that is not dense is stepped over and never receives a gradient: the support can shrink and
 *            never grows.  The first test is free on the image walks (the walk returns the half), so only a dense leaf pays for
 *            its address.
 *   formats  RGBA (D = 4) and SH with basis_dim B in {1, 4, 9, 16, 25} (D = 3 B + 1).  RTO_E_UNSUPPORTED: SG / ASG trees, trees
 *            loaded with RTO_TREE_QUANT_DIRECT or RTO_TREE_COMPACT_RECORDS, a tree with neither an image nor child[] / data[]
 *            resident.
 *   ray      that of the leaf weights, word for word: the set-up (NDC warp included), the entry with tmax_bg = 1e9f, the loop and
 *            the three ways it ends (t >= tmax, T < stop_thresh, a step that does not advance).  A ray whose set-up is not finite
 *            or that misses the box is not marched: out = bg.  Of rto_options step_size, sigma_thresh, stop_thresh, render_bbox
 *            and background_brightness (bg) are read; rot_dirs and basis_minmax are NOT, and a call with non-default values of
 *            either is RTO_E_INVALID.
 *   colour   c[ch] of a dense leaf, p = params[slot]:  RGBA: p[ch].  SH: Y = the tree's SH basis (lumisphere.hpp:38-80: double
 *            literals, one rounding per assignment) at vdir, the unit direction of the set-up before the NDC warp and before the
 *            entry scales it;  z = Y[0] * p[ch*B];  z = z + Y[k] * p[ch*B + k] for k = 1 .. B-1;  c[ch] = 1.f / (1.f + expf(-z)),
 *            expf the library's deterministic one (the probe's colour, above).
 *   forward  float32, every operation rounded once, no contraction:
 *                T = 1.f;  acc[ch] = 0.f;  t = tmin
 *                while (t < tmax):
 *                    pos, leaf, cube_sz, local, dt       as the leaf weights
 *                    if (dense):   sigma = p[D-1]
 *                        delta = dt * delta_scale
 *                        att   = fminf(expf(-(delta * sigma)), 1.f)
 *                        w     = T * (1.f - att)
 *                        acc[ch] = acc[ch] + w * c[ch]
 *                        T = T * att;  if (T < stop_thresh) break
 *                    tn = t + dt;  if (!(tn > t)) break;  t = tn
 *                out[ch] = acc[ch] + T * bg
 *                r[ch] = out[ch] - target[ch];   loss_ray = (r[0]*r[0] + r[1]*r[1]) + r[2]*r[2]
 *            A pixel whose target holds a NaN in any channel is MASKED: not marched, not counted, no loss, no gradient, and its
 *            image pixel is not written.
 *   backward the ray is marched a second time by the same operations, so T, att, w, c and acc repeat bit for bit.  At a dense
 *            sample, with acc the accumulator AFTER the sample and T the transmittance BEFORE it:
 *                g[D-1] = delta * s,   s = r[0] * x[0];  s = s + r[1] * x[1];  s = s + r[2] * x[2],
 *                                      x[ch] = (T * att) * c[ch] - (out[ch] - acc[ch])
 *                gc = r[ch] * w;   RGBA: g[ch] = gc;   SH: gz = gc * (c[ch] * (1.f - c[ch])),  g[ch*B + k] = gz * Y[k]
 *            The clamp in att and the early stop are treated as constants.
 *   sums     grad is int64 with the shape of params.  A contribution g enters as q = (int64_t)rint((double)g' * 2^36) (to nearest
 *            even), g' = 0 for a NaN g, else g clamped to +-2^16 -- so |q| <= 2^52 and the product, the rounding and the
 *            conversion are exact -- added with a wrapping 64-bit integer add.  stats[0] += q(loss_ray) in the same way;
 *            stats[1] += 1 per unmasked ray (the rays that are not marched included).  Integer adds commute and associate: the
 *            words do not depend on the order of the rays, on how the cameras are split over calls, on thread counts or on any
 *            pre-reduction.  The device entry, the host twin and the numpy restatement of the tests give the same bytes.
 *            Headroom (a choice, not a measurement): 2^-36 = 1.5e-11 per contribution, against SH gradients bounded by about
 *            |r| w / 4 |Y| < 1; a word takes 2^27 contributions of magnitude 1 before it wraps.
 *   step     p = p - lr * g,  g = (float)((double)q * 2^-36): two float roundings, no FMA; then the grad word is zeroed.
 *            Elementwise over the whole array.  The entry takes no normaliser: fold 2 / (3 rays) of a mean squared error into lr.
 * rto_tree_fit_grad: asynchronous on `stream`; no allocation, no host synchronisation, no host-to-device copy (cameras, targets
 * and images travel in the kernel arguments, 32 per launch; runs of one size become launches); n == 0 launches nothing.  images:
 * NULL, or per camera NULL or where out is written.  grad == NULL: only the forward march runs -- the deterministic render of the
 * field.  targets may be NULL only with grad == NULL and stats == NULL (nothing is masked then).  The call ACCUMULATES into grad
 * and stats; the caller zeroes them.
 * RTO_E_INVALID, decided before anything is enqueued, with a text naming the argument and the camera: a null tree, params,
 * options, cams with n > 0, or targets[k]; n < 0; the camera checks of the leaf weights; params, targets[k] or images[k] not
 * 4-byte aligned, grad or stats not 8-byte aligned; params or grad overlapping a target or an image; on the device entry any of
 * them not memory of the tree's device.
 * rto_fit_sgd_step: asynchronous; params and grad (count elements each) memory of one device.
 * rto_fit_grad_host / rto_fit_sgd_step_host are the host twins: host pointers, no device; `data` (fp16 bits) gives the support,
 * data_format is "RGBA" or "SH<B>"; links are checked as rto_leaf_weights_host checks them; the result does not depend on
 * threads. */
int rto_tree_fit_grad(const rto_tree* tree, const float* params, const rto_camera* cams /* host [n] */,
                      const float* const* targets /* host [n] of device [H][W][3] f32 */,
                      float* const* images /* host [n] of device [H][W][3] f32, or NULL; entries may be NULL */, int n,
                      const rto_options* opt, int64_t* grad /* or NULL: forward only */, uint64_t* stats /* device [2] or NULL */,
                      void* stream);
int rto_fit_sgd_step(float* params, int64_t* grad, int64_t count, float lr, void* stream);
int rto_fit_grad_host(const int32_t* child, const uint16_t* data, const float* params, int64_t capacity, int N, int data_dim,
                      const char* data_format, const float scale[3], const float offset[3], const float* ndc /* {w,h,focal} or NULL */,
                      const rto_camera* cams, const float* const* targets, float* const* images, int n, const rto_options* opt,
                      int threads, int64_t* grad, uint64_t* stats);
int rto_fit_sgd_step_host(float* params, int64_t* grad, int64_t count, float lr);
/* The fit on rays the CALLER supplies -- the counterpart of rto_launch_rays: shuffled ray batches across all images, rays of
 * non-pinhole cameras, rays kept after a mask or picked by a sampler.  origins, dirs, targets, out: [n][3] float32.
 *   set-up   Ray i is a pixel whose set-up produced  dir = vdir = normalize3(dirs[i])  (invnorm = 1.f / sqrtf(x*x + y*y + z*z),
 *            three products: the operations of the camera set-up; dirs[i] may have any length)  and  cen = origins[i];  then the
 *            NDC warp of an NDC tree and offset + scale * cen, exactly the tail of the camera set-up.  The SH basis is taken at
 *            vdir.  EVERYTHING AFTER THE SET-UP is rto_tree_fit_grad's, word for word: the entry with tmax_bg = 1e9f, both
 *            marches, the fixed point, the sums.  A NaN in targets[i] MASKS ray i: not marched, not counted, out[i] not
 *            written.  A component of dir or cen that is not finite after the set-up, or a miss of the box: not marched,
 *            out[i] = bg, and the ray is counted; a zero or non-finite direction and a non-finite origin fall under this by
 *            arithmetic (0 * inf), there is no separate test.  No per-ray t_max and no per-ray backdrop: every ray ends at the
 *            box or at tmax_bg, and background_brightness is the backdrop.
 *   identity Integer adds commute: on the rays of a camera (dirs[i] = M xyz(x, y) before normalising, origins[i] = the camera's
 *            position), in any order and any split over calls, the entry gives the grad, stats and image bytes that
 *            rto_tree_fit_grad gives on the camera.
 * Formats, the support, the RTO_E_UNSUPPORTED cases and the walks are rto_tree_fit_grad's.  grad == NULL: only the forward
 * march runs; targets == NULL only with grad == NULL and stats == NULL; out may be NULL.  The call ACCUMULATES into grad and
 * stats; the caller zeroes them.  The device entry is asynchronous on `stream`: no allocation, no host synchronisation, no copy;
 * n == 0 launches nothing; a call becomes launches of at most 2^30 rays, every ray index is 64-bit.
 * RTO_E_INVALID, decided before anything is enqueued, with a text naming the argument: a null tree, params or options; null
 * origins or dirs with n > 0; n < 0; params, origins, dirs, targets or out not 4-byte aligned, grad or stats not 8-byte aligned;
 * null targets with grad or stats set; params or grad overlapping origins, dirs, targets or out; out overlapping origins, dirs or
 * targets; non-default rot_dirs or basis_minmax; on the device entry any of them not memory of the tree's device.
 * rto_fit_grad_rays_host is the host twin (host pointers, no device; the tree's arrays as rto_fit_grad_host takes them): threads
 * run over contiguous ranges of rays, and the result does not depend on threads. */
int rto_tree_fit_grad_rays(const rto_tree* tree, const float* params, const float* origins /* device [n][3] */,
                           const float* dirs /* device [n][3] */, const float* targets /* device [n][3] or NULL */,
                           float* out /* device [n][3] or NULL */, int64_t n, const rto_options* opt, int64_t* grad /* or NULL */,
                           uint64_t* stats /* device [2] or NULL */, void* stream);
int rto_fit_grad_rays_host(const int32_t* child, const uint16_t* data, const float* params, int64_t capacity, int N, int data_dim,
                           const char* data_format, const float scale[3], const float offset[3], const float* ndc /* {w,h,focal} or NULL */,
                           const float* origins, const float* dirs, const float* targets, float* out, int64_t n, const rto_options* opt,
                           int threads, int64_t* grad, uint64_t* stats);
/* The SPARSE step: remember which leaves a batch reached, and step those rows only -- so that a small batch does not stream the
 * whole of params and grad, and so that an optimiser with moments (RMSProp, Adam) touches its state only there.
 *   touched  a bitmap uint32_t[(slots + 31) / 32], slots = capacity * N^3: slot s is bit s & 31 of word s >> 5, in the numbering
 *            of params.  A call sets the bit of every slot that the backward march of an unmasked ray visits as a DENSE sample:
 *            exactly the slots for which the backward march adds a contribution, whether or not its fixed-point value is zero.
 *            The call ACCUMULATES into the bitmap as it does into grad; the caller zeroes it.  The set does not depend on the
 *            order of the rays, on splits over calls or on threads, and every slot with a non-zero grad word has its bit set.
 *            A masked ray, a miss and a ray that is not marched mark nothing.
 * rto_tree_fit_grad_rays_touched: rto_tree_fit_grad_rays plus the bitmap.  grad and touched are both REQUIRED (a forward-only
 * call uses rto_tree_fit_grad_rays); the out, grad and stats bytes are those of rto_tree_fit_grad_rays.  RTO_E_INVALID, decided
 * before anything is enqueued, with a text naming the argument: everything rto_tree_fit_grad_rays refuses; a null grad or
 * touched; touched not 4-byte aligned; touched overlapping params, grad, stats, origins, dirs, targets or out; touched not
 * memory of the tree's device.  Cameras need no entry of their own: on the rays of a camera the ray entry gives the camera
 * entry's bytes (the identity above).  rto_fit_grad_rays_touched_host is the host twin.
 *   list     rto_fit_touched_list writes the set slots in ASCENDING order to list[] and their total number to count[0]; only
 *            the first min(count, list_capacity) are written.  clear != 0 zeroes the bitmap in the same pass.  Bits at or beyond
 *            `slots` in the last word are ignored, and cleared under clear.  Asynchronous on `stream`: no allocation, no host
 *            synchronisation, no copy; three launches (a popcount sum per block of RTO_FIT_TOUCHED_BLOCK_WORDS words, one
 *            workgroup that scans the block sums, the scatter), no workgroup waits for another.  scratch: device memory of
 *            rto_fit_touched_scratch_bytes(slots) bytes, 4-byte aligned.  0 <= slots < 2^31.  RTO_E_INVALID: a null touched,
 *            count or scratch, a null list with list_capacity > 0, slots or list_capacity out of range, scratch_bytes too
 *            small, touched / list / scratch not 4-byte or count not 8-byte aligned, memory of different devices.
 *            rto_fit_touched_list_host is the host twin, without scratch.
 *   step     rto_fit_step_sparse: for every list position j < min(count[0], list_capacity), s = list[j] (an entry >= slots is
 *            skipped) and every k < row, on element i = s * row + k, all in float32, every operation rounded once, no FMA,
 *            IEEE division and sqrtf (csrc/rto_fit_optim.h states it once for the kernel and the host twin):
 *                g = from_fixed(grad[i]) * grad_scale;   grad[i] = 0
 *                RTO_FIT_SGD      p = p - lr * g
 *                RTO_FIT_RMSPROP  v = beta2 * v + ((1.f - beta2) * g) * g
 *                                 p = p - lr * (g / (sqrtf(v) + eps))
 *                RTO_FIT_ADAM     m = beta1 * m + (1.f - beta1) * g
 *                                 v = beta2 * v + ((1.f - beta2) * g) * g
 *                                 p = p - lr * ((m / bias1) / (sqrtf(v / bias2) + eps))
 *            bias1 and bias2 are the CALLER's floats, 1 - beta^t for step t: the entry counts no steps.  The moments of a leaf
 *            that was not listed do NOT decay: the lazy rule of torch.optim.SparseAdam and of Plenoxels.  With grad_scale == 1.f
 *            and a finite lr >= 0, RTO_FIT_SGD over a list that covers every non-zero grad row leaves the bytes of
 *            rto_fit_sgd_step in params and an all-zero grad.  m and v are float32 arrays like params (m: ADAM only; v: RMSPROP
 *            and ADAM; else ignored).  count is read ON THE DEVICE: a step needs no host round trip; count[0] == 0 does nothing.
 *            Asynchronous; a grid of fixed size, no atomics.  RTO_E_INVALID: a null params, grad, list, count or options; a
 *            pointer not aligned (4 bytes, grad and count 8); row < 1; slots or list_capacity out of range; an unknown kind; a
 *            null m for ADAM or v for RMSPROP / ADAM; memory of different devices.  rto_fit_step_sparse_host is the host twin. */
#define RTO_FIT_SGD 0
#define RTO_FIT_RMSPROP 1
#define RTO_FIT_ADAM 2
#define RTO_FIT_TOUCHED_BLOCK_WORDS 2048 /* bitmap words per workgroup of the list's sum and scatter launches */
typedef struct rto_fit_optim {
    int kind; /* RTO_FIT_SGD, RTO_FIT_RMSPROP, RTO_FIT_ADAM */
    float lr, grad_scale, beta1, beta2, eps, bias1, bias2;
} rto_fit_optim;
int rto_tree_fit_grad_rays_touched(const rto_tree* tree, const float* params, const float* origins, const float* dirs,
                                   const float* targets, float* out, int64_t n, const rto_options* opt, int64_t* grad,
                                   uint64_t* stats, uint32_t* touched /* device [(slots + 31) / 32] */, void* stream);
int rto_fit_grad_rays_touched_host(const int32_t* child, const uint16_t* data, const float* params, int64_t capacity, int N, int data_dim,
                                   const char* data_format, const float scale[3], const float offset[3], const float* ndc,
                                   const float* origins, const float* dirs, const float* targets, float* out, int64_t n,
                                   const rto_options* opt, int threads, int64_t* grad, uint64_t* stats, uint32_t* touched);
int rto_fit_touched_block_words(void); /* RTO_FIT_TOUCHED_BLOCK_WORDS of the library */
int64_t rto_fit_touched_scratch_bytes(int64_t slots); /* -1: slots out of range */
int rto_fit_touched_list(uint32_t* touched, int64_t slots, int clear, uint32_t* list, int64_t list_capacity,
                         uint64_t* count /* device [1] */, void* scratch, int64_t scratch_bytes, void* stream);
int rto_fit_touched_list_host(uint32_t* touched, int64_t slots, int clear, uint32_t* list, int64_t list_capacity, uint64_t* count);
int rto_fit_step_sparse(float* params, int64_t* grad, float* m /* ADAM only */, float* v /* RMSPROP, ADAM */, int64_t slots,
                        int row /* D */, const uint32_t* list, const uint64_t* count /* device [1] */, int64_t list_capacity,
                        const rto_fit_optim* o, void* stream);
int rto_fit_step_sparse_host(float* params, int64_t* grad, float* m, float* v, int64_t slots, int row, const uint32_t* list,
                             const uint64_t* count, int64_t list_capacity, const rto_fit_optim* o);

/* ---- grid builder (the first step of PlenOctree extraction: a field evaluated on a regular grid becomes an octree; svox does
 * it on the CPU, the reference holds no counterpart) ----
 * Builds child[] / data[] (N = 2) from a dense grid of records.  The result is the tree the simplifier leaves of the grid's full
 * octree: grid -> tree -> rto_tree_query at the voxel centres returns the grid's bits (+0 in all D halves where a voxel was
 * killed).
 *   input    grid[R][R][R][D], fp16 bit patterns, R = 2^L with 1 <= L <= 10, D >= 1; the density is the last of the D halves, as
 *            in data[].  grid[i][j][k] is the voxel that covers the tree coordinates [i/R,(i+1)/R) x [j/R,(j+1)/R) x
 *            [k/R,(k+1)/R): the first index is x, the axis order of child[n][i][j][k] (slot 4 i + 2 j + k).  kill_thresh: a
 *            float, NaN = no kill.  Every index into the grid is 64-bit.
 *   kill     The simplifier's rule: th = kill_thresh rounded to fp16 (to nearest even, beyond 65504 an infinity); a voxel whose
 *            density half d is not IEEE d > th is DEAD (a NaN density is dead; -0 == +0) and its record counts as D halves +0.
 *   cells    The cell of level l (0 <= l <= L) with Morton code m covers 2^(L-l) voxels per side; m holds three bits per level, x
 *            the most significant of each triple, so the children of cell m are the cells 8 m + slot of level l + 1.  A cell of
 *            level L (a voxel) is UNIFORM.  A cell of level 1 <= l < L is uniform when its eight children are uniform and
 *            their records (after the kill) are equal bit for bit: +0 and -0 differ, two NaNs with the same bits are equal.  A
 *            uniform cell's record is the record of its min-corner voxel.
 *   tree     The root (level 0) is always node 0, even over a uniform grid.  Nodes are numbered breadth-first: all nodes of
 *            level l before any of level l + 1, within a level by Morton code.  Slot s of the node of cell m at level l looks at
 *            cell 8 m + s of level l + 1: uniform -> child = 0 and the slot holds that cell's record; not uniform -> child is
 *            the relative offset to that cell's node and the slot holds D halves +0 (no averaged level-of-detail records).
 *   stats    nodes; killed: dead voxels, whatever they held; levels: 1 + the deepest level of a node.
 * Nothing is left to the implementation: the device entries, the host twin and the numpy model of the tests give the same
 * bytes, and they are the bytes rto_tree_simplify gives for the grid's full octree (every cell subdivided to level L,
 * breadth-first in Morton order, interior slots zero) with the same kill_thresh.
 * Two passes, because the outputs cannot be sized before the grid has been read.  rto_tree_build_plan reads the grid once,
 * leaves the flags of all cells and the node lists of all levels in the handle, synchronises `stream` once to read the counts back
 * and sets *out_capacity = nodes (also when it refuses the result as too large).  rto_tree_build_write enqueues the kernels that
 * write child_out[nodes][2][2][2] and data_out[nodes][2][2][2][D] of the handle's last successful plan and returns without
 * waiting; the grid must be unchanged and stay alive until they have run.  A TOOL path like rto_tree_simplify: kernel
 * boundaries are the only grid-wide synchronisation, integer counts the only atomics, the scans are reduce-then-scan: two runs
 * give the same bytes.  The handle owns all scratch -- one flag byte per cell of levels 0 .. L - 1, one 32-bit Morton code per
 * possible node of those levels and a word per 256 of them: 5/7 of a byte per VOXEL (0.72), independent of D and of the node
 * count; pass 2 needs none per node -- which grows on demand and is reused; growing synchronises the device once.
 * One handle serves one stream at a time.  A data_out aligned to 16 bytes is written in 16-byte words, another half by half.
 * RTO_E_INVALID, decided before anything is enqueued: a null pointer (stats may be NULL), L outside 1 .. 10, D < 1, a pointer
 * not aligned to its element, an output that overlaps the grid or the other output, grid / child_out / data_out not memory of
 * the handle's device (out_capacity and stats are host memory), rto_tree_build_write without a preceding successful plan on the
 * handle.  A result with nodes * 8 >= 2^31 (the simplifier's bound on a tree) is refused by the plan, with a text.
 * rto_tree_build_host is the host twin: host pointers, no handle, no device.  child_out == data_out == NULL counts only; `room` =
 * the nodes the outputs can hold -- too small is RTO_E_INVALID with *out_capacity and *stats set all the same. */
typedef struct rto_grid_build_stats {
    int64_t nodes, killed, levels;
} rto_grid_build_stats;
typedef struct rto_tree_builder rto_tree_builder;
int rto_tree_builder_create(int device, rto_tree_builder** out);
void rto_tree_builder_free(rto_tree_builder* b);
int rto_tree_build_plan(rto_tree_builder* b, void* stream, const uint16_t* grid /* device */, int L, int D, float kill_thresh,
                        int64_t* out_capacity /* host */, rto_grid_build_stats* stats /* host, or NULL */);
int rto_tree_build_write(rto_tree_builder* b, void* stream, int32_t* child_out, uint16_t* data_out);
int rto_tree_build_host(const uint16_t* grid, int L, int D, float kill_thresh, int32_t* child_out, uint16_t* data_out,
                        int64_t room, int64_t* out_capacity, rto_grid_build_stats* stats);

/* ---- refiner (svox's N3Tree.refine(sel=...): the one structural step that makes a tree FINER; PlenOctree extraction refines where
 * the weights are high; the reference holds no counterpart) ----
 * Splits the K most important leaves: each becomes a node of N^3 leaves that all hold the leaf's record, so every point query of
 * the result returns the bits the input returns, and rto_tree_simplify of the result is rto_tree_simplify of the input.
 *   input    child[cap][N^3] (int32, relative offsets, 0 = leaf) and data[cap][N^3][D] (fp16 bit patterns), as the simplifier
 *            takes them; key[cap * N^3] (uint32, one word per slot, indexed like child; NULL = every key is 1); key_thresh
 *            (uint32); max_new (int64, negative = unbounded); max_level (1 .. 31).
 *   links    The simplifier's rules and refusals, word for word: RTO_E_FORMAT for an n + c outside [1, cap), for a node referred
 *            to by more than one slot, for a node at level 32; every read is bounds-checked before the dereference it guards.
 *            Unreachable nodes are copied unchanged and their slots are never candidates.
 *   candidate  Slot i of a reachable node of level l is a CANDIDATE when child[i] == 0, l + 1 <= max_level and
 *            key[i] >= key_thresh, compared as unsigned integers.  There is no density test: the caller folds it into the key.
 *   selection  C = the number of candidates; K = C when max_new < 0, else min(C, max_new).  SELECTED are the first K candidates
 *            in the order (key descending, slot index ascending) -- a complete order, so nothing depends on the run.
 *   output   cap_out = cap + K.  Nodes 0 .. cap - 1 are the input's bytes except the selected slots' child words: with the
 *            selected slots numbered j = 0 .. K - 1 in ASCENDING SLOT ORDER, selected slot i of node n gets
 *            child_out[i] = (cap + j) - n and keeps its record; node cap + j has child all 0 and each of its N^3 slots holds the
 *            D halves of data[i].  New nodes are appended, as svox appends them.
 *   slot_src (optional, int32 [cap_out * N^3]) slot_src[s] = s for s < cap * N^3 and = i for the slots of node cap + j, so
 *            data_out.reshape(-1, D) == data.reshape(-1, D)[slot_src]; the same gather carries the fit's float32 params and leaf
 *            weights across a refinement.
 *   stats    reachable; candidates = C; selected = K; levels: 1 + the deepest level of a reachable node of the RESULT; cut_key:
 *            the smallest selected key, 0 when K == 0.
 * Nothing is left to the implementation: the device entries, the host twin and the numpy model of the tests give the same bytes.
 * Two passes, like the grid builder, because the outputs cannot be sized before the selection.  rto_tree_refine_plan reads child
 * and key, leaves the per-slot selection and the ranks j in the handle, synchronises `stream` once to read the counts and the link
 * flags back and sets *out_capacity = cap_out and *stats (also when it refuses the result as too large).  rto_tree_refine_write
 * enqueues the kernels that write the outputs of the handle's last successful plan and returns without waiting; child must be
 * unchanged since the plan.  A TOOL path like rto_tree_simplify: kernel boundaries are the only grid-wide synchronisation; integer
 * counts, maxima, minima and one compare-and-swap per link the only atomics; no float arithmetic; the top K come from a radix
 * select over the keys (four 8-bit passes of a 256-bin histogram, the digit picked on the device) and the ranks from a
 * reduce-then-scan over tiles of slots: two runs give the same bytes.  The handle owns all scratch (8 bytes per slot and 8 per
 * node), which grows on demand and is reused; growing synchronises the device once.  One handle serves one stream at a time.
 * data and data_out aligned to 16 bytes with N^3 * D a multiple of 8 are written in 16-byte words, anything else half by half.
 * RTO_E_INVALID, decided before anything is enqueued: a null pointer (key, slot_src and stats may be NULL), cap < 1, N < 2, D < 1,
 * cap * N^3 >= 2^31, max_level outside 1 .. 31, a pointer not aligned to its element, an output that overlaps an input or another
 * output; on the device entries any array that is not memory of the handle's device (out_capacity and stats are host memory);
 * rto_tree_refine_write without a preceding successful plan on the handle.  A result with cap_out * N^3 >= 2^31 is refused by the
 * plan, with a text.
 * rto_tree_refine_host is the host twin: host pointers, no handle, no device.  child_out == data_out == NULL counts only; `room` =
 * the nodes the outputs can hold -- too small is RTO_E_INVALID with *out_capacity and *stats set all the same. */
typedef struct rto_refine_stats {
    int64_t reachable, candidates, selected, levels, cut_key;
} rto_refine_stats;
typedef struct rto_refiner rto_refiner;
int rto_refiner_create(int device, rto_refiner** out);
void rto_refiner_free(rto_refiner* r);
int rto_tree_refine_plan(rto_refiner* r, void* stream, const int32_t* child, const uint32_t* key /* or NULL */, int64_t cap, int N,
                         uint32_t key_thresh, int64_t max_new, int max_level, int64_t* out_capacity /* host */,
                         rto_refine_stats* stats /* host, or NULL */);
int rto_tree_refine_write(rto_refiner* r, void* stream, const int32_t* child, const uint16_t* data, int D, int32_t* child_out,
                          uint16_t* data_out, int32_t* slot_src /* or NULL */);
int rto_tree_refine_host(const int32_t* child, const uint16_t* data, const uint32_t* key, int64_t cap, int N, int D,
                         uint32_t key_thresh, int64_t max_new, int max_level, int32_t* child_out, uint16_t* data_out, int64_t room,
                         int64_t* out_capacity, int32_t* slot_src, rto_refine_stats* stats);

/* ---- GuidanceNet under training (denoiser/network.py:49-118; denoiser/runner.py:71-84; denoiser/metrics.py:7-9) ----
 * A RepVGG block (network.py:49-75) has no normalisation layer: before its ReLU6 it is linear in its input, so the sum of its
 * branches is ONE 3x3 convolution with the summed weights, and the gradient of every branch is a slice of the gradient of that
 * kernel.  The caller sums the branches (differentiably) and passes each layer's EFFECTIVE kernel and bias, float32 in device
 * memory -- they change every step, so there is no packing step.  The domain is the fused inference network's: 8 -> c1 [-> c1]
 * -> 2 * levels, c1 in 1..64, levels in 1..6, two or three layers.  All arithmetic is float32 with float32 accumulation.
 *   forward (network.py:86-118):  z_l = conv3x3(x_{l-1}, W_l, zero padding "same") + b_l,  x_l = min(max(z_l, 0), 6);
 *       weight_map = softmax over channels 0..levels-1 of the last x, guidance_map = its channels levels..2 levels - 1, both
 *       [n][levels][H][W] as rto_filtering_train_forward takes them.  Every x_l is stored in `acts`: float32 planes
 *       [n][cout_l][H][W], layer after layer (rto_guidance_train_acts_bytes gives the size).  That layout is part of the ABI.
 *   backward:  softmax dx_k = w_k (g_k - sum_j g_j w_j); ReLU6 passes the gradient where 0 < x_l < 6 and nothing where x_l is
 *       exactly 0 or 6 (torch's hardtanh_backward), read from `acts`; layers[l].grad_weight [cout][cin][3][3] and .grad_bias
 *       [cout] are OVERWRITTEN for every layer.  There is no gradient for aux.
 * No floating-point atomics: workgroups write partial sums to the handle's scratch and a finishing kernel adds them in a fixed
 * order, so the same inputs give the same bits.  The calls keep no state between forward and backward other than the caller's
 * `acts`: forwards and backwards of different inputs may interleave in any order on one stream.  The handle owns the backward's
 * and the loss's scratch, which grows on demand; growing synchronises the device once.  One handle serves one stream at a time.
 * Refused before any device use -- RTO_E_INVALID: a null pointer; n, H or W < 1; num_layers outside 2..3; layers[0].cin != 8,
 * layers[l].cin != layers[l-1].cout or the last cout != 2 * levels; n H W > 2^31 - 1.  RTO_E_UNSUPPORTED: c1 outside 1..64, levels
 * outside 1..6, a middle layer that is not c1 -> c1. */
typedef struct rto_guidance_train rto_guidance_train;
typedef struct rto_guidance_train_layer {
    const float* weight; /* device, [cout][cin][3][3] */
    const float* bias;   /* device, [cout] */
    float* grad_weight;  /* device, backward only (forward and the size query ignore them) */
    float* grad_bias;
    int cin, cout;
} rto_guidance_train_layer;
int rto_guidance_train_create(int device, rto_guidance_train** out);
void rto_guidance_train_free(rto_guidance_train* t);
int rto_guidance_train_acts_bytes(const rto_guidance_train_layer* layers, int num_layers, int levels, int n, int H, int W, size_t* bytes);
int rto_guidance_train_forward(rto_guidance_train* t, void* stream, const float* aux, const rto_guidance_train_layer* layers, int num_layers,
                               int levels, int n, int H, int W, float* acts, float* weight_map, float* guidance_map);
int rto_guidance_train_backward(rto_guidance_train* t, void* stream, const float* grad_weight_map, const float* grad_guidance_map,
                                const float* aux, const float* acts, const rto_guidance_train_layer* layers, int num_layers, int levels, int n,
                                int H, int W);
/* The training loss and its gradient in one call (runner.py:78; metrics.py:7-9, 21-33): the mean over the r, g, b of pred against
 * truth, [n][H][W][4] float32 each (16-byte aligned), of |p - t| / (|p| + |t| + 1e-5) (RTO_LOSS_SMAPE) or (p - t)^2 (RTO_LOSS_MSE).
 * Terms in float64 from the float32 inputs, reduced by fixed-order partial sums (the convention of the image metrics); *device_loss
 * is one double in device memory.  grad_pred [n][H][W][4] = d loss / d pred, alpha component 0: for SMAPE
 * (sign(p - t) / D - |p - t| sign(p) / D^2) / (3 n H W) with D = |p| + |t| + 1e-5 and sign(0) = 0, so p == t gives exactly 0 as
 * torch's abs does.  Non-finite inputs propagate.  RTO_E_INVALID: a null or misaligned pointer, n, H or W < 1, an unknown kind. */
#define RTO_LOSS_SMAPE 0
#define RTO_LOSS_MSE 1
int rto_loss_forward_backward(rto_guidance_train* t, void* stream, const float* pred, const float* truth, int n, int H, int W, int kind,
                              double* device_loss, float* grad_pred);

/* ---- profiling aid ---- */
/* Counter calibration (MI355X_MICROARCH.md "HBM"): launches `repeats` kernels in which every lane
 * loads one dword from its own never-repeated 128-byte line of a zero-filled n_lines*128-byte buffer
 * (the render path's access shape).  Known lines per launch = n_lines; compare with FETCH_SIZE. */
int rto_probe_gather(uint64_t n_lines, int repeats);
/* Ceiling probes for the traversal kernel (DESIGN.md "What bounds the traversal"; tools/probe_ceiling.py).
 * rto_probe_gather_sweep: persistent waves (`wps` per SIMD on every CU) issue `iters` wave-level dword
 * gathers each; every gather touches exactly `lines_per_gather` (1..64) distinct 64-byte lines of a
 * zero-filled table of `table_bytes` (rounded down to a power of two), the lanes dealt over the lines
 * interleaved (blocked = 0) or in runs (blocked = 1); dependent = 1 chains each gather's address on the
 * previous one's value (the traversal's shape), 0 keeps four in flight per wave.
 * out = {wall ms per launch, mean shader-clock cycles per wave, waves, gathers per wave}.
 * rto_probe_valu: persistent waves (`wps` per SIMD on every CU) run `iters` times ONE asm block of exactly 32
 * wave-level VALU instructions on independent registers; `kind` picks the opcode (rto_probe_valu_name(kind) names
 * it, NULL past the last kind).  out = {wall ms, mean s_memtime ticks per wave, waves, VALU instructions per wave
 * (exact), ticks from the first wave's start to the last wave's end, CUs}. */
int rto_probe_gather_sweep(uint64_t table_bytes, int lines_per_gather, int blocked, int dependent, int wps,
                           int iters, int repeats, double out[4]);
int rto_probe_valu(int kind, int wps, int iters, double out[6]);
const char* rto_probe_valu_name(int kind);
/* rto_probe_scratch: one launch (null stream, asynchronous) of a kernel with a private segment (kind bit 0: a dynamically
 * indexed per-thread array), 34 KB of static LDS (bit 1), an MFMA loop (bit 2) -- the would-be trigger in
 * tools/contention_determinism.py's experiment on determinism when processes share the GPU. */
int rto_probe_scratch(int kind, int blocks, int iters);
/* Test hook: host_out[i] = the threshold the renderer draws from the RNG float k / 2^23, k = first_k + i
 * (rt_core.cuh:67-88 `-logf(1 - rng.next_float())` in the library's deterministic arithmetic), computed on the
 * device by the very function the kernels call.  first_k + count <= 2^23: the whole domain can be compared with
 * the oracle value by value. */
int rto_probe_thresholds(uint32_t first_k, uint32_t count, float* host_out);
/* Test hook: host_out[i] = f(x_i) computed on the device, x_i = the float with bit pattern first_bits + i * stride
 * (wrapping), f = the library's deterministic logf (fn 0: thresholds), expf (fn 1: the SH colour's sigmoid) or the
 * filter's fp32 exp (fn 2) -- the functions DESIGN.md "Math" defines in place of `__logf` / `__expf`
 * (rt_core.cuh:74,95,314; filtering.cu:191).  Lets a test sweep the whole float range against the oracle. */
int rto_probe_math(int fn, uint32_t first_bits, uint32_t stride, uint32_t count, float* host_out);
/* Test hook (round 6): the shading kernels evaluate `cnt / (1.f + expf(-t))` (rt_core.cuh:314-318) through a short form --
 * the library's expf for |t| <= 87 in fused multiply-adds, the division as reciprocal + one exact-residual correction --
 * that must return the float of the plain statement for every argument.  mode 0: the short sigmoid against the plain one
 * for the floats t with bit patterns first_bits + i, i < count (<= 2^32), times every sample count cnt_lo .. cnt_hi
 * (1 .. 32); mode 1: the short division cnt / d alone, for d = those floats (callers pass [1, 2^126)).  Both sides run on
 * the device.  out3[0] = pairs that differ, out3[1] = the first of them (bits << 8 | cnt; ~0 if none), out3[2] = pairs compared.
 * Modes 2 / 3: the shading kernels' one-instruction `(float)half * b` (v_fma_mix_f32 with a -0.0 addend; rt_core.cuh:286-312's
 * 48 products per hit entry) against convert-then-multiply, for the floats b = first_bits + i (mode 2; times the 16 special
 * halves selected by cnt 1 .. 16) or first_bits + 4099 i (mode 3; times halves 2048 (cnt - 1) .. 2048 cnt - 1: all 65536 over
 * cnt 1 .. 32), in both packed positions. */
int rto_probe_sigmoid(int mode, uint32_t first_bits, uint64_t count, int cnt_lo, int cnt_hi, uint64_t* out3);
/* Test hook: host_out[i][0..24] = the basis the kernels evaluate for the tree and options at view direction dirs[i][3] (the
 * ray's unit direction before the rot_dirs rotation; rt_core.cuh:277-284, lumisphere.hpp:14-80) -- rotation, basis and the
 * basis_minmax mask -- computed on the device by the kernels' own code.  path 0: the run-time form (generic and fast kernels,
 * the shading kernel's mode 0); path 1: the per-basis-size form the shading kernel uses for its record modes (SG / ASG any
 * basis_dim, SH 4 / 9 / 16 / 25, else RTO_E_UNSUPPORTED), whose entries from basis_dim on are 0. */
int rto_probe_basis(const rto_tree* tree, const rto_options* options, const float* dirs, int64_t n, int path, float* host_out);

#ifdef __cplusplus
}
#endif
#endif /* RTO_H */
