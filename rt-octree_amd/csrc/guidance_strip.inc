// guidance_strip.inc -- the strip frame under both fused GuidanceNet kernels (included by guidance_kernels.hip inside
// namespace rto { namespace {, before guidance_fused and guidance_general.inc).  Everything around the convolutions that does
// not depend on the network's shape, written once and templated on the halo (= number of layers) and the input mode: the
// tile and strip constants, the cull arguments, the render-tile marks of a strip and the skip decisions made from them, the
// background fill of skipped tiles, and stage A (the input tile's loads and its fp32 -> fp16 HWC store into LDS).
// __device__ __forceinline__ templates and one struct; no kernel.

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float float4v __attribute__((ext_vector_type(4)));

constexpr int kGW = kNetTileW, kGH = kNetTileH;  // output tile (rto_denoise_launch.h: filter_fast restates the skip rule in them)
// Tiles per workgroup, along x.  Round 2 chose 5 when every tile was computed (strips of 1 / 2 / 5 / 7..25: 0.70 / 0.64 / 0.60 /
// 0.59-0.62 ms per 50 frames).  With the culling two thirds of the workgroups only test their tiles' marks and leave, and each of
// those costs a launch and a dependent load: round 6 re-measured 5 / 7 / 9 / 13 tiles per workgroup at 0.686 / 0.862 / 0.626 /
// 0.616 ms per 100 C2 frames (7 splits a 25-tile row 7 + 7 + 7 + 4) and 1.86 / - / 1.45 / 1.38 ms on C4 (60-tile rows):
// 13 = the most that the one-thread-per-(tile, render tile) mark test of that round fitted into 256 threads
// (profiles/r6_m_ab_strips*.txt); the 64-column mark window below holds 4 * 12 + 6 = 54
constexpr int kStrip = 13;
constexpr int kCIn = 8;  // aux channels (render_context.hpp:23)
// Activation pixel stride in LDS = channels + kActPad halves, i.e. 80 B instead of 64 B for 32 channels -- with a 64-byte stride
// the 16 pixels a ds_read_b128 gathers start on only two distinct bank groups (8-way conflict); at 80 B every bank is touched
// exactly twice, the minimum for 256 B
constexpr int kActPad = 8;

// Empty-space culling carried into the network (round 3): the render context's tile marks (FrameBatch::tile_mask) and the
// network's output for a pixel whose whole aux neighbourhood is background, measured once by the kernel itself on a synthetic
// background frame.  mask == nullptr: off.
struct NetCull {
    const uint32_t* mask;
    int mask_words, tiles_x;
    uint4 fill;        // guidance_fused, PACK: the 8 fp16 outputs of such a pixel
    float planes[12];  // fp32 planes: 6 softmax weights, then 6 guidance values (the first `levels` of each)
    // SPARSE lean frames (round 6, rto_ctx_set_lean_outputs level 2; guidance_fused with IN = 2, PACK): the renderer stored no
    // pixel of an unmarked (culled) render tile -- such a pixel IS the background (bg, bg, bg, alpha 0), so stage A substitutes
    // it -- and the kernel stores no maps for the tiles it skips: the filter substitutes `fill` for them the same way
    int sparse;
    float bg;
};

// ---- marks.  Tiles of the strip whose input region (tile + HALO) lies inside the image and in culled render tiles read
// nothing but background: every output pixel is the background fill.  Bit ts of the result (`skip_tiles`); workgroup-uniform.
// Round 6: every wave builds the marks of the render tiles under the strip's input regions for itself -- 3 tile rows from
// (y0 - HALO) >> 3, 64 columns from 4 tx_first - 1 (a tile's region spans 6 of them from bit 4 ts), lane = column, the three
// mark words of a lane requested together, the rows by ballot: one memory round trip, no LDS, no barrier (the first form
// tested one (tile, render tile) per thread into LDS words under two barriers).
// bit c of rmk[r]: render tile (4 tx_first - 1 + c, ((y0 - HALO) >> 3) + r) is marked
template <int HALO>
__device__ __forceinline__ uint32_t strip_marks(const NetCull& cull, unsigned long long (&rmk)[3], int lane, int tx_first, int y0,
                                                int strip, int tiles_x, int H, int W) {
    constexpr int IW = kGW + 2 * HALO, IH = kGH + 2 * HALO;
    constexpr int RX = (IW + 7) / 8 + 1, RY = (IH + 7) / 8 + 1;  // render tiles an input region can touch, per axis
    static_assert(RX == 6 && RY == 3 && 4 * (kStrip - 1) + RX <= 64, "64 columns x 3 rows of render tiles cover a strip's input regions");
    uint32_t skip_tiles = 0;
    rmk[0] = rmk[1] = rmk[2] = 0ull;
    if (cull.mask) {
        const uint32_t* const fm = cull.mask + (size_t)blockIdx.z * cull.mask_words;
        const uint32_t keep_all = fm[cull.mask_words - 1] & 1u;
        uint32_t word[RY];
        bool inside[RY];
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const int tx = 4 * tx_first - 1 + lane, ty = ((y0 - HALO) >> 3) + r;
            inside[r] = tx >= 0 && ty >= 0 && tx < cull.tiles_x && ty * 8 < H;
            const uint32_t t = inside[r] ? (uint32_t)(ty * cull.tiles_x + tx) : 0u;
            word[r] = fm[t >> 5] >> (t & 31u);
        }
#pragma unroll
        for (int r = 0; r < RY; ++r) rmk[r] = __builtin_amdgcn_ballot_w64(inside[r] && ((word[r] | keep_all) & 1u) != 0u);
        const unsigned long long any_row = rmk[0] | rmk[1] | rmk[2];
        for (int ts = 0; ts < strip && tx_first + ts < tiles_x; ++ts) {
            const int x0 = (tx_first + ts) * kGW - HALO, ry0 = y0 - HALO;
            // (outside the image the zero padding is not background: computed)
            if (x0 >= 0 && ry0 >= 0 && x0 + IW <= W && ry0 + IH <= H && ((any_row >> (4 * ts)) & 0x3full) == 0ull) skip_tiles |= 1u << ts;
        }
    }
    return skip_tiles;
}

// sparse input: bit sy * 6 + sx = render tile (sx, sy) of strip tile ts's input region is marked (its pixels were stored)
__device__ __forceinline__ uint32_t region_marks(const unsigned long long (&rmk)[3], int ts) {
    return (uint32_t)((rmk[0] >> (4 * ts)) & 0x3full) | (uint32_t)((rmk[1] >> (4 * ts)) & 0x3full) << 6 |
           (uint32_t)((rmk[2] >> (4 * ts)) & 0x3full) << 12;
}

// first tile >= ts of the strip that has to be computed (kStrip: none)
__device__ __forceinline__ int next_live(uint32_t skip_tiles, int ts, int strip, int tx_first, int tiles_x) {
#pragma clang loop vectorize(disable)  // (at most kStrip scalar steps; as a free function the loop was vectorised eight wide)
    while (ts < strip && tx_first + ts < tiles_x && ((skip_tiles >> ts) & 1u)) ++ts;
    return (ts < strip && tx_first + ts < tiles_x) ? ts : kStrip;
}

// ---- the skipped tiles' fp32 planes (interior tiles: every pixel of them is inside the image); thread = pixel of the tile.
// weight_out / guidance_out: this frame's [L][H][W]
__device__ __forceinline__ void fill_skipped_planes(const NetCull& cull, uint32_t skip_tiles, float* __restrict__ weight_out,
                                                    float* __restrict__ guidance_out, int L, int64_t HW, int W, int tid, int tx_first, int y0,
                                                    int strip, int tiles_x) {
    for (int ts = 0; ts < strip && tx_first + ts < tiles_x; ++ts)
        if ((skip_tiles >> ts) & 1u) {
            const int64_t pix = (int64_t)(y0 + (tid >> 5)) * W + (tx_first + ts) * kGW + (tid & 31);
#pragma unroll
            for (int l = 0; l < 6; ++l)
                if (l < L) {
                    weight_out[l * HW + pix] = cull.planes[l];
                    guidance_out[l * HW + pix] = cull.planes[6 + l];
                }
        }
}

// ---- stage A: input tile with halo HALO, fp32 -> HWC fp16 in LDS (zero outside the image).  One thread = one tile pixel per
// iteration: its channel loads are independent (all in flight at once) and become one 16-byte LDS store.  fetch() issues the
// loads of strip tile ts into v -- the kernels call it for the next computed tile before the layers of this one, a tile's input
// fetch being 37 % of its time when nothing hides it -- and stage() converts and stores them.
// IN: 0 = all 8 aux planes [8][H][W]; 1 = SQ: planes 4..7 are the squares of planes 0..3 (what the renderer writes,
// volrend.cu:195-202: a[4 + c] = out[c] * out[c], one fp32 multiply) -- read only planes 0..3 and square them here: the same fp32
// product, so the same fp16 inputs, from half the bytes; 2 (round 5) = SQ from the INTERLEAVED image a lean batched launch
// leaves ([H][W][4] = r, g, b, alpha -- the values of aux planes 0..3, rto_ctx_set_lean_outputs): one 16-byte load per pixel.
// SPARSE (IN = 2): compile the substitution of cull.sparse frames in.
template <int HALO>
constexpr int kStageIters = ((kGW + 2 * HALO) * (kGH + 2 * HALO) + 255) / 256;
template <int IN>
constexpr int kStagePlanes = IN ? kCIn / 2 : kCIn;  // planes actually read

template <int HALO, int IN, bool SPARSE>
__device__ __forceinline__ void fetch(float (&v)[kStageIters<HALO>][kStagePlanes<IN>], const float* __restrict__ aux, const NetCull& cull,
                                      const unsigned long long (&rmk)[3], int tx_first, int ts, int y0, int H, int W, int64_t HW, int tid) {
    static_assert(!SPARSE || IN == 2, "sparse frames are interleaved images");
    constexpr int IW = kGW + 2 * HALO, NPIX = IW * (kGH + 2 * HALO);
    const int x0 = (tx_first + ts) * kGW;  // the tile's first output column
    // (sparse: the marks of the render tiles under this tile's input region, in an SGPR -- whether a pixel was stored is known
    //  before its load is issued, which is then simply not issued: no dependent mask load, no select that waits for the pixel)
    const bool sparse = SPARSE && cull.sparse;
    const uint32_t rtm = sparse ? region_marks(rmk, ts) : 0u;
    const int rtx0 = (x0 - HALO) >> 3, rty0 = (y0 - HALO) >> 3;
#pragma unroll
    for (int it = 0; it < kStageIters<HALO>; ++it) {
        const int e = tid + it * 256;
        const int ty = e / IW, tx = e - ty * IW;
        const int gx = x0 - HALO + tx, gy = y0 - HALO + ty;
        const bool in = e < NPIX && gx >= 0 && gx < W && gy >= 0 && gy < H;
        const int gi = in ? gy * W + gx : 0;  // (8 * H * W < 2^31: rto_ctx_create's size check)
        if constexpr (IN == 2) {
            // (sparse: a pixel of an unmarked render tile was never stored -- it is the background)
            const bool stored = !sparse || ((rtm >> (((gy >> 3) - rty0) * 6 + ((gx >> 3) - rtx0))) & 1u) != 0u;
            const float bgv = in && sparse ? cull.bg : 0.f;
            float4 t = make_float4(bgv, bgv, bgv, 0.f);
            if (in && stored) t = reinterpret_cast<const float4*>(aux)[gi];
            v[it][0] = t.x;
            v[it][1] = t.y;
            v[it][2] = t.z;
            v[it][3] = t.w;
        } else {
#pragma unroll
            for (int c = 0; c < kStagePlanes<IN>; ++c) {
                const float t = aux[c * (int)HW + gi];
                v[it][c] = in ? t : 0.f;
            }
        }
    }
}

template <int HALO, int IN>
__device__ __forceinline__ void stage(const float (&v)[kStageIters<HALO>][kStagePlanes<IN>], _Float16* s_in, int tid) {
    constexpr int NPIX = (kGW + 2 * HALO) * (kGH + 2 * HALO);
#pragma unroll
    for (int it = 0; it < kStageIters<HALO>; ++it) {
        const int e = tid + it * 256;
        if (e < NPIX) {
            half8 h;
#pragma unroll
            for (int c = 0; c < kStagePlanes<IN>; ++c) h[c] = (_Float16)v[it][c];
            if (IN) {
#pragma unroll
                for (int c = 0; c < kCIn / 2; ++c) h[kCIn / 2 + c] = (_Float16)(v[it][c] * v[it][c]);
            }
            *reinterpret_cast<half8*>(s_in + (size_t)e * kCIn) = h;
        }
    }
}
