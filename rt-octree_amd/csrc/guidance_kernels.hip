// guidance_kernels.hip -- the compact GuidanceNet as ONE fused gfx950 kernel.
//
// Reference network (denoiser/network.py:123-168 after compact_and_compile :170-208, run by
// renderer/src/denoiser/denoiser.cpp:46):  x = aux.half();  x = relu6(conv3x3(x; 8 -> C1));
// x = relu6(conv3x3(x; C1 -> 2L));  x = x.float();  weight = softmax(x[:L]);  guidance = x[L:].
// Default C1 = 32, L = 4 (denoiser/configs/blender.txt:21-25): 5.9 GFLOP per 800x800 frame, which
// PyTorch-ROCm runs as two MIOpen Winograd convolutions plus seven elementwise launches
// (~0.2 ms/frame, profiles/r1_b_*).  Here one workgroup produces a 32x8 pixel tile end to end:
//
//   stage A  aux tile + 2-pixel halo, fp32 planar -> fp16 HWC in LDS (zero outside the image);
//            one thread per tile pixel, its 8 channel loads in flight together
//   stage B  layer 1 on the tile + 1-pixel halo with v_mfma_f32_16x16x32_f16: M = 16 output
//            channels (weights, A operand, register-resident), N = 16 pixels (B operand: ONE
//            ds_read_b128 per lane = the 8 input channels of one tap), K = 9 taps x 8 channels
//            padded to 96; + bias, ReLU6, fp16, HWC in LDS (zero outside the image = the second
//            convolution's "same" padding)
//   stage C  layer 2 the same way: K = 9 taps x 32 channels = 9 MFMAs per 16 pixels, output
//            channels padded 8 -> 16, each activation-row fragment shared by the three output rows
//            it serves; + bias, ReLU6, fp16 rounding (the reference keeps fp16 activations), then
//            softmax over the L weight channels in fp32 and the stores
//
// The frame around the stages -- the strip of tiles a workgroup walks, the render-tile marks and skip decisions, the fill of
// skipped tiles, stage A -- is guidance_strip.inc, shared with guidance_general.inc (every other trained shape); stages B
// and C, the packed outputs and the sparse route's early exit are this kernel's own.
//
// Accumulation is fp32 inside the MFMA like cuDNN/MIOpen fp16 convolutions; rounding points
// (fp16 input, fp16 activations after each ReLU6) are the reference's.  Results agree with the fp32
// PyTorch network to fp16 accuracy (tests/test_guidance_fused.py), not bit for bit: libtorch 1.11 /
// cuDNN results are not pinned by the reference either.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <type_traits>

#include "rto_launch.h"
#include "rto_denoise_launch.h"

namespace rto {

namespace {

#include "guidance_strip.inc"

// C1 = mid channels (multiple of 16, <= 64), L = kernel levels (2L <= 16); IN = input mode (guidance_strip.inc, stage A)
// PACK: write the network's 8 output channels as they leave the last ReLU6 -- fp16 values, [n][H][W][8]: the 4
// softmax logits, then the 4 guidance values -- instead of fp32 weight_map / guidance_map planes.  16 B per pixel
// instead of 32, nothing lost: the reference's `.float()` (network.py:112) only widens those fp16 values, and the
// consumer (filter_fast<L, true>) applies softmax_weights() below to the logits itself.
// Launch bounds per instantiation: with all 8 aux planes in flight (IN = 0) the kernel needs 134 VGPRs; bounded to 128
// (4 workgroups per CU) it spilled 2-4 of them to scratch and ran slower.  It was also the kernel in whose company the
// bit-exact filter first lost its determinism on a shared GPU (DESIGN_HISTORY.md "Determinism when the GPU is shared": the cause
// turned out to be v_pk_fma_f32 under MFMA load from other processes, this kernel being the longest MFMA kernel around); no
// kernel of the denoise stage uses scratch now (tests/test_codegen.py).
constexpr int kSq0Workgroups = 3;  // workgroups per CU the IN = 0 instantiations are bounded to
template <int C1, int L, int IN, bool PACK>
__global__ void __launch_bounds__(256, IN ? 4 : kSq0Workgroups) guidance_fused(const float* __restrict__ aux,    // [n][8][H][W] (IN = 2: [n][H][W][4])
                                                       const _Float16* __restrict__ w1,  // [C1][96]   k = tap*8 + ci; k = 72: bias
                                                       const _Float16* __restrict__ w2,  // [16][9*C1] k = tap*C1 + ci
                                                       const float* __restrict__ b2,     // [16]
                                                       float* __restrict__ weight_out,   // [n][L][H][W]
                                                       float* __restrict__ guidance_out, // [n][L][H][W]
                                                       int H, int W, const NetCull cull, const int strip /* tiles per workgroup, <= kStrip */) {
    constexpr int HALO = kNetHalo;             // two 3x3 convolutions
    constexpr int IW = kGW + 2 * HALO, IH = kGH + 2 * HALO;  // input tile
    constexpr int AW = kGW + 2, AH = kGH + 2;  // layer-1 activation tile with halo 1
    constexpr int NT1 = C1 / 16;               // output-channel tiles of layer 1
    constexpr int KS2 = 9 * C1 / 32;           // k-steps of layer 2
    constexpr int AS = C1 + kActPad;           // activation pixel stride in halves
    __shared__ __attribute__((aligned(16))) _Float16 s_in[IH * IW * kCIn];
    __shared__ __attribute__((aligned(16))) _Float16 s_act[AH * AW * AS];
    __shared__ __attribute__((aligned(16))) _Float16 s_pad[16];  // B fragments of the padding taps: {1,0,..,0} (bias slot), {0,..,0}
    __shared__ __attribute__((aligned(16))) float s_b2[16];      // layer-2 bias

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 16) {  // (published by the barrier after stage A)
        s_pad[tid] = (_Float16)(tid == 0 ? 1.f : 0.f);
        s_b2[tid] = b2[tid];
    }
    // A workgroup walks a strip of up to kStrip tiles along x with the input of tile t + 1 on its way into registers while
    // layers 1 and 2 of tile t run.  Measured per 50 frames of 800x800 once the stages had been slimmed down to fit the
    // prefetch registers without spills: strip 1 0.70 ms, 2 0.64, 5 0.60, 7..25 0.59-0.62.  (While stage B still spent ~75
    // VALU instructions per group the kernel was issue-bound and strips gained nothing.)
    const int tiles_x = (W + kGW - 1) / kGW;
    const int tx_first = blockIdx.x * strip;
    const int y0 = blockIdx.y * kGH;
    const int64_t HW = (int64_t)H * W;
    aux += (int64_t)blockIdx.z * (IN == 2 ? 4 : kCIn) * HW;
    weight_out += (int64_t)blockIdx.z * L * HW;  // (PACK: [H][W][8] fp16 = 4 floats per pixel = L * HW floats per image too)
    guidance_out += (int64_t)blockIdx.z * L * HW;

    const int col = lane & 15, kg = lane >> 4;  // MFMA lane roles: pixel (B/C column), k-group / row block

    // The strip's marks and skip decisions (guidance_strip.inc).  A workgroup with nothing to compute leaves before it has
    // requested a single weight.
    unsigned long long rmk[3];
    const uint32_t skip_tiles = strip_marks<HALO>(cull, rmk, lane, tx_first, y0, strip, tiles_x, H, W);
    int ts_live = next_live(skip_tiles, 0, strip, tx_first, tiles_x);
    if (PACK && cull.sparse && ts_live == kStrip) return;  // (sparse maps: nothing is stored for a skipped tile either)

    // Weights first: their loads overlap stage A instead of stalling the first MFMAs of each layer.
    half8 wa[NT1][3];
#pragma unroll
    for (int t = 0; t < NT1; ++t)
#pragma unroll
        for (int ks = 0; ks < 3; ++ks)
            wa[t][ks] = *reinterpret_cast<const half8*>(w1 + (size_t)(t * 16 + col) * 96 + ks * 32 + kg * 8);
    half8 wb[KS2];
#pragma unroll
    for (int ks = 0; ks < KS2; ++ks)
        wb[ks] = *reinterpret_cast<const half8*>(w2 + (size_t)col * (9 * C1) + ks * 32 + kg * 8);

    // Biases cost no registers: layer 1's rides in the weights (k-slot 72, the first padding tap, whose B element is
    // the constant 1 of s_pad; the packer rounds it to fp16 like the reference's `.half()` does), layer 2's is read from
    // LDS once per tile.

    if (cull.mask && !(PACK && cull.sparse)) {  // the skipped tiles first
        if (PACK) {
            for (int ts = 0; ts < strip && tx_first + ts < tiles_x; ++ts)
                if ((skip_tiles >> ts) & 1u)
                    reinterpret_cast<uint4*>(weight_out)[(int64_t)(y0 + (tid >> 5)) * W + (tx_first + ts) * kGW + (tid & 31)] = cull.fill;
        } else {
            fill_skipped_planes(cull, skip_tiles, weight_out, guidance_out, L, HW, W, tid, tx_first, y0, strip, tiles_x);
        }
    }
    // ---- stage A (guidance_strip.inc); the sparse substitution exists for the interleaved image only
    constexpr bool SPARSE = IN == 2;
    float v[kStageIters<HALO>][kStagePlanes<IN>];
    if (ts_live < kStrip) fetch<HALO, IN, SPARSE>(v, aux, cull, rmk, tx_first, ts_live, y0, H, W, HW, tid);

#pragma nounroll
    while (ts_live < kStrip) {  // (workgroup-uniform)
    const int x0 = (tx_first + ts_live) * kGW;
    ts_live = next_live(skip_tiles, ts_live + 1, strip, tx_first, tiles_x);
    const bool tile_interior = x0 >= 1 && x0 + kGW + 1 <= W && y0 >= 1 && y0 + kGH + 1 <= H;  // layer-1 region inside the image
    stage<HALO, IN>(v, s_in, tid);
    __syncthreads();  // s_in complete; every wave is also done with stage C of the previous tile (s_act is free)
    // next computed tile's input: in flight during stages B and C
    if (ts_live < kStrip) fetch<HALO, IN, SPARSE>(v, aux, cull, rmk, tx_first, ts_live, y0, H, W, HW, tid);

    // ---- stage B: layer 1 on the AH x AW region
    // The kernel is VALU-bound (stamps: stage B 38 % of a tile's time at ~75 VALU instructions per 16-pixel group
    // around 6 MFMAs), so the loop carries its indices instead of recomputing them: group g + 4 of a wave is 64
    // pixels = one row + 30 columns further on; a tap's LDS address is the group's base plus a per-lane constant; the
    // three padding taps of the last k-step read a zeroed 16-byte slot; tiles whose activation region lies inside the
    // image (all but the border ring) skip the zero-padding mask altogether.
    {
        constexpr int NG1 = (AH * AW + 15) / 16;
        static_assert(AW > 30 && AW <= 64, "the row / column carry below assumes one wrap per 64 pixels");
        uint32_t tapoff[2];  // byte offset of this lane's tap in k-steps 0 and 1, relative to the group's base pixel
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int tap = ks * 4 + kg, ky = tap / 3, kx = tap - ky * 3;
            tapoff[ks] = (uint32_t)((ky * IW + kx) * kCIn * 2);
        }
        constexpr uint32_t kTap8Off = (uint32_t)((2 * IW + 2) * kCIn * 2);
        const bool tap2_real = kg == 0;  // k-step 2 holds tap 8, the bias slot (kg 1) and two padding taps
        const char* tap2_pad = reinterpret_cast<const char*>(s_pad) + (kg == 1 ? 0 : 16);
        auto layer1 = [&](auto interior_tag) {
            constexpr bool INTERIOR = decltype(interior_tag)::value;
            int p = wave * 16 + col;
            int ry = p >= AW ? 1 : 0, rx = p - ry * AW;
            for (int g = wave; g < NG1; g += 4) {
                const uint32_t base = (uint32_t)((ry * IW + rx) * kCIn * 2);  // bytes into s_in
                const char* sin_b = reinterpret_cast<const char*>(s_in);
                half8 bf1[3];
                bf1[0] = *reinterpret_cast<const half8*>(sin_b + base + tapoff[0]);
                bf1[1] = *reinterpret_cast<const half8*>(sin_b + base + tapoff[1]);
                bf1[2] = *reinterpret_cast<const half8*>(tap2_real ? sin_b + base + kTap8Off : tap2_pad);
                float4v acc[NT1];
#pragma unroll
                for (int t = 0; t < NT1; ++t) acc[t] = (float4v){0.f, 0.f, 0.f, 0.f};  // (the bias is one of the products)
#pragma unroll
                for (int ks = 0; ks < 3; ++ks)
#pragma unroll
                    for (int t = 0; t < NT1; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[t][ks], bf1[ks], acc[t], 0, 0, 0);
                if (p < AH * AW) {  // (a lane beyond the region computed on whatever its addresses held: unused)
                    // outside the image the activation is the second convolution's zero padding: border tiles scale by
                    // 0 or 1 (relu6(...) is finite and >= 0, so x * 1 = x and x * 0 = +0 exactly)
                    float inside = 1.f;
                    if (!INTERIOR) {
                        const int gx = x0 - 1 + rx, gy = y0 - 1 + ry;
                        inside = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? 1.f : 0.f;
                    }
#pragma unroll
                    for (int t = 0; t < NT1; ++t) {
                        half4 o;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float r = __builtin_amdgcn_fmed3f(acc[t][i], 0.f, 6.f);  // ReLU6
                            o[i] = (_Float16)(INTERIOR ? r : r * inside);
                        }
                        *reinterpret_cast<half4*>(s_act + __umul24((unsigned)p, AS) + t * 16 + kg * 4) = o;
                    }
                }
                p += 64;
                rx += 64 - AW;
                ry += 1;
                if (rx >= AW) {
                    rx -= AW;
                    ry += 1;
                }
            }
        };
        if (tile_interior)  // workgroup-uniform
            layer1(std::true_type{});
        else
            layer1(std::false_type{});
    }
    __syncthreads();

    // ---- stage C: layer 2 on the kGH x kGW tile, softmax, stores
    // A wave owns 16 columns x 4 rows of the tile and walks the 6 activation rows under them: each row's three
    // B fragments (kx = 0..2; one ds_read_b128 per lane each) feed the MFMAs of up to three output rows (ky = row -
    // output row), so a group costs 4.5 fragment reads instead of 9 -- the stage was bound by LDS reads (144 KB per
    // tile against 576 clocks of MFMA).  Every accumulator still receives its taps in the order 0..8.
    {
        static_assert(kGW == 32 && kGH == 8, "stage C assigns (column block, row half) = wave");
        const float4v bias = *reinterpret_cast<const float4v*>(s_b2 + kg * 4);
        const int ox = (wave & 1) * 16 + col, oy0 = (wave >> 1) * 4;
        float4v acc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = bias;  // the bias: the first MFMA's C operand
        const _Float16* arow = s_act + __umul24(__umul24((unsigned)oy0, AW) + ox, AS) + kg * 8;
        half8 cur[3], nxt[3];
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) cur[kx] = *reinterpret_cast<const half8*>(arow + kx * AS);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            if (a < 5) {  // the next activation row is on its way while this one is multiplied
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) nxt[kx] = *reinterpret_cast<const half8*>(arow + ((a + 1) * AW + kx) * AS);
            }
            // (kx outside, output row inside: consecutive MFMAs write different accumulators, and each accumulator
            //  still sees ky = 0..2, kx = 0..2 in order)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ky = a - r;
                    if (ky >= 0 && ky < 3)
                        acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb[ky * 3 + kx], cur[kx], acc[r], 0, 0, 0);
                }
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) cur[kx] = nxt[kx];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gx = x0 + ox, gy = y0 + oy0 + r;
            if (gx < W && gy < H && kg * 4 < 2 * L) {
                float v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = (float)(_Float16)__builtin_amdgcn_fmed3f(acc[r][i], 0.f, 6.f);  // ReLU6 -> fp16 activations, then .float()
                const int64_t pix = (int64_t)gy * W + gx;
                if (PACK) {  // (weight_out = the packed buffer of image blockIdx.z; kg 0: logits, kg 1: guidance)
                    half4 h;
#pragma unroll
                    for (int i = 0; i < 4; ++i) h[i] = (_Float16)v[i];
                    *reinterpret_cast<half4*>(reinterpret_cast<_Float16*>(weight_out) + pix * 8 + kg * 4) = h;
                } else if (L == 4) {
                    if (kg == 0) {  // channels 0..3: softmax -> weight_map (network.py:113-114)
                        float wgt[4];
                        softmax_weights4(v, wgt);
#pragma unroll
                        for (int i = 0; i < 4; ++i) weight_out[i * HW + pix] = wgt[i];
                    } else {  // channels 4..7: guidance_map (:116)
#pragma unroll
                        for (int i = 0; i < 4; ++i) guidance_out[i * HW + pix] = v[i];
                    }
                }
            }
        }
    }
    }  // strip
}

#include "guidance_general.inc"

}  // namespace

// tiles per workgroup of guidance_fused / guidance_general for a launch of n frames of H x W: strips of kStrip tiles when that
// still leaves every CU its workgroups (a batch of frames), shorter ones for a lone frame.  The one statement of the rule: both
// launchers below and rto_denoise_launch_strips call it.
int guidance_net_strip(int n, int H, int W) {
    const int tiles_x = (W + kGW - 1) / kGW, tiles_y = (H + kGH - 1) / kGH;
    int strip = kStrip;
    while (strip > 1 && (int64_t)((tiles_x + strip - 1) / strip) * tiles_y * n < 2048) --strip;
    return strip;
}

// grid, strip and the cull arguments both launchers share.  mask == nullptr: no culling; fill_planes (with a mask): the fp32
// background maps, `levels` weights, then `levels` guidance values
static NetCull strip_launch(int n, int H, int W, const uint32_t* mask, int mask_words, const float* fill_planes, int levels, dim3* grid,
                            int* strip) {
    const int tiles_x = (W + kGW - 1) / kGW, tiles_y = (H + kGH - 1) / kGH;
    *strip = guidance_net_strip(n, H, W);
    *grid = dim3((tiles_x + *strip - 1) / *strip, tiles_y, n);
    NetCull cull = {};
    cull.mask = mask;
    cull.mask_words = mask_words;
    cull.tiles_x = (W + 7) / 8;
    if (mask && fill_planes)
        for (int l = 0; l < levels; ++l) {
            cull.planes[l] = fill_planes[l];
            cull.planes[6 + l] = fill_planes[levels + l];
        }
    return cull;
}

hipError_t launch_guidance_net(const float* aux, const void* w1, const void* w2, const float* b2, int c1,
                               int levels, int n, int H, int W, float* weight_out, float* guidance_out,
                               int in_mode, const uint32_t* tile_mask, int mask_words, const uint32_t* fill_k,
                               const float* fill_planes, int sparse, float background, hipStream_t stream) {
    if (c1 != 32 || levels != 4 || in_mode < 0 || in_mode > 2) return hipErrorInvalidValue;  // the reference configuration (blender.txt:21-25)
    const bool pack = guidance_out == nullptr;  // weight_out is then the packed fp16 buffer [n][H][W][8]
    dim3 grid;
    int strip;
    NetCull cull = strip_launch(n, H, W, (pack ? fill_k != nullptr : fill_planes != nullptr) ? tile_mask : nullptr, mask_words,
                                pack ? nullptr : fill_planes, levels, &grid, &strip);
    if (cull.mask && pack) cull.fill = make_uint4(fill_k[0], fill_k[1], fill_k[2], fill_k[3]);
    cull.sparse = sparse && cull.mask && pack && in_mode == 2 ? 1 : 0;
    if (sparse && !cull.sparse) return hipErrorInvalidValue;  // (sparse frames come with tile marks, as the RGBA image, on the packed route)
    cull.bg = background;
#define RTO_NET(IN, PK)                                                                                                   \
    hipLaunchKernelGGL((guidance_fused<32, 4, IN, PK>), grid, dim3(256), 0, stream, aux, (const _Float16*)w1, (const _Float16*)w2, \
                       b2, weight_out, guidance_out, H, W, cull, strip)
    if (pack) {
        if (in_mode == 2) RTO_NET(2, true); else if (in_mode == 1) RTO_NET(1, true); else RTO_NET(0, true);
    } else {
        if (in_mode == 2) RTO_NET(2, false); else if (in_mode == 1) RTO_NET(1, false); else RTO_NET(0, false);
    }
#undef RTO_NET
    return hipGetLastError();
}

hipError_t launch_guidance_general(const float* aux, const void* w1, const void* wm, const void* wl, const float* bm, const float* bl,
                                   int c1p, int num_layers, int levels, int n, int H, int W, float* weight_out, float* guidance_out,
                                   int in_mode, const uint32_t* tile_mask, int mask_words, const float* fill_planes, hipStream_t stream) {
    if ((c1p != 16 && c1p != 32 && c1p != 64) || (num_layers != 2 && num_layers != 3) || levels < 1 || levels > 6 || in_mode < 0 ||
        in_mode > 2 || !weight_out || !guidance_out)
        return hipErrorInvalidValue;
    dim3 grid;
    int strip;
    const NetCull cull = strip_launch(n, H, W, fill_planes ? tile_mask : nullptr, mask_words, fill_planes, levels, &grid, &strip);
#define RTO_GEN(C, NLAYERS, IN) \
    return launch_general_one<C, NLAYERS, IN>(grid, stream, aux, w1, wm, wl, bm, bl, weight_out, guidance_out, H, W, levels, cull, strip)
#define RTO_GEN_IN(C, NLAYERS)                                         \
    do {                                                               \
        if (in_mode == 2) RTO_GEN(C, NLAYERS, 2);                      \
        if (in_mode == 1) RTO_GEN(C, NLAYERS, 1);                      \
        RTO_GEN(C, NLAYERS, 0);                                        \
    } while (0)
    if (num_layers == 2) {
        if (c1p == 16) RTO_GEN_IN(16, 2);
        if (c1p == 32) RTO_GEN_IN(32, 2);
        RTO_GEN_IN(64, 2);
    }
    if (c1p == 16) RTO_GEN_IN(16, 3);
    if (c1p == 32) RTO_GEN_IN(32, 3);
    RTO_GEN_IN(64, 3);
#undef RTO_GEN_IN
#undef RTO_GEN
}

}  // namespace rto
