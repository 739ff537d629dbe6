// guidance_general.inc -- the fused GuidanceNet for every other trained shape (included by guidance_kernels.hip, inside
// namespace rto { namespace { , after guidance_strip.inc: the strip frame -- constants, NetCull, marks, skipped-tile fill,
// stage A -- is that file's, with halo NL and without the sparse substitution).
//
// guidance_fused<32, 4> above is tuned for the reference configuration: both weight sets live in registers, the second layer
// shares activation rows between output rows, the maps can leave packed.  None of that survives C1 = 64 (288 weight registers)
// or a third layer, so the shapes the trainer can produce besides the default -- 8 -> c1 [-> c1] -> 2 levels, c1 in 1..64, levels
// in 1..6 -- run through this kernel: the same tile (32 x 8 outputs per step of a strip), the same arithmetic
// (v_mfma_f32_16x16x32_f16, fp16 inputs / weights / biases, ReLU6 and fp16 rounding after every layer, softmax in fp32), written
// for generality:
//
//   * c1 is padded by the host packer to C1P in {16, 32, 64} with zero weights and biases: a padded channel is relu6(0) = +0
//     and contributes exact zeros to the next layer
//   * NL layers, halo NL: the input tile is (32 + 2 NL) x (8 + 2 NL); layer l produces the region with halo NL - l into an
//     activation buffer in LDS, zero outside the image (the next convolution's "same" padding)
//   * one conv_layer() for every layer: a wave keeps the accumulators of ALL its pixel groups and output-channel tiles and walks
//     the k-steps once, so each weight fragment is fetched once per wave and tile (from global memory / L2, the next k-step's
//     on its way during the MFMAs of this one) and each activation fragment is read from LDS once
//   * the last layer leaves its 16 (padded) channels per pixel in LDS; after a barrier thread t owns pixel t of the tile, so
//     the softmax over `levels` logits -- which lie in two MFMA lane groups for levels > 4 -- needs no cross-lane exchange
//   * LDS is dynamic: C1P = 64 with three layers needs 128 KB (one workgroup per CU), see DESIGN.md "General GuidanceNet shapes"

template <int C1P>
struct GenShape {
    static_assert(C1P == 16 || C1P == 32 || C1P == 64, "mid channels are padded to 16, 32 or 64");
    static constexpr int KS = C1P == 16 ? 5 : 9 * C1P / 32;  // k-steps of a C1P-input layer (C1P = 16: tap pairs, the tenth half-step zero)
    static constexpr int AS = C1P + kActPad;                 // activation pixel stride in halves
};

constexpr int gen_region(int NL, int l) { return (kGW + 2 * (NL - l)) * (kGH + 2 * (NL - l)); }  // pixels of layer l's output region
template <int C1P, int NL>
constexpr int gen_lds_halves() {
    return gen_region(NL, 0) * kCIn + gen_region(NL, 1) * GenShape<C1P>::AS + (NL == 3 ? gen_region(NL, 2) * GenShape<C1P>::AS : 0) +
           kGW * kGH * 16 + 16;
}

// softmax_weights4 (rto_device_math.h) for LL terms: maximum, __expf(v - m), sum left to right, the refined reciprocal
template <int LL>
__device__ __forceinline__ void softmax_weights_n(const float* v, float* out) {
    float m = v[0];
#pragma unroll
    for (int i = 1; i < LL; ++i) m = fmaxf(m, v[i]);
    float e[LL], s = 0.f;
#pragma unroll
    for (int i = 0; i < LL; ++i) {
        e[i] = __expf(v[i] - m);
        s += e[i];
    }
    const float inv = rcp_refined(s);  // s in [1, LL]
#pragma unroll
    for (int i = 0; i < LL; ++i) out[i] = e[i] * inv;
}

// One 3x3 convolution + bias + ReLU6 + fp16 rounding on an OW x OH output region whose pixel (rx, ry) reads the input pixels
// (rx + kx, ry + ky) of an INW-wide region in LDS (pixel stride INS halves).  CIN = 8: the first layer (k = tap * 8 + ci padded
// to 96, bias in k-slot 72 against the constant 1 of s_pad); else k = tap * CIN + ci in KS k-steps, bias = the accumulators'
// initial value.  NT = output-channel tiles of 16.  MASK: zero the outputs outside the image.
template <int CIN, int NT, int KS, int INW, int INS, int OW, int OH, int DS, bool MASK>
__device__ __forceinline__ void conv_layer(const _Float16* __restrict__ src, _Float16* __restrict__ dst, const _Float16* __restrict__ w,
                                           const float* __restrict__ bias, const _Float16* s_pad, int gx0, int gy0, int H, int W,
                                           int wave, int col, int kg) {
    constexpr int NPIX = OW * OH, NG = (NPIX + 15) / 16, G = (NG + 3) / 4;
    constexpr int ROW = KS * 32;  // halves per weight row
    uint32_t base[G];             // halves into src of this lane's pixel in group wave + 4 g (clamped into the region)
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int p = (wave + 4 * g) * 16 + col, pc = p < NPIX ? p : NPIX - 1;
        const int ry = pc / OW, rx = pc - ry * OW;
        base[g] = (uint32_t)((ry * INW + rx) * INS);
    }
    float4v acc[NT][G];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        float4v b = (float4v){0.f, 0.f, 0.f, 0.f};
        if constexpr (CIN != 8) b = *reinterpret_cast<const float4v*>(bias + t * 16 + kg * 4);
#pragma unroll
        for (int g = 0; g < G; ++g) acc[t][g] = b;
    }
    const _Float16* wl = w + (size_t)col * ROW + kg * 8;  // this lane's A-fragment column: output channel t * 16 + col
    half8 wcur[NT], wnxt[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) wcur[t] = *reinterpret_cast<const half8*>(wl + (size_t)t * 16 * ROW);
#pragma unroll 1
    for (int ks = 0; ks < KS; ++ks) {
        const int kn = ks + 1 < KS ? ks + 1 : ks;  // the next k-step's weights: in flight during this one's MFMAs
#pragma unroll
        for (int t = 0; t < NT; ++t) wnxt[t] = *reinterpret_cast<const half8*>(wl + (size_t)t * 16 * ROW + kn * 32);
        // this lane's B fragment: 8 input channels of one tap
        int tap, ch;
        if constexpr (CIN == 8) {
            tap = ks * 4 + kg;
            ch = 0;
        } else if constexpr (CIN == 16) {
            tap = 2 * ks + (kg >> 1);
            ch = (kg & 1) * 8;
        } else if constexpr (CIN == 32) {
            tap = ks;
            ch = kg * 8;
        } else {
            tap = ks >> 1;
            ch = (ks & 1) * 32 + kg * 8;
        }
        const bool real = tap < 9;  // (CIN = 8: taps 9..11 are the bias slot and two zero slots; CIN = 16: tap 9 has zero weights)
        const int tc = real ? tap : 8, ky = tc / 3, kx = tc - ky * 3;
        const uint32_t off = (uint32_t)((ky * INW + kx) * INS + ch);
        const _Float16* padp = s_pad + (tap == 9 ? 0 : 8);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if ((wave + 4 * g) < NG) {  // (wave-uniform)
                half8 bf;
                if constexpr (CIN == 8)
                    bf = *reinterpret_cast<const half8*>(real ? src + base[g] + off : padp);
                else
                    bf = *reinterpret_cast<const half8*>(src + base[g] + off);
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t][g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wcur[t], bf, acc[t][g], 0, 0, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) wcur[t] = wnxt[t];
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int p = (wave + 4 * g) * 16 + col;
        if (p < NPIX) {
            // outside the image the activation is the next convolution's zero padding (relu6(...) is finite and >= 0, so
            // x * 1 = x and x * 0 = +0 exactly)
            float inside = 1.f;
            if constexpr (MASK) {
                const int ry = p / OW, rx = p - ry * OW;
                const int gx = gx0 + rx, gy = gy0 + ry;
                inside = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? 1.f : 0.f;
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                half4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float r = __builtin_amdgcn_fmed3f(acc[t][g][i], 0.f, 6.f);  // ReLU6
                    o[i] = (_Float16)(MASK ? r * inside : r);
                }
                *reinterpret_cast<half4*>(dst + (size_t)p * DS + t * 16 + kg * 4) = o;
            }
        }
    }
}

// C1P = padded mid channels, NL = layers (2 or 3), IN = input mode as in guidance_fused; L = levels (1..6), workgroup-uniform
template <int C1P, int NL, int IN>
__global__ void __launch_bounds__(256) guidance_general(const float* __restrict__ aux,   // [n][8][H][W] (IN = 2: [n][H][W][4])
                                                        const _Float16* __restrict__ w1, // [C1P][96]  k = tap*8 + ci; k = 72: bias
                                                        const _Float16* __restrict__ wm, // [C1P][KS*32] k = tap*C1P + ci (NL = 3)
                                                        const _Float16* __restrict__ wl, // [16][KS*32]
                                                        const float* __restrict__ bm,    // [C1P] (NL = 3)
                                                        const float* __restrict__ bl,    // [16]
                                                        float* __restrict__ weight_out,   // [n][L][H][W]
                                                        float* __restrict__ guidance_out, // [n][L][H][W]
                                                        int H, int W, int L, const NetCull cull, const int strip) {
    static_assert(NL == 2 || NL == 3, "two or three layers");
    constexpr int IW = kGW + 2 * NL, IH = kGH + 2 * NL;              // input tile with halo NL
    constexpr int AW = kGW + 2 * (NL - 1), AH = kGH + 2 * (NL - 1);  // layer-1 output region
    constexpr int BW = kGW + 2, BH = kGH + 2;                        // NL = 3: layer-2 output region
    constexpr int NT1 = C1P / 16, KS = GenShape<C1P>::KS, AS = GenShape<C1P>::AS;
    extern __shared__ __attribute__((aligned(16))) _Float16 s_gen[];
    _Float16* const s_in = s_gen;                                       // [IH * IW][8]
    _Float16* const s_a = s_in + IH * IW * kCIn;                        // [AH * AW][AS]
    _Float16* const s_b = s_a + AH * AW * AS;                           // [BH * BW][AS] (NL = 3)
    _Float16* const s_out = s_b + (NL == 3 ? BH * BW * AS : 0);         // [kGH * kGW][16]: the last layer's channels per pixel
    _Float16* const s_pad = s_out + kGW * kGH * 16;                     // {1, 0 x 7} (bias slot), {0 x 8}
    static_assert((IH * IW * kCIn) % 8 == 0 && AS % 8 == 0, "16-byte aligned LDS regions");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 16) s_pad[tid] = (_Float16)(tid == 0 ? 1.f : 0.f);  // (published by the barrier after stage A)
    const int tiles_x = (W + kGW - 1) / kGW;
    const int tx_first = blockIdx.x * strip;
    const int y0 = blockIdx.y * kGH;
    const int64_t HW = (int64_t)H * W;
    aux += (int64_t)blockIdx.z * (IN == 2 ? 4 : kCIn) * HW;
    weight_out += (int64_t)blockIdx.z * L * HW;
    guidance_out += (int64_t)blockIdx.z * L * HW;
    const int col = lane & 15, kg = lane >> 4;

    // Tile skipping as in guidance_fused, with halo NL (guidance_strip.inc): a tile whose input region lies inside the image and
    // in unmarked render tiles is filled with the background maps.
    unsigned long long rmk[3];
    const uint32_t skip_tiles = strip_marks<NL>(cull, rmk, lane, tx_first, y0, strip, tiles_x, H, W);
    if (cull.mask) fill_skipped_planes(cull, skip_tiles, weight_out, guidance_out, L, HW, W, tid, tx_first, y0, strip, tiles_x);

    // ---- stage A (guidance_strip.inc); the next computed tile's loads are issued before this tile's layers
    float v[kStageIters<NL>][kStagePlanes<IN>];
    int ts_live = next_live(skip_tiles, 0, strip, tx_first, tiles_x);
    if (ts_live < kStrip) fetch<NL, IN, false>(v, aux, cull, rmk, tx_first, ts_live, y0, H, W, HW, tid);

#pragma nounroll
    while (ts_live < kStrip) {  // (workgroup-uniform)
        const int x0 = (tx_first + ts_live) * kGW;
        ts_live = next_live(skip_tiles, ts_live + 1, strip, tx_first, tiles_x);
        stage<NL, IN>(v, s_in, tid);
        __syncthreads();  // s_in complete; every thread is also done with the previous tile's s_out
        if (ts_live < kStrip) fetch<NL, IN, false>(v, aux, cull, rmk, tx_first, ts_live, y0, H, W, HW, tid);

        // ---- layer 1: s_in -> s_a (halo NL - 1)
        conv_layer<8, NT1, 3, IW, kCIn, AW, AH, AS, true>(s_in, s_a, w1, nullptr, s_pad, x0 - (NL - 1), y0 - (NL - 1), H, W, wave, col, kg);
        __syncthreads();
        if constexpr (NL == 3) {  // ---- middle layer: s_a -> s_b (halo 1)
            conv_layer<C1P, NT1, KS, AW, AS, BW, BH, AS, true>(s_a, s_b, wm, bm, s_pad, x0 - 1, y0 - 1, H, W, wave, col, kg);
            __syncthreads();
        }
        // ---- last layer on the tile itself: 2 L channels padded to 16, per pixel into s_out
        conv_layer<C1P, 1, KS, BW, AS, kGW, kGH, 16, false>(NL == 3 ? s_b : s_a, s_out, wl, bl, s_pad, x0, y0, H, W, wave, col, kg);
        __syncthreads();

        // ---- .float(), softmax over the first L channels, stores: thread = pixel of the tile
        {
            const int gx = x0 + (tid & 31), gy = y0 + (tid >> 5);
            if (gx < W && gy < H) {
                const half8 lo = *reinterpret_cast<const half8*>(s_out + tid * 16), hi = *reinterpret_cast<const half8*>(s_out + tid * 16 + 8);
                float c[12];
#pragma unroll
                for (int i = 0; i < 8; ++i) c[i] = (float)lo[i];
#pragma unroll
                for (int i = 0; i < 4; ++i) c[8 + i] = (float)hi[i];
                const int64_t pix = (int64_t)gy * W + gx;
                auto finish = [&](auto level_tag) {
                    constexpr int LL = decltype(level_tag)::value;
                    float wgt[LL];
                    softmax_weights_n<LL>(c, wgt);  // network.py:113-114
#pragma unroll
                    for (int i = 0; i < LL; ++i) {
                        weight_out[i * HW + pix] = wgt[i];
                        guidance_out[i * HW + pix] = c[LL + i];  // (:116)
                    }
                };
                switch (L) {  // (workgroup-uniform)
                    case 1: finish(std::integral_constant<int, 1>{}); break;
                    case 2: finish(std::integral_constant<int, 2>{}); break;
                    case 3: finish(std::integral_constant<int, 3>{}); break;
                    case 4: finish(std::integral_constant<int, 4>{}); break;
                    case 5: finish(std::integral_constant<int, 5>{}); break;
                    default: finish(std::integral_constant<int, 6>{}); break;
                }
            }
        }
    }  // strip
}

template <int C1P, int NL, int IN>
hipError_t launch_general_one(dim3 grid, hipStream_t stream, const float* aux, const void* w1, const void* wm, const void* wl, const float* bm,
                              const float* bl, float* weight_out, float* guidance_out, int H, int W, int L, const NetCull& cull, int strip) {
    constexpr size_t lds = (size_t)gen_lds_halves<C1P, NL>() * sizeof(_Float16);
    static_assert(lds <= 160 * 1024, "the CU has 160 KB of LDS");
    if (lds > 64 * 1024) {  // beyond the default dynamic-LDS window: ask for it
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&guidance_general<C1P, NL, IN>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((guidance_general<C1P, NL, IN>), grid, dim3(256), lds, stream, aux, (const _Float16*)w1, (const _Float16*)wm,
                       (const _Float16*)wl, bm, bl, weight_out, guidance_out, H, W, L, cull, strip);
    return hipGetLastError();
}
