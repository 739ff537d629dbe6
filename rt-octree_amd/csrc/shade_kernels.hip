// shade_kernels.hip -- the shading stage of the batched path: shade_kernel / shade_kernel_layers, their knobs (RTO_SHADE_*) and the
// one launcher that owns their grid and dispatch, launch_shade (rto_render_internal.h); and the basis probe, which reports the
// shading kernel's per-B basis forms (launch_probe_basis, rto_launch.h).  One of the render stage's units: see the map in
// render_kernels.hip.
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"
#include "rto_tree_device.h"

#pragma clang fp contract(off)

// hit entries, the bases, packed leaf shading: shared with the other render units
#include "rto_render_shared.h"

namespace rto {

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

}  // namespace rto

// ------------------------------------------------------------------ host launchers (C++ linkage,
// declared in rto_render_internal.h and rto_launch.h)
#include "rto_dispatch.h"
#include "rto_launch.h"
#include "rto_render_internal.h"

namespace rto {

#ifndef RTO_SHADE_P
#define RTO_SHADE_P 2
#endif
hipError_t launch_shade(int spp, const TreeDev& tree, const OptDev& opt, const FrameBatch& fb, const uint32_t* hits, const LayerDev* layers,
                        hipStream_t stream) {
    const bool color_layer = layers && layers->color;
    const int64_t size = (int64_t)fb.width * fb.height;
    return with_spp(spp, [&](auto SPP) {
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
                    else
                        hipLaunchKernelGGL((shade_kernel_layers<SPP, SP, mode, lobes>), sgrid, sblock, 0, stream, tree, opt, fb, (const uint32_t*)hits, *layers);
                });
            });
        }
        return hipGetLastError();
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

}  // namespace rto
