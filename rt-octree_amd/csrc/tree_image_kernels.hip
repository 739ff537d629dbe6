// tree_image_kernels.hip -- the kernels that build a tree's derived device arrays (traversal image, top grid, aligned and
// quantised records) and rebuild the reference layout from them, and the two small helpers of a launch (frame table, u8
// conversion), with their launchers (rto_launch.h).  One of the render stage's units: see the map in render_kernels.hip.
#include <hip/hip_runtime.h>

#include "rto_kernel_types.h"
#include "rto_launch.h"
#include "rto_tree_device.h"

#pragma clang fp contract(off)

namespace rto {

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

// ------------------------------------------------------------------ host launchers (declared in rto_launch.h)

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

hipError_t launch_pack_quant(const uint16_t* qmap, const uint16_t* retained, int64_t ns, int nr, int nq, int rec,
                             uint16_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(pack_quant_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, stream, qmap, retained, ns, nr,
                       nq, rec, out);
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
