// guidance_train_kernels.hip -- the GuidanceNet under training (denoiser/network.py:49-118) and its loss (denoiser/runner.py:71-84,
// denoiser/metrics.py:7-9) in float32 with float32 accumulation.  DESIGN.md 7i.
//
// A RepVGG block has no normalisation: before its ReLU6 it is linear in its input, so the sum of its branches IS one 3x3
// convolution with the summed weights.  The caller sums the branches (denoiser.effective_layers, differentiably) and hands
// each layer's effective kernel W_l [cout][cin][3][3] and bias b_l over; autograd deals this file's dW_l / db_l back out.
//
//   gt_conv<COP>    one 32 x 16 pixel tile per workgroup, two pixels and all (padded to COP) output channels per thread; input
//                   channels pass through LDS eight at a time together with their weights.  Three uses of the one loop:
//                   a forward layer (bias, ReLU6, store x_l), the last forward layer (... plus the softmax and the two maps), and
//                   the backward's dx_{l-1} = conv(dz_l, W_l transposed and flipped), masked at once into dz_{l-1}.
//   gt_dz_last      dz of the last layer from the two map gradients: softmax backward, ReLU6 mask.
//   gt_wgrad        dW_l and db_l: thread = one (cout, cin) pair with its nine taps in registers, walking 32 x 4 pixel tiles of
//                   dz_l and x_{l-1} in LDS; workgroup g takes tiles g, g + G, ...; its sums go to partials[g].
//   gt_wgrad_finish adds the partials in workgroup order.  No atomics anywhere: same inputs, same bits.
//   loss_terms / loss_finish   the loss in float64 (the convention of metrics_kernels.hip) and its gradient.
// The Makefile compiles this file with -ffp-contract=off and without the SLP vectoriser like the rest; the multiply-adds that
// are meant to be fused are written as fmaf.
#include <hip/hip_runtime.h>

#include "rto_guidance_train_launch.h"

namespace rto {
namespace {

constexpr int kThreads = 256;

// ---------------------------------------------------------------- gt_conv
constexpr int kCTW = 32, kCTH = 16;                // tile
constexpr int kCK = 8;                             // input channels per LDS chunk
constexpr int kInW = kCTW + 2, kInH = kCTH + 2;    // staged 34 x 18
constexpr int kInPlane = kInW * kInH;
enum { kConvMid = 0, kConvLast = 1, kConvData = 2 };

struct ConvArgs {
    const float* in;    // [n][cin][H][W]
    const float* w;     // the LAYER's kernel [cout_l][cin_l][3][3]
    const float* bias;  // forward modes
    const float* mask;  // kConvData: x_{l-1} [n][cout][H][W], whose ReLU6 mask the result takes
    float* out;         // x_l, or dz_{l-1}
    float* wmap;        // kConvLast
    float* gmap;
    int cin, cout;      // of THIS convolution (kConvData: cin = cout_l, cout = cin_l)
    int H, W, levels, mode;
};

__device__ __forceinline__ float relu6_mask(float x) { return (x > 0.0f && x < 6.0f) ? 1.0f : 0.0f; }  // hardtanh_backward

template <int COP>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& a, float (&acc)[COP], int frame, int gy, int gx) {
    const size_t plane = (size_t)a.H * a.W;
    const size_t pix = (size_t)gy * a.W + gx;
    const size_t base = (size_t)frame * a.cout * plane + pix;
    if (a.mode == kConvData) {
#pragma unroll
        for (int co = 0; co < COP; ++co)
            if (co < a.cout) a.out[base + co * plane] = acc[co] * relu6_mask(a.mask[base + co * plane]);
        return;
    }
#pragma unroll
    for (int co = 0; co < COP; ++co)
        if (co < a.cout) {
            acc[co] = fminf(fmaxf(acc[co] + a.bias[co], 0.0f), 6.0f);
            a.out[base + co * plane] = acc[co];
        }
    if constexpr (COP <= 2 * kTrainMaxLevels) {
        if (a.mode == kConvLast) {  // network.py:111-118
            const int L = a.levels;
            float m = acc[0];
#pragma unroll
            for (int k = 1; k < COP; ++k)
                if (k < L) m = fmaxf(m, acc[k]);
            float sum = 0.0f;
#pragma unroll
            for (int k = 0; k < COP; ++k)
                if (k < L) sum += expf(acc[k] - m);
            const size_t mbase = (size_t)frame * L * plane + pix;
#pragma unroll
            for (int k = 0; k < COP; ++k) {
                if (k < L) a.wmap[mbase + k * plane] = expf(acc[k] - m) / sum;
                else if (k < 2 * L) a.gmap[mbase + (k - L) * plane] = acc[k];
            }
        }
    }
}

template <int COP>
__global__ __launch_bounds__(kThreads) void gt_conv(ConvArgs a) {
    __shared__ float s_in[kCK * kInPlane];
    __shared__ __attribute__((aligned(16))) float s_w[kCK * 9 * COP];
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int x0 = blockIdx.x * kCTW, y0 = blockIdx.y * kCTH, frame = blockIdx.z;
    const size_t plane = (size_t)a.H * a.W;
    const float* in = a.in + (size_t)frame * a.cin * plane;

    float acc0[COP], acc1[COP];
#pragma unroll
    for (int co = 0; co < COP; ++co) acc0[co] = acc1[co] = 0.0f;

    for (int c0 = 0; c0 < a.cin; c0 += kCK) {
        const int nck = min(kCK, a.cin - c0);
        __syncthreads();  // (the previous chunk has been read)
        for (int i = tid; i < nck * kInPlane; i += kThreads) {
            const int cl = i / kInPlane, r = i - cl * kInPlane;
            const int ly = r / kInW, lx = r - ly * kInW;
            const int gy = y0 + ly - 1, gx = x0 + lx - 1;
            float v = 0.0f;  // zero padding "same"
            if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) v = in[(size_t)(c0 + cl) * plane + (size_t)gy * a.W + gx];
            s_in[i] = v;
        }
        for (int i = tid; i < nck * 9 * COP; i += kThreads) {
            const int co = i % COP, t = (i / COP) % 9, ci = c0 + i / (COP * 9);
            float v = 0.0f;
            if (co < a.cout)
                v = a.mode == kConvData ? a.w[((size_t)ci * a.cout + co) * 9 + (8 - t)]  // W_l[ci][co] flipped: the transposed convolution
                                        : a.w[((size_t)co * a.cin + ci) * 9 + t];
            s_w[i] = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int cl = 0; cl < nck; ++cl) {
            const float* p = s_in + cl * kInPlane + ty * kInW + tx;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float xa = p[(t / 3) * kInW + (t % 3)];
                const float xb = p[(t / 3 + kCTH / 2) * kInW + (t % 3)];
                const float4* wv = reinterpret_cast<const float4*>(s_w + (cl * 9 + t) * COP);
#pragma unroll
                for (int q = 0; q < COP / 4; ++q) {
                    const float4 w = wv[q];  // (one address for the whole wave: a broadcast)
                    acc0[4 * q + 0] = fmaf(xa, w.x, acc0[4 * q + 0]);
                    acc0[4 * q + 1] = fmaf(xa, w.y, acc0[4 * q + 1]);
                    acc0[4 * q + 2] = fmaf(xa, w.z, acc0[4 * q + 2]);
                    acc0[4 * q + 3] = fmaf(xa, w.w, acc0[4 * q + 3]);
                    acc1[4 * q + 0] = fmaf(xb, w.x, acc1[4 * q + 0]);
                    acc1[4 * q + 1] = fmaf(xb, w.y, acc1[4 * q + 1]);
                    acc1[4 * q + 2] = fmaf(xb, w.z, acc1[4 * q + 2]);
                    acc1[4 * q + 3] = fmaf(xb, w.w, acc1[4 * q + 3]);
                }
            }
        }
    }
    const int gx = x0 + tx;
    if (gx < a.W) {
        if (y0 + ty < a.H) conv_epilogue<COP>(a, acc0, frame, y0 + ty, gx);
        if (y0 + ty + kCTH / 2 < a.H) conv_epilogue<COP>(a, acc1, frame, y0 + ty + kCTH / 2, gx);
    }
}

// ---------------------------------------------------------------- gt_dz_last
// x [n][2L][H][W] = the last layer's activations; dz the same shape.  Softmax backward dx_k = w_k (g_k - sum_j g_j w_j) with the
// forward's own w_k recomputed from x; guidance channels pass their gradient; both under the ReLU6 mask of x.
__global__ __launch_bounds__(kThreads) void gt_dz_last(const float* __restrict__ x, const float* __restrict__ gw, const float* __restrict__ gg,
                                                       int L, size_t plane, size_t pixels, float* __restrict__ dz) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= pixels) return;
    const size_t frame = i / plane, pix = i - frame * plane;
    const size_t xb = frame * 2 * L * plane + pix, mb = frame * L * plane + pix;
    float v[kTrainMaxLevels], e[kTrainMaxLevels];
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < kTrainMaxLevels; ++k) {
        v[k] = k < L ? x[xb + k * plane] : 0.0f;
        m = k == 0 ? v[0] : (k < L ? fmaxf(m, v[k]) : m);
    }
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < kTrainMaxLevels; ++k)
        if (k < L) sum += (e[k] = expf(v[k] - m));
    float dot = 0.0f;
#pragma unroll
    for (int k = 0; k < kTrainMaxLevels; ++k)
        if (k < L) {
            e[k] = e[k] / sum;
            dot = fmaf(gw[mb + k * plane], e[k], dot);
        }
#pragma unroll
    for (int k = 0; k < kTrainMaxLevels; ++k)
        if (k < L) {
            dz[xb + k * plane] = e[k] * (gw[mb + k * plane] - dot) * relu6_mask(v[k]);
            const float xg = x[xb + (size_t)(L + k) * plane];
            dz[xb + (size_t)(L + k) * plane] = gg[mb + k * plane] * relu6_mask(xg);
        }
}

// ---------------------------------------------------------------- gt_wgrad
constexpr int kWTW = 32, kWTH = 4;
constexpr int kWInW = kWTW + 2, kWInH = kWTH + 2;
constexpr int kWXStride = kWInW * kWInH + 1;  // 205: odd, so the lanes' consecutive channels fall on distinct banks
constexpr int kWDStride = kWTW * kWTH + 1;    // 129

struct WgradGeom {
    int grid_y, G, tiles_x, tiles_y, nco;
    size_t tiles, pstride, lds_bytes;
};

WgradGeom wgrad_geom(int cin, int cout, int n, int H, int W) {
    WgradGeom g;
    const int pairs = cin * cout;
    g.grid_y = (pairs + kThreads - 1) / kThreads;
    g.tiles_x = (W + kWTW - 1) / kWTW;
    g.tiles_y = (H + kWTH - 1) / kWTH;
    g.tiles = (size_t)g.tiles_x * g.tiles_y * n;
    const size_t cap = (size_t)(2048 / g.grid_y);
    g.G = (int)(g.tiles < cap ? g.tiles : cap);
    g.nco = (kThreads - 1) / cin + 2;  // output channels 256 consecutive pairs can touch
    if (g.nco > cout) g.nco = cout;
    g.pstride = (size_t)pairs * 9 + cout;
    g.lds_bytes = ((size_t)cin * kWXStride + (size_t)g.nco * kWDStride) * sizeof(float);
    return g;
}

// dz [n][cout][H][W], x [n][cin][H][W]; partials [G][cout * cin * 9 + cout]
__global__ __launch_bounds__(kThreads) void gt_wgrad(const float* __restrict__ dz, const float* __restrict__ x, int cin, int cout, int H,
                                                     int W, int tiles_x, int tiles_y, int tiles, size_t pstride,
                                                     float* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_x = smem;
    float* s_d = smem + cin * kWXStride;
    const int tid = threadIdx.x;
    const int pairs = cin * cout;
    const int qbase = blockIdx.y * kThreads, q = qbase + tid;
    const bool active = q < pairs;
    const int co_lo = qbase / cin;
    const int co_hi = min(cout - 1, (qbase + kThreads - 1) / cin);
    const int nco = co_hi - co_lo + 1;
    const int co = active ? q / cin : co_lo, ci = active ? q - co * cin : 0;
    const size_t plane = (size_t)H * W;
    const int per_frame = tiles_x * tiles_y;

    float acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = 0.0f;
    float accb = 0.0f;

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int frame = tile / per_frame, r0 = tile - frame * per_frame;
        const int ty = r0 / tiles_x, tx = r0 - ty * tiles_x;
        const int x0 = tx * kWTW, y0 = ty * kWTH;
        __syncthreads();
        for (int i = tid; i < cin * (kWInW * kWInH); i += kThreads) {
            const int c = i / (kWInW * kWInH), r = i - c * (kWInW * kWInH);
            const int ly = r / kWInW, lx = r - ly * kWInW;
            const int gy = y0 + ly - 1, gx = x0 + lx - 1;
            float v = 0.0f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = x[((size_t)frame * cin + c) * plane + (size_t)gy * W + gx];
            s_x[c * kWXStride + r] = v;
        }
        for (int i = tid; i < nco * (kWTW * kWTH); i += kThreads) {
            const int c = i / (kWTW * kWTH), r = i - c * (kWTW * kWTH);
            const int gy = y0 + r / kWTW, gx = x0 + (r % kWTW);
            float v = 0.0f;  // (pixels past the frame add nothing)
            if (gy < H && gx < W) v = dz[((size_t)frame * cout + co_lo + c) * plane + (size_t)gy * W + gx];
            s_d[c * kWDStride + r] = v;
        }
        __syncthreads();
        if (active) {
            const float* px = s_x + ci * kWXStride;
            const float* pd = s_d + (co - co_lo) * kWDStride;
#pragma unroll 1
            for (int ly = 0; ly < kWTH; ++ly) {
#pragma unroll
                for (int lx = 0; lx < kWTW; ++lx) {
                    const float d = pd[ly * kWTW + lx];
                    accb += d;
#pragma unroll
                    for (int t = 0; t < 9; ++t) acc[t] = fmaf(d, px[(ly + t / 3) * kWInW + lx + t % 3], acc[t]);
                }
            }
        }
    }
    if (active) {
        float* p = partials + (size_t)blockIdx.x * pstride;
#pragma unroll
        for (int t = 0; t < 9; ++t) p[(size_t)q * 9 + t] = acc[t];
        if (ci == 0) p[(size_t)pairs * 9 + co] = accb;
    }
}

__global__ __launch_bounds__(kThreads) void gt_wgrad_finish(const float* __restrict__ partials, int G, size_t pstride, size_t nw,
                                                            float* __restrict__ dw, float* __restrict__ db) {
    const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= pstride) return;
    float s = 0.0f;
    for (int g = 0; g < G; ++g) s += partials[(size_t)g * pstride + e];
    if (e < nw) dw[e] = s;
    else db[e - nw] = s;
}

// ---------------------------------------------------------------- loss
__device__ __forceinline__ double sign_of(double v) { return (double)(v > 0.0) - (double)(v < 0.0); }

// one channel's term and its derivative with respect to p, float64 from the float32 inputs
template <int KIND>
__device__ __forceinline__ double loss_term(float pf, float tf, double& dp) {
    const double p = (double)pf, t = (double)tf, d = p - t;
    if (KIND == kLossMse) {
        dp = 2.0 * d;
        return d * d;
    }
    const double D = fabs(p) + fabs(t) + 1e-5;  // metrics.py:7-9
    dp = sign_of(d) / D - fabs(d) * sign_of(p) / (D * D);
    return fabs(d) / D;
}

template <int KIND>
__global__ __launch_bounds__(kThreads) void loss_terms(const float4* __restrict__ pred, const float4* __restrict__ truth, size_t pixels,
                                                       double scale, double* __restrict__ partials, float4* __restrict__ grad) {
    __shared__ double red[kThreads];
    const int tid = threadIdx.x;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kLossPixelsPerGroup / kThreads; ++k) {
        const size_t i = (size_t)blockIdx.x * kLossPixelsPerGroup + (size_t)k * kThreads + tid;
        if (i < pixels) {
            const float4 p = pred[i], t = truth[i];
            double gx, gy, gz;
            s += loss_term<KIND>(p.x, t.x, gx);
            s += loss_term<KIND>(p.y, t.y, gy);
            s += loss_term<KIND>(p.z, t.z, gz);
            grad[i] = make_float4((float)(gx * scale), (float)(gy * scale), (float)(gz * scale), 0.0f);
        }
    }
    red[tid] = s;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {  // a tree over the thread index, the same additions every time
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) partials[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(kThreads) void loss_finish(const double* __restrict__ partials, size_t count, double scale,
                                                        double* __restrict__ out) {
    __shared__ double red[kThreads];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (size_t i = tid; i < count; i += kThreads) s += partials[i];
    red[tid] = s;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) *out = red[0] * scale;
}

// ---------------------------------------------------------------- launchers
int conv_cop(int cout) { return cout <= 4 ? 4 : cout <= 8 ? 8 : cout <= 12 ? 12 : cout <= 16 ? 16 : cout <= 32 ? 32 : 64; }

hipError_t launch_conv(const ConvArgs& a, int n, hipStream_t stream) {
    const dim3 grid((unsigned)((a.W + kCTW - 1) / kCTW), (unsigned)((a.H + kCTH - 1) / kCTH), (unsigned)n), block(kThreads);
    switch (conv_cop(a.cout)) {
        case 4: gt_conv<4><<<grid, block, 0, stream>>>(a); break;
        case 8: gt_conv<8><<<grid, block, 0, stream>>>(a); break;
        case 12: gt_conv<12><<<grid, block, 0, stream>>>(a); break;
        case 16: gt_conv<16><<<grid, block, 0, stream>>>(a); break;
        case 32: gt_conv<32><<<grid, block, 0, stream>>>(a); break;
        default: gt_conv<64><<<grid, block, 0, stream>>>(a); break;
    }
    return hipGetLastError();
}

int widest(const TrainLayer* layers, int num_layers) {
    int c = 0;
    for (int l = 0; l < num_layers; ++l) c = layers[l].cout > c ? layers[l].cout : c;
    return c;
}

}  // namespace

size_t train_acts_floats(const TrainLayer* layers, int num_layers, int n, int H, int W) {
    size_t c = 0;
    for (int l = 0; l < num_layers; ++l) c += (size_t)layers[l].cout;
    return c * (size_t)n * H * W;
}

size_t train_dz_floats(const TrainLayer* layers, int num_layers, int n, int H, int W) {
    return (size_t)widest(layers, num_layers) * n * H * W;
}

size_t train_partial_floats(const TrainLayer* layers, int num_layers, int n, int H, int W) {
    size_t need = 0;
    for (int l = 0; l < num_layers; ++l) {
        const WgradGeom g = wgrad_geom(layers[l].cin, layers[l].cout, n, H, W);
        const size_t f = (size_t)g.G * g.pstride;
        need = f > need ? f : need;
    }
    return need;
}

hipError_t launch_train_forward(const float* aux, const TrainLayer* layers, int num_layers, int levels, int n, int H, int W, float* acts,
                                float* weight_map, float* guidance_map, hipStream_t stream) {
    const size_t pixels = (size_t)n * H * W;
    const float* in = aux;
    float* out = acts;
    for (int l = 0; l < num_layers; ++l) {
        ConvArgs a{};
        a.in = in, a.w = layers[l].w, a.bias = layers[l].b, a.out = out;
        a.wmap = weight_map, a.gmap = guidance_map;
        a.cin = layers[l].cin, a.cout = layers[l].cout;
        a.H = H, a.W = W, a.levels = levels, a.mode = l == num_layers - 1 ? kConvLast : kConvMid;
        if (const hipError_t e = launch_conv(a, n, stream)) return e;
        in = out;
        out += (size_t)layers[l].cout * pixels;
    }
    return hipSuccess;
}

hipError_t launch_train_backward(const float* grad_weight_map, const float* grad_guidance_map, const float* aux, const float* acts,
                                 const TrainLayer* layers, int num_layers, int levels, int n, int H, int W, float* dz0, float* dz1,
                                 float* partials, hipStream_t stream) {
    const size_t plane = (size_t)H * W, pixels = plane * n;
    const float* x[kTrainMaxLayers + 1];  // x[l] = the input of layer l; x[num_layers] = the last activations
    x[0] = aux;
    for (int l = 0; l < num_layers; ++l) x[l + 1] = (l == 0 ? acts : x[l]) + (l == 0 ? 0 : (size_t)layers[l - 1].cout * pixels);
    float* dz = dz0;
    float* other = dz1;
    gt_dz_last<<<dim3((unsigned)((pixels + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream>>>(
        x[num_layers], grad_weight_map, grad_guidance_map, levels, plane, pixels, dz);
    if (const hipError_t e = hipGetLastError()) return e;
    for (int l = num_layers - 1; l >= 0; --l) {
        const int cin = layers[l].cin, cout = layers[l].cout;
        const WgradGeom g = wgrad_geom(cin, cout, n, H, W);
        gt_wgrad<<<dim3((unsigned)g.G, (unsigned)g.grid_y), dim3(kThreads), g.lds_bytes, stream>>>(
            dz, x[l], cin, cout, H, W, g.tiles_x, g.tiles_y, (int)g.tiles, g.pstride, partials);
        if (const hipError_t e = hipGetLastError()) return e;
        gt_wgrad_finish<<<dim3((unsigned)((g.pstride + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream>>>(
            partials, g.G, g.pstride, (size_t)cin * cout * 9, layers[l].dw, layers[l].db);
        if (const hipError_t e = hipGetLastError()) return e;
        if (l == 0) break;  // (no gradient for the aux planes)
        ConvArgs a{};
        a.in = dz, a.w = layers[l].w, a.mask = x[l], a.out = other;
        a.cin = cout, a.cout = cin;
        a.H = H, a.W = W, a.levels = levels, a.mode = kConvData;
        if (const hipError_t e = launch_conv(a, n, stream)) return e;
        float* t = dz;
        dz = other, other = t;
    }
    return hipSuccess;
}

hipError_t launch_loss(const float* pred, const float* truth, int n, int H, int W, int kind, double* partials, double* loss_out,
                       float* grad, hipStream_t stream) {
    const size_t pixels = (size_t)n * H * W, groups = loss_partial_doubles(n, H, W);
    const double scale = 1.0 / (3.0 * (double)pixels);
    const float4* p = reinterpret_cast<const float4*>(pred);
    const float4* t = reinterpret_cast<const float4*>(truth);
    float4* g = reinterpret_cast<float4*>(grad);
    if (kind == kLossMse)
        loss_terms<kLossMse><<<dim3((unsigned)groups), dim3(kThreads), 0, stream>>>(p, t, pixels, scale, partials, g);
    else
        loss_terms<kLossSmape><<<dim3((unsigned)groups), dim3(kThreads), 0, stream>>>(p, t, pixels, scale, partials, g);
    if (const hipError_t e = hipGetLastError()) return e;
    loss_finish<<<dim3(1), dim3(kThreads), 0, stream>>>(partials, groups, scale, loss_out);
    return hipGetLastError();
}

}  // namespace rto
