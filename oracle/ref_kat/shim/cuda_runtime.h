// Stand-in for NVIDIA's <cuda_runtime.h>, written for oracle/ref_kat only.  It lets g++ read the reference's headers as
// plain host C++ (__CUDACC__ stays undefined): the execution-space qualifiers vanish, the handful of runtime types and
// calls that render_context.hpp names exist and do nothing, and the device intrinsics the ray core calls are given host
// meanings:
//   __mul24(a, b)   a * b
//   min / max       std::min / std::max
//   __logf, __expf  orc_det_logf / orc_det_expf of oracle/rto_oracle.c -- the definitions this project puts in the place
//                   of NVIDIA's approximations (DESIGN.md "Math definitions"), so that the reference's control flow,
//                   operation order and rounding points run over the same log and exp as the oracle and the kernels.
// Nothing here comes from the reference or from the CUDA toolkit.
#ifndef RTO_REF_KAT_SHIM_CUDA_RUNTIME_H
#define RTO_REF_KAT_SHIM_CUDA_RUNTIME_H
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __inline__ inline
#define __restrict__ __restrict

using std::max;
using std::min;

extern "C" float orc_det_logf(float x);
extern "C" float orc_det_expf(float x);
// (macros, after <cmath>: glibc declares functions of these names itself)
#define __logf(x) orc_det_logf(x)
#define __expf(x) orc_det_expf(x)

static inline int __mul24(int a, int b) { return a * b; }

struct float4 {
    float x, y, z, w;
};

typedef int cudaError_t;
enum { cudaSuccess = 0 };
typedef struct rto_shim_stream* cudaStream_t;
typedef struct rto_shim_event* cudaEvent_t;
typedef struct rto_shim_array* cudaArray_t;
typedef unsigned long long cudaSurfaceObject_t;
typedef unsigned long long cudaTextureObject_t;

struct cudaChannelFormatDesc {
    int x, y, z, w, f;
};
template <typename T>
inline cudaChannelFormatDesc cudaCreateChannelDesc() {
    return cudaChannelFormatDesc{(int)sizeof(T) * 8, 0, 0, 0, 0};
}

enum cudaResourceType { cudaResourceTypeArray = 0 };
struct cudaResourceDesc {
    cudaResourceType resType;
    struct {
        struct {
            cudaArray_t array;
        } array;
    } res;
};
enum cudaTextureFilterMode { cudaFilterModePoint = 0 };
enum cudaTextureAddressMode { cudaAddressModeWrap = 0 };
enum cudaTextureReadMode { cudaReadModeElementType = 0 };
struct cudaTextureDesc {
    cudaTextureAddressMode addressMode[3];
    cudaTextureFilterMode filterMode;
    cudaTextureReadMode readMode;
    int normalizedCoords;
};

template <typename T>
inline cudaError_t cudaMalloc(T** p, size_t n) {
    *p = (T*)std::malloc(n);
    return cudaSuccess;
}
inline cudaError_t cudaFree(void* p) {
    std::free(p);
    return cudaSuccess;
}
inline cudaError_t cudaMallocArray(cudaArray_t* a, const cudaChannelFormatDesc*, size_t, size_t) {
    *a = nullptr;
    return cudaSuccess;
}
inline cudaError_t cudaFreeArray(cudaArray_t) { return cudaSuccess; }
inline cudaError_t cudaCreateSurfaceObject(cudaSurfaceObject_t* s, const cudaResourceDesc*) {
    *s = 0;
    return cudaSuccess;
}
inline cudaError_t cudaDestroySurfaceObject(cudaSurfaceObject_t) { return cudaSuccess; }
inline cudaError_t cudaCreateTextureObject(cudaTextureObject_t* t, const cudaResourceDesc*, const cudaTextureDesc*, const void*) {
    *t = 0;
    return cudaSuccess;
}
inline cudaError_t cudaEventCreate(cudaEvent_t* e) {
    *e = nullptr;
    return cudaSuccess;
}
inline cudaError_t cudaEventDestroy(cudaEvent_t) { return cudaSuccess; }
inline cudaError_t cudaEventRecord(cudaEvent_t, cudaStream_t) { return cudaSuccess; }
inline cudaError_t cudaEventSynchronize(cudaEvent_t) { return cudaSuccess; }
inline cudaError_t cudaEventElapsedTime(float* ms, cudaEvent_t, cudaEvent_t) {
    *ms = 0.f;
    return cudaSuccess;
}

#endif
