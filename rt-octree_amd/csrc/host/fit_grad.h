// host/fit_grad.h -- the host twin of rto_tree_fit_grad / rto_fit_sgd_step (include/rto.h "tree fit") and the argument checks
// both entries share.  Plain C++: no HIP header, compiles with g++ -ffp-contract=off (tools/sanitize/fit_fuzz.cpp).
#pragma once
#include <stdint.h>

#include <string>

#include "rto.h"

namespace rto {

// basis_dim of a tree the fit takes (SH 1 / 4 / 9 / 16 / 25), 0 for RGBA, -1: not taken.  data_format: "RGBA" or "SH<B>"
int fit_basis_of_format(const char* data_format, int data_dim);
// the same from a tree's (format, basis_dim, data_dim)
int fit_basis_of_tree(int format, int basis_dim, int data_dim);

// "" or what is wrong with a call's pointers, cameras and options (checked before anything is enqueued or marched); bytes of
// params = param_count * 4, of grad = param_count * 8
std::string fit_check_call(const float* params, const rto_camera* cams, const float* const* targets, float* const* images, int n,
                           const rto_options* opt, const int64_t* grad, const uint64_t* stats, int64_t param_count);

// Both marches over child[] / data[] with the root-restart float descent, `threads` threads (<= 0: one) over the rows of each
// camera.  data: the fp16 arrays the support is read from; params float32 [capacity][N][N][N][D]; targets / images: host
// [H][W][3] per camera.  grad / stats are accumulated into with integer adds: the result does not depend on `threads`.
// RTO_OK, or RTO_E_INVALID / RTO_E_UNSUPPORTED / RTO_E_FORMAT with *err set; child[] is walked from the root first.
int fit_grad_host(const int32_t* child, const uint16_t* data, const float* params, int64_t capacity, int N, int D, const char* data_format,
                  const float scale[3], const float offset[3], const float* ndc, const rto_camera* cams, const float* const* targets,
                  float* const* images, int n, const rto_options* opt, int threads, int64_t* grad, uint64_t* stats, std::string* err);

// the same for a call on rays (rto_tree_fit_grad_rays / rto_fit_grad_rays_host): origins, dirs, targets, out are [n][3] floats
std::string fit_check_rays_call(const float* params, const float* origins, const float* dirs, const float* targets, const float* out, int64_t n,
                                const rto_options* opt, const int64_t* grad, const uint64_t* stats, int64_t param_count);

// fit_grad_host on n rays of the caller's (rto_fit_grad_rays_host): `threads` threads (<= 0: one) over contiguous ranges of rays;
// the result does not depend on `threads`.
int fit_grad_rays_host(const int32_t* child, const uint16_t* data, const float* params, int64_t capacity, int N, int D, const char* data_format,
                       const float scale[3], const float offset[3], const float* ndc, const float* origins, const float* dirs,
                       const float* targets, float* out, int64_t n, const rto_options* opt, int threads, int64_t* grad, uint64_t* stats,
                       std::string* err);

// fit_grad_rays_host that also marks the touched bitmap (rto_fit_grad_rays_touched_host, marking = true: grad and touched are
// required; marking = false is fit_grad_rays_host).  fit_check_touched: "" or what is wrong with the bitmap of a marking call
// (slots = capacity * N^3), shared with the device entry
std::string fit_check_touched(const float* params, const float* origins, const float* dirs, const float* targets, const float* out, int64_t n,
                              const int64_t* grad, const uint64_t* stats, const uint32_t* touched, int64_t slots, int D);
int fit_grad_rays_touched_host(const int32_t* child, const uint16_t* data, const float* params, int64_t capacity, int N, int D,
                               const char* data_format, const float scale[3], const float offset[3], const float* ndc, const float* origins,
                               const float* dirs, const float* targets, float* out, int64_t n, const rto_options* opt, int threads,
                               int64_t* grad, uint64_t* stats, uint32_t* touched, bool marking, std::string* err);

// p = p - lr * g over count parameters, g from the fixed-point word, which is zeroed
int fit_sgd_step_host(float* params, int64_t* grad, int64_t count, float lr, std::string* err);

}  // namespace rto
