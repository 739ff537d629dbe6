// host/fit_sparse.h -- the host twins of rto_fit_touched_list and rto_fit_step_sparse (include/rto.h "tree fit") and the argument
// checks both entries share.  Plain C++: no HIP header, compiles with g++ -ffp-contract=off (tools/sanitize/fit_sparse_fuzz.cpp).
// The marking twin, rto_fit_grad_rays_touched_host, is host/fit_grad.cpp's.
#pragma once
#include <stdint.h>

#include <string>

#include "rto.h"

namespace rto {

// "" or what is wrong with a call of the list (scratch is the device entry's: with_scratch = false on the host)
std::string fit_check_list_call(const uint32_t* touched, int64_t slots, const uint32_t* list, int64_t list_capacity, const uint64_t* count,
                                const void* scratch, int64_t scratch_bytes, bool with_scratch);
// bytes of scratch the device list needs for a bitmap of `slots` bits; -1: slots out of range
int64_t fit_touched_scratch_bytes(int64_t slots);
// "" or what is wrong with a call of the sparse step
std::string fit_check_step_call(const float* params, const int64_t* grad, const float* m, const float* v, int64_t slots, int row,
                                const uint32_t* list, const uint64_t* count, int64_t list_capacity, const rto_fit_optim* o);

// the set slots in ascending order to list[], their number to count[0]; clear: the bitmap is zeroed
int fit_touched_list_host(uint32_t* touched, int64_t slots, int clear, uint32_t* list, int64_t list_capacity, uint64_t* count,
                          std::string* err);
// the step of rto_fit_optim.h over the listed rows
int fit_step_sparse_host(float* params, int64_t* grad, float* m, float* v, int64_t slots, int row, const uint32_t* list,
                         const uint64_t* count, int64_t list_capacity, const rto_fit_optim* o, std::string* err);

}  // namespace rto
