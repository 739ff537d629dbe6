// host/leaf_weights.h -- the host twin of rto_tree_leaf_weights (include/rto.h "leaf weights") and the argument checks both
// entries share.  Plain C++: no HIP header, compiles with g++ -ffp-contract=off (tools/sanitize/leaf_weights_fuzz.cpp).
#pragma once
#include <stdint.h>

#include <string>

#include "rto.h"

namespace rto {

// "" or what is wrong with the cameras / the weights pointer of a call (checked before anything is enqueued or marched)
std::string leaf_weights_check_cams(const rto_camera* cams, int n, const void* weights);

// "" or what is wrong with child[]: a link of the walk from the root outside [1, capacity), or a node reached twice
std::string leaf_weights_check_links(const int32_t* child, int64_t capacity, int64_t N3);

// The march over child[] / data[] with the root-restart float descent, `threads` threads (<= 0: one) over the rows of each
// camera; weights (capacity * N^3 words) is accumulated into with an atomic unsigned max: the result does not depend on
// `threads`.  ndc: {width, height, focal} or nullptr.  RTO_OK, or RTO_E_INVALID / RTO_E_FORMAT with *err set; child[] is
// walked from the root first (every link inside [1, capacity), no node reached twice), so a malformed array is refused and
// never read out of bounds or descended for ever.
int leaf_weights_host(const int32_t* child, const uint16_t* data, int64_t capacity, int N, int data_dim, const float scale[3],
                      const float offset[3], const float* ndc, const rto_camera* cams, int n, const rto_options* opt, int threads,
                      uint32_t* weights, std::string* err);

}  // namespace rto
