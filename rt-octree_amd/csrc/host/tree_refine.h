// tree_refine.h -- the tree refiner of include/rto.h "refiner": the arithmetic both implementations share (the candidate test, the
// selection test, the bounds of a result) and the host twin.  The links and levels are the simplifier's: simp_link_target and
// kSimplifyMaxLevels come from host/tree_simplify.h and are not restated.
// Plain C++17, no HIP include: g++ compiles host/tree_refine.cpp alone (tools/sanitize/run_refine.sh); the kernels
// (refine_kernels.hip) include this header for the RTO_MC_HD functions, so both sides run the same statements.
#pragma once
#include <cstdint>
#include <string>

#include "host/tree_simplify.h"
#include "rto.h"

namespace rto {

// Is the leaf slot (c = its child word, key = its key) of a reachable node of level `level` a candidate?
RTO_MC_HD bool refine_candidate(int32_t c, int32_t level, int max_level, uint32_t key, uint32_t key_thresh) {
    return c == 0 && level >= 0 && level + 1 <= max_level && key >= key_thresh;
}

// Is a candidate with `key`, the eq_rank-th (from 0, in slot order) of the candidates whose key equals cut_key, selected?
RTO_MC_HD bool refine_selected(uint32_t key, uint32_t cut_key, uint64_t eq_rank, uint64_t rem) {
    return key > cut_key || (key == cut_key && eq_rank < rem);
}

// a tree of `nodes` nodes of S slots is beyond what the index arithmetic takes
RTO_MC_HD bool refine_too_large(int64_t nodes, int64_t S) { return nodes * S >= ((int64_t)1 << 31); }

// The refusals of the inputs every entry shares (everything but the device checks); an empty string = accepted.
std::string refine_check_inputs(const int32_t* child, const uint32_t* key, int64_t cap, int N, int max_level);
// Those of the pass that writes: data, D and the outputs, which hold `nodes` nodes (slot_src may be null).
std::string refine_check_outputs(const int32_t* child, const uint16_t* data, const uint32_t* key, int64_t cap, int N, int D,
                                 const int32_t* child_out, const uint16_t* data_out, const int32_t* slot_src, int64_t nodes);

// The host twin: the definition followed literally.  Host memory; key, slot_src and stats may be null; child_out == data_out ==
// null counts only.  RTO_OK, or RTO_E_INVALID / RTO_E_FORMAT with *err set.
int tree_refine_host(const int32_t* child, const uint16_t* data, const uint32_t* key, int64_t cap, int N, int D, uint32_t key_thresh,
                     int64_t max_new, int max_level, int32_t* child_out, uint16_t* data_out, int64_t room, int64_t* out_capacity,
                     int32_t* slot_src, rto_refine_stats* stats, std::string* err);

}  // namespace rto
