// host/fit_sparse.cpp -- the host twins of rto_fit_touched_list and rto_fit_step_sparse: the list by a walk over the words, the
// step by rto_fit_optim.h, the text the kernel compiles too.  Same bits as the kernels (tests/test_fit_sparse_gpu.py) and as the
// numpy restatement (tests/fit_sparse_ref.py).  No HIP header.
#include "fit_sparse.h"

#include "../rto_fit_optim.h"

namespace rto {

namespace {

constexpr int64_t kMaxSlots = ((int64_t)1 << 31) - 1;
constexpr int64_t kBlockWords = RTO_FIT_TOUCHED_BLOCK_WORDS;

}  // namespace

int64_t fit_touched_scratch_bytes(int64_t slots) {
    if (slots < 0 || slots > kMaxSlots) return -1;
    const int64_t blocks = (fo::touched_words(slots) + kBlockWords - 1) / kBlockWords;
    return (blocks > 0 ? blocks : 1) * 4;
}

std::string fit_check_list_call(const uint32_t* touched, int64_t slots, const uint32_t* list, int64_t list_capacity, const uint64_t* count,
                                const void* scratch, int64_t scratch_bytes, bool with_scratch) {
    if (!touched) return "null touched";
    if (!count) return "null count";
    if (slots < 0 || slots > kMaxSlots) return "slots must be in [0, 2^31)";
    if (list_capacity < 0) return "list_capacity must be >= 0";
    if (!list && list_capacity > 0) return "null list with list_capacity > 0";
    if ((uintptr_t)touched % 4 != 0) return "touched must be 4-byte aligned";
    if ((uintptr_t)list % 4 != 0) return "list must be 4-byte aligned";
    if ((uintptr_t)count % 8 != 0) return "count must be 8-byte aligned";
    if (with_scratch) {
        if (!scratch) return "null scratch";
        if ((uintptr_t)scratch % 4 != 0) return "scratch must be 4-byte aligned";
        if (scratch_bytes < fit_touched_scratch_bytes(slots)) return "scratch_bytes is below rto_fit_touched_scratch_bytes(slots)";
    }
    return "";
}

std::string fit_check_step_call(const float* params, const int64_t* grad, const float* m, const float* v, int64_t slots, int row,
                                const uint32_t* list, const uint64_t* count, int64_t list_capacity, const rto_fit_optim* o) {
    if (!params) return "null params";
    if (!grad) return "null grad";
    if (!list) return "null list";
    if (!count) return "null count";
    if (!o) return "null options";
    if (row < 1) return "row must be >= 1";
    if (slots < 0 || slots > kMaxSlots) return "slots must be in [0, 2^31)";
    if (list_capacity < 0) return "list_capacity must be >= 0";
    if (o->kind != RTO_FIT_SGD && o->kind != RTO_FIT_RMSPROP && o->kind != RTO_FIT_ADAM)
        return "unknown kind " + std::to_string(o->kind) + " (RTO_FIT_SGD, RTO_FIT_RMSPROP or RTO_FIT_ADAM)";
    if (o->kind == RTO_FIT_ADAM && !m) return "null m: RTO_FIT_ADAM keeps a first moment";
    if (o->kind != RTO_FIT_SGD && !v) return "null v: RTO_FIT_RMSPROP and RTO_FIT_ADAM keep a second moment";
    if ((uintptr_t)params % 4 != 0) return "params must be 4-byte aligned";
    if ((uintptr_t)grad % 8 != 0) return "grad must be 8-byte aligned";
    if (o->kind == RTO_FIT_ADAM && (uintptr_t)m % 4 != 0) return "m must be 4-byte aligned";
    if (o->kind != RTO_FIT_SGD && (uintptr_t)v % 4 != 0) return "v must be 4-byte aligned";
    if ((uintptr_t)list % 4 != 0) return "list must be 4-byte aligned";
    if ((uintptr_t)count % 8 != 0) return "count must be 8-byte aligned";
    return "";
}

int fit_touched_list_host(uint32_t* touched, int64_t slots, int clear, uint32_t* list, int64_t list_capacity, uint64_t* count,
                          std::string* err) {
    const std::string bad = fit_check_list_call(touched, slots, list, list_capacity, count, nullptr, 0, false);
    if (!bad.empty()) {
        if (err) *err = bad;
        return RTO_E_INVALID;
    }
    const int64_t words = fo::touched_words(slots);
    int64_t pos = 0;
    for (int64_t w = 0; w < words; ++w) {
        uint32_t b = touched[w] & fo::touched_valid_mask(w, slots);
        while (b != 0u) {
            const int lo = __builtin_ctz(b);
            if (pos < list_capacity) list[pos] = (uint32_t)((w << 5) + lo);
            ++pos;
            b &= b - 1u;
        }
        if (clear) touched[w] = 0u;
    }
    count[0] = (uint64_t)pos;
    return RTO_OK;
}

namespace {

template <int KIND>
void step_rows(float* params, int64_t* grad, float* m, float* v, int64_t slots, int row, const uint32_t* list, int64_t rows,
               const rto_fit_optim& o) {
    for (int64_t j = 0; j < rows; ++j) {
        const uint32_t s = list[j];
        if ((int64_t)s >= slots) continue;
        for (int k = 0; k < row; ++k) {
            const int64_t i = (int64_t)s * row + k;
            float mm = 0.f, vv = 0.f;
            if (KIND == RTO_FIT_ADAM) mm = m[i];
            if (KIND != RTO_FIT_SGD) vv = v[i];
            fo::step<KIND>(o, grad[i], params[i], mm, vv);
            grad[i] = 0;
            if (KIND == RTO_FIT_ADAM) m[i] = mm;
            if (KIND != RTO_FIT_SGD) v[i] = vv;
        }
    }
}

}  // namespace

int fit_step_sparse_host(float* params, int64_t* grad, float* m, float* v, int64_t slots, int row, const uint32_t* list,
                         const uint64_t* count, int64_t list_capacity, const rto_fit_optim* o, std::string* err) {
    const std::string bad = fit_check_step_call(params, grad, m, v, slots, row, list, count, list_capacity, o);
    if (!bad.empty()) {
        if (err) *err = bad;
        return RTO_E_INVALID;
    }
    const int64_t rows = count[0] < (uint64_t)list_capacity ? (int64_t)count[0] : list_capacity;
    if (o->kind == RTO_FIT_SGD) step_rows<RTO_FIT_SGD>(params, grad, m, v, slots, row, list, rows, *o);
    if (o->kind == RTO_FIT_RMSPROP) step_rows<RTO_FIT_RMSPROP>(params, grad, m, v, slots, row, list, rows, *o);
    if (o->kind == RTO_FIT_ADAM) step_rows<RTO_FIT_ADAM>(params, grad, m, v, slots, row, list, rows, *o);
    return RTO_OK;
}

}  // namespace rto
