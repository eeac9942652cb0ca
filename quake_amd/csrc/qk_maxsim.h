// qk_maxsim.h -- what multi-vector search (qk_maxsim.hip) and multi-vector rerank (qk_rerank.hip) share: the score word and the order
// of the records both selections sort by (not part of the C ABI).
#pragma once
#include "qk_facet.h"

namespace {

constexpr unsigned long long MS_EMPTY = ~0ull;
constexpr unsigned long long MS_SIGN = 0x8000000000000000ull;
constexpr int MS_SEL = QK_MAXSIM_MAX_K;  // records the selection sorts in LDS

// the score as an unsigned word that orders as asked (smaller = better): -0 counts as +0, a NaN is 0xFFFFFFFF, the word no number has
__device__ __forceinline__ uint32_t maxsim_score_word(float s, int metric) {
    if (s != s) return 0xFFFFFFFFu;
    uint32_t b = __float_as_uint(s);
    b = b == 0x80000000u ? 0u : b;
    const uint32_t asc = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    return metric == QK_METRIC_IP ? ~asc : asc;
}
__device__ __forceinline__ float maxsim_score_of(uint32_t w, int metric) {
    if (w == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
    const uint32_t asc = metric == QK_METRIC_IP ? ~w : w;
    return __uint_as_float((asc & 0x80000000u) ? (asc ^ 0x80000000u) : ~asc);
}

// a record of the selection: (score word, value ^ sign bit) is the 96-bit order key; m (the matched count, all ones for padding)
// only separates a record from padding that looks like it
struct MKey {
    uint32_t hi;
    unsigned long long lo;
    uint32_t m;
};
__device__ __forceinline__ bool mkey_less(const MKey &a, const MKey &b) {
    if (a.hi != b.hi) return a.hi < b.hi;
    if (a.lo != b.lo) return a.lo < b.lo;
    return a.m < b.m;
}

}  // namespace
