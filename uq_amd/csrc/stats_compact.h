// stats_compact.h -- one counter of a uq_stats into the list form (uq_stats_compact): shared by uq_stats_fetch_compact's own kernel
// (stats.hip) and the epilogue launch behind the pack kernel (qname_fused.hip).  out->n is zero before the first counter is looked at.
#pragma once
#include "common.h"

__device__ __forceinline__ void stats_compact_one(const uq_stats* __restrict__ st, uq_stats_compact* __restrict__ out, uint32_t i) {
    if (i == 0) {
        out->len_min = st->len_min; out->len_max = st->len_max; out->max_record_bytes = st->max_record_bytes; out->reserved = st->reserved;
        out->bad_plus = st->bad_plus; out->bad_len = st->bad_len;
    }
    if (i >= 65536) return;
    const uint64_t c = st->counts[i];
    if (c) {
        const uint32_t k = atomicAdd(&out->n, 1u);
        if (k < UQ_STATS_COMPACT_CAP) { out->key[k] = i; out->count[k] = c; }
    }
}
