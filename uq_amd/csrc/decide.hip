// decide.hip -- the host decisions between the passes, as plain host C++ inside the library (no kernel, no context).
// The encode step ends on the host: the statistics and the fused QNAME structure arrive, and the alphabets / N-trick / bit widths
// (uq.py:448-545), the pack tables and the QNAME column types (uq.py:586-678) are decided from a few hundred numbers while the
// device waits for the next step.  In numpy that is 65 + 24 + 40 us of array set-up per step; here it is a few microseconds.
// Each function has a Python twin that the tests hold it to: analysis.decide_from_pairs_py, ops.make_pack_params_py,
// ops.same_pack_params_py, qname_device.fused_columns_py.
#include <algorithm>
#include "common.h"

namespace {
// the width ladder of uq.py:497-503 / 534-540
int bits_for(uint32_t n_symbols, bool pad) {
    if (n_symbols <= 4) return 2;
    if (n_symbols <= 8 && !pad) return 3;
    if (n_symbols <= 16) return 4;
    if (n_symbols <= 32 && !pad) return 5;
    if (n_symbols <= 64 && !pad) return 6;
    if (n_symbols <= 128 && !pad) return 7;
    return 8;
}

// qname._LADDER: the narrowest unsigned type that holds x -> (its limit, its bytes)
void ladder(uint64_t x, uint64_t& lim, uint32_t& itemsize) {
    if (x <= 255u) { lim = 255u; itemsize = 1; }
    else if (x <= 65535u) { lim = 65535u; itemsize = 2; }
    else if (x <= 4294967295ull) { lim = 4294967295ull; itemsize = 4; }
    else { lim = ~0ull; itemsize = 8; }
}
}  // namespace

extern "C" int uq_decide_from_stats(const uq_stats_compact* h_compact, const uint64_t* h_dense, uint32_t len_min, uint32_t len_max, int notricks,
                                    int pad, const uint64_t* h_first_seen, uq_decisions* h_out) {
    UQ_REQUIRE(h_out && (h_compact || h_dense), "uq_decide_from_stats: null argument");
    UQ_REQUIRE(!h_compact || h_compact->n <= UQ_STATS_COMPACT_CAP, "uq_decide_from_stats: the compact list was cut short (%u counters): pass the dense table",
               h_compact ? h_compact->n : 0u);
    uq_decisions& d = *h_out;
    memset(&d, 0, sizeof(d));
    // per base: the distinct qualities it occurs with, and the last such (quality, count) -- the only one where it matters
    uint32_t nq[256], one_q[256];
    uint64_t one_c[256];
    memset(nq, 0, sizeof(nq)); memset(one_q, 0, sizeof(one_q)); memset(one_c, 0, sizeof(one_c));
    auto take = [&](uint32_t key, uint64_t c) {
        if (c == 0) return;
        const uint32_t b = (key >> 8) & 255u, q = key & 255u;
        d.base_tot[b] += c; d.qual_tot[q] += c;
        nq[b] += 1; one_q[b] = q; one_c[b] = c;
    };
    if (h_compact) for (uint32_t i = 0; i < h_compact->n; ++i) take(h_compact->key[i], h_compact->count[i]);
    else for (uint32_t k = 0; k < 65536u; ++k) take(k, h_dense[k]);
    uint32_t qindex[256];                                        // quals.index(q)
    for (uint32_t x = 0; x < 256; ++x) {
        if (d.base_tot[x]) { d.all_bases[d.nall++] = (uint8_t)x; }
        if (d.qual_tot[x]) { qindex[x] = d.nquals; d.qualities[d.nquals++] = (uint8_t)x; }
    }
    if (d.nall == 0) { d.status = 1; return 0; }                 // no bases counted
    bool gone[256];
    memset(gone, 0, sizeof(gone));
    uint32_t left = d.nall;
    d.total_quals = (int32_t)d.nquals;
    if (!notricks) {                                             // uq.py:479-494
        uint8_t cand[256];
        uint32_t ncand = 0;
        for (uint32_t i = 0; i < d.nall; ++i) if (nq[d.all_bases[i]] == 1) cand[ncand++] = d.all_bases[i];
        d.ncand = ncand;
        if (ncand > 1 && h_first_seen)                           // the reference's dict order: first appearance (uq.py:480)
            std::stable_sort(cand, cand + ncand, [&](uint8_t a, uint8_t b) { return h_first_seen[a] < h_first_seen[b]; });
        for (uint32_t i = 0; i < ncand; ++i) {
            const uint8_t x = cand[i];
            if (left == 1) continue;
            gone[x] = true; --left;
            d.nq_base[d.nnq] = x;
            if (one_c[x] == d.qual_tot[one_q[x]]) d.nq_code[d.nnq] = (int32_t)qindex[one_q[x]];
            else { d.total_quals += 1; d.nq_code[d.nnq] = d.total_quals; }      // replicated
            ++d.nnq;
        }
    }
    for (uint32_t i = 0; i < d.nall; ++i) if (!gone[d.all_bases[i]]) d.bases[d.nbases++] = d.all_bases[i];
    d.bits_per_base = bits_for(d.nbases, pad != 0);
    d.bits_per_quality = bits_for((uint32_t)d.total_quals, pad != 0);
    d.variable = len_min != len_max;                             // uq.py:512-513
    const int64_t lv = (int64_t)len_max + (d.variable ? 1 : 0);
    d.dna_max = (int32_t)len_max; d.dna_min = (int32_t)len_min;
    d.dna_bytes_per_row = (int32_t)((d.bits_per_base * lv + 7) / 8);
    d.quality_bytes_per_row = (int32_t)((d.bits_per_quality * lv + 7) / 8);
    return 0;
}

extern "C" int uq_make_pack_params(const uint8_t* bases, uint32_t nbases, const uint8_t* qualities, uint32_t nquals, const uint8_t* nq_base,
                                   const int32_t* nq_code, uint32_t nnq, int32_t bits_per_base, int32_t bits_per_quality, int32_t variable,
                                   int32_t dna_bytes_per_row, int32_t quality_bytes_per_row, int32_t dna_max, int32_t max_record_bytes,
                                   int32_t avg_record_bytes, uq_pack_params* h_out) {
    UQ_REQUIRE(h_out && (bases || !nbases) && (qualities || !nquals) && ((nq_base && nq_code) || !nnq), "uq_make_pack_params: null argument");
    UQ_REQUIRE(nbases <= 32767u && nquals <= 32767u, "uq_make_pack_params: more symbols than a 16-bit code holds");
    uq_pack_params& p = *h_out;
    for (int i = 0; i < 256; ++i) { p.dna_code[i] = -1; p.qual_code[i] = -1; p.n_qual[i] = -1; }
    for (uint32_t i = 0; i < nbases; ++i) p.dna_code[bases[i]] = (int16_t)i;
    for (uint32_t i = 0; i < nquals; ++i) p.qual_code[qualities[i]] = (int16_t)i;
    for (uint32_t i = 0; i < nnq; ++i) p.n_qual[nq_base[i]] = nq_code[i];
    p.bits_per_base = bits_per_base; p.bits_per_quality = bits_per_quality; p.variable = variable ? 1 : 0;
    p.dna_bytes_per_row = dna_bytes_per_row; p.quality_bytes_per_row = quality_bytes_per_row;
    p.max_record_bytes = max_record_bytes; p.dna_max = dna_max; p.avg_record_bytes = avg_record_bytes;
    return 0;
}

extern "C" int uq_same_pack_params(const uq_pack_params* a, const uq_pack_params* b, int* h_same) {
    UQ_REQUIRE(a && b && h_same, "uq_same_pack_params: null argument");
    *h_same = a->bits_per_base == b->bits_per_base && a->bits_per_quality == b->bits_per_quality && a->variable == b->variable &&
              a->dna_bytes_per_row == b->dna_bytes_per_row && a->quality_bytes_per_row == b->quality_bytes_per_row && a->dna_max == b->dna_max &&
              memcmp(a->dna_code, b->dna_code, sizeof(a->dna_code)) == 0 && memcmp(a->qual_code, b->qual_code, sizeof(a->qual_code)) == 0 &&
              memcmp(a->n_qual, b->n_qual, sizeof(a->n_qual)) == 0;
    return 0;
}

extern "C" int uq_qname_fused_columns(const uq_qname_fused* h_q, uint64_t n, uq_qname_columns* h_out) {
    UQ_REQUIRE(h_q && h_out, "uq_qname_fused_columns: null argument");
    constexpr int64_t INT_RANGE_SMALL = 4096;                    // qname_device.INT_RANGE_SMALL
    constexpr uint64_t INT_PREFIX = 1ull << 21;                  // qname_device.INT_PREFIX
    const uq_qname_fused& r = *h_q;
    uq_qname_columns& o = *h_out;
    memset(&o, 0, sizeof(o));
    o.status = 1;
    if (!r.ok || r.flags || n == 0 || r.nreads != n || r.nsep >= UQ_QF_MAXC) return 0;
    // the reads after which the reference re-examines its formats (uq.py:586-602: 10 000, 20 000, 40 000, ...) and the last one
    uint64_t th[64];
    uint32_t nth = 0;
    for (uint64_t t = 10000; t <= n - 1 && nth < 62; t *= 2) th[nth++] = t;
    if (nth == 0 || th[nth - 1] != n - 1) th[nth++] = n - 1;
    if (r.nth != nth || nth > UQ_QF_MAXT) return 0;
    for (uint32_t k = 0; k < nth; ++k) if (r.thresholds[k] != th[k]) return 0;
    uint32_t nhead = 0;
    while (nhead < nth && th[nhead] < INT_PREFIX) ++nhead;
    for (uint32_t c = 0; c <= r.nsep; ++c) {
        const int64_t vmin = r.vmin[c], vmax = r.vmax[c];
        // distinct strings = distinct values, counted per checkpoint: over the whole column for small ranges, else over the checkpoints
        // below INT_PREFIX, where the `len(map) > entries_read / 10` rule fires at once or the values have to be sorted
        uint32_t ncnt = 0;
        bool have = false, have_nu = false;
        if (!r.undetermined[c] && vmax - vmin + 1 <= INT_RANGE_SMALL) { ncnt = nth; have = have_nu = true; }
        else if (!r.undetermined[c]) {
            ncnt = nhead;
            bool fired = false;
            for (uint32_t k = 0; k < ncnt; ++k) fired = fired || r.counts[c][k] > th[k] / 10;
            if (fired) have = true;
            else if (nhead == nth) have = have_nu = true;
        }
        if (!have) { o.status = 2; return 0; }
        bool integers = false;
        for (uint32_t k = 0; k < ncnt; ++k) if (r.counts[c][k] > th[k] / 10) { integers = true; break; }   // check_format(): mapping -> integers
        uint64_t lim;
        uint32_t isz;
        if (!integers) {
            if (!have_nu) { o.status = 2; return 0; }            // (cannot happen: without a count of the whole column a checkpoint fired)
            ladder(r.counts[c][ncnt - 1], lim, isz);
            if (vmax - vmin > 0 && (uint64_t)(vmax - vmin) > lim) { o.status = 1; return 0; }      // stays a mapping: the exact path's sorted map
            o.from_mapping[c] = 1;
        } else {
            ladder(vmax - vmin > 0 ? (uint64_t)(vmax - vmin) : 0u, lim, isz);
        }
        o.itemsize[c] = isz; o.offset[c] = (uint64_t)vmax > lim ? 1u : 0u;
        o.vmin[c] = (uint32_t)vmin; o.vmax[c] = (uint32_t)vmax;
    }
    o.ncols = r.nsep + 1;
    o.status = 0;
    return 0;
}
