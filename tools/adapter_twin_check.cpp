// adapter_twin_check.cpp -- the adapter step's host twins (uq_adapter_report_init_host, uq_adapter_mark_host) in a
// stand-alone program, for a run under the host sanitizers.  Needs no GPU and calls none:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         uq_amd/csrc/adapter.hip tools/adapter_twin_check.cpp -o adapter_twin_check && ./adapter_twin_check
// 2 000 random records (empty lines, N, lower case, lines of different lengths among them) and one record of 70 000 bases, every buffer a
// heap block of its exact size; four parameter sets, with FRESH and with given windows, PAIRED, and a slice.  Each result is checked against
// a second, independent statement of the definition and against the report's invariants.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../include/uqhip.h"

void uq_set_error(const char* fmt, ...) {          // (the library's own lives in api.hip, which this program does not link)
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}

static uint64_t rng_state = 0x2026102100000001ull;
static uint32_t rnd(uint32_t n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % n);
}
static int cls(uint8_t c) {
    switch (c | 0x20) { case 'a': return 0; case 'c': return 1; case 'g': return 2; case 't': return 3; case 'n': return 4; default: return 5; }
}
#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

int main() {
    const char* adapter = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCACGTACGTTAGCCTAGGATCCATGGCATGCAAT";      // 64 letters
    std::string text;
    std::vector<uint64_t> ls;
    const char letters[] = "ACGTACGTACGTACGTacgtNn";
    for (int i = 0; i < 2001; ++i) {
        const uint32_t L = i == 1000 ? 70000 : rnd(160);
        std::string s(L, 'A'), u(i % 17 == 3 ? L + 1 + rnd(3) : L, 'I');
        for (auto& c : s) c = letters[rnd(sizeof(letters) - 1)];
        if (L && i % 3 == 0) {                                  // the adapter somewhere, over the end in every other one
            const uint32_t at = i % 6 == 0 ? rnd(L) : L - 1 - rnd(L < 40 ? L : 40), la = 1 + rnd(64);
            for (uint32_t j = 0; j < la && at + j < L; ++j) s[at + j] = adapter[j];
        }
        ls.push_back(text.size()); text += "@r" + std::to_string(i) + "\n";
        ls.push_back(text.size()); text += s + "\n";
        ls.push_back(text.size()); text += "+\n";
        ls.push_back(text.size()); text += u + "\n";
    }
    ls.push_back(text.size());
    const uint64_t n = 2001;
    uint8_t* buf = (uint8_t*)malloc(text.size());               // exact sizes: a read one byte beyond is seen
    memcpy(buf, text.data(), text.size());
    uint64_t* index = (uint64_t*)malloc(ls.size() * 8);
    memcpy(index, ls.data(), ls.size() * 8);

    const struct { uint32_t len1, len2, overlap, err, flags; } sets[4] = {
        {13, 0, 3, 10, UQ_ADAPTER_FRESH}, {33, 20, 1, 30, UQ_ADAPTER_FRESH | UQ_ADAPTER_PAIRED}, {64, 0, 64, 0, 0}, {1, 5, 1, 0, UQ_ADAPTER_PAIRED}};
    for (const auto& set : sets) {
        uq_adapter_params p;
        memset(&p, 0, sizeof p);
        p.len1 = set.len1; p.len2 = set.len2; p.overlap = set.overlap; p.err_pct = set.err; p.flags = set.flags;
        for (uint32_t j = 0; j < p.len1; ++j) p.seq1[j] = (uint8_t)cls(adapter[j]);
        for (uint32_t j = 0; j < p.len2; ++j) p.seq2[j] = (uint8_t)cls(adapter[63 - j]);
        const uint64_t slices[2][2] = {{0, n}, {997, 7}};       // the whole text; a slice with an odd first record around the long read
        for (const auto& sl : slices) {
            const uint64_t first = sl[0], k = sl[1];
            uint32_t* w = (uint32_t*)malloc(k * 8);
            uint32_t* w0 = (uint32_t*)malloc(k * 8);
            for (uint64_t i = 0; i < k; ++i) {                  // windows handed in: a little off both ends
                const uint64_t* q = index + 4 * (first + i);
                const uint32_t Ls = (uint32_t)(q[2] - q[1] - 1), Lu = (uint32_t)(q[4] - q[3] - 1);
                const uint32_t a = Ls == Lu ? (Ls < 2 ? Ls : 2) : 0, b = Ls == Lu ? (Ls - a < 3 ? Ls : Ls - 3) : Ls;
                w0[2 * i] = w[2 * i] = a; w0[2 * i + 1] = w[2 * i + 1] = b;
            }
            uq_adapter_report* rep = (uq_adapter_report*)malloc(sizeof(uq_adapter_report));
            memset(rep, 0xEE, sizeof *rep);
            REQUIRE(uq_adapter_report_init_host(rep) == 0);
            REQUIRE(uq_adapter_mark_host(buf, index, first, k, &p, w, rep) == 0);
            uint64_t cut = 0, in = 0, out = 0;
            for (uint64_t i = 0; i < k; ++i) {
                const uint64_t* q = index + 4 * (first + i);
                const uint32_t Ls = (uint32_t)(q[2] - q[1] - 1), Lu = (uint32_t)(q[4] - q[3] - 1);
                if (Ls != Lu) { REQUIRE(w[2 * i] == 0 && w[2 * i + 1] == Ls); in += Ls; out += Ls; continue; }
                const uint32_t a = (p.flags & UQ_ADAPTER_FRESH) ? 0 : w0[2 * i], b = (p.flags & UQ_ADAPTER_FRESH) ? Ls : w0[2 * i + 1];
                const bool second = (p.flags & UQ_ADAPTER_PAIRED) && ((first + i) & 1);
                const uint8_t* A = second ? p.seq2 : p.seq1;
                const uint32_t La = second ? p.len2 : p.len1;
                uint32_t want = b;
                for (uint32_t pos = a; pos < b; ++pos) {        // the definition once more, every position to the end
                    const uint32_t m = b - pos < La ? b - pos : La;
                    uint32_t bad = 0;
                    for (uint32_t j = 0; j < m; ++j) bad += cls(buf[q[1] + pos + j]) != A[j];
                    if (m >= p.overlap && bad <= m * p.err_pct / 100) { want = pos; break; }
                }
                REQUIRE(w[2 * i] == a && w[2 * i + 1] == want);
                cut += want < b; in += b - a; out += want - a;
            }
            REQUIRE(rep->reads_in == k && rep->reads_cut == cut && rep->reads_cut == rep->full + rep->partial);
            REQUIRE(rep->bases_in == in && rep->bases_out == out && rep->mate2 <= rep->reads_cut && rep->emptied <= rep->reads_cut);
            printf("len %u/%u overlap %u err %u flags %u, records %llu+%llu: %llu cut (%llu full, %llu partial, %llu emptied), %llu unequal\n", p.len1, p.len2,
                   p.overlap, p.err_pct, p.flags, (unsigned long long)first, (unsigned long long)k, (unsigned long long)rep->reads_cut,
                   (unsigned long long)rep->full, (unsigned long long)rep->partial, (unsigned long long)rep->emptied, (unsigned long long)rep->len_mismatch);
            free(rep); free(w); free(w0);
        }
    }
    free(index); free(buf);
    puts("adapter twins: ok");
    return 0;
}
