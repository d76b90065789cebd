// dedup_twin_check.cpp -- the duplicate remover's host twins (uq_dedup_report_init_host, uq_dedup_keys_host, uq_dedup_mark_host; DESIGN.md
// section 32) in a stand-alone program, for a run under the host sanitizers.  Needs no GPU and calls none:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         uq_amd/csrc/dedup.hip tools/dedup_twin_check.cpp -o dedup_twin_check && ./dedup_twin_check
// 2 000 random records (empty lines and copies of earlier records among them) and one line of 70 000 bases, twice, every buffer a heap block of
// its exact size; both units, hash_bits 3 and 64, first and best, a prefix, and a slice.  Each result is checked against a second,
// independent statement of what a duplicate is (a map from the compared text to its first unit) and against the report's invariants.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
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

static uint64_t rng_state = 0x2026102100000002ull;
static uint32_t rnd(uint32_t n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % n);
}
#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

int main() {
    std::string text;
    std::vector<uint64_t> ls;
    std::vector<std::string> seqs;
    const char letters[] = "ACGTACGTACGTacgtNn";
    for (int i = 0; i < 2002; ++i) {
        std::string s;
        if (i == 1000 || i == 1501) { s.assign(70000, 'A'); for (size_t j = 0; j < s.size(); ++j) s[j] = letters[(j * 7 + j / 13) % 16]; }
        else if (i > 20 && (i % 20 == 10 || i % 20 == 11)) s = seqs[i - 10];      // a whole pair once more
        else if (i > 10 && i % 4 == 0) s = seqs[rnd((uint32_t)i)];
        else { s.assign(rnd(160), 'A'); for (auto& c : s) c = letters[rnd(sizeof(letters) - 1)]; }
        seqs.push_back(s);
        std::string u(s.size() + (i % 17 == 3 ? 2 : 0), '!');
        for (auto& c : u) c = (char)(33 + rnd(94));
        ls.push_back(text.size()); text += "@r" + std::to_string(i) + "\n";
        ls.push_back(text.size()); text += s + "\n";
        ls.push_back(text.size()); text += "+\n";
        ls.push_back(text.size()); text += u + "\n";
    }
    ls.push_back(text.size());
    const uint64_t total = 2002;
    uint8_t* buf = (uint8_t*)malloc(text.size());               // exact sizes: a read one byte beyond is seen
    memcpy(buf, text.data(), text.size());
    uint64_t* index = (uint64_t*)malloc(ls.size() * 8);
    memcpy(index, ls.data(), ls.size() * 8);

    const struct { uint32_t unit, prefix, bits, flags; } sets[] = {
        {1, 0, 64, 0}, {1, 0, 3, 0}, {2, 0, 64, UQ_DEDUP_BEST}, {2, 0, 3, 0}, {1, 9, 64, UQ_DEDUP_BEST}, {1, 60000, 64, 0}, {2, 8, 3, UQ_DEDUP_BEST}};
    for (const auto& set : sets) {
        const uint64_t slices[2][2] = {{0, total}, {996, 10}};  // the whole text; a slice around the first long line
        for (const auto& sl : slices) {
            const uint64_t first = sl[0], n = sl[1], units = n / set.unit;
            uq_dedup_params p;
            p.unit = set.unit; p.prefix = set.prefix; p.hash_bits = set.bits; p.flags = set.flags; p.seed = 5;
            uint8_t* keys = (uint8_t*)malloc(units * 16);
            uint8_t* verdict = (uint8_t*)malloc(n);
            uint32_t* perm = (uint32_t*)malloc(units * 4);
            memset(verdict, 0xEE, n);
            uq_dedup_report* rep = (uq_dedup_report*)malloc(sizeof(uq_dedup_report));
            memset(rep, 0xEE, sizeof *rep);
            REQUIRE(uq_dedup_report_init_host(rep) == 0);
            REQUIRE(uq_dedup_keys_host(buf, index, first, n, first, &p, keys, rep) == 0);
            for (uint64_t w = 0; w < units; ++w) perm[w] = (uint32_t)w;
            std::sort(perm, perm + units, [&](uint32_t a, uint32_t b) { return memcmp(keys + 16 * (uint64_t)a, keys + 16 * (uint64_t)b, 16) < 0; });
            REQUIRE(uq_dedup_mark_host(buf, index, first, n, first, &p, keys, perm, verdict, rep) == 0);
            // the plain meaning: a unit whose compared text was seen before is a duplicate of some kept unit
            std::map<std::string, uint64_t> seen;
            uint64_t dups = 0, bases = 0, dup_bases = 0;
            for (uint64_t w = 0; w < units; ++w) {
                std::string c;
                uint64_t mine = 0;
                for (uint32_t m = 0; m < set.unit; ++m) {
                    const std::string& s = seqs[first + w * set.unit + m];
                    c += s.substr(0, set.prefix ? set.prefix : std::string::npos) + "\n";
                    mine += s.size();
                }
                bases += mine;
                REQUIRE(keys[16 * w + 12] == (uint8_t)((first / set.unit + w) >> 24) && keys[16 * w + 15] == (uint8_t)(first / set.unit + w));
                for (uint32_t m = 0; m < set.unit; ++m) REQUIRE(verdict[w * set.unit + m] == verdict[w * set.unit] && verdict[w * set.unit] <= 1);
                const bool dup = verdict[w * set.unit] == 1;
                if (!(set.flags & UQ_DEDUP_BEST) && rep->collisions == 0) REQUIRE(dup == (seen.count(c) != 0));
                if (dup) { REQUIRE(set.flags & UQ_DEDUP_BEST ? true : seen.count(c) != 0); ++dups; dup_bases += mine; }
                seen.emplace(c, w);
            }
            REQUIRE(rep->reads_in == n && rep->units_in == units && rep->bases_in == bases);
            REQUIRE(rep->dup_units == dups && rep->dup_reads == dups * set.unit && rep->dup_bases == dup_bases);
            REQUIRE(rep->classes + rep->dup_units == units);
            if (rep->collisions == 0) REQUIRE(rep->classes == seen.size());
            else REQUIRE(rep->classes > seen.size() - 1 && set.bits == 3);
            if (set.bits == 64) REQUIRE(rep->collisions == 0);
            printf("unit %u prefix %u bits %u flags %u, records %llu+%llu: %llu classes, %llu duplicate units, %llu collisions\n", set.unit, set.prefix,
                   set.bits, set.flags, (unsigned long long)first, (unsigned long long)n, (unsigned long long)rep->classes,
                   (unsigned long long)rep->dup_units, (unsigned long long)rep->collisions);
            free(rep); free(perm); free(verdict); free(keys);
        }
    }
    free(index); free(buf);
    puts("dedup twins: ok");
    return 0;
}
