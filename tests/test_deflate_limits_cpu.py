"""The deflate compressor's code builder past its length limits, on the CPU.

uq_def_huffman (deflate_core.h) rebuilds a tree that came out deeper than the format allows (15 bits, 7 for the code-length code) with
its small weights raised to t = 2, 4, 8, ...  The blocks of deflate_limit_inputs.py reach that loop through ops.bgzf_block_host, at
both levels; here every member is read back by the plain reader of deflate_reader.py, and from what the reader saw:

  the path is taken   the unconstrained Huffman tree (the compressor's own tie rule) over the histogram of the named alphabet is deeper
                      than its limit -- for every named block, none skipped
  the code is sound   lengths within the limit, Kraft's sum exactly complete, HLIT / HDIST / HCLEN trimmed as far as the format allows
  its cost            at least the optimum of a length-limited code (package-merge); the excess is printed, and DESIGN.md records it.
                      It is not capped: the clamp is a heuristic, and what it costs is a measurement
  the sizer           ops.deflate_size_host gives the member's length

and the header-shape blocks show the 16 / 17 / 18 runs, HDIST and the run across the two codes that each was built for.  A g++ driver
with its own main calls uq_def_huffman and uq_def_codes under AddressSanitizer / UBSan on histograms no block gives: all three real
configurations, (286, 15), (30, 15) and (19, 7).

Run as a script, it prints the table of the excess that DESIGN.md holds.
"""
import functools
import os
import random
import struct
import subprocess
import sys

import pytest

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import deflate_reader as R
from deflate_limit_inputs import LIMIT_OF, fib, header_blocks, limit_blocks
from deflate_writer import ORDER, canonical_codes, distance_symbol
from test_deflate_cpu import BLOCK, CORE, _gxx, member_ok
from uq_amd import ops

LEVELS = (1, 2)
ALPHABETS = {'lit': (286, 15), 'dist': (30, 15), 'clen': (19, 7)}


@functools.lru_cache(maxsize=None)
def analysed(name, level):
    """(member, the reader's one block, {alphabet: (histogram, lengths as written)}) of a named block at a level"""
    block = dict(limit_blocks() + header_blocks())[name]
    m = ops.bgzf_block_host(block, level=level)
    data, blocks = R.read_member(m)
    assert data == block and len(blocks) == 1 and blocks[0]['final'], name
    blk = blocks[0]
    codes = {}
    if blk['btype'] == 2:
        lf, df = R.histograms(blk)
        codes = {'lit': (lf, blk['llens'] + [0] * (286 - blk['hlit'])), 'dist': (df, blk['dlens'] + [0] * (30 - blk['hdist'])),
                 'clen': (R.codelen_histogram(blk), blk['clens'])}
    return m, blk, codes


def check_code(freq, lens, limit, what):
    """The soundness of one written code and its cost against the optimum; returns (cost, optimum)."""
    m = sum(1 for f in freq if f)
    assert len(lens) == len(freq) and max(lens) <= limit, what
    assert all(l for f, l in zip(freq, lens) if f), '%s: a symbol in use has no code' % what
    assert R.kraft_units(lens, limit) == 1 << limit, '%s: Kraft sum %d / %d' % (what, R.kraft_units(lens, limit), 1 << limit)
    if m < 2:                                               # two codes of one bit: the symbol in use (or 0) and 0 or 1
        a = [s for s, f in enumerate(freq) if f][0] if m else 0
        assert [s for s, l in enumerate(lens) if l] == sorted([a, 1 if a == 0 else 0]), what
    cost, best = R.code_cost(freq, lens), R.package_merge_cost(freq, limit)
    assert cost >= best, what
    if R.unlimited_depth(freq) <= limit:                    # no clamp: the code is Huffman's, and optimal
        assert cost == best, '%s: %d bits where an unconstrained Huffman code takes %d' % (what, cost, best)
    return cost, best


def _names(blocks): return [n for n, _ in blocks()]


# ------------------------------------------------------------------ the blocks
@pytest.mark.parametrize('level', LEVELS)
def test_members_inflate_and_the_sizer_agrees(level):
    for name, block in limit_blocks() + header_blocks():
        m, blk, _ = analysed(name, level)
        member_ok(m, block)
        assert ops.deflate_size_host(block, level=level) == (len(m) if block else 0), name
        assert ops.deflate_size_host(block[3:], prefix=block[:3], level=level) == (len(m) if block else 0), name


def test_named_block_sizes():
    """Two blocks and more per limit, one of exactly 65 280 bytes (it can sit in the middle of a stream) and a shorter one."""
    for kind in LIMIT_OF:
        sizes = [len(b) for n, b in limit_blocks() if n.startswith(kind + '/')]
        assert len(sizes) >= 2 and BLOCK in sizes and min(sizes) < BLOCK, kind
    assert all(len(b) <= 4000 for _, b in header_blocks())


@pytest.mark.parametrize('level', LEVELS)
def test_the_rebuild_path_is_taken(level):
    """A condition on every named block: when a change to the matcher breaks it, the block's recipe has to be searched again."""
    twice = 0
    for name in _names(limit_blocks):
        alphabet, limit = LIMIT_OF[name.split('/')[0]]
        _, blk, codes = analysed(name, level)
        assert blk['btype'] == 2, name
        freq, lens = codes[alphabet]
        depth = R.unlimited_depth(freq)
        print('%s level %d: unconstrained %s depth %d, written maximum %d' % (name, level, alphabet, depth, max(lens)))
        assert depth > limit, '%s no longer reaches the %d-bit limit of its %s code at level %d (unconstrained depth %d): search the ' \
                              'recipe of deflate_limit_inputs.py again' % (name, limit, alphabet, level, depth)
        twice += R.unlimited_depth([max(f, 2) if f else 0 for f in freq]) > limit
    assert twice >= 2                                       # and some blocks need t = 4: the loop goes round more than once


@pytest.mark.parametrize('level', LEVELS)
def test_written_codes_are_sound_and_cost_at_least_the_optimum(level):
    for name in _names(limit_blocks) + _names(header_blocks):
        _, blk, codes = analysed(name, level)
        if blk['btype'] != 2:
            assert name in ('hdr/empty', 'hdr/one_byte'), name
            continue
        for alphabet, (freq, lens) in codes.items():
            cost, best = check_code(freq, lens, ALPHABETS[alphabet][1], '%s level %d %s' % (name, level, alphabet))
            if cost != best: print('%s level %d %s: %d bits, optimum %d, excess %d' % (name, level, alphabet, cost, best, cost - best))
        # trimmed as far as the format allows
        lf, df = codes['lit'][0], codes['dist'][0]
        llens, dlens, clens = codes['lit'][1], codes['dist'][1], codes['clen'][1]
        assert blk['hlit'] == max(257, max(s for s, l in enumerate(llens) if l) + 1), name
        assert blk['hdist'] == max(1, max(s for s, l in enumerate(dlens) if l) + 1), name
        assert blk['hclen'] == max(4, max(k for k in range(19) if clens[ORDER[k]]) + 1), name
        assert blk['clens_written'] == [clens[ORDER[k]] for k in range(blk['hclen'])], name


@pytest.mark.parametrize('level', LEVELS)
def test_header_shapes(level):
    def spans(name):
        m, blk, codes = analysed(name, level)
        assert blk['btype'] == 2, name
        return blk, codes, [(s, ex, n) for s, ex, _, n in R.run_spans(blk)], R.run_spans(blk)

    for name in ('hdr/empty', 'hdr/one_byte'):              # smaller stored than with any header
        m, blk, _ = analysed(name, level)
        assert blk['btype'] == 0 and len(m) == 18 + 5 + len(blk['stored']) + 8
    # literals 0x00 and 0xFF only: the 254 zero lengths between them are one 18 of 138 and one of 116
    blk, codes, sp, _ = spans('hdr/only_00_ff')
    assert sp[0][0] > 0 and sp[1:3] == [(18, 127, 138), (18, 105, 116)] and sp[3][0] > 0
    assert [s for s, f in enumerate(codes['lit'][0][:256]) if f] == [0, 255]
    # no match: a distance code of two 1-bit codes, HDIST written as 1
    blk, codes, sp, _ = spans('hdr/no_match')
    assert not any(isinstance(t, tuple) for t in blk['tokens']) and blk['hdist'] - 1 == 1 and blk['dlens'] == [1, 1]
    # one distance symbol in use: one bit for it and one for symbol 0
    blk, codes, sp, _ = spans('hdr/one_distance_symbol')
    used = {distance_symbol(t[1])[0] for t in blk['tokens'] if isinstance(t, tuple)}
    assert len(used) == 1 and min(used) > 1
    assert [s for s, l in enumerate(blk['dlens']) if l] == [0, min(used)] and blk['dlens'][0] == 1 == blk['dlens'][-1]
    # a repeat (16) that starts in the literal/length lengths and ends in the distance lengths
    blk, codes, sp, full = spans('hdr/run_crosses_hlit')
    cross = [(s, i, n) for s, _, i, n in full if i < blk['hlit'] < i + n]
    assert len(cross) == 1 and cross[0][0] == 16 and blk['llens'][-1] == blk['dlens'][0] != 0
    # zero runs of exactly 10 and 11: 17 with its last extra value, 18 with its first
    blk, codes, sp, _ = spans('hdr/zero_runs_10_11')
    assert (17, 7, 10) in sp and (18, 0, 11) in sp
    assert sp[sp.index((17, 7, 10)) + 1][0] not in (0, 17, 18) and sp[sp.index((18, 0, 11)) + 1][0] not in (0, 17, 18)
    # 6, 7 and 8 equal lengths in a row: the length, then 16 x 5; 16 x 6 (all it holds); 16 x 6 and the length again
    blk, codes, sp, _ = spans('hdr/repeats_6_7_8')
    runs = {}
    for s in (0x30, 0x41, 0x61):
        k = [i for i, (_, _, at, _) in enumerate(R.run_spans(blk)) if at == s][0]
        runs[s] = sp[k:k + 4]
    l6, l8, l7 = blk['llens'][0x30], blk['llens'][0x41], blk['llens'][0x61]
    assert runs[0x30][:2] == [(l6, 0, 1), (16, 2, 5)] and runs[0x30][2][0] == 18
    assert runs[0x61][:2] == [(l7, 0, 1), (16, 3, 6)] and runs[0x61][2][0] == 18
    assert runs[0x41][:3] == [(l8, 0, 1), (16, 3, 6), (l8, 0, 1)] and runs[0x41][3][0] == 18


# ------------------------------------------------------------------ uq_def_huffman and uq_def_codes themselves, under the sanitizers
DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "deflate_core.h"

struct Env { void sync() {} };

int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    uint32_t hdr[2];
    while (fread(hdr, 4, 2, f) == 2) {
        const uint32_t n = hdr[0], limit = hdr[1];
        uint32_t* freq = (uint32_t*)malloc(4 * n);                  // exactly n of each: a step past them is a report
        uint8_t* lens = (uint8_t*)malloc(n);
        uint8_t* deep = (uint8_t*)malloc(n);
        uint16_t* codes = (uint16_t*)malloc(2 * n);
        if (fread(freq, 4, n, f) != n) return 3;
        UqDefHuffScratch* h = (UqDefHuffScratch*)malloc(sizeof(UqDefHuffScratch));
        Env env;
        memset(h, 0xA5, sizeof(*h)); memset(lens, 0xA5, n);
        uq_def_huffman(env, freq, n, limit, lens, h, 0, 1);
        uq_def_codes(lens, n, codes);
        memset(h, 0x5A, sizeof(*h)); memset(deep, 0x5A, n);
        uq_def_huffman(env, freq, n, 255, deep, h, 0, 1);           // no limit to speak of: the tree of the first pass
        fwrite(lens, 1, n, g); fwrite(codes, 2, n, g); fwrite(deep, 1, n, g);
        free(freq); free(lens); free(deep); free(codes); free(h);
    }
    fclose(f); fclose(g);
    return 0;
}
'''


def driver_histograms():
    """[(what, n, limit, weights)] for the three configurations the compressor uses"""
    rnd = random.Random(20261019)
    out = []
    for n, limit in ALPHABETS.values():
        def add(what, w, spread=True):
            w = list(w)[:n]
            out.append((what, n, limit, w + [0] * (n - len(w))))
            if spread and len(w) < n:                       # the same weights on other symbols, the last one among them
                at = sorted(rnd.sample(range(n - 1), len(w) - 1) + [n - 1]) if w else []
                v = [0] * n
                for s, x in zip(at, rnd.sample(w, len(w))): v[s] = x
                out.append((what + ' spread', n, limit, v))
        for k in sorted({limit + 1, limit + 2, limit + 3, limit + 6, min(n, 30), min(n, 44)}):
            if k <= n: add('fibonacci %d' % k, fib(k))
        for k in sorted({limit + 1, limit + 2, limit + 5, min(n, 24), min(n, 31)}):
            if k <= n: add('powers of two %d' % k, [1 << i for i in range(k)])
        add('one huge weight among ones', [1] * (n - 1) + [65281])
        add('one huge weight first', [65281] + [1] * (n - 1))
        add('all equal', [7] * n)
        add('all ones', [1] * n)
        add('nothing', [])
        for s in (0, 1, n - 1):
            v = [0] * n; v[s] = 5
            add('one symbol %d' % s, v, spread=False)
        for a, b in ((0, 1), (0, n - 1), (n - 2, n - 1), (3, 4)):
            v = [0] * n; v[a] = 1; v[b] = 65280
            add('two symbols %d %d' % (a, b), v, spread=False)
        add('ties: pairs of powers of two', [1 << (i // 2) for i in range(min(n, 40))])
        add('ties: ones and twos', [1 + i % 2 for i in range(n)])
        add('ties: one two three', [1 + i % 3 for i in range(n)])
        add('ties: fibonacci twice', sorted(fib(min(n // 2, 22)) * 2))
        add('ties: sums of the ones below', [1, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536][:n])
        for i in range(40):
            k = rnd.randrange(2, n + 1)
            add('random %d' % i, [rnd.choice([1, 1, 2, 3, rnd.randrange(1, 50), rnd.randrange(1, 65281)]) for _ in range(k)])
    return out


def test_code_builder_under_address_sanitizer(tmp_path):
    gxx = _gxx()
    if gxx is None:
        pytest.skip('no host C++ compiler')
    (tmp_path / 'drv.cpp').write_text(DRIVER)
    exe = tmp_path / 'drv'
    subprocess.check_call([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                           os.path.dirname(CORE), str(tmp_path / 'drv.cpp'), '-o', str(exe)])
    cases = driver_histograms()
    with open(tmp_path / 'cases.bin', 'wb') as f:
        for _, n, limit, w in cases: f.write(struct.pack('<II%dI' % n, n, limit, *w))
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:exitcode=99', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1:exitcode=98')
    r = subprocess.run([str(exe), str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, env=env, timeout=600)
    assert r.returncode == 0 and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]
    out = (tmp_path / 'out.bin').read_bytes()
    at, limited = 0, {}
    for what, n, limit, w in cases:
        what = '%s (%d, %d)' % (what, n, limit)
        lens = list(out[at:at + n]); codes = struct.unpack('<%dH' % n, out[at + n:at + 3 * n]); deep = list(out[at + 3 * n:at + 4 * n])
        at += 4 * n
        cost, best = check_code(w, lens, limit, what)
        want = R.huffman_depths(w)
        if len(want) >= 2:                                  # the reference's tie rule is the compressor's
            assert deep == [want.get(s, 0) for s in range(n)], what
            assert not any(l for f, l in zip(w, lens) if not f), what
        if max(deep) > limit:
            limited[(n, limit)] = limited.get((n, limit), 0) + 1
            print('%s: unconstrained depth %d, written maximum %d, %d bits, optimum %d, excess %d' % (what, max(deep), max(lens), cost, best, cost - best))
        canon = canonical_codes(lens)                       # and the codes are the canonical ones, bit-reversed
        for s in range(n):
            c, l = canon.get(s, (0, 0))
            assert codes[s] == (int(format(c, '0%db' % l)[::-1], 2) if l else 0), what
    assert at == len(out) and all(limited.get(k, 0) >= 10 for k in ALPHABETS.values()), limited


def excess_table():
    """The rows of DESIGN.md's table: per named block and alphabet that reached its limit, the excess over package-merge at each level."""
    rows = []
    for name in _names(limit_blocks) + _names(header_blocks):
        for alphabet, (_, limit) in ALPHABETS.items():
            cells = []
            for level in LEVELS:
                codes = analysed(name, level)[2]
                if not codes or R.unlimited_depth(codes[alphabet][0]) <= limit:
                    cells.append(None)
                    continue
                freq, lens = codes[alphabet]
                cells.append((R.unlimited_depth(freq), max(lens), R.code_cost(freq, lens), R.package_merge_cost(freq, limit)))
            if any(cells): rows.append((name, alphabet, cells))
    return rows


if __name__ == '__main__':
    for name, alphabet, cells in excess_table():
        print('| %s | %s | %s |' % (name, alphabet, ' | '.join(
            '-' if c is None else '%d -> %d, %d bits, optimum %d, +%d (%.3f %%)' % (c[0], c[1], c[2], c[3], c[2] - c[3], 100.0 * (c[2] - c[3]) / c[3])
            for c in cells)))
