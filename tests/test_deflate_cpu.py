"""BGZF output on the CPU: the deflate compressor that the GPU runs (deflate_core.h, through uq_bgzf_compress_block_host and, under
AddressSanitizer, a small g++ driver) checked with zlib / gzip, its compression ratio against zlib on the same blocks, and the CLI's
refusal of --bgzf without --decode."""
import glob
import gzip
import os
import random
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from test_gzip_cpu import BGZF_EOF
from uq_amd import ops, synth, uq

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORE = os.path.join(REPO, 'uq_amd', 'csrc', 'deflate_core.h')
GOLD = os.path.join(REPO, 'tests', 'golden')
BLOCK = 65280


def blocks_of(data):
    return [data[i:i + BLOCK] for i in range(0, len(data), BLOCK)]


def block_matrix():
    """(name, block) pairs: the edge cases, the golden inputs, synthetic reads in full blocks and a short tail block."""
    rnd = random.Random(7)
    r32 = bytes(rnd.getrandbits(8) for _ in range(32768))
    out = [('empty', b''), ('one_byte', b'G'), ('one_byte_run', b'A' * BLOCK), ('two_byte_run', b'AC' * (BLOCK // 2)),
           ('distance_32768', r32 + r32[:BLOCK - 32768]), ('random', bytes(rnd.getrandbits(8) for _ in range(BLOCK))),
           ('random_short', bytes(rnd.getrandbits(8) for _ in range(1000))), ('three_bytes', b'@r\n')]
    for p in sorted(glob.glob(os.path.join(GOLD, '*.fastq'))):
        if p.endswith('.refdecode.fastq'): continue
        for k, b in enumerate(blocks_of(open(p, 'rb').read())[:2]):
            out.append(('golden/%s/%d' % (os.path.basename(p), k), b))
    for name, kw in (('fixed', dict(length=150)), ('variable', dict(length=(36, 301))),
                     ('dup', dict(length=(36, 151), dup='both', dup_templates=40))):
        data = synth.fastq(20261005, 900, kw.pop('length'), **kw)
        bl = blocks_of(data)
        out += [('synth/%s/%d' % (name, k), b) for k, b in enumerate(bl)]
    return out


def member_ok(m, data):
    """One complete BGZF member whose header, BSIZE, CRC-32 and ISIZE are right, inflating to `data`."""
    assert m[:4] == b'\x1f\x8b\x08\x04' and m[10:16] == b'\x06\x00BC\x02\x00'
    assert struct.unpack('<H', m[16:18])[0] == len(m) - 1 <= 65535
    crc, isize = struct.unpack('<II', m[-8:])
    assert crc == zlib.crc32(data) and isize == len(data)
    d = zlib.decompressobj(-15)
    assert d.decompress(m[18:-8]) == data and d.eof and not d.unused_data
    assert gzip.decompress(m) == data


def zlib_bgzf_size(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    total = 0
    for b in blocks_of(data):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        total += 26 + len(c.compress(b) + c.flush())
    return total


def test_host_members_inflate_to_the_input():
    for name, b in block_matrix():
        m = ops.bgzf_block_host(b)
        member_ok(m, b)
        assert len(m) <= min(len(b) + 31, 65536), name


def test_edge_cases_take_the_expected_paths():
    run = ops.bgzf_block_host(b'A' * BLOCK)
    assert len(run) < 1000                                          # long matches: lengths of 258
    rnd = random.Random(3)
    noise = bytes(rnd.getrandbits(8) for _ in range(BLOCK))
    m = ops.bgzf_block_host(noise)
    assert len(m) == 18 + 5 + BLOCK + 8 == 65311 and m[18] == 1 and m[23:23 + BLOCK] == noise      # a stored block
    r32 = noise[:32768]
    rep = ops.bgzf_block_host(r32 + r32[:BLOCK - 32768])
    assert len(rep) < 65311                                         # some of the second half matches (the hash table is 4 096 wide)
    assert len(ops.bgzf_block_host(b'')) == 31


def test_too_large_and_too_small():
    st, size, out = ops.bgzf_block_host(b'x' * (BLOCK + 1), capacity=65536)
    assert st == 2
    data = synth.fastq(11, 300, 100)[:BLOCK]
    m = ops.bgzf_block_host(data)
    st, size, out = ops.bgzf_block_host(data, capacity=len(m))
    assert st == 0 and size == len(m) and out == m
    st, size, out = ops.bgzf_block_host(data, capacity=len(m) - 1)
    assert st == 1 and size == len(m) and out == b'\x00' * (len(m) - 1)


def test_concatenation_scans_as_bgzf():
    data = synth.fastq(20261005, 2000, (36, 301))
    bl = blocks_of(data)
    blob = b''.join(ops.bgzf_block_host(b) for b in bl) + BGZF_EOF
    kind, m, total, err = ops.gzip_scan(np.frombuffer(blob, dtype=np.uint8))
    assert kind == ops.GZIP_BGZF and err is None and total == len(data) and len(m) == len(bl) + 1
    assert gzip.decompress(blob) == data
    for k, b in enumerate(bl):                                      # and the project's own inflate reads every member back
        st, out = ops.inflate_member_host(blob[m[k]['data_offset']:m[k]['data_offset'] + m[k]['comp_bytes']], m[k]['isize'], m[k]['crc32'])
        assert st == 0 and out == b


def test_output_is_deterministic():
    for name, b in block_matrix()[::5]:
        assert ops.bgzf_block_host(b) == ops.bgzf_block_host(bytes(b)), name


@pytest.mark.parametrize('length', [150, (36, 301)], ids=['150bp', '36-301bp'])
def test_ratio_against_zlib(length):
    data = synth.fastq(20261005, 100000, length)
    ours = sum(len(ops.bgzf_block_host(b)) for b in blocks_of(data))
    assert ours <= zlib_bgzf_size(data, 1)                          # at least zlib level 1's ratio
    assert ours < zlib_bgzf_size(data, 6, zlib.Z_HUFFMAN_ONLY)      # the matches pay


def test_ratio_on_duplicated_reads_near_level_6():
    data = synth.fastq(20261005, 100000, (36, 151), dup='both', dup_templates=40)
    ours = sum(len(ops.bgzf_block_host(b)) for b in blocks_of(data))
    assert ours <= 1.10 * zlib_bgzf_size(data, 6)


# ------------------------------------------------------------------ the compressor under AddressSanitizer / UBSan
DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "deflate_core.h"

struct Env {
    uint8_t* out; uint32_t limit; uint16_t* dist; uint32_t n; const uint32_t* x2n;
    void sync() {}
    void lds_max(uint32_t* p, uint32_t v) { if (v > *p) *p = v; }
    void lds_add(uint32_t* p, uint32_t v) { *p += v; }
    void lds_xor(uint32_t* p, uint32_t v) { *p ^= v; }
    void dist_put(uint32_t p, uint32_t d) { if (p >= n) abort(); dist[p] = (uint16_t)d; }
    uint32_t dist_get(uint32_t p) const { if (p >= n) abort(); return dist[p]; }
    void word_store(uint32_t w, uint32_t v) { for (uint32_t k = 0; k < 4; ++k) if (4ull * w + k < limit) out[4 * w + k] = (uint8_t)(v >> (8 * k)); }
    void word_or(uint32_t w, uint32_t v) { for (uint32_t k = 0; k < 4; ++k) if (4ull * w + k < limit) out[4 * w + k] |= (uint8_t)(v >> (8 * k)); }
};

int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    uint32_t x2n[32];
    uq_crc_x2n_init(x2n);
    UqDeflateLds* s = (UqDeflateLds*)malloc(sizeof(UqDeflateLds));
    uint32_t hdr[2];
    while (fread(hdr, 4, 2, f) == 2) {
        const uint32_t n = hdr[0], cap = hdr[1];
        uint8_t* in = (uint8_t*)malloc(n ? n : 1);
        if (fread(in, 1, n, f) != n) return 3;
        memset(s, 0xA5, sizeof(UqDeflateLds));                      // whatever LDS held before
        if (n <= UQ_DEF_MAX_IN) memcpy(s->in, in, n);
        uint8_t* out = (uint8_t*)calloc(cap ? cap : 1, 1);          // exactly `cap` bytes: a write past them is a report
        uint16_t* dist = (uint16_t*)malloc(2 * (n ? n : 1));
        Env env{out, cap, dist, n, x2n};
        uint32_t mb = 0;
        const int st = uq_deflate_block(env, s, n, cap, 0, 1, &mb);
        const uint32_t res[2] = {(uint32_t)st, mb};
        fwrite(res, 4, 2, g);
        if (st == 0) fwrite(out, 1, mb, g);
        free(in); free(out); free(dist);
    }
    free(s);
    fclose(f); fclose(g);
    return 0;
}
'''


def _gxx():
    for c in ('g++', 'c++', 'clang++'):
        p = shutil.which(c)
        if p: return p
    return None


def test_compressor_under_address_sanitizer(tmp_path):
    gxx = _gxx()
    if gxx is None:
        pytest.skip('no host C++ compiler')
    src = tmp_path / 'drv.cpp'
    src.write_text(DRIVER)
    exe = tmp_path / 'drv'
    subprocess.check_call([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                           os.path.dirname(CORE), str(src), '-o', str(exe)])
    rnd = random.Random(29)
    fq = synth.fastq(20261005, 3000, (36, 301), n_rate=1)
    alphabet = [b'ACGT', b'A', b'AB', bytes(range(256)), b'@:+\n0123456789']
    cases = []
    for i in range(3000):
        kind = i % 6
        n = rnd.choice([0, 1, 2, 3, 4, 5, 17, 258, 259, 511, 512, 513, 4096, 32768, 32769, 65279, BLOCK, rnd.randrange(BLOCK + 1)])
        if kind == 0:
            data = bytes(rnd.getrandbits(8) for _ in range(n))
        elif kind == 1:
            a = rnd.choice(alphabet)
            data = bytes(a[rnd.randrange(len(a))] for _ in range(n))
        elif kind == 2:
            at = rnd.randrange(len(fq) - BLOCK)
            data = fq[at:at + n]
        elif kind == 3:                                             # repeats at chosen distances
            d = rnd.choice([1, 2, 3, 4, 255, 256, 257, 4096, 32767, 32768, 32769])
            seed = bytes(rnd.getrandbits(8) for _ in range(min(d, n)))
            data = (seed * (n // max(len(seed), 1) + 1))[:n] if seed else b''
        else:
            data = bytes(rnd.getrandbits(2) + 65 for _ in range(n))
        if i % 3 == 0:
            want = len(ops.bgzf_block_host(data))
            cap = rnd.choice([want, want - 1, want + 3, max(want // 2, 0), 0])
        else:
            cap = 65536
        cases.append((data, cap))
    cases.append((b'x' * (BLOCK + 1), 65536))
    with open(tmp_path / 'cases.bin', 'wb') as f:
        for data, cap in cases:
            f.write(struct.pack('<II', len(data), cap) + data)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:exitcode=99', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1:exitcode=98')
    r = subprocess.run([str(exe), str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, env=env, timeout=900)
    assert r.returncode == 0 and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]
    out = (tmp_path / 'out.bin').read_bytes()
    at, short = 0, 0
    for data, cap in cases:
        st, mb = struct.unpack('<II', out[at:at + 8]); at += 8
        if len(data) > BLOCK:
            assert st == 2
            continue
        if mb > cap:
            assert st == 1
            short += 1
            continue
        assert st == 0
        m = out[at:at + mb]; at += mb
        member_ok(m, data)
        if cap == 65536:
            assert m == ops.bgzf_block_host(data)                   # the driver's build = the library's
    assert at == len(out) and short > 100


# ------------------------------------------------------------------ the CLI
def test_bgzf_without_decode_is_refused(tmp_path, capsys):
    p = tmp_path / 'in.fastq'
    p.write_bytes(synth.fastq(3, 20, 50))
    assert uq.main(['-i', str(p), '--bgzf', '--quiet']) == 1
    assert 'ERROR: --bgzf' in capsys.readouterr().out
    assert not (tmp_path / 'in.fastq.uQ').exists()
