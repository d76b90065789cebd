"""Level 2 of the deflate compressor (deflate_core.h: more candidates per position, a lazy parse) on the CPU: its members checked with
zlib / gzip and the project's own inflate, the size-only path against them, level 1 byte for byte what it was, the ratio conditions
against level 1 and zlib, the CLI's rules for --bgzf-level, `python -m uq_amd.bgzf_host --level`, and both level-2 entries under
AddressSanitizer / UBSan through a small g++ driver."""
import ctypes as C
import glob
import gzip
import os
import random
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from test_deflate_cpu import BLOCK, CORE, GOLD, REPO, _gxx, block_matrix, blocks_of, member_ok, zlib_bgzf_size
from test_gzip_cpu import BGZF_EOF
from uq_amd import _lib, ops, synth, uq

sys.path.insert(0, os.path.join(REPO, 'tools'))
ROUND, SUB, WIN = 512, 128, 8192


def _planted(n, plants, seed):
    """n random bytes with byte strings planted at positions: [(position, bytes)]."""
    rnd = random.Random(seed)
    a = bytearray(rnd.getrandbits(8) for _ in range(n))
    for at, b in plants:
        a[at:at + len(b)] = b
    return bytes(a[:n])


def _lazy_at(q, seed):
    """A match of 4 bytes at q and one of 10 bytes at q + 1, both from rounds before q's: the lazy parse makes q a literal."""
    rnd = random.Random(seed)
    long_, first = bytes(rnd.getrandbits(8) for _ in range(10)), bytes([rnd.getrandbits(8)])
    return _planted(q + 700, [(200, long_), (299, first + long_[:3]), (q, first + long_)], seed + 1)


def edge_blocks():
    """(name, block) pairs that put level 2 on its edges: the ends of a sub-segment, a round, a parse window and the block; matches that
    end with the block; a longer match one position on, at a sub-segment's and a window's last position; candidates of one hash."""
    text = synth.fastq(20261018, 600, (36, 151), dup='both', dup_templates=10)
    out = [('text/%d' % n, text[:n]) for n in (0, 1, 3, 4, 5, SUB - 1, SUB, SUB + 1, ROUND - 1, ROUND, ROUND + 1, WIN - 1, WIN, WIN + 1,
                                               BLOCK - 1, BLOCK)]
    out += [('run/%d' % n, b'Q' * n) for n in (3, 4, 5, SUB + 1, ROUND + 1, BLOCK - 1)]
    rnd = random.Random(11)
    p = bytes(rnd.getrandbits(8) for _ in range(20))
    for tail in (3, 4, 5, 9):                                       # the block's last `tail` bytes are a match: its last token ends at n
        for n in (700, 4 * SUB, 2 * ROUND, WIN):
            out.append(('match_to_end/%d/%d' % (tail, n), _planted(n, [(100, p), (n - tail, p[:tail])], n + tail)))
    out.append(('match_at_last_position', _planted(1000, [(100, p), (996, p[:3] + p[:1])], 5)))      # p + 1 == n behind a match
    out.append(('run_to_end', _planted(1000, [(990, b'z' * 10)], 6)))
    out.append(('lazy_at_sub_end', _lazy_at(8 * SUB - 1, 21)))
    out.append(('lazy_at_window_end', _lazy_at(WIN - 1, 22)))
    out.append(('lazy_at_round_end', _lazy_at(3 * ROUND - 1, 23)))
    # one 4-byte hash three times before the position that looks it up: the middle occurrence is the longest match
    out.append(('middle_candidate_best', _planted(3000, [(600, p[:4]), (1200, p[:12]), (1800, p[:4]), (2400, p[:12])], 31)))
    out.append(('oldest_candidate_lost', _planted(3000, [(600, p[:12]), (1200, p[:4]), (1800, p[:4]), (2400, p[:12])], 32)))
    out.append(('equal_candidates_two_distances', _planted(3000, [(1200, p[:8]), (1800, p[:8]), (2400, p[:8])], 33)))
    out.append(('copy_longer_than_a_round', _planted(9000, [(5000, _planted(2000, [], 34)), (100, _planted(2000, [], 34))], 35)))
    return out


def all_blocks():
    return block_matrix() + edge_blocks()


def S2(data):
    return sum(len(ops.bgzf_block_host(b, level=2)) for b in blocks_of(data))


# ------------------------------------------------------------------ 1, 2: validity on the matrix and the edge shapes
def test_level2_members_inflate_to_the_input():
    members = []
    for name, b in all_blocks():
        m = ops.bgzf_block_host(b, level=2)
        member_ok(m, b)
        assert len(m) <= min(len(b) + 31, 65536), name
        st, back = ops.inflate_member_host(m[18:-8], len(b), zlib.crc32(b))
        assert st == 0 and back == b, name
        assert ops.bgzf_block_host(bytes(b), level=2) == m, name   # deterministic
        members.append(m)
    blob = b''.join(members) + BGZF_EOF
    kind, m, total, err = ops.gzip_scan(np.frombuffer(blob, dtype=np.uint8))
    assert kind == ops.GZIP_BGZF and err is None and len(m) == len(members) + 1 and total == sum(len(b) for _, b in all_blocks())
    assert gzip.decompress(blob) == b''.join(b for _, b in all_blocks())


def test_level2_too_large_and_too_small():
    st, size, out = ops.bgzf_block_host(b'x' * (BLOCK + 1), capacity=65536, level=2)
    assert st == 2
    data = synth.fastq(11, 300, 100)[:BLOCK]
    m = ops.bgzf_block_host(data, level=2)
    assert ops.bgzf_block_host(data, capacity=len(m), level=2) == (0, len(m), m)
    assert ops.bgzf_block_host(data, capacity=len(m) - 1, level=2) == (1, len(m), b'\x00' * (len(m) - 1))


# ------------------------------------------------------------------ 3: the sizer
@pytest.mark.parametrize('n', [0, 1, BLOCK, BLOCK + 1, 3 * BLOCK + 77])
def test_level2_host_sizer_and_host_command(n):
    data = (synth.fastq(20261005, n // 200 + 2, (36, 301), n_rate=1) * 2)[:n]
    rnd = random.Random(n)
    for p in (0, 1, 128, 256):
        prefix = bytes(rnd.getrandbits(7) for _ in range(p))
        assert ops.deflate_size_host(data, prefix, level=2) == S2(prefix + data), p
    r = subprocess.run([sys.executable, '-m', 'uq_amd.bgzf_host', '--no-eof', '--level', '2'], input=data, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, cwd=REPO, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert len(r.stdout) == S2(data) == ops.deflate_size_host(data, level=2)
    assert r.stdout == b''.join(ops.bgzf_block_host(b, level=2) for b in blocks_of(data))
    if n: assert gzip.decompress(r.stdout) == data


def test_level2_sizer_on_every_block():
    for name, b in all_blocks():
        assert ops.deflate_size_host(b, level=2) == (len(ops.bgzf_block_host(b, level=2)) if b else 0), name


# ------------------------------------------------------------------ 4: level 1 is what it was
def test_level1_bytes_through_every_entry():
    lib = _lib.load()
    for name, b in block_matrix():
        m = ops.bgzf_block_host(b)
        assert ops.bgzf_block_host(b, level=1) == m, name
        out = np.zeros(65536, dtype=np.uint8)
        nout, st = C.c_uint64(), C.c_uint32()
        _lib.call('uq_bgzf_compress_block_host_l', C.c_char_p(b), len(b), C.c_void_p(out.ctypes.data), 65536, C.byref(nout), C.byref(st), 0)
        assert st.value == 0 and out[:nout.value].tobytes() == m, name
        assert ops.deflate_size_host(b, level=1) == ops.deflate_size_host(b) == (len(m) if b else 0), name
        tot = C.c_uint64()
        _lib.call('uq_deflate_size_host_l', None, 0, C.c_char_p(b), len(b), C.byref(tot), 0)
        assert tot.value == (len(m) if b else 0), name
    assert lib is not None


def test_unknown_flag_bits_and_levels_are_errors():
    out = np.zeros(65536, dtype=np.uint8)
    nout, st, tot = C.c_uint64(), C.c_uint32(), C.c_uint64()
    with pytest.raises(Exception, match='unknown flags'):
        _lib.call('uq_bgzf_compress_block_host_l', C.c_char_p(b'abc'), 3, C.c_void_p(out.ctypes.data), 65536, C.byref(nout), C.byref(st), 4)
    with pytest.raises(Exception, match='unknown flags'):
        _lib.call('uq_bgzf_compress_block_host_l', C.c_char_p(b'abc'), 3, C.c_void_p(out.ctypes.data), 65536, C.byref(nout), C.byref(st), 1)
    with pytest.raises(Exception, match='unknown flags'):
        _lib.call('uq_deflate_size_host_l', None, 0, C.c_char_p(b'abc'), 3, C.byref(tot), 8)
    for level in (0, 3, 9, None):
        with pytest.raises(ValueError):
            ops.bgzf_block_host(b'abc', level=level)
        with pytest.raises(ValueError):
            ops.deflate_size_host(b'abc', level=level)


# ------------------------------------------------------------------ 5: the ratio conditions (host twin)
def _totals(data):
    return (sum(len(ops.bgzf_block_host(b)) for b in blocks_of(data)), S2(data), zlib_bgzf_size(data, 1), zlib_bgzf_size(data, 6))


def _binned():
    from bench_inflate import binned_fastq
    return binned_fastq(20000, 20261016, length=150)


def _golden():
    return b''.join(open(p, 'rb').read() for p in sorted(glob.glob(os.path.join(GOLD, '*.fastq'))) if not p.endswith('.refdecode.fastq'))


CORPORA = {'150bp': lambda: synth.fastq(20261005, 100000, 150),
           '36-301bp': lambda: synth.fastq(20261005, 100000, (36, 301)),
           'dup': lambda: synth.fastq(20261005, 100000, (36, 151), dup='both', dup_templates=40),
           'binned': _binned,
           'golden': _golden}


@pytest.mark.parametrize('name', list(CORPORA))
def test_level2_is_smaller_than_level1(name):
    l1, l2, z1, z6 = _totals(CORPORA[name]())
    print('%s: level 1 %d, level 2 %d, zlib 1 %d, zlib 6 %d' % (name, l1, l2, z1, z6))
    assert l2 < l1
    if name == 'dup':
        assert l2 <= 1.10 * z6                                      # level 1's bound
        assert abs(l2 - z6) < abs(l1 - z6)                          # and strictly nearer to level 6 than level 1 is


@pytest.mark.parametrize('name', ['one_byte_run', 'two_byte_run', 'distance_32768'])
def test_level2_on_the_shapes_level1_loses_on(name):
    b = dict(block_matrix())[name]
    l1, l2 = len(ops.bgzf_block_host(b)), len(ops.bgzf_block_host(b, level=2))
    print('%s: level 1 %d, level 2 %d' % (name, l1, l2))
    assert l2 < l1


# ------------------------------------------------------------------ 6: the CLI's rules
def _args(tmp_path, flags):
    p = tmp_path / 'in.fastq'
    p.write_bytes(synth.fastq(3, 20, 50))
    return uq.build_parser().parse_args(['-i', str(p), '--quiet'] + flags)


@pytest.mark.parametrize('flags', [[], ['--test'], ['--decode'], ['--test', '--compressor', 'gzip']],
                         ids=lambda f: '_'.join(f).replace('--', '') or 'alone')
def test_bgzf_level_without_a_host_is_refused(tmp_path, capsys, flags):
    with pytest.raises(uq.UqError, match='--bgzf-level'):
        uq.validate_args(_args(tmp_path, ['--bgzf-level', '2'] + flags))
    assert uq.main(['-i', str(tmp_path / 'in.fastq'), '--quiet', '--bgzf-level', '2'] + flags) == 1
    out = capsys.readouterr().out
    assert 'ERROR: --bgzf-level' in out and '--decode --bgzf' in out and '--gz' in out and '--test --device-compressor' in out
    assert not (tmp_path / 'in.fastq.uQ').exists()


def test_bgzf_level_3_is_refused(tmp_path, capsys):
    for host in (['--gz'], ['--decode', '--bgzf'], ['--test', '--device-compressor']):
        with pytest.raises(uq.UqError, match='--bgzf-level'):
            uq.validate_args(_args(tmp_path, host + ['--bgzf-level', '3']))
    assert uq.main(['-i', str(tmp_path / 'in.fastq'), '--quiet', '--gz', '--bgzf-level', '3']) == 1
    assert 'ERROR: --bgzf-level' in capsys.readouterr().out
    assert not (tmp_path / 'in.fastq.uQ.gz').exists()


def test_bgzf_level_with_its_hosts_is_accepted(tmp_path):
    for host in (['--gz'], ['--decode', '--bgzf'], ['--test', '--device-compressor']):
        for level in (1, 2):
            assert uq.validate_args(_args(tmp_path, host + ['--bgzf-level', str(level)])).bgzf_level == level
        assert uq.validate_args(_args(tmp_path, host)).bgzf_level is None


@pytest.mark.parametrize('flags', [['--level', '3'], ['--level'], ['--level', '0'], ['--level', '2x'], ['--level', '2', '--fast']])
def test_host_command_refuses_other_levels(flags):
    r = subprocess.run([sys.executable, '-m', 'uq_amd.bgzf_host'] + flags, input=b'abc', stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=REPO)
    assert r.returncode == 2 and r.stdout == b''


def test_host_command_level_1_is_the_default():
    data = synth.fastq(5, 400, 100)
    run = lambda flags: subprocess.run([sys.executable, '-m', 'uq_amd.bgzf_host'] + flags, input=data, stdout=subprocess.PIPE, cwd=REPO).stdout
    assert run(['--level', '1']) == run([]) != run(['--level', '2'])


# ------------------------------------------------------------------ 7: both level-2 entries under AddressSanitizer / UBSan
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
    void dist_put(uint32_t p, uint32_t d) { if (p >= n || d < 1 || d > 32768 || d > p) abort(); dist[p] = (uint16_t)d; }
    uint32_t dist_get(uint32_t p) const { if (p >= n) abort(); return dist[p]; }
    void word_store(uint32_t w, uint32_t v) { for (uint32_t k = 0; k < 4; ++k) if (4ull * w + k < limit) out[4 * w + k] = (uint8_t)(v >> (8 * k)); }
    void word_or(uint32_t w, uint32_t v) { for (uint32_t k = 0; k < 4; ++k) if (4ull * w + k < limit) out[4 * w + k] |= (uint8_t)(v >> (8 * k)); }
};

struct SizeEnv {
    uint8_t* dist; uint32_t n;
    void sync() {}
    void lds_max(uint32_t* p, uint32_t v) { if (v > *p) *p = v; }
    void lds_add(uint32_t* p, uint32_t v) { *p += v; }
    void dist_put(uint32_t p, uint32_t sym) { if (p >= n || sym > 29) abort(); dist[p] = (uint8_t)sym; }
    uint32_t dist_get(uint32_t p) const { if (p >= n) abort(); return dist[p]; }
};

int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    uint32_t x2n[32];
    uq_crc_x2n_init(x2n);
    UqDeflateLds2* s = (UqDeflateLds2*)malloc(sizeof(UqDeflateLds2));
    UqDeflateSizeLds2* z = (UqDeflateSizeLds2*)malloc(sizeof(UqDeflateSizeLds2));
    uint32_t hdr[2];
    while (fread(hdr, 4, 2, f) == 2) {
        const uint32_t n = hdr[0], cap = hdr[1];
        uint8_t* in = (uint8_t*)malloc(n ? n : 1);
        if (fread(in, 1, n, f) != n) return 3;
        memset(s, 0xA5, sizeof(UqDeflateLds2));                     // whatever LDS held before
        memset(z, 0x5A, sizeof(UqDeflateSizeLds2));
        if (n <= UQ_DEF_MAX_IN) { memcpy(s->in, in, n); memcpy(z->in, in, n); }
        uint8_t* out = (uint8_t*)calloc(cap ? cap : 1, 1);          // exactly `cap` bytes: a write past them is a report
        uint16_t* dist = (uint16_t*)malloc(2 * (n ? n : 1));        // exactly n distances, n distance symbols
        uint8_t* dsym = (uint8_t*)malloc(n ? n : 1);
        Env env{out, cap, dist, n, x2n};
        SizeEnv senv{dsym, n};
        uint32_t mb = 0, sb = 0;
        const int st = uq_deflate_block_l<2>(env, s, n, cap, 0, 1, &mb);
        const int sst = uq_deflate_block_size_l<2>(senv, z, n, 0, 1, &sb);
        const uint32_t res[4] = {(uint32_t)st, mb, (uint32_t)sst, sb};
        fwrite(res, 4, 4, g);
        if (st == 0) fwrite(out, 1, mb, g);
        if (st == 1) fwrite(out, 1, cap, g);                        // too small: the capacity's bytes, to be all zero
        free(in); free(out); free(dist); free(dsym);
    }
    free(s); free(z);
    fclose(f); fclose(g);
    return 0;
}
'''


def test_level2_under_address_sanitizer(tmp_path):
    gxx = _gxx()
    if gxx is None:
        pytest.skip('no host C++ compiler')
    src = tmp_path / 'drv.cpp'
    src.write_text(DRIVER)
    exe = tmp_path / 'drv'
    subprocess.check_call([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                           os.path.dirname(CORE), str(src), '-o', str(exe)])
    rnd = random.Random(37)
    fq = synth.fastq(20261005, 3000, (36, 301), n_rate=1)
    alphabet = [b'ACGT', b'A', b'AB', bytes(range(256)), b'@:+\n0123456789', b'FFFFFFF:,#']
    blocks = [b for _, b in edge_blocks()]
    for i in range(400):
        kind = i % 5
        n = rnd.choice([0, 1, 2, 3, 4, 5, 17, 127, 128, 129, 258, 259, 511, 512, 513, 4096, 8191, 8192, 8193, 32768, 32769, 65279, BLOCK,
                        rnd.randrange(BLOCK + 1)])
        if kind == 0:
            n = min(n, 8193)
            blocks.append(bytes(rnd.getrandbits(8) for _ in range(n)))
        elif kind == 1:
            a = rnd.choice(alphabet)
            blocks.append(bytes(rnd.choices(a, k=n)))
        elif kind == 2:
            at = rnd.randrange(len(fq) - BLOCK)
            blocks.append(fq[at:at + n])
        elif kind == 3:                                             # repeats at chosen distances
            d = rnd.choice([1, 2, 3, 4, 255, 256, 257, 511, 512, 513, 4096, 32767, 32768, 32769])
            seed = bytes(rnd.getrandbits(8) for _ in range(min(d, n)))
            blocks.append((seed * (n // max(len(seed), 1) + 1))[:n] if seed else b'')
        else:
            blocks.append(bytes(rnd.choices(b'ACGT', k=n)))
    cases = []
    for i, data in enumerate(blocks):
        cap = 65536
        if i % 3 == 0:
            want = len(ops.bgzf_block_host(data, level=2))
            cap = [want, want - 1, max(want // 2, 0), 0, want + 3][(i // 3) % 5]
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
        st, mb, sst, sb = struct.unpack('<IIII', out[at:at + 16]); at += 16
        if len(data) > BLOCK:
            assert st == 2 and sst == 2
            continue
        want = ops.bgzf_block_host(data, level=2)                   # the driver's build = the library's, emit and size-only
        assert sst == 0 and sb == mb == len(want)
        if mb > cap:
            assert st == 1 and out[at:at + cap] == b'\x00' * cap
            at += cap; short += 1
            continue
        assert st == 0 and out[at:at + mb] == want
        at += mb
        member_ok(want, data)
    assert at == len(out) and short > 40
