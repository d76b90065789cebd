"""The --test sizer on the CPU: uq_deflate_size_host (deflate_core.h's size-only path) against the sizes of the members that
uq_bgzf_compress_block_host writes, the same under AddressSanitizer / UBSan through a small g++ driver, the CLI's rules for
--device-compressor, and `python -m uq_amd.bgzf_host`."""
import gzip
import os
import random
import struct
import subprocess
import sys
import zlib

import pytest

from test_deflate_cpu import BLOCK, CORE, REPO, _gxx, blocks_of
from uq_amd import ops, synth, uq


def S(data):
    """The size the issue fixes: the members of the compressor itself, block by block, no EOF member."""
    return sum(len(ops.bgzf_block_host(b)) for b in blocks_of(data))


def corpus(kind, n):
    rnd = random.Random(n * 7 + len(kind))
    if kind == 'text': return (synth.fastq(20261005, n // 200 + 2, (36, 301), n_rate=1) * 2)[:n]
    if kind == 'runs': return (b'A' * 700 + b'CG' * 300 + b'T' * 5)[:max(n, 1)] * (n // 1305 + 1)
    if kind == 'zeros': return bytes(n)
    if kind == 'random': return bytes(rnd.getrandbits(8) for _ in range(n))           # ends up stored
    if kind == 'halves':
        h = bytes(rnd.getrandbits(8) for _ in range(n // 2))
        return h + h
    raise ValueError(kind)


KINDS = ['text', 'runs', 'zeros', 'random', 'halves']
LENGTHS = [0, 1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 77, 5 * BLOCK]
PREFIXES = [0, 1, 128, 256]


def cases():
    rnd = random.Random(5)
    for kind in KINDS:
        for n in LENGTHS:
            data = corpus(kind, n)[:n]
            for p in PREFIXES:
                yield kind, bytes(rnd.getrandbits(7) for _ in range(p)), data


def test_host_sizer_equals_the_sum_of_the_members():
    stored = 0
    for kind, prefix, data in cases():
        want = S(prefix + data)
        assert ops.deflate_size_host(data, prefix) == want, (kind, len(prefix), len(data))
        assert ops.deflate_size_host(prefix + data) == want
        stored += kind == 'random' and len(data) == BLOCK and not prefix and want == BLOCK + 31
    assert stored == 1                                             # the random block did take the stored path
    assert ops.deflate_size_host(b'') == 0


def test_prefix_longer_than_256_bytes_is_refused():
    with pytest.raises(Exception):
        ops.deflate_size_host(b'abc', bytes(257))


DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "deflate_core.h"

struct Env {
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
    UqDeflateSizeLds* s = (UqDeflateSizeLds*)malloc(sizeof(UqDeflateSizeLds));
    uint32_t n;
    while (fread(&n, 4, 1, f) == 1) {
        uint8_t* in = (uint8_t*)malloc(n ? n : 1);
        if (fread(in, 1, n, f) != n) return 3;
        memset(s, 0xA5, sizeof(UqDeflateSizeLds));                  // whatever LDS held before
        if (n <= UQ_DEF_MAX_IN) memcpy(s->in, in, n);
        uint8_t* dist = (uint8_t*)malloc(n ? n : 1);                // exactly n symbols
        Env env{dist, n};
        uint32_t mb = 0;
        const int st = uq_deflate_block_size(env, s, n, 0, 1, &mb);
        const uint32_t res[2] = {(uint32_t)st, mb};
        fwrite(res, 4, 2, g);
        free(in); free(dist);
    }
    free(s);
    fclose(f); fclose(g);
    return 0;
}
'''


def test_sizer_under_address_sanitizer(tmp_path):
    gxx = _gxx()
    if gxx is None:
        pytest.skip('no host C++ compiler')
    src = tmp_path / 'drv.cpp'
    src.write_text(DRIVER)
    exe = tmp_path / 'drv'
    subprocess.check_call([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                           os.path.dirname(CORE), str(src), '-o', str(exe)])
    blocks = []
    for kind, prefix, data in cases():
        blocks += blocks_of(prefix + data)
    rnd = random.Random(31)
    fq = synth.fastq(20261005, 3000, (36, 301), n_rate=1)
    for i in range(600):
        n = rnd.choice([0, 1, 2, 3, 4, 5, 17, 258, 259, 511, 512, 513, 4096, 32768, 32769, BLOCK - 1, BLOCK, rnd.randrange(BLOCK + 1)])
        if i % 3 == 0:
            d = rnd.choice([1, 2, 3, 4, 255, 256, 257, 4096, 32767, 32768, 32769])
            seed = bytes(rnd.getrandbits(8) for _ in range(min(d, n)))
            blocks.append((seed * (n // max(len(seed), 1) + 1))[:n] if seed else b'')
        elif i % 3 == 1:
            at = rnd.randrange(len(fq) - BLOCK)
            blocks.append(fq[at:at + n])
        else:
            blocks.append(bytes(rnd.getrandbits(2) + 65 for _ in range(n)))
    blocks.append(b'x' * (BLOCK + 1))
    with open(tmp_path / 'cases.bin', 'wb') as f:
        for b in blocks:
            f.write(struct.pack('<I', len(b)) + b)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:exitcode=99', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1:exitcode=98')
    r = subprocess.run([str(exe), str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, env=env, timeout=900)
    assert r.returncode == 0 and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]
    out = (tmp_path / 'out.bin').read_bytes()
    assert len(out) == 8 * len(blocks)
    for k, b in enumerate(blocks):
        st, mb = struct.unpack('<II', out[8 * k:8 * k + 8])
        if len(b) > BLOCK:
            assert st == 2
            continue
        assert st == 0 and mb == len(ops.bgzf_block_host(b)), (k, len(b))


# ------------------------------------------------------------------ the CLI's rules
def _args(tmp_path, flags):
    p = tmp_path / 'in.fastq'
    p.write_bytes(synth.fastq(3, 20, 50))
    return uq.build_parser().parse_args(['-i', str(p), '--quiet'] + flags)


def test_flag_with_compressor_is_refused(tmp_path, capsys):
    with pytest.raises(uq.UqError, match='--device-compressor and --compressor'):
        uq.validate_args(_args(tmp_path, ['--test', '--device-compressor', '--compressor', 'gzip']))
    assert uq.main(['-i', str(tmp_path / 'in.fastq'), '--quiet', '--test', '--device-compressor', '--compressor', 'gzip']) == 1
    assert 'ERROR: --device-compressor' in capsys.readouterr().out
    assert not (tmp_path / 'in.fastq.uQ').exists()


def test_flag_without_test_is_refused(tmp_path, capsys):
    with pytest.raises(uq.UqError, match='together with --test'):
        uq.validate_args(_args(tmp_path, ['--device-compressor']))
    assert uq.main(['-i', str(tmp_path / 'in.fastq'), '--quiet', '--device-compressor']) == 1
    assert 'ERROR: --device-compressor' in capsys.readouterr().out
    assert not (tmp_path / 'in.fastq.uQ').exists()


def test_flag_with_test_alone_is_accepted(tmp_path):
    args = uq.validate_args(_args(tmp_path, ['--test', '--device-compressor']))
    assert args.device_compressor and args.test and args.compressor is None
    args = uq.validate_args(_args(tmp_path, ['--test', '--device-compressor', '--sort', 'None', '--raw', 'DNA', '--pattern', '0.1', '2.2']))
    assert args.device_compressor and args.sort == (None,) and args.raw == {'DNA'}
    assert not uq.validate_args(_args(tmp_path, ['--test', '--compressor', 'gzip'])).device_compressor       # the old path is as it was


# ------------------------------------------------------------------ python -m uq_amd.bgzf_host
def _host_command(data, flags=()):
    r = subprocess.run([sys.executable, '-m', 'uq_amd.bgzf_host'] + list(flags), input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       cwd=REPO, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout


@pytest.mark.parametrize('n', [0, 1, BLOCK, BLOCK + 1, 3 * BLOCK + 77])
def test_host_command_round_trips_and_has_the_size(n):
    data = corpus('text', n)[:n]
    blob = _host_command(data)
    assert gzip.decompress(blob) == data
    d, rest, out = zlib.decompressobj(31), blob, b''
    while rest:                                                     # member by member with zlib
        out += d.decompress(rest)
        assert d.eof
        rest = d.unused_data
        d = zlib.decompressobj(31)
    assert out == data
    bare = _host_command(data, ['--no-eof'])
    assert len(bare) == S(data) == ops.deflate_size_host(data) and blob == bare + blob[len(bare):] and len(blob) == len(bare) + 28
    if n: assert gzip.decompress(bare) == data


def test_host_command_refuses_unknown_flags():
    r = subprocess.run([sys.executable, '-m', 'uq_amd.bgzf_host', '--level', '9'], input=b'', stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=REPO)
    assert r.returncode == 2 and r.stdout == b''
