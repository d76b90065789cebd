"""gzip input on the CPU: the member scan (uq_gzip_scan), the deflate decoder that the GPU runs (inflate_core.h, through
uq_inflate_member_host and, under AddressSanitizer, a small g++ driver) against zlib, and the sharded encoder's refusal.
Every compressed input is made here with zlib / gzip."""
import gzip
import os
import random
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from deflate_writer import Bits, crafted_invalid, crafted_members, fixed_lit
from uq_amd import ops, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORE = os.path.join(REPO, 'uq_amd', 'csrc', 'inflate_core.h')
BGZF_CHUNK = 65280
BGZF_EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=()):
    """Raw deflate of `data`; `flushes`: (offset, zlib flush mode) pairs to cut the stream at."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, at = [], 0
    for off, mode in flushes:
        out.append(c.compress(data[at:off]))
        out.append(c.flush(mode))
        at = off
    out.append(c.compress(data[at:]))
    out.append(c.flush())
    return b''.join(out)


def bgzf_member(chunk, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    d = raw_deflate(chunk, level, strategy)
    bsize = 18 + len(d) + 8 - 1
    return (b'\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00' + struct.pack('<H', bsize) + d +
            struct.pack('<II', zlib.crc32(chunk), len(chunk)))


def bgzf(data, level=6, eof=True, chunk=BGZF_CHUNK, strategy=zlib.Z_DEFAULT_STRATEGY):
    """What `bgzip` writes: independent members of <= `chunk` bytes of output, each with its size in a BC extra subfield."""
    parts = [bgzf_member(data[i:i + chunk], level, strategy) for i in range(0, len(data), chunk)]
    return b''.join(parts) + (BGZF_EOF if eof else b'')


def gzip_header(flags=0, extra=None, name=None, comment=None, hcrc=False):
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    h = bytes([0x1f, 0x8b, 8, flg | flags]) + b'\x00\x00\x00\x00\x00\x03'
    if extra is not None: h += struct.pack('<H', len(extra)) + extra
    if name is not None: h += name + b'\x00'
    if comment is not None: h += comment + b'\x00'
    if hcrc: h += struct.pack('<H', zlib.crc32(h) & 0xFFFF)
    return h


def gzip_member(data, level=6, **hdr):
    return gzip_header(**hdr) + raw_deflate(data, level) + struct.pack('<II', zlib.crc32(data), len(data) & 0xFFFFFFFF)


def fastq(n=2000, seed=5):
    return synth.fastq(seed, n, (36, 151), n_rate=1)


def scan(data):
    return ops.gzip_scan(np.frombuffer(data, dtype=np.uint8))


# ------------------------------------------------------------------ the member scan
@pytest.mark.parametrize('eof', [True, False])
def test_scan_bgzf_members_agree_with_zlib(eof):
    data = fastq(3000)
    blob = bgzf(data, eof=eof)
    kind, m, total, err = scan(blob)
    assert kind == ops.GZIP_BGZF and err is None and total == len(data)
    chunks = [data[i:i + BGZF_CHUNK] for i in range(0, len(data), BGZF_CHUNK)]
    assert len(m) == len(chunks) + (1 if eof else 0)
    for k, c in enumerate(chunks):
        assert m[k]['isize'] == len(c) and m[k]['crc32'] == zlib.crc32(c) and m[k]['out_offset'] == k * BGZF_CHUNK
        d = blob[m[k]['data_offset']:m[k]['data_offset'] + m[k]['comp_bytes']]
        assert zlib.decompress(d, -15) == c
    if eof:
        assert m[-1]['isize'] == 0 and m[-1]['out_offset'] == len(data)
    assert gzip.decompress(blob) == data


def test_scan_accepts_trailing_empty_members():
    data = fastq(100)
    blob = bgzf(data, eof=True) + bgzf_member(b'') + BGZF_EOF
    kind, m, total, _ = scan(blob)
    assert kind == ops.GZIP_BGZF and total == len(data) and len(m) == 4 and list(m['isize'][1:]) == [0, 0, 0]


def test_scan_large_offsets_are_64_bit_prefix_sums():
    # the out_offset column is a 64-bit prefix sum: 70 000 full members sum past 2^32 (only the headers are real here)
    member = bgzf_member(b'\x00' * 65536, level=1)
    kind, m, total, _ = scan(member * 70000)
    assert kind == ops.GZIP_BGZF and total == 70000 * 65536 > 1 << 32
    assert int(m['out_offset'][-1]) == 69999 * 65536 and int(m['data_offset'][-1]) == 69999 * len(member) + 18


def test_scan_single_member_with_every_header_field_is_other():
    data = fastq(200)
    blob = gzip_member(data, extra=b'XY\x03\x00abc', name=b'reads.fastq', comment=b'a comment', hcrc=True)
    kind, m, total, err = scan(blob)
    assert kind == ops.GZIP_OTHER and err is None and len(m) == 1
    hl = len(gzip_header(extra=b'XY\x03\x00abc', name=b'reads.fastq', comment=b'a comment', hcrc=True))
    assert m[0]['data_offset'] == hl and m[0]['comp_bytes'] == len(blob) - hl
    assert zlib.decompressobj(-15).decompress(blob[hl:]) == data
    assert gzip.decompress(blob) == data


def test_scan_multi_member_without_bsize_is_other():
    a, b = fastq(100, 1), fastq(100, 2)
    blob = gzip.compress(a) + gzip.compress(b)
    kind, m, _, _ = scan(blob)
    assert kind == ops.GZIP_OTHER and len(m) == 1


def test_scan_bgzf_then_plain_member_is_other():
    data = fastq(2000)
    lead = bgzf(data, eof=False)
    blob = lead + gzip.compress(b'@r\nA\n+\nI\n')
    kind, m, total, _ = scan(blob)
    nb = -(-len(data) // BGZF_CHUNK)
    assert kind == ops.GZIP_OTHER and len(m) == nb + 1 and total == len(data)
    assert m[-1]['data_offset'] == len(lead) + 10


def test_scan_truncated_at_every_header_field():
    blob = gzip_member(fastq(50), extra=b'BC\x02\x00\x00\x00', name=b'n', comment=b'c', hcrc=True)
    # fix BSIZE so the member is BGZF, then cut it everywhere inside the header and member
    hdr = gzip_header(extra=b'BC\x02\x00' + struct.pack('<H', len(blob) - 1), name=b'n', comment=b'c', hcrc=True)
    blob = hdr + blob[len(hdr):]
    kind, m, _, _ = scan(blob)
    assert kind == ops.GZIP_BGZF and len(m) == 1
    for cut in range(1, len(blob)):
        kind, m, _, err = scan(blob[:cut])
        assert kind == ops.GZIP_MALFORMED, cut
        assert err[1] == 0 and 'member 0 at offset 0' in err[0], (cut, err)


@pytest.mark.parametrize('mutate,needle', [
    (lambda b: b[:2] + b'\x07' + b[3:], 'method 7'),
    (lambda b: b[:16] + struct.pack('<H', len(b) + 100) + b[18:], 'past the end'),
    (lambda b: b[:3] + bytes([b[3] | 0x20]) + b[4:], 'reserved flag'),
    (lambda b: b + b'junk' * 4, 'no gzip magic'),
    (lambda b: b[:-4] + struct.pack('<I', 65537), 'ISIZE 65537'),
    (lambda b: b[:16] + b'\x05\x00' + b[18:], 'smaller than its header'),
])
def test_scan_rejects_malformed(mutate, needle):
    blob = bgzf_member(fastq(50))
    kind, _, _, err = scan(mutate(blob))
    assert kind == ops.GZIP_MALFORMED and needle in err[0], err


def test_scan_bad_header_crc_is_malformed():
    blob = bytearray(gzip_member(b'x' * 100, name=b'n', hcrc=True))
    blob[12] ^= 1                                           # inside the name: the header CRC no longer matches
    kind, _, _, err = scan(bytes(blob))
    assert kind == ops.GZIP_MALFORMED and 'header CRC' in err[0]


def test_scan_second_member_error_names_its_offset():
    a = bgzf_member(fastq(50))
    b = bytearray(bgzf_member(fastq(60, 2)))
    b[2] = 9
    kind, m, _, err = scan(a + bytes(b))
    assert kind == ops.GZIP_MALFORMED and err[1] == len(a) and 'member 1 at offset %d' % len(a) in err[0]


# ------------------------------------------------------------------ the decoder (inflate_core.h) on the host
def _payloads():
    rnd = random.Random(7)
    return {'fastq': fastq(400)[:60000], 'random': bytes(rnd.getrandbits(8) for _ in range(40000)), 'one_byte': b'G' * 65536, 'empty': b'',
            'short': b'@r\nACGT\n+\nIIII\n'}


STRATEGIES = {'default': zlib.Z_DEFAULT_STRATEGY, 'filtered': zlib.Z_FILTERED, 'huffman_only': zlib.Z_HUFFMAN_ONLY, 'rle': zlib.Z_RLE,
              'fixed': zlib.Z_FIXED}


def member_matrix():
    """(name, raw deflate, data): levels 0-9 x strategies x payloads, plus flushes mid-member."""
    out = []
    for pname, data in _payloads().items():
        for level in range(10):
            for sname, s in STRATEGIES.items():
                out.append(('%s/l%d/%s' % (pname, level, sname), raw_deflate(data, level, s), data))
        if len(data) > 1000:
            for mode in (zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH):
                out.append(('%s/flush%d' % (pname, mode), raw_deflate(data, 6, flushes=[(100, mode), (100, mode), (len(data) // 2, mode)]), data))
    return out


def test_host_inflate_matches_zlib_on_the_matrix():
    for name, d, data in member_matrix():
        assert zlib.decompress(d, -15) == data
        st, out = ops.inflate_member_host(d, len(data), zlib.crc32(data))
        assert st == 0 and out == data, (name, st)


def test_host_inflate_checks_trailer():
    data = fastq(100)
    d = raw_deflate(data)
    assert ops.inflate_member_host(d, len(data), zlib.crc32(data) ^ 1)[0] == 10
    assert ops.inflate_member_host(d, len(data) + 1, zlib.crc32(data))[0] == 9
    assert ops.inflate_member_host(d, len(data) - 1, zlib.crc32(data))[0] == 8
    assert ops.inflate_member_host(d[:len(d) // 2], len(data), zlib.crc32(data))[0] == 1
    assert ops.inflate_member_host(d, 65537, 0)[0] == 12


def crafted():
    """(name, stream, isize, expected status) of hand-made bad streams."""
    out = []
    b = Bits().put(1, 1).put(1, 2); fixed_lit(b, 65); fixed_lit(b, 257); b.code(4, 5).put(0, 1); fixed_lit(b, 256)
    out.append(('distance beyond the output', b.bytes(), 4, 7))
    b = Bits().put(1, 1).put(1, 2); fixed_lit(b, 286)
    out.append(('length symbol 286', b.bytes(), 4, 6))
    b = Bits().put(1, 1).put(1, 2); fixed_lit(b, 65); fixed_lit(b, 257); b.code(30, 5)
    out.append(('distance symbol 30', b.bytes(), 4, 6))
    out.append(('block type 3', Bits().put(1, 1).put(3, 2).bytes() + b'\x00', 0, 2))
    out.append(('stored NLEN', Bits().put(1, 1).put(0, 2).bytes() + b'\x05\x00\x00\x00hello', 5, 3))
    out.append(('stored past the end', Bits().put(1, 1).put(0, 2).bytes() + b'\x05\x00\xfa\xffhel', 5, 1))
    out.append(('HLIT 287', Bits().put(1, 1).put(2, 2).put(30, 5).put(0, 5).put(0, 4).put(0, 60).bytes(), 0, 11))
    # dynamic: code-length code with 19 one-bit lengths (over-subscribed)
    b = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(15, 4)
    for _ in range(19): b.put(1, 3)
    out.append(('over-subscribed code lengths', b.put(0, 32).bytes(), 0, 4))
    # dynamic: code-length code {0: 1 bit, 16: 2 bits, 18: 2 bits}; first symbol 16 (repeat with no previous)
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    cl = {0: 1, 16: 2, 18: 2}
    b = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(19 - 4, 4)
    for s in order: b.put(cl.get(s, 0), 3)
    b.code(2, 2).put(0, 2)                                  # symbol 16 (codes: 0 -> '0', 16 -> '10', 18 -> '11')
    out.append(('repeat with no previous length', b.put(0, 32).bytes(), 0, 5))
    # dynamic: every literal/length length zero (18 x 2 = 276 zeros, then 258 - 276?): 257 + 1 lengths of zero -> no end-of-block code
    b = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(19 - 4, 4)
    for s in order: b.put(cl.get(s, 0), 3)
    b.code(3, 2).put(138 - 11, 7).code(3, 2).put(120 - 11, 7)
    out.append(('no end-of-block code', b.put(0, 32).bytes(), 0, 4))
    # dynamic: incomplete literal/length code (one code of 2 bits)
    b = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(19 - 4, 4)
    cl2 = {0: 1, 2: 2, 18: 2}
    for s in order: b.put(cl2.get(s, 0), 3)
    b.code(3, 2).put(138 - 11, 7).code(3, 2).put(118 - 11, 7).code(2, 2).code(0, 1)        # 245 zeros, lens[256] = 2, one distance 0
    out.append(('incomplete literal/length code', b.put(0, 32).bytes(), 0, 4))
    return out


@pytest.mark.parametrize('case', crafted(), ids=lambda c: c[0])
def test_host_inflate_rejects_crafted_streams(case):
    name, stream, isize, want = case
    st, _ = ops.inflate_member_host(stream, isize, 0)
    assert st == want, (name, st)


def corrupt_cases(seed=11, count=3000):
    """(stream, isize, crc, original) : bit flips, truncations, byte smears and random bytes on the matrix's members."""
    rnd = random.Random(seed)
    base = [(d, data) for _, d, data in member_matrix() if 0 < len(d) < 70000]
    cases = []
    for i in range(count):
        d, data = base[rnd.randrange(len(base))]
        b = bytearray(d)
        k = i % 4
        if k == 0:
            for _ in range(rnd.randint(1, 4)): b[rnd.randrange(len(b))] ^= 1 << rnd.randrange(8)
        elif k == 1:
            b = b[:rnd.randrange(len(b))]
        elif k == 2:
            at = rnd.randrange(len(b)); n = rnd.randint(1, 16)
            b[at:at + n] = bytes(rnd.getrandbits(8) for _ in range(min(n, len(b) - at)))
        else:
            b = bytearray(rnd.getrandbits(8) for _ in range(rnd.randint(1, 300)))
        cases.append((bytes(b), len(data), zlib.crc32(data), data))
    for _, stream, isize, _ in crafted():
        cases.append((stream, isize, 0, None))
    return cases


def test_host_inflate_corrupt_input_ends_in_status_or_right_bytes():
    for stream, isize, crc, data in corrupt_cases(count=1500):
        st, out = ops.inflate_member_host(stream, isize, crc)
        assert st != 0 or out == data


DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "inflate_core.h"
struct Src { const uint8_t* p; uint32_t len;
    uint32_t word(uint32_t off) const { uint32_t v = 0; for (uint32_t k = 0; k < 4; ++k) if ((uint64_t)off + k < len) v |= (uint32_t)p[off + k] << (8 * k); return v; } };
struct Out { uint8_t* o; const uint8_t* src;
    void put(uint32_t pos, uint8_t b) { o[pos] = b; }
    void copy(uint32_t pos, uint32_t dist, uint32_t len) { for (uint32_t i = 0; i < len; ++i) o[pos + i] = o[pos - dist + i % dist]; }
    void stored(uint32_t pos, uint32_t at, uint32_t len) { for (uint32_t i = 0; i < len; ++i) o[pos + i] = src[at + i]; }
    void sync() {} };
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    uint32_t hdr[4], table[256], x2n[32];
    for (uint32_t e = 0; e < 256; ++e) table[e] = uq_crc_table_entry(e);
    uq_crc_x2n_init(x2n);
    while (fread(hdr, 4, 4, f) == 4) {       /* comp_len, isize, crc, expected length (0xFFFFFFFF: none) */
        uint8_t* comp = (uint8_t*)malloc(hdr[0] ? hdr[0] : 1);
        uint8_t* want = (uint8_t*)malloc(hdr[3] != 0xFFFFFFFFu && hdr[3] ? hdr[3] : 1);
        if (fread(comp, 1, hdr[0], f) != hdr[0]) return 2;
        if (hdr[3] != 0xFFFFFFFFu && fread(want, 1, hdr[3], f) != hdr[3]) return 2;
        uint8_t* out = (uint8_t*)malloc(hdr[1] ? hdr[1] : 1);    /* exactly isize: a write past it is a heap overflow */
        UqInflateTables* t = (UqInflateTables*)malloc(sizeof(UqInflateTables));
        Src s{comp, hdr[0]};
        Out o{out, comp};
        int st = uq_inflate_core(s, hdr[0], o, hdr[1], t, 0, 1);
        if (st == 0) {
            uint32_t c0 = uq_crc0_bytes(table, 0, out, hdr[1]);
            if (uq_crc_finish(x2n, c0, hdr[1]) != hdr[2]) st = UQ_INF_CRC_MISMATCH;
        }
        int right = st == 0 && hdr[3] == hdr[1] && memcmp(out, want, hdr[1]) == 0;
        printf("%d %d\n", st, right);
        free(comp); free(want); free(out); free(t);
    }
    fclose(f);
    return 0;
}
'''


def _gxx():
    for c in ('g++', 'c++', 'clang++'):
        p = shutil.which(c)
        if p: return p
    return None


def test_decoder_fuzz_under_address_sanitizer(tmp_path):
    gxx = _gxx()
    if gxx is None:
        pytest.skip('no host C++ compiler')
    src = tmp_path / 'fuzz.cpp'
    src.write_text(DRIVER)
    exe = tmp_path / 'fuzz'
    subprocess.check_call([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                           os.path.dirname(CORE), str(src), '-o', str(exe)])
    cases = corrupt_cases(seed=23, count=4000)
    for _, d, data in member_matrix()[::7]:
        cases.append((d, len(data), zlib.crc32(data), data))
    ncorrupt = len(cases)
    for _, d, data in crafted_members():                              # valid deflate that zlib's compressor does not write, and
        cases.append((d, len(data), zlib.crc32(data), data))
    for _, d, isize, _ in crafted_invalid():                          # its nearest invalid neighbours
        cases.append((d, isize, 0, None))
    blob = bytearray()
    for stream, isize, crc, data in cases:
        blob += struct.pack('<IIII', len(stream), isize, crc, 0xFFFFFFFF if data is None else len(data)) + stream + (data or b'')
    (tmp_path / 'cases.bin').write_bytes(bytes(blob))
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:exitcode=99', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1:exitcode=98')
    r = subprocess.run([str(exe), str(tmp_path / 'cases.bin')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=600)
    assert r.returncode == 0 and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.split('\n')[:-1]
    assert len(lines) == len(cases)
    for (stream, isize, crc, data), line in zip(cases, lines):
        st, right = map(int, line.split())
        assert st != 0 or right, (len(stream), isize)
    assert sum(1 for l in lines[:ncorrupt] if l.split()[0] != '0') > ncorrupt // 2   # the corruptions mostly end in a status
    for (name, _, _), line in zip(crafted_members(), lines[ncorrupt:]):
        assert line == '0 1', name
    for (name, _, _, want), line in zip(crafted_invalid(), lines[ncorrupt + len(crafted_members()):]):
        assert line == '%d 0' % want, name


# ------------------------------------------------------------------ the sharded encoder
def test_sharded_encoder_refuses_gzip_before_any_setup(tmp_path, capsys, monkeypatch):
    from uq_amd import dist_encode
    p = tmp_path / 'in.fastq.gz'
    p.write_bytes(bgzf(fastq(50)))
    monkeypatch.setenv('UQ_DIST_BACKEND', 'no-such-backend')           # any set-up attempt would fail differently
    assert dist_encode.main(['-i', str(p)]) == 1
    assert 'sharded encoder reads plain FASTQ only' in capsys.readouterr().out
