"""gzip that is not BGZF, inflated in parallel chunks: the host entry (uq_gzip_stream_host) runs the finder, chunk decoder, chain check and
marker resolution of inflate_stream.h serially on the CPU.  Its output is compared with zlib over levels, strategies, flushes, pigz-style
streams and multi-member files at many chunk sizes; wrong chunk starts must never change the output; corrupt streams are refused whenever
the host zlib path refuses them; and a g++ AddressSanitizer/UBSan driver runs the header on corrupt streams and random starts."""
import gzip
import os
import random
import struct
import subprocess
import zlib

import pytest

from deflate_writer import behind_valid_front, crafted_invalid, crafted_members, crafted_streams, gzip_wrap
from test_gzip_cpu import _gxx, bgzf, gzip_member, raw_deflate
from uq_amd import ops, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'uq_amd', 'csrc')
STRATEGIES = {'default': zlib.Z_DEFAULT_STRATEGY, 'filtered': zlib.Z_FILTERED, 'huffman_only': zlib.Z_HUFFMAN_ONLY, 'rle': zlib.Z_RLE,
              'fixed': zlib.Z_FIXED}


def fastq(n=2000, seed=5):
    return synth.fastq(seed, n, (36, 151), n_rate=1)


def gz(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=()):
    """One gzip member (no BSIZE) of raw deflate made with the given level / strategy / flush points."""
    return (b'\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03' + raw_deflate(data, level, strategy, flushes) +
            struct.pack('<II', zlib.crc32(data), len(data) & 0xFFFFFFFF))


def pigz_like(data, piece=16384, level=6):
    """What pigz writes: pieces deflated independently, each with the previous 32 KiB as its dictionary, Z_SYNC_FLUSH between them, into
    one member: back-references cross the pieces."""
    out = []
    for i in range(0, len(data), piece):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, *( (data[max(0, i - 32768):i],) if i else ()))
        out.append(c.compress(data[i:i + piece]))
        out.append(c.flush(zlib.Z_SYNC_FLUSH if i + piece < len(data) else zlib.Z_FINISH))
    return (b'\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03' + b''.join(out) + struct.pack('<II', zlib.crc32(data), len(data) & 0xFFFFFFFF))


def host_path(blob):
    """What Staging.gzip_to_device computes (zlib member after member); raises zlib.error / EOFError where it refuses."""
    out, buf = [], blob
    while True:
        d = zlib.decompressobj(31)
        out.append(d.decompress(buf))
        if not d.eof:
            raise EOFError('the gzip stream ends inside a member')
        buf = d.unused_data
        if not buf:
            return b''.join(out)


def stream_matrix():
    """(name, gzip file, expected output)"""
    data = fastq(1500)
    rnd = random.Random(3)
    rand = bytes(rnd.getrandbits(8) for _ in range(60000))
    out = []
    for level in range(10):
        for sname, s in STRATEGIES.items():
            if level in (0, 1, 6, 9) or sname == 'default':
                out.append(('l%d/%s' % (level, sname), gz(data, level, s), data))
    for mode in (zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH):
        cuts = [(k, mode) for k in range(7000, len(data), 23000)]
        out.append(('flush%d' % mode, gz(data, 6, flushes=cuts), data))
    out.append(('pigz', pigz_like(data), data))
    out.append(('pigz_small_pieces', pigz_like(data, 4096, 9), data))
    out.append(('random', gz(rand, 6), rand))
    out.append(('one_byte', gz(b'G' * 300000, 9), b'G' * 300000))
    parts = [fastq(300, s) for s in range(4)]
    out.append(('multi', b''.join(gzip.compress(p, 6) for p in parts), b''.join(parts)))
    out.append(('multi_with_empty', gzip.compress(parts[0]) + gzip.compress(b'') + gzip.compress(parts[1]) + gzip.compress(b''),
                parts[0] + parts[1]))
    out.append(('bgzf_then_plain', bgzf(data, eof=False) + gzip.compress(parts[2]), data + parts[2]))
    out.append(('header_fields', gzip_member(parts[3], extra=b'XY\x03\x00abc', name=b'r.fq', comment=b'c', hcrc=True), parts[3]))
    out.append(('empty', gzip.compress(b''), b''))
    return out


CHUNKS = [1 << 10, 3000, 1 << 14, 1 << 20]


@pytest.mark.parametrize('chunk', CHUNKS)
def test_host_stream_matches_zlib_on_the_matrix(chunk):
    for name, blob, data in stream_matrix():
        assert host_path(blob) == data, name
        out, info = ops.gzip_stream_host(blob, chunk)
        assert out == data, (name, chunk)
        assert info['out_bytes'] == len(data) and info['chunks'] >= 1


def test_small_chunks_give_many_chunks_and_windows_across_chunks():
    data = fastq(3000)
    blob = pigz_like(data, 4096)
    out, info = ops.gzip_stream_host(blob, 1 << 10)
    assert out == data
    assert info['chunks'] > 20 and info['resolve_rounds'] >= 1


def _flush_starts(data, piece=5000):
    """A stream with a full flush every `piece` bytes and the canonical positions of the empty stored blocks the flushes wrote."""
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
    body, starts = bytearray(), []
    for i in range(0, len(data), piece):
        body += c.compress(data[i:i + piece])
        body += c.flush(zlib.Z_FULL_FLUSH)
        starts.append(8 * (10 + len(body) - 4) << 2 | ops.GZS_UNCOMPRESSED)       # LEN of the 00 00 ff ff block
    body += c.flush()
    blob = b'\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03' + bytes(body) + struct.pack('<II', zlib.crc32(data), len(data))
    return blob, starts


def test_any_starts_give_the_zlib_answer():
    data = fastq(2500)
    blob, true = _flush_starts(data)
    rnd = random.Random(17)
    nbits = 8 * len(blob)
    cases = {
        'true': true,
        'every_other_true': true[::2],
        'one_bit_off': [((s >> 2) + d) << 2 | k for s in true for d in (-1, 1) for k in (0, 1, 2)],
        'random': [rnd.randrange(1, nbits) << 2 | rnd.randrange(3) for _ in range(60)],
        'random_bytes': [rnd.randrange(1, len(blob)) * 8 << 2 | rnd.randrange(3) for _ in range(60)],
        'mixed': sorted(true[1::3] + [rnd.randrange(1, nbits) << 2 | 2 for _ in range(20)]),
        'none': [],
    }
    for name, starts in cases.items():
        out, info = ops.gzip_stream_host(blob, 1 << 12, starts=starts)
        assert out == data, name
    out, info = ops.gzip_stream_host(blob, 1 << 12, starts=true)
    assert info['rounds'] == 1 and info['chunks'] == len(true) + 1             # true starts: one round, every chunk kept
    for name, blob2, data2 in stream_matrix()[::3]:
        nb = 8 * len(blob2)
        starts = [rnd.randrange(1, nb) << 2 | rnd.randrange(3) for _ in range(30)]
        assert ops.gzip_stream_host(blob2, 1 << 12, starts=starts)[0] == data2, name


def corrupt_streams(seed=11, count=600):
    """(gzip file) : bit flips, truncations, smeared bytes, trailing bytes, on the matrix's files."""
    rnd = random.Random(seed)
    base = [blob for _, blob, _ in stream_matrix() if 0 < len(blob) < 400000]
    out = []
    for i in range(count):
        b = bytearray(base[rnd.randrange(len(base))])
        k = i % 5
        if k == 0:
            for _ in range(rnd.randint(1, 3)): b[rnd.randrange(len(b))] ^= 1 << rnd.randrange(8)
        elif k == 1:
            b = b[:rnd.randrange(1, len(b))]
        elif k == 2:
            at = rnd.randrange(len(b)); n = rnd.randint(1, 16)
            b[at:at + n] = bytes(rnd.getrandbits(8) for _ in range(min(n, len(b) - at)))
        elif k == 3:
            b += bytes(rnd.getrandbits(8) for _ in range(rnd.randint(1, 20))) if rnd.random() < 0.5 else b'\x00' * rnd.randint(1, 20)
        else:
            b[-8 + rnd.randrange(8)] ^= 1 << rnd.randrange(8)            # the trailer
        out.append(bytes(b))
    return out


def test_corrupt_streams_refused_like_the_host_path():
    refused = 0
    for i, blob in enumerate(corrupt_streams()):
        try:
            want = host_path(blob)
        except (zlib.error, EOFError):
            want = None
        try:
            got = ops.gzip_stream_host(blob, (1 << 10) if i % 2 else (1 << 14))[0]
        except ops.GzipStreamError as e:
            assert 'at byte %d' % e.offset in str(e)
            got = None
        assert got == want, i
        refused += want is None
    assert refused > 300


def test_refusals_name_the_byte_offset():
    data = fastq(500)
    blob = gzip.compress(data)
    with pytest.raises(ops.GzipStreamError) as e:
        ops.gzip_stream_host(blob[:-100], 1 << 12)
    assert e.value.status == 1 and 'truncated' in str(e.value)
    bad = bytearray(blob); bad[-8] ^= 1
    with pytest.raises(ops.GzipStreamError) as e:
        ops.gzip_stream_host(bytes(bad), 1 << 12)
    assert e.value.status == 10 and e.value.offset == len(blob) - 8 and 'at byte %d' % (len(blob) - 8) in str(e.value)
    bad = bytearray(blob); bad[-4] ^= 1
    with pytest.raises(ops.GzipStreamError) as e:
        ops.gzip_stream_host(bytes(bad), 1 << 12)
    assert e.value.status == 9 and e.value.offset == len(blob) - 8
    with pytest.raises(ops.GzipStreamError) as e:
        ops.gzip_stream_host(blob + b'junk', 1 << 12)
    assert e.value.status == 13 and e.value.offset == len(blob)
    # a back-reference before the start of its member (the second member reaches into the first): zlib's "distance too far back"
    b = gzip.compress(b'ACGT' * 100)
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, b'ACGT' * 100)
    tail = c.compress(b'ACGT' * 50) + c.flush()
    second = b'\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03' + tail + struct.pack('<II', zlib.crc32(b'ACGT' * 50), 200)
    with pytest.raises(zlib.error):
        host_path(b + second)
    for starts in (None, [8 * len(b) << 2 | ops.GZS_MEMBER], [(8 * (len(b) + 10)) << 2 | ops.GZS_DYNAMIC]):
        with pytest.raises(ops.GzipStreamError) as e:
            ops.gzip_stream_host(b + second, 1 << 12, starts=starts)
        assert 'too far back' in str(e.value)


def test_wrong_start_into_the_previous_member_is_only_a_bad_start():
    # a speculative chunk that starts mid-stream and references its (unknown) window is fine; the chain check keeps the output right
    parts = [fastq(400, s) for s in range(3)]
    blob = b''.join(gzip.compress(p) for p in parts)
    for chunk in (256, 1000, 5000):
        assert ops.gzip_stream_host(blob, chunk)[0] == b''.join(parts)


DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "inflate_stream.h"
struct Src { const uint8_t* p; uint64_t len;
    uint32_t word(uint64_t off) const { uint32_t v = 0; for (uint32_t k = 0; k < 4; ++k) if (off + k < len) v |= (uint32_t)p[off + k] << (8 * k); return v; }
    uint32_t byte(uint64_t o) const { return o < len ? p[o] : 0u; } };
struct Env { void order() {} bool any(bool b) { return b; } void sync() {} void store16(uint8_t* d, const uint32_t* w) { memcpy(d, w, 16); } };
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    uint32_t table[256];
    for (uint32_t e = 0; e < 256; ++e) table[e] = uq_crc_table_entry(e);
    uint64_t hdr[3];                         /* comp_len, start (packed), stop bit */
    Env env;
    while (fread(hdr, 8, 3, f) == 3) {
        uint8_t* comp = (uint8_t*)malloc(hdr[0] ? hdr[0] : 1);
        if (fread(comp, 1, hdr[0], f) != hdr[0]) return 2;
        Src s{comp, hdr[0]};
        UqGzsProbe* p = (UqGzsProbe*)malloc(sizeof(UqGzsProbe));
        uint64_t found = uq_gzs_find(s, hdr[0], 0, 8 * hdr[0], p);
        UqInflateTables* t = (UqInflateTables*)malloc(sizeof(UqInflateTables));
        uint16_t* ring = (uint16_t*)malloc(2 * UQ_GZS_RING);
        uint64_t cap = 64 * 1024;             /* small: overflow is exercised too */
        uint8_t* slot = (uint8_t*)aligned_alloc(64, cap);
        UqGzsChunk c; memset(&c, 0, sizeof c);
        c.start = hdr[1]; c.stop = hdr[2]; c.slot = (uint64_t)(uintptr_t)slot; c.cap = cap;
        uq_gzs_chunk(s, hdr[0], &c, ring, t, table, 0u, 1u, env);
        printf("%u %llu %llu %llu\n", c.status, (unsigned long long)c.len, (unsigned long long)c.end, (unsigned long long)found);
        free(comp); free(p); free(t); free(ring); free(slot);
    }
    fclose(f);
    return 0;
}
'''


def test_stream_decoder_under_address_sanitizer(tmp_path):
    gxx = _gxx()
    if gxx is None:
        pytest.skip('no host C++ compiler')
    src = tmp_path / 'fuzz.cpp'
    src.write_text(DRIVER)
    exe = tmp_path / 'fuzz'
    subprocess.check_call([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', CSRC,
                           str(src), '-o', str(exe)])
    rnd = random.Random(29)
    blob = bytearray()
    ncases = 0
    streams = corrupt_streams(seed=41, count=300) + [b for _, b, _ in stream_matrix()[::4]]
    nold = 3 * len(streams)
    # valid deflate that zlib's compressor does not write (whole and from random starts), and its invalid neighbours, alone and behind
    # a valid front
    valid = [(b, data) for _, b, data in crafted_streams()] + [(gzip_wrap(raw, data), data) for _, raw, data in crafted_members()[::4]]
    streams += [b for b, _ in valid]
    streams += [gzip_wrap(raw, b'') for _, raw, _, _ in crafted_invalid()] + [behind_valid_front(raw) for _, raw, isize, _ in crafted_invalid()
                                                                               if isize == 0]
    to_the_end = []                          # per case: does it run to the end of its whole stream?
    for s in streams:
        whole = len(s) <= 150000
        s = s[:150000]
        nb = 8 * len(s)
        for start in (0, rnd.randrange(nb) << 2 | rnd.randrange(3), rnd.randrange(max(1, len(s))) * 8 << 2 | rnd.randrange(2)):
            stop = rnd.choice([(1 << 64) - 1, rnd.randrange(nb + 64)])
            to_the_end.append(whole and stop == (1 << 64) - 1)
            blob += struct.pack('<QQQ', len(s), start, stop) + s
            ncases += 1
    (tmp_path / 'cases.bin').write_bytes(bytes(blob))
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:exitcode=99', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1:exitcode=98')
    r = subprocess.run([str(exe), str(tmp_path / 'cases.bin')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=900)
    assert r.returncode == 0 and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.split('\n')[:-1]
    assert len(lines) == ncases
    statuses = [int(l.split()[0]) for l in lines]
    old = statuses[:nold]
    assert any(s == 0 for s in old) and any(s == 14 for s in old) and sum(1 for s in old if s not in (0, 14)) > nold // 4
    # the valid crafted streams from their header: nothing but the end, `stop` or a full slot ends them.  A chunk from a member header
    # writes bytes, so 65 536 bytes of slot hold 60 000 of output and its few member records, and do not hold more than 65 536.
    for k, (_, data) in enumerate(valid):
        st = statuses[nold + 3 * k]
        assert st in (0, 14), (k, st)
        if to_the_end[nold + 3 * k] and len(data) <= 60000: assert st == 0, (k, st)
        if to_the_end[nold + 3 * k] and len(data) > 65536: assert st == 14, (k, st)


def _binned(n, p):
    import sys
    tools = os.path.join(REPO, 'tools')
    if tools not in sys.path: sys.path.insert(0, tools)
    import bench_inflate
    return bench_inflate.binned_fastq(n, 7, p)


@pytest.mark.parametrize('p', [0.05, 0.3])
def test_real_ratio_fastq_fits_the_first_slot(p):
    # FASTQ that compresses like a real run's (3.8x - 5x): the markers live to each chunk's end, so the slots stay u16; the first slot must
    # hold that, so no chunk overflows and at most the finder's false positives cost a second round
    data = _binned(40000, p)
    blob = gzip.compress(data, 6)
    assert len(data) / len(blob) > 3.5
    out, info = ops.gzip_stream_host(blob, 1 << 18)
    assert out == data
    assert info['chunks'] > 8 and info['overflows'] == 0 and info['rounds'] <= 2 and info['redecoded'] <= 3


def test_overflowed_slot_is_sized_from_the_ratio_seen():
    # 1 000x compression: the first slot is far too small; the second is sized from how far the first lasted, so each chunk is decoded at
    # most a few times rather than once per doubling
    data = b'@r\n' + b'A' * 3_000_000 + b'\n+\n' + b'F' * 3_000_000 + b'\n'
    blob = gzip.compress(data, 9)
    out, info = ops.gzip_stream_host(blob, 1 << 10)
    assert out == data
    assert info['overflows'] >= 1 and info['rounds'] == 2                      # doubling from 176 KiB to ~3 MB would take 5 rounds
