"""gzip that is not BGZF, inflated on the MI355X in parallel chunks (uq_gzip_stream_*): the device output against zlib and the host entry
over the stream matrix at several chunk sizes and with wrong chunk starts, refusals against the host zlib path (Staging.gzip_to_device),
slot overflow, the CLI on every golden fixture as single- and multi-member gzip, and a single member of more than 4 GiB of output."""
import gzip
import json
import os
import random
import struct
import zlib

import numpy as np
import pytest

from test_gpu_gzip import GOLD, REFUSED, WRITTEN, _encode
from test_gzip_stream_cpu import _flush_starts, corrupt_streams, fastq, host_path, stream_matrix
from uq_amd import ops, synth, uq

pytestmark = pytest.mark.gpu


def _dev(ctx, blob, chunk, starts=None):
    out, info = ops.gzip_stream_to_device(ctx, ctx.bytes_to_device(blob) if blob else ctx.torch.empty(0, dtype=ctx.torch.uint8,
                                                                                                       device=ctx.device), chunk, starts)
    return ctx.to_numpy(out).tobytes(), info


@pytest.mark.parametrize('chunk', [1 << 10, 3000, 1 << 14, 1 << 18])
def test_device_stream_matches_zlib_and_host_entry(ctx, chunk):
    for name, blob, data in stream_matrix():
        got, info = _dev(ctx, blob, chunk)
        assert got == data, (name, chunk)
        assert ops.gzip_stream_host(blob, chunk)[0] == got, name
        assert info['out_bytes'] == len(data)


def test_device_finder_agrees_with_the_host_finder(ctx):
    # a wrong start only costs time, so output equality cannot see a broken finder: the device finder must find the same starts as the host
    # one (the same predicates), which shows in the chunk and round counts of the two drivers
    from test_gzip_stream_cpu import _binned, pigz_like
    data = fastq(3000)
    for blob, chunk in ((pigz_like(data), 1 << 12), (gzip.compress(data, 6), 1 << 12), (gzip.compress(_binned(20000, 0.15), 6), 1 << 14)):
        got, dinfo = _dev(ctx, blob, chunk)
        hout, hinfo = ops.gzip_stream_host(blob, chunk)
        assert got == hout
        for k in ('starts', 'chunks', 'rounds', 'redecoded', 'overflows', 'members', 'out_bytes'):
            assert dinfo[k] == hinfo[k], (k, dinfo[k], hinfo[k])
        assert dinfo['chunks'] > 5


def test_device_stream_with_wrong_starts(ctx):
    data = fastq(2500)
    blob, true = _flush_starts(data)
    rnd = random.Random(5)
    nbits = 8 * len(blob)
    for starts in (true, true[::3], [((s >> 2) + 1) << 2 | (s & 3) for s in true], [rnd.randrange(1, nbits) << 2 | rnd.randrange(3) for _ in range(50)]):
        got, info = _dev(ctx, blob, 1 << 12, starts)
        assert got == data
        assert ops.gzip_stream_host(blob, 1 << 12, starts=starts)[0] == got
    for name, b2, d2 in stream_matrix()[::2]:
        starts = [rnd.randrange(1, 8 * len(b2)) << 2 | rnd.randrange(3) for _ in range(25)]
        assert _dev(ctx, b2, 1 << 12, starts)[0] == d2, name


def test_device_refusals_match_the_host_zlib_path(ctx, tmp_path):
    from uq_amd.hostio import Staging
    io = Staging(ctx)
    p = tmp_path / 'c.gz'
    for i, blob in enumerate(corrupt_streams(seed=77, count=120)):
        p.write_bytes(blob)
        try:
            want = ctx.to_numpy(io.gzip_to_device(str(p))).tobytes()
        except (zlib.error, EOFError):
            want = None
        try:
            got = _dev(ctx, blob, (1 << 10) if i % 2 else (1 << 14))[0]
        except ops.GzipStreamError as e:
            assert 'at byte %d' % e.offset in str(e)
            got = None
        assert got == want, i


def test_slot_overflow_is_decoded_again(ctx):
    reads = b''.join(b'@r%d\n%s\n+\n%s\n' % (i, b'N' * 150, b'!' * 150) for i in range(40000))
    blob = gzip.compress(reads, 9)
    got, info = _dev(ctx, blob, 1 << 10)
    assert got == reads
    assert info['overflows'] > 0 and info['rounds'] > 1


@pytest.mark.parametrize('form', ['single', 'multi'])
@pytest.mark.parametrize('name', WRITTEN)
def test_cli_on_golden_fixtures(ctx, tmp_path, monkeypatch, name, form):
    monkeypatch.setattr(uq, 'GZIP_STREAM_CHUNK', 1 << 10)
    meta = json.load(open(os.path.join(GOLD, name + '.json')))
    fq = open(os.path.join(GOLD, name + '.fastq'), 'rb').read()
    third = len(fq) // 3
    blob = gzip.compress(fq, 6) if form == 'single' else b''.join(gzip.compress(x) for x in (fq[:third], fq[third:2 * third], fq[2 * third:]))
    cfg, members, s = _encode(ctx, tmp_path, blob, meta['flags'])
    assert s.gzip_path.startswith('gzip, ') and 'inflated on the device' in s.gzip_path
    cfg2, members2, _ = _encode(ctx, tmp_path, fq, meta['flags'], name='in.fastq')
    assert members2 == members and cfg2 == cfg


@pytest.mark.parametrize('name', REFUSED)
def test_cli_refused_fixtures_like_plain(ctx, tmp_path, monkeypatch, name):
    from uq_amd import qname
    monkeypatch.setattr(uq, 'GZIP_STREAM_CHUNK', 1 << 10)
    meta = json.load(open(os.path.join(GOLD, name + '.json')))
    fq = open(os.path.join(GOLD, name + '.fastq'), 'rb').read()
    with pytest.raises((uq.UqError, qname.QnameError)) as plain:
        _encode(ctx, tmp_path, fq, meta['flags'], name='in.fastq')
    for blob in (gzip.compress(fq), gzip.compress(fq[:len(fq) // 2]) + gzip.compress(fq[len(fq) // 2:])):
        with pytest.raises((uq.UqError, qname.QnameError)) as comp:
            _encode(ctx, tmp_path, blob, meta['flags'])
        assert type(comp.value) is type(plain.value) and str(comp.value) == str(plain.value)


def test_cli_host_inflate_flag_takes_the_host_path(ctx, tmp_path):
    fq = fastq(300)
    cfg, members, s = _encode(ctx, tmp_path, gzip.compress(fq), ['--host-inflate'])
    assert s.gzip_path == 'gzip inflated on the host'
    cfg2, members2, s2 = _encode(ctx, tmp_path, gzip.compress(fq), [])
    assert s2.gzip_path.startswith('gzip, ') and members2 == members and cfg2 == cfg
    with pytest.raises(uq.UqError) as e:
        _encode(ctx, tmp_path, gzip.compress(fq)[:-50], [])
    assert 'not a readable gzip file' in str(e.value) and 'at byte' in str(e.value)


def test_single_member_past_4_gib_on_the_device(ctx):
    """One gzip member of synthetic FASTQ of more than 4 GiB: stored blocks across 2^31 and 2^32 (compressed and output offsets), then a
    level-1 tail; ISIZE wraps mod 2^32.  Inflated on the device = the generator's bytes."""
    t = ctx.torch
    spec = synth.Spec(20261016, 150)
    n = 13_000_000
    d_ref = ops.synth_fastq(ctx, spec, 0, n)
    size = d_ref.numel()
    assert size > (1 << 32) + (64 << 20)
    host = d_ref.cpu().numpy()
    blk = 65535
    stored = ((1 << 32) + (32 << 20)) // blk * blk
    nst = stored // blk
    head = np.empty((nst, 5 + blk), dtype=np.uint8)
    head[:, :5] = np.frombuffer(b'\x00' + blk.to_bytes(2, 'little') + (blk ^ 0xFFFF).to_bytes(2, 'little'), dtype=np.uint8)
    head[:, 5:] = host[:stored].reshape(nst, blk)
    c = zlib.compressobj(1, zlib.DEFLATED, -15, 8)
    tail = c.compress(host[stored:].tobytes()) + c.flush()
    crc = zlib.crc32(memoryview(host))
    hdr = b'\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03'
    trailer = struct.pack('<II', crc, size & 0xFFFFFFFF)
    total = len(hdr) + head.size + len(tail) + len(trailer)
    d_comp = t.empty(total, dtype=t.uint8, device=ctx.device)
    d_comp[:len(hdr)].copy_(t.from_numpy(np.frombuffer(hdr, dtype=np.uint8).copy()))
    d_comp[len(hdr):len(hdr) + head.size].copy_(t.from_numpy(head.reshape(-1)))
    rest = np.frombuffer(tail + trailer, dtype=np.uint8).copy()
    d_comp[len(hdr) + head.size:].copy_(t.from_numpy(rest))
    del head, host
    out, info = ops.gzip_stream_to_device(ctx, d_comp, uq.GZIP_STREAM_CHUNK)
    del d_comp
    assert info['members'] == 1 and info['out_bytes'] == size and info['chunks'] > 1000
    assert t.equal(out, d_ref)
