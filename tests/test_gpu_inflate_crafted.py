"""The inflate kernels on the MI355X on valid deflate that zlib's compressor never writes, and on its nearest invalid neighbours (the
streams of tests/deflate_writer.py, each checked there against zlib's inflate): uq_inflate_members on every crafted member in one launch,
the parallel-chunk decoder on every crafted gzip file against zlib and against the host entry (output and driver counts), refusals with
the host entry's status and offset, and crafted FASTQ files through the CLI."""
import random
import zlib

import numpy as np
import pytest

from deflate_writer import (behind_valid_front, bgzf_wrap, crafted_invalid, crafted_members, crafted_streams, crafted_text_members,
                            gzip_wrap)
from test_gpu_gzip import _encode, _table
from test_gzip_cpu import BGZF_EOF, fastq
from uq_amd import ops, uq
from uq_amd._lib import call

pytestmark = pytest.mark.gpu
INFO_KEYS = ('starts', 'chunks', 'rounds', 'redecoded', 'overflows', 'members', 'out_bytes')


def _launch(ctx, cases):
    """uq_inflate_members on (raw, isize, crc) cases through the raw entry: (statuses, output bytes, bytes past the table's last member)"""
    comp, table, total = _table(cases)
    t = ctx.torch
    d_st = t.zeros(len(table), dtype=t.int32, device=ctx.device)
    out = t.zeros(total + 64, dtype=t.uint8, device=ctx.device)
    d_members = ctx.to_device(table.view(np.uint8))
    d_comp = ctx.bytes_to_device(comp)
    call('uq_inflate_members', ctx.h, ops._p(d_comp), d_comp.numel(), ops._p(d_members), len(table), ops._p(out), total, ops._p(d_st))
    host = ctx.to_numpy(out).tobytes()
    return list(ctx.to_numpy(d_st, np.int32)), host[:total], host[total:]


@pytest.mark.parametrize('order', ['forward', 'reverse'])
def test_crafted_members_in_one_launch(ctx, order):
    mem = crafted_members() if order == 'forward' else crafted_members()[::-1]      # reversed: other waves, other alignments
    cases = [(raw, len(data), zlib.crc32(data)) for _, raw, data in mem]
    want = b''.join(data for _, _, data in mem)
    ops.scribble_lds(ctx, 0x5A5A5A5A)
    comp, table, total = _table(cases)
    out, bad = ops.inflate_members(ctx, ctx.bytes_to_device(comp), table, total)
    assert bad is None, (mem[bad[0]][0], bad[1])
    assert ctx.to_numpy(out).tobytes() == want
    ops.scribble_lds(ctx, 0xC3C3C3C3)
    st, got, past = _launch(ctx, cases)
    assert [mem[k][0] for k, s in enumerate(st) if s] == []
    assert got == want and past == bytes(64)


def test_invalid_members_status_matches_host_decoder(ctx):
    cases = [(raw, isize, 0) for _, raw, isize, _ in crafted_invalid()]
    ops.scribble_lds(ctx)
    st, _, past = _launch(ctx, cases)
    assert st == [ops.inflate_member_host(raw, isize, crc)[0] for raw, isize, crc in cases] == [c[3] for c in crafted_invalid()]
    assert past == bytes(64)


def _dev(ctx, blob, chunk, starts=None):
    out, info = ops.gzip_stream_to_device(ctx, ctx.bytes_to_device(blob), chunk, starts)
    return ctx.to_numpy(out).tobytes(), info


@pytest.mark.parametrize('chunk', [1 << 10, 3000, 1 << 14])
def test_crafted_streams_match_zlib_and_the_host_entry(ctx, chunk):
    for name, blob, data in crafted_streams():
        got, dinfo = _dev(ctx, blob, chunk)
        assert got == data, (name, chunk)
        hout, hinfo = ops.gzip_stream_host(blob, chunk)
        assert hout == got, name
        for k in INFO_KEYS:
            assert dinfo[k] == hinfo[k], (name, chunk, k, dinfo[k], hinfo[k])


def test_crafted_streams_with_wrong_starts(ctx):
    rnd = random.Random(31)
    for name, blob, data in crafted_streams():
        starts = [rnd.randrange(1, 8 * len(blob)) << 2 | rnd.randrange(3) for _ in range(25)]
        assert _dev(ctx, blob, 1 << 12, starts)[0] == data, name


def test_invalid_streams_refused_like_the_host_entry(ctx):
    blobs = []
    for name, raw, isize, _ in crafted_invalid():
        blobs.append((name, gzip_wrap(raw, b'')[:-4] + isize.to_bytes(4, 'little')))
        if isize == 0:
            blobs.append((name + '/behind_valid_front', behind_valid_front(raw)))
    for name, blob in blobs:
        for chunk in (64, 256, 1 << 14):
            with pytest.raises(ops.GzipStreamError) as h:
                ops.gzip_stream_host(blob, chunk)
            with pytest.raises(ops.GzipStreamError) as d:
                _dev(ctx, blob, chunk)
            assert (d.value.status, d.value.offset) == (h.value.status, h.value.offset), (name, chunk)


@pytest.mark.parametrize('kind', ['deep', 'fixed'])
def test_cli_on_crafted_fastq_files(ctx, tmp_path, monkeypatch, kind):
    """FASTQ text tokenised into crafted blocks -- 'deep': matches at distance 32 768 and 15-bit codes; 'fixed': fixed blocks only, across
    the chunks of the stream decoder -- as BGZF and as plain multi-member gzip: the same .uQ members as the plain text gives."""
    monkeypatch.setattr(uq, 'GZIP_STREAM_CHUNK', 1 << 10)
    fq = fastq(700)
    members = crafted_text_members(fq, kind, 49152 if kind == 'deep' else 65280)
    assert len(members) >= 3
    cfg0, plain, _ = _encode(ctx, tmp_path, fq, [], name='in.fastq')
    cfg, got, s = _encode(ctx, tmp_path, b''.join(bgzf_wrap(r, d) for r, d in members) + BGZF_EOF, [])
    assert s.gzip_path.startswith('BGZF') and got == plain and cfg == cfg0
    cfg, got, s = _encode(ctx, tmp_path, b''.join(gzip_wrap(r, d) for r, d in members), [])
    assert s.gzip_path.startswith('gzip, ') and 'inflated on the device' in s.gzip_path and got == plain and cfg == cfg0
