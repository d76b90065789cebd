"""The --test sizer on the MI355X: uq_deflate_size against the host definition S (the members uq_bgzf_compress_block_host writes, block by
block) on pattern payloads and 1-D members, queued and one at a time, past 4 GiB against uq_bgzf_compress, and the CLI's
`--test --device-compressor` against `--test --compressor "python -m uq_amd.bgzf_host --no-eof"`: the same report, the same container,
no subprocess and nothing but the totals copied to the host."""
import io
import json
import os
import re
import sys
import tarfile

import numpy as np
import pytest

from test_deflate_cpu import BLOCK, REPO
from test_gpu_gzip import GOLD
from test_gpu_tables import SHAPES
from test_sizer_cpu import S
from uq_amd import ops, synth, uq

pytestmark = pytest.mark.gpu


def _payload(T, pat):
    """The bytes numpy.save writes after the header for pattern `pat` of table T: rot90, then C or F order."""
    a = np.rot90(T, int(pat[0]))
    return (np.ascontiguousarray(a) if pat.endswith('.1') else np.asfortranarray(a)).tobytes(order='A')


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_device_total_equals_host_size_on_pattern_payloads(ctx, shape):
    R, C = shape
    T = np.random.RandomState(R * 131 + C).randint(0, 4, size=(R, C)).astype(np.uint8) * 37      # compressible: dynamic blocks
    if R * C > 1000: T[::7] = np.random.RandomState(C).randint(0, 256, size=T[::7].shape)
    d_T = ctx.to_device(T.ravel())
    q = ops.DeflateSizes(ctx, len(uq.PATTERNS))
    want = []
    for pat in uq.PATTERNS:
        header = uq.pattern_header(R, C, pat)
        payload = ops.pattern(ctx, d_T, R, C, pat)
        assert ctx.to_numpy(payload).tobytes() == _payload(T, pat), pat
        q.add(header, payload)
        want.append(S(header + _payload(T, pat)))
    assert q.fetch() == want


@pytest.mark.parametrize('itemsize', [1, 2, 4, 8])
def test_one_dimensional_members(ctx, itemsize):
    dtype = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[itemsize]
    for n in (1, 1000, 70001):
        a = (np.arange(n, dtype=np.uint64) * 2654435761 % 5003).astype(dtype)
        header = uq.npy_header(a.shape, False, a.dtype)
        assert ops.deflate_size(ctx, header, ctx.to_device(a)) == S(header + a.tobytes()), n


def test_empty_array_and_nothing(ctx):
    header = uq.npy_header((0,), False, np.uint32)
    assert ops.deflate_size(ctx, header, ctx.empty(0)) == S(header) > 0
    assert ops.deflate_size(ctx, b'', ctx.empty(0)) == 0


def test_last_block_of_one_byte(ctx):
    R, C = 5671, 23
    header = uq.pattern_header(R, C, '0.1')
    assert (len(header) + R * C) % BLOCK == 1
    T = np.random.RandomState(9).randint(0, 5, size=(R, C)).astype(np.uint8)
    assert ops.deflate_size(ctx, header, ctx.to_device(T.ravel())) == S(header + T.tobytes())


def test_misaligned_buffers_and_odd_prefixes(ctx):
    data = synth.fastq(20261005, 1500, (36, 301))
    back = ctx.empty(len(data) + 64)
    for off, plen in [(0, 0), (1, 0), (0, 1), (3, 17), (16, 128), (5, 256), (16, 255)]:
        d = back[off:off + len(data)]
        d.copy_(ctx.bytes_to_device(data))
        prefix = bytes(range(plen))
        assert ops.deflate_size(ctx, prefix, d) == S(prefix + data), (off, plen)


def test_queued_totals_equal_one_at_a_time(ctx):
    rs = np.random.RandomState(4)
    bufs = [(bytes(rs.randint(32, 127, size=k % 200).astype(np.uint8)), rs.randint(0, 1 + k % 7, size=40000 * (k + 1)).astype(np.uint8)) for k in range(8)]
    dev = [ctx.to_device(b) for _, b in bufs]
    q = ops.DeflateSizes(ctx, 8)
    for (prefix, _), d in zip(bufs, dev): q.add(prefix, d)
    queued = q.fetch()
    assert queued == [ops.deflate_size(ctx, prefix, d) for (prefix, _), d in zip(bufs, dev)]
    assert queued == [S(prefix + b.tobytes()) for prefix, b in bufs]
    # one buffer reused behind every call, as test_patterns does
    q = ops.DeflateSizes(ctx, 8)
    buf = ctx.empty(max(d.numel() for d in dev))
    for (prefix, _), d in zip(bufs, dev):
        buf[:d.numel()].copy_(d)
        q.add(prefix, buf[:d.numel()])
    assert q.fetch() == queued
    with pytest.raises(ValueError):
        q.add(b'', dev[0])                                          # full


def test_total_past_4_gib_equals_the_compressor_output(ctx):
    """4.3 GB of random bytes (stored members) and synthetic reads behind them (dynamic members): the total passes 2^32."""
    t = ctx.torch
    g = t.Generator(device=ctx.device)
    g.manual_seed(20261016)
    head = (1 << 32) + (40 << 20)
    tail = ops.synth_fastq(ctx, synth.Spec(20261005, 150), 0, 300000)
    src = t.empty(head + tail.numel(), dtype=t.uint8, device=ctx.device)
    src[:head] = t.randint(0, 256, (head,), dtype=t.uint8, device=ctx.device, generator=g)
    src[head:] = tail
    del tail
    want = ops.bgzf_compress(ctx, src, eof=False).numel()
    assert want > 1 << 32
    assert ops.deflate_size(ctx, b'', src) == want


# ------------------------------------------------------------------ the CLI
HOST_COMMAND = '%s -m uq_amd.bgzf_host --no-eof' % sys.executable


def _cli(ctx, tmp_path, fq, flags, tag):
    inp = tmp_path / 'in.fastq'
    inp.write_bytes(fq)
    out = tmp_path / (tag + '.uQ')
    args = uq.build_parser().parse_args(['-i', str(inp), '-o', str(out)] + flags)
    uq.validate_args(args)
    report = io.StringIO()
    s = uq.Session(args, ctx=ctx, out=report)
    s.encode()
    with tarfile.open(out) as t:
        members = {m.name: t.extractfile(m).read() for m in t.getmembers()}
    lines = [re.sub(r'\(\S+ minutes\)\s*', '', l) for l in report.getvalue().split('\n')]          # the time column
    return lines, json.loads(members.pop('config.json').decode()), members, s


def _both_ways(ctx, tmp_path, monkeypatch, fq, flags):
    monkeypatch.setenv('PYTHONPATH', REPO + os.pathsep + os.environ.get('PYTHONPATH', ''))
    dev = _cli(ctx, tmp_path, fq, ['--test', '--device-compressor'] + flags, 'dev')
    host = _cli(ctx, tmp_path, fq, ['--test', '--compressor', HOST_COMMAND] + flags, 'host')
    assert dev[3].last_subprocess_used == 0 and host[3].last_subprocess_used > 0
    assert dev[0] == host[0]                                        # the report, line for line
    assert any(l.startswith('Size (compressed)') for l in dev[0]) and any('Parameters found to be the best' in l for l in dev[0])
    assert dev[1] == host[1] and dev[2] == host[2]                  # config.json and every member
    return dev


def _golden(name):
    return open(os.path.join(GOLD, name + '.fastq'), 'rb').read()


@pytest.mark.parametrize('name', ['var_tiny_alphabets', 'qn_u4_u8_negative'])
def test_cli_full_grid_equals_the_host_command(ctx, tmp_path, monkeypatch, name):
    lines, cfg, members, s = _both_ways(ctx, tmp_path, monkeypatch, _golden(name), [])
    assert sum(bool(re.match(r'\s+\d+\s+(DNA|QUAL|QNAME|None)\s', l)) for l in lines) == 32        # 8 raw sets x 4 sorts


@pytest.mark.parametrize('name,flags', [
    ('variable_ntrick', ['--sort', 'None', '--raw', 'DNA', 'QUAL', 'QNAME']),
    ('qn_illumina_comment', ['--raw', 'QUAL']),
    ('nosort_keyed', ['--sort', 'DNA', '--pattern', '1.1', '2.2']),
    ('cfg1_10k_100bp', ['--sort', 'None', '--raw', 'DNA', 'QUAL', 'QNAME', '--pattern', '3.2', '0.2']),
    ('qn_u4_u8_negative', ['--sort', 'QNAME', '--raw', 'None']),
], ids=lambda v: v if isinstance(v, str) else '_'.join(v).replace('--', ''))
def test_cli_restricted_equals_the_host_command(ctx, tmp_path, monkeypatch, name, flags):
    _both_ways(ctx, tmp_path, monkeypatch, _golden(name), flags)


def test_peek_behaves_as_with_a_compressor(ctx, tmp_path):
    lines, out = {}, tmp_path / 'peek.uQ'
    (tmp_path / 'in.fastq').write_bytes(_golden('variable_ntrick'))
    for tag, flags in (('dev', ['--device-compressor']), ('host', ['--compressor', 'gzip -1'])):
        args = uq.build_parser().parse_args(['-i', str(tmp_path / 'in.fastq'), '-o', str(out), '--peek', '--test'] + flags)
        uq.validate_args(args)
        report = io.StringIO()
        uq.Session(args, ctx=ctx, out=report).encode()
        lines[tag] = re.sub(r'\(\S+ minutes\)', '', report.getvalue())                  # the time column
    assert lines['dev'] == lines['host'] and 'The config.json would look like' in lines['dev'] and not out.exists()


def _test_phase_traffic(ctx, tmp_path, monkeypatch, nreads):
    """run_tests of one mix with all layouts: (bytes ctx.to_numpy returned, candidates sized, subprocesses)."""
    inp = tmp_path / ('in%d.fastq' % nreads)
    inp.write_bytes(synth.fastq(20261005, nreads, 150))
    args = uq.build_parser().parse_args(['-i', str(inp), '--quiet', '--test', '--device-compressor', '--sort', 'None',
                                         '--raw', 'DNA', 'QUAL', 'QNAME'])
    uq.validate_args(args)
    s = uq.Session(args, ctx=ctx)
    s.load(str(inp)); s.analyse(); s.pack()
    seen = {'bytes': 0, 'candidates': 0}
    real_to_numpy, real_add = ctx.to_numpy, ops.DeflateSizes.add

    def to_numpy(*a, **k):
        out = real_to_numpy(*a, **k)
        seen['bytes'] += out.nbytes
        return out

    def add(self, *a, **k):
        seen['candidates'] += 1
        return real_add(self, *a, **k)

    monkeypatch.setattr(ctx, 'to_numpy', to_numpy, raising=False)
    monkeypatch.setattr(ops.DeflateSizes, 'add', add)
    try:
        s.run_tests()
    finally:
        monkeypatch.undo()
    return seen['bytes'], seen['candidates'], s.last_subprocess_used


def test_no_candidate_leaves_the_device(ctx, tmp_path, monkeypatch):
    small = _test_phase_traffic(ctx, tmp_path, monkeypatch, 2000)
    large = _test_phase_traffic(ctx, tmp_path, monkeypatch, 60000)
    assert small[2] == 0 and large[2] == 0                         # no subprocess
    assert small[1] == large[1] >= 16                              # 8 DNA + 8 QUAL layouts and the QNAME columns
    assert small[0] == large[0] <= 16 * small[1]                   # a 64-bit total and a status word per candidate, whatever the table size
