"""BGZF output on the MI355X: uq_bgzf_compress against the host build of the same compressor (byte for byte), read back by zlib and by the
device inflate kernel, the CLI's `--decode --bgzf` on the golden containers, the QNAME host fallback, a stream past 2^32 bytes, and the
sharded decoder with --bgzf."""
import gzip
import io
import json
import os

import numpy as np
import pytest

import uq_oracle as O
from test_deflate_cpu import BLOCK, block_matrix, member_ok
from test_gpu_dist import DECODE_CASES, _run_sharded
from test_gpu_gzip import GOLD, WRITTEN, _encode
from test_gzip_cpu import BGZF_EOF
from uq_amd import ops, synth, uq

pytestmark = pytest.mark.gpu


def test_device_members_equal_the_host_build(ctx):
    for name, b in block_matrix():
        d = ctx.to_numpy(ops.bgzf_compress(ctx, ctx.bytes_to_device(b), eof=False)).tobytes()
        assert d == (ops.bgzf_block_host(b) if b else b''), name           # no input: no data member


def test_stream_round_trips_through_zlib_and_the_device_inflate(ctx):
    data = synth.fastq(20261005, 30000, (36, 301), n_rate=1)
    d_text = ctx.bytes_to_device(data)
    blob = ctx.to_numpy(ops.bgzf_compress(ctx, d_text)).tobytes()
    assert gzip.decompress(blob) == data and blob.endswith(BGZF_EOF)
    want = b''.join(ops.bgzf_block_host(data[i:i + BLOCK]) for i in range(0, len(data), BLOCK)) + BGZF_EOF
    assert blob == want
    kind, m, total, _ = ops.gzip_scan(np.frombuffer(blob, dtype=np.uint8))
    assert kind == ops.GZIP_BGZF and total == len(data)
    out, bad = ops.inflate_members(ctx, ctx.bytes_to_device(blob), m, total)
    assert bad is None and ctx.torch.equal(out, d_text)
    assert ctx.to_numpy(ops.bgzf_compress(ctx, d_text[:0])).tobytes() == BGZF_EOF        # nothing to compress: the EOF member alone
    assert ops.bgzf_compress(ctx, d_text[:0], eof=False).numel() == 0


def _decode(ctx, path, bgzf):
    args = uq.build_parser().parse_args(['-i', str(path), '--decode', '--quiet'] + (['--bgzf'] if bgzf else []))
    uq.validate_args(args)
    out = io.BytesIO()
    s = uq.Session(args, ctx=ctx)
    s.decode(out=out)
    return out.getvalue(), s


@pytest.mark.parametrize('name', WRITTEN)
def test_cli_decode_bgzf_on_the_golden_containers(ctx, tmp_path, name):
    meta = json.load(open(os.path.join(GOLD, name + '.json')))
    plain, _ = _decode(ctx, os.path.join(GOLD, name + '.uQ'), False)
    blob, _ = _decode(ctx, os.path.join(GOLD, name + '.uQ'), True)
    assert gzip.decompress(blob) == plain
    kind, m, total, _ = ops.gzip_scan(np.frombuffer(blob, dtype=np.uint8))
    assert kind == ops.GZIP_BGZF and total == len(plain) and m['isize'][-1] == 0 and int((m['isize'] == 0).sum()) == 1
    # the .fastq.gz encodes to the same .uQ as the plain decode output
    cfg, members, s = _encode(ctx, tmp_path, blob, meta['flags'])
    assert s.gzip_path.startswith('BGZF')
    cfg2, members2, _ = _encode(ctx, tmp_path, plain, meta['flags'], name='in.fastq')
    assert members == members2 and cfg == cfg2


def test_cli_decode_bgzf_host_qname_fallback(ctx, tmp_path):
    # 40 numeric QNAME columns: more than the device text kernel emits, so the text is built on the host
    names = [b'@' + b':'.join(b'%d' % (i * 7 + k) for k in range(40)) for i in range(400)]
    fq = b''.join(n + b'\nACGTACGTAC\n+\nIIIIHHHHII\n' for n in names)
    _encode(ctx, tmp_path, fq, [], name='in.fastq')
    enc = tmp_path / 'out.uQ'
    plain, s = _decode(ctx, enc, False)
    cfg = s.open_container()[1]
    assert not uq.Session.device_text_possible(cfg)
    blob, _ = _decode(ctx, enc, True)
    assert plain == fq and gzip.decompress(blob) == fq
    assert ops.gzip_scan(np.frombuffer(blob, dtype=np.uint8))[0] == ops.GZIP_BGZF


def test_bgzf_past_4_gib_on_the_device(ctx):
    """4.3 GB of random bytes (stored members: input and output offsets both pass 2^32) followed by synthetic reads (dynamic members);
    the stream inflated by uq_inflate_members on the device = the source."""
    t = ctx.torch
    g = t.Generator(device=ctx.device)
    g.manual_seed(20261016)
    head = (1 << 32) + (40 << 20)
    tail = ops.synth_fastq(ctx, synth.Spec(20261005, 150), 0, 300000)
    src = t.empty(head + tail.numel(), dtype=t.uint8, device=ctx.device)
    src[:head] = t.randint(0, 256, (head,), dtype=t.uint8, device=ctx.device, generator=g)
    src[head:] = tail
    del tail
    blob = ops.bgzf_compress(ctx, src)
    assert blob.numel() > (1 << 32) + (40 << 20)
    host = blob.cpu().numpy()
    kind, m, total, _ = ops.gzip_scan(host)
    del host
    assert kind == ops.GZIP_BGZF and total == src.numel()
    assert int(m['data_offset'][-2]) > 1 << 32 and int(m['out_offset'][-2]) > 1 << 32
    assert int(m['comp_bytes'][-2]) < BLOCK // 2                   # the last data member holds reads: a dynamic block
    out, bad = ops.inflate_members(ctx, blob, m, total)
    assert bad is None and t.equal(out, src)


def _sharded_bgzf(tmp_path, world, fq, flags):
    inp = tmp_path / 'in.fastq'; inp.write_bytes(fq)
    enc = tmp_path / 'out.uQ'
    _run_sharded(1, inp, enc, flags)
    cfg, members = O.read_tar(str(enc))
    out = tmp_path / 'back.fastq.gz'
    _run_sharded(world, enc, out, ['--decode', '--bgzf'])
    blob = out.read_bytes()
    kind, m, total, _ = ops.gzip_scan(np.frombuffer(blob, dtype=np.uint8))
    assert kind == ops.GZIP_BGZF and blob.endswith(BGZF_EOF)
    assert int((m['isize'] == 0).sum()) == 1 and m['isize'][-1] == 0     # exactly one EOF member, at the end
    return gzip.decompress(blob), cfg, members


@pytest.mark.parametrize('world,flags', DECODE_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_sharded_decode_bgzf(tmp_path, world, flags):
    fq = synth.fastq(20261003 + 41, 2500, (30, 61), n_rate=2, dup='both', dup_templates=40)
    text, cfg, members = _sharded_bgzf(tmp_path, world, fq, flags)
    assert text.decode('latin-1') == O.decode(cfg, members)
    if '--sort' not in flags: assert text == fq


def test_sharded_decode_bgzf_with_idle_ranks(tmp_path):
    fq = b'@a:1:7\nACGTN\n+\nIHIH#\n@a:2:9\nACGTA\n+\nHIHII\n'
    text, _, _ = _sharded_bgzf(tmp_path, 3, fq, ['--raw', 'DNA', 'QUAL', 'QNAME'])
    assert text == fq
