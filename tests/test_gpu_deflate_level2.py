"""Level 2 of the deflate compressor on the MI355X: uq_bgzf_compress, uq_bgzf_compress_parts and uq_deflate_size_l with UQ_BGZF_LEVEL2
against the host build of the same code (byte for byte: the members do not depend on the thread count), read back by zlib and by the
device inflate, and --bgzf-level through the CLI's three hosts and the sharded decoder."""
import gzip
import io
import json
import os
import re
import subprocess
import sys
import tarfile
import zlib

import numpy as np
import pytest

from test_deflate_cpu import BLOCK, REPO, blocks_of
from test_deflate_level2_cpu import S2, all_blocks
from test_gpu_dist import _run_sharded
from test_gpu_sizer import _payload
from test_gpu_tables import SHAPES
from test_gzip_cpu import BGZF_EOF
from uq_amd import container, ops, synth, uq

pytestmark = pytest.mark.gpu

GOLD = os.path.join(REPO, 'tests', 'golden')
NAMES = ['var_tiny_alphabets', 'qn_u4_u8_negative', 'variable_ntrick']
MTIME = 1760572800


def _host2(data, eof=False):
    return b''.join(ops.bgzf_block_host(b, level=2) for b in blocks_of(data)) + (BGZF_EOF if eof else b'')


# ------------------------------------------------------------------ 1: the device's members are the host build's
def test_level2_device_members_equal_the_host_build(ctx):
    """Every block of the matrix and the edge shapes.  Only a stream's last block can be short, so: the full blocks as one stream, and
    every short block as the second block of a stream of its own."""
    blocks = all_blocks()
    full = [b for _, b in blocks if len(b) == BLOCK]
    stream = b''.join(full)
    got = ctx.to_numpy(ops.bgzf_compress(ctx, ctx.bytes_to_device(stream), eof=False, level=2)).tobytes()
    assert got == b''.join(ops.bgzf_block_host(b, level=2) for b in full)
    lead = full[0]
    lead_member = ops.bgzf_block_host(lead, level=2)
    for name, b in blocks:
        if len(b) == BLOCK: continue
        got = ctx.to_numpy(ops.bgzf_compress(ctx, ctx.bytes_to_device(lead + b), eof=False, level=2)).tobytes()
        assert got == lead_member + (ops.bgzf_block_host(b, level=2) if b else b''), name
    # and level 1 through the same entry is what it was
    for name, b in blocks[::7]:
        want = ops.bgzf_block_host(b) if b else b''
        assert ctx.to_numpy(ops.bgzf_compress(ctx, ctx.bytes_to_device(b), eof=False)).tobytes() == want, name
        assert ctx.to_numpy(ops.bgzf_compress(ctx, ctx.bytes_to_device(b), eof=False, level=1)).tobytes() == want, name


def test_unknown_flags_are_refused(ctx):
    import ctypes as C
    from uq_amd._lib import UqHipError, call
    d = ctx.bytes_to_device(b'abc' * 100)
    out = ctx.empty(70000)
    nout = C.c_uint64()
    with pytest.raises(UqHipError, match='unknown flags'):
        call('uq_bgzf_compress', ctx.h, C.c_void_p(d.data_ptr()), d.numel(), C.c_void_p(out.data_ptr()), out.numel(), C.byref(nout), 4)
    slots = ctx.torch.zeros(2, dtype=ctx.torch.int64, device=ctx.device)
    with pytest.raises(UqHipError, match='unknown flags'):
        call('uq_deflate_size_l', ctx.h, None, 0, C.c_void_p(d.data_ptr()), d.numel(), C.c_void_p(slots.data_ptr()),
             C.c_void_p(slots[1:].data_ptr()), 1)
    with pytest.raises(ValueError):
        ops.bgzf_compress(ctx, d, level=3)


# ------------------------------------------------------------------ 2: parts
@pytest.mark.parametrize('shift', [1, 3, 16])
def test_level2_parts_equal_the_host_twin(ctx, shift):
    text = synth.fastq(20261018, 1500, (36, 151), dup='both', dup_templates=20)
    rs = np.random.RandomState(shift)
    host_parts = [(bytes(range(17)), np.frombuffer(text[:BLOCK + 1], dtype=np.uint8)),
                  (b'', np.zeros(0, np.uint8)),
                  (bytes(range(255)), np.frombuffer(b'Q', dtype=np.uint8)),
                  (bytes(rs.randint(0, 128, 129).astype(np.uint8)), (rs.randint(0, 4, 3 * BLOCK + 77) * 21 + 33).astype(np.uint8)),
                  (b'x', np.frombuffer(text[1000:1000 + 2 * BLOCK - 1], dtype=np.uint8))]
    dev = []
    for prefix, data in host_parts:
        buf = ctx.to_device(np.concatenate([np.zeros(shift, np.uint8), data]))
        dev.append((prefix, buf[shift:]))
    out, sizes = ops.bgzf_compress_parts(ctx, dev, level=2)
    want, want_sizes = ops.bgzf_compress_parts_host([(p, d.tobytes()) for p, d in host_parts], level=2)
    assert sizes == want_sizes == [S2(p + d.tobytes()) for p, d in host_parts]
    assert ctx.to_numpy(out).tobytes() == want
    for (prefix, d), n in zip(dev, sizes):
        assert ops.deflate_size(ctx, prefix, d, level=2) == n
    out1, sizes1 = ops.bgzf_compress_parts(ctx, dev)                # level 1 is what it was
    assert (ctx.to_numpy(out1).tobytes(), sizes1) == ops.bgzf_compress_parts_host([(p, d.tobytes()) for p, d in host_parts])


# ------------------------------------------------------------------ 3: the sizer
@pytest.mark.parametrize('shape', sorted(SHAPES, key=lambda s: s[0] * s[1])[:3], ids=lambda s: '%dx%d' % s)
def test_level2_device_total_equals_host_size_on_pattern_payloads(ctx, shape):
    R, C = shape
    T = np.random.RandomState(R * 131 + C).randint(0, 4, size=(R, C)).astype(np.uint8) * 37
    if R * C > 1000: T[::7] = np.random.RandomState(C).randint(0, 256, size=T[::7].shape)
    d_T = ctx.to_device(T.ravel())
    q = ops.DeflateSizes(ctx, len(uq.PATTERNS), level=2)
    one, want = [], []
    for pat in uq.PATTERNS:
        header = uq.pattern_header(R, C, pat)
        payload = ops.pattern(ctx, d_T, R, C, pat)
        q.add(header, payload)                                      # queued back to back ...
        one.append((header, payload))
        want.append(S2(header + _payload(T, pat)))
    assert q.fetch() == want
    assert [ops.deflate_size(ctx, h, p, level=2) for h, p in one] == want       # ... and one at a time
    assert want == [ops.deflate_size_host(_payload(T, pat), h, level=2) for (h, _), pat in zip(one, uq.PATTERNS)]


def test_level2_sizer_past_one_block_and_with_odd_prefixes(ctx):
    data = synth.fastq(20261005, 1500, (36, 301))
    back = ctx.empty(len(data) + 64)
    for off, plen in [(0, 0), (1, 1), (3, 128), (16, 256)]:
        d = back[off:off + len(data)]
        d.copy_(ctx.bytes_to_device(data))
        prefix = bytes(range(plen))
        assert ops.deflate_size(ctx, prefix, d, level=2) == S2(prefix + data), (off, plen)
    assert ops.deflate_size(ctx, b'', ctx.empty(0), level=2) == 0


# ------------------------------------------------------------------ 4: read back
def test_level2_stream_round_trips_through_zlib_and_the_device_inflate(ctx):
    data = synth.fastq(20261005, 8000, (36, 301), n_rate=1, dup='both', dup_templates=40)
    d_text = ctx.bytes_to_device(data)
    blob = ctx.to_numpy(ops.bgzf_compress(ctx, d_text, level=2)).tobytes()
    assert blob == _host2(data, eof=True) and gzip.decompress(blob) == data
    assert len(blob) < ops.bgzf_compress(ctx, d_text).numel()
    kind, m, total, _ = ops.gzip_scan(np.frombuffer(blob, dtype=np.uint8))
    assert kind == ops.GZIP_BGZF and total == len(data)
    for k, b in enumerate(blocks_of(data)):
        assert int(m['crc32'][k]) == zlib.crc32(b) and int(m['isize'][k]) == len(b)
    out, bad = ops.inflate_members(ctx, ctx.bytes_to_device(blob), m, total)          # checks every member's CRC-32
    assert bad is None and ctx.torch.equal(out, d_text)
    assert ctx.to_numpy(ops.bgzf_compress(ctx, d_text[:0], level=2)).tobytes() == BGZF_EOF


# ------------------------------------------------------------------ 5: the CLI
def _session(ctx, argv):
    args = uq.build_parser().parse_args(argv)
    uq.validate_args(args)
    s = uq.Session(args, ctx=ctx)
    s.tar_mtime = MTIME
    return s


def _decode(ctx, path, flags=()):
    out = io.BytesIO()
    _session(ctx, ['-i', str(path), '--decode', '--quiet'] + list(flags)).decode(out=out)
    return out.getvalue()


@pytest.mark.parametrize('name', NAMES)
def test_cli_decode_bgzf_level(ctx, name):
    path = os.path.join(GOLD, name + '.uQ')
    plain = _decode(ctx, path)
    blob = _decode(ctx, path, ['--bgzf', '--bgzf-level', '2'])
    assert gzip.decompress(blob) == plain and blob == _host2(plain, eof=True)
    r = subprocess.run([sys.executable, '-m', 'uq_amd.bgzf_host', '--level', '2'], input=plain, stdout=subprocess.PIPE, cwd=REPO, timeout=300)
    assert r.returncode == 0 and r.stdout == blob
    assert _decode(ctx, path, ['--bgzf', '--bgzf-level', '1']) == _decode(ctx, path, ['--bgzf'])


@pytest.mark.parametrize('name', NAMES)
def test_cli_gz_level(ctx, tmp_path, name):
    meta = json.load(open(os.path.join(GOLD, name + '.json')))
    inp = tmp_path / 'in.fastq'
    inp.write_bytes(open(os.path.join(GOLD, name + '.fastq'), 'rb').read())
    files = {}
    for tag, flags in (('plain', []), ('gz', ['--gz']), ('gz1', ['--gz', '--bgzf-level', '1']), ('gz2', ['--gz', '--bgzf-level', '2'])):
        out = tmp_path / (tag + ('.uQ.gz' if flags else '.uQ'))
        s = _session(ctx, ['-i', str(inp), '-o', str(out), '--quiet'] + meta['flags'] + flags)
        s.encode()
        files[tag] = (out, s)
    tar = files['plain'][0].read_bytes()
    blob = files['gz2'][0].read_bytes()
    assert files['gz1'][0].read_bytes() == files['gz'][0].read_bytes()
    want, layout, names = container.member_aligned_host(tar, level=2)
    assert blob == want and gzip.decompress(blob) == tar
    with tarfile.open(files['gz2'][0]) as a, tarfile.open(files['plain'][0]) as b:
        assert [(m.name, a.extractfile(m).read()) for m in a.getmembers()] == [(m.name, b.extractfile(m).read()) for m in b.getmembers()]
    assert _decode(ctx, files['gz2'][0]) == _decode(ctx, files['plain'][0])
    # every table's bytes in the file = what --test --device-compressor --bgzf-level 2 sizes it at
    s = files['gz2'][1]
    sizer = _session(ctx, ['-i', str(inp), '--quiet', '--test', '--device-compressor', '--bgzf-level', '2'])
    sizer1 = _session(ctx, ['-i', str(inp), '--quiet', '--test', '--device-compressor'])
    total2 = total1 = 0
    for mname, lay in zip(names, layout):
        assert s.gz_layout[mname] == lay
        if mname == 'config.json': continue
        header, payload = s.members[mname]
        if isinstance(payload, np.ndarray): payload = ctx.to_device(np.ascontiguousarray(payload).reshape(-1).view(np.uint8))
        assert sizer.compressed_size(header, payload) == lay['data'][1], mname
        total2 += lay['data'][1]
        total1 += sizer1.compressed_size(header, payload)
    print('%s: tables at level 1 %d bytes, at level 2 %d bytes' % (name, total1, total2))


def test_cli_test_report_with_level_equals_the_host_command(ctx, tmp_path, monkeypatch):
    """--test --device-compressor --bgzf-level 2 prints what --test --compressor "bgzf_host --no-eof --level 2" prints."""
    monkeypatch.setenv('PYTHONPATH', REPO + os.pathsep + os.environ.get('PYTHONPATH', ''))
    inp = tmp_path / 'in.fastq'
    inp.write_bytes(open(os.path.join(GOLD, 'variable_ntrick.fastq'), 'rb').read())
    reports = {}
    for tag, flags in (('dev', ['--device-compressor', '--bgzf-level', '2']),
                       ('host', ['--compressor', '%s -m uq_amd.bgzf_host --no-eof --level 2' % sys.executable])):
        args = uq.build_parser().parse_args(['-i', str(inp), '-o', str(tmp_path / (tag + '.uQ')), '--test', '--sort', 'None', '--raw', 'DNA',
                                             'QUAL', 'QNAME'] + flags)
        uq.validate_args(args)
        report = io.StringIO()
        uq.Session(args, ctx=ctx, out=report).encode()
        reports[tag] = [re.sub(r'\(\S+ minutes\)\s*', '', l) for l in report.getvalue().split('\n')]
    assert reports['dev'] == reports['host']
    assert any(l.startswith('Size (compressed)') for l in reports['dev'])


def test_sharded_decode_bgzf_level(ctx, tmp_path):
    """Two ranks: each deflates its own rows' text into whole members from its own start, so the file's members are cut elsewhere than
    the single-GPU file's; it inflates to the single-GPU file's text, and every member is the level-2 member of its bytes."""
    fq = synth.fastq(20261003 + 41, 2500, (30, 61), n_rate=2, dup='both', dup_templates=40)
    inp = tmp_path / 'in.fastq'; inp.write_bytes(fq)
    enc = tmp_path / 'out.uQ'
    _session(ctx, ['-i', str(inp), '-o', str(enc), '--quiet']).encode()
    single = _decode(ctx, enc, ['--bgzf', '--bgzf-level', '2'])
    one, two = tmp_path / 'one.fastq.gz', tmp_path / 'two.fastq.gz'
    _run_sharded(1, enc, one, ['--decode', '--bgzf', '--bgzf-level', '2'])
    assert one.read_bytes() == single                               # one rank: the single-GPU file itself
    _run_sharded(2, enc, two, ['--decode', '--bgzf', '--bgzf-level', '2'])
    blob = two.read_bytes()
    assert gzip.decompress(blob) == gzip.decompress(single) == fq and blob.endswith(BGZF_EOF)
    kind, m, total, _ = ops.gzip_scan(np.frombuffer(blob, dtype=np.uint8))
    assert kind == ops.GZIP_BGZF and int((m['isize'] == 0).sum()) == 1
    at = 0
    for k in range(len(m) - 1):
        piece = fq[at:at + int(m['isize'][k])]
        member = ops.bgzf_block_host(piece, level=2)
        lo = int(m['data_offset'][k]) - 18
        assert blob[lo:lo + len(member)] == member, k
        at += len(piece)
    assert at == len(fq)
