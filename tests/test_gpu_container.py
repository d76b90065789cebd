"""BGZF-compressed containers on the MI355X: uq_bgzf_compress_parts against its host twin, `--gz` encodes against the host-built
member-aligned file, decodes from every compressed form of the golden containers, damage, the sharded decoder, and a table past 2^32."""
import gzip
import io
import json
import os
import tarfile

import numpy as np
import pytest

from test_gpu_dist import _run_sharded
from uq_amd import container, ops, synth, uq

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GOLDEN = sorted(f[:-5] for f in os.listdir(GOLD) if f.endswith('.json'))
WRITTEN = [n for n in GOLDEN if not n.endswith('_refused')]          # the WRITTEN list of test_gpu_gzip.py
BLOCK = 65280
MTIME = 1760572800


def _mixed_bytes(n, seed):
    """Compressible and not: runs of few symbols, then noise."""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 4, n).astype(np.uint8) + 65
    a[n // 2:n // 2 + n // 8] = rng.randint(0, 256, n // 8).astype(np.uint8)
    return a


def _check_parts(ctx, host_parts, shift=0):
    """host_parts: [(prefix bytes, numpy uint8)].  The data of every part sits `shift` bytes into an allocation of its own."""
    t = ctx.torch
    dev = []
    for prefix, data in host_parts:
        buf = ctx.to_device(np.concatenate([np.zeros(shift, np.uint8), data]))
        dev.append((prefix, buf[shift:]))
    out, sizes = ops.bgzf_compress_parts(ctx, dev)
    want, want_sizes = ops.bgzf_compress_parts_host([(p, d.tobytes()) for p, d in host_parts])
    assert sizes == want_sizes
    assert ctx.to_numpy(out).tobytes() == want
    for (prefix, d), n in zip(dev, sizes):
        assert n == ops.deflate_size(ctx, prefix, d)
    return dev, out, sizes


@pytest.mark.parametrize('shift', [0, 1, 4, 16])
def test_parts_equal_the_host_twin(ctx, shift):
    sizes = [0, 1, BLOCK - 128, BLOCK, BLOCK + 1, 3 * BLOCK + 77, (2 << 20) + 13]
    prefixes = [0, 1, 127, 128, 256]
    parts = []
    for i, n in enumerate(sizes):
        for j, p in enumerate(prefixes):
            if n > (1 << 20) and p not in (0, 128, 127): continue
            parts.append((bytes((7 * k + j) & 255 for k in range(p)), _mixed_bytes(n, 100 * i + j + shift)))
    _check_parts(ctx, parts, shift)


def test_parts_chunks_span_parts_and_capacity_is_enforced(ctx):
    # 2 300 blocks in all: the first chunk of 2 048 ends inside the third part
    parts = [(b'a' * 128, _mixed_bytes(900 * BLOCK + 5, 1)), (b'', _mixed_bytes(17, 2)), (b'b' * 128, _mixed_bytes(1400 * BLOCK - 128, 3)),
             (b'c' * 3, _mixed_bytes(5 * BLOCK, 4))]
    dev, out, sizes = _check_parts(ctx, parts, 0)
    nblocks = sum((len(p) + d.size + BLOCK - 1) // BLOCK for p, d in parts)
    assert nblocks > 2048
    kind, m, total, _ = ops.gzip_scan(ctx.to_numpy(out))
    assert kind == ops.GZIP_BGZF and len(m) == nblocks and total == sum(len(p) + d.size for p, d in parts)
    # with the EOF member; and a capacity one byte short: refused, the byte past it untouched
    full, _ = ops.bgzf_compress_parts(ctx, dev, eof=True)
    assert ctx.to_numpy(full).tobytes() == ctx.to_numpy(out).tobytes() + ops.BGZF_EOF
    need = int(out.numel())
    from uq_amd._lib import UqHipError, BgzfPart, call
    import ctypes as C
    arr, keep = ops._bgzf_parts_arg(dev)
    buf = ctx.torch.full((need + 64,), 0xA5, dtype=ctx.torch.uint8, device=ctx.device)
    ps, nout = (C.c_uint64 * len(dev))(), C.c_uint64()
    with pytest.raises(UqHipError, match='capacity'):
        call('uq_bgzf_compress_parts', ctx.h, arr, len(dev), C.c_void_p(buf.data_ptr()), need - 1, ps, C.byref(nout), 0)
    assert bool((buf[need - 1:] == 0xA5).all())
    call('uq_bgzf_compress_parts', ctx.h, arr, len(dev), C.c_void_p(buf.data_ptr()), need, ps, C.byref(nout), 0)
    assert nout.value == need and ctx.torch.equal(buf[:need], out) and bool((buf[need:] == 0xA5).all())
    assert ops.bgzf_parts_bound(dev) >= need + 28
    assert ops.bgzf_compress_parts(ctx, [])[0].numel() == 0


def _session(ctx, argv):
    args = uq.build_parser().parse_args(argv)
    uq.validate_args(args)
    s = uq.Session(args, ctx=ctx)
    s.tar_mtime = MTIME
    return s


def _encode(ctx, tmp_path, fq, flags, gz):
    inp = tmp_path / 'in.fastq'
    inp.write_bytes(fq)
    out = tmp_path / ('out.uQ.gz' if gz else 'out.uQ')
    s = _session(ctx, ['-i', str(inp), '-o', str(out), '--quiet'] + flags + (['--gz'] if gz else []))
    s.encode()
    return out, s


def _decode(ctx, path, flags=()):
    s = _session(ctx, ['-i', str(path), '--decode', '--quiet'] + list(flags))
    out = io.BytesIO()
    s.decode(out=out)
    return out.getvalue(), s


def _tar_dict(path):
    with tarfile.open(path) as t:
        return [(m.name, t.extractfile(m).read()) for m in t.getmembers()]


@pytest.mark.parametrize('name', WRITTEN)
def test_cli_gz_encode_is_the_host_twin_and_decodes_from_every_form(ctx, tmp_path, name):
    meta = json.load(open(os.path.join(GOLD, name + '.json')))
    fq = open(os.path.join(GOLD, name + '.fastq'), 'rb').read()
    plain_path, _ = _encode(ctx, tmp_path, fq, meta['flags'], False)
    gz_path, s = _encode(ctx, tmp_path, fq, meta['flags'], True)
    tar = plain_path.read_bytes()
    blob = gz_path.read_bytes()
    want, layout, names = container.member_aligned_host(tar)
    assert blob == want and gzip.decompress(blob) == tar and len(blob) == s.gz_bytes
    assert _tar_dict(gz_path) == _tar_dict(plain_path)
    # every table's bytes in the file = what --test --device-compressor reports for it
    sizer = _session(ctx, ['-i', str(tmp_path / 'in.fastq'), '--quiet', '--test', '--device-compressor'])
    for mname, lay in zip(names, layout):
        assert s.gz_layout[mname] == lay
        if mname == 'config.json': continue
        header, payload = s.members[mname]
        if isinstance(payload, np.ndarray): payload = ctx.to_device(np.ascontiguousarray(payload).reshape(-1).view(np.uint8))
        assert sizer.compressed_size(header, payload) == lay['data'][1], mname
    assert s.gz_layout[None] == layout[-1]

    # decode: the same text from every form of the container
    text, _ = _decode(ctx, plain_path)
    assert text.count(b'\n') == fq.count(b'\n')
    forms = {'gz': blob,
             'whole_stream_bgzf': ctx.to_numpy(ops.bgzf_compress(ctx, ctx.bytes_to_device(tar))).tobytes(),
             'gzip6': gzip.compress(tar, 6),
             'two_members': gzip.compress(tar[:len(tar) // 3], 6) + gzip.compress(tar[len(tar) // 3:], 1)}
    for form, data in forms.items():
        p = tmp_path / (form + '.uQ.gz')
        p.write_bytes(data)
        got, ds = _decode(ctx, p)
        assert got == text, form
        assert ds.source.kind == (container.BGZF if form in ('gz', 'whole_stream_bgzf') else container.GZIP), form
    got, _ = _decode(ctx, tmp_path / 'gzip6.uQ.gz', ['--host-inflate'])
    assert got == text


def test_golden_refdecode_from_the_gz_form(ctx, tmp_path):
    """The committed containers themselves (written by the reference), member-aligned on the host, decode to the text of the plain file;
    against the reference decoder's own output (.refdecode.fastq) that is what test_oracle_golden.py pins for the oracle: lines 2 and 4
    of every record, and line 1 where the fixture's json says the reference decoder reproduces it (Q6)."""
    seen = 0
    for name in WRITTEN:
        tar_path = os.path.join(GOLD, name + '.uQ')
        p = tmp_path / (name + '.uQ.gz')
        p.write_bytes(container.member_aligned_host(open(tar_path, 'rb').read())[0])
        got = _decode(ctx, p)[0]
        assert got == _decode(ctx, tar_path)[0], name
        ref = os.path.join(GOLD, name + '.refdecode.fastq')
        if not os.path.exists(ref): continue
        seen += 1
        rd = json.load(open(os.path.join(GOLD, name + '.json')))['reference_decode']
        lines, ref_lines = got.decode('latin-1').split('\n')[:-1], open(ref, 'rb').read().decode('latin-1').split('\n')[:-1]
        assert len(lines) == len(ref_lines), name
        assert lines[1::4] == ref_lines[1::4] and lines[2::4] == ref_lines[2::4] and lines[3::4] == ref_lines[3::4], name
        if rd['qname_lines'] == 'equal to the input': assert got == open(ref, 'rb').read(), name
    assert seen > 10


def test_damage_is_found_before_any_text_is_written(ctx, tmp_path):
    fq = synth.fastq(20261016, 20000, (36, 151), n_rate=1)
    gz_path, s = _encode(ctx, tmp_path, fq, ['--raw', 'DNA', 'QUAL', 'QNAME'], True)
    blob = gz_path.read_bytes()
    assert _decode(ctx, gz_path)[0] == fq
    kind, m, total, _ = ops.gzip_scan(np.frombuffer(blob, dtype=np.uint8))
    k = len(m) // 2
    lo, n = int(m['data_offset'][k]), int(m['comp_bytes'][k])

    def attempt(data):
        p = tmp_path / 'bad.uQ.gz'
        p.write_bytes(data)
        sink = io.BytesIO()
        with pytest.raises(uq.UqError) as e:
            _session(ctx, ['-i', str(p), '--decode', '--quiet']).decode(out=sink)
        assert sink.getvalue() == b''
        return str(e.value)

    flipped = bytearray(blob); flipped[lo + n // 2] ^= 0x10
    msg = attempt(bytes(flipped))
    assert 'gzip member %d' % k in msg and 'byte %d' % lo in msg
    crc = bytearray(blob); crc[lo + n] ^= 0x01                 # the trailer follows the deflate data: CRC-32, then ISIZE
    msg = attempt(bytes(crc))
    assert 'gzip member %d' % k in msg and 'CRC-32' in msg
    msg = attempt(blob[:lo + n // 2])                          # cut mid-member
    assert 'gzip member' in msg and 'byte' in msg
    # without the EOF member: accepted (with a warning when not --quiet)
    p = tmp_path / 'noeof.uQ.gz'
    p.write_bytes(blob[:-28])
    assert _decode(ctx, p)[0] == fq


def _sharded_decode(tmp_path, world, enc, tag):
    out = tmp_path / ('back_%s_%d.fastq' % (tag, world))
    logs = _run_sharded(world, enc, out, ['--decode'], extra_env={'UQ_TIMING': '1'})
    counts = []
    for log in logs:
        for line in log.splitlines():
            if line.startswith('{') and '"uq_container"' in line: counts.append(json.loads(line))
    return out.read_bytes(), counts


def test_sharded_decode_of_a_gz_container(ctx, tmp_path):
    fq = synth.fastq(20261017, 60000, (36, 151), n_rate=1)
    gz_path, _ = _encode(ctx, tmp_path, fq, ['--raw', 'DNA', 'QUAL', 'QNAME'], True)
    single, _ = _decode(ctx, gz_path)
    assert single == fq
    for world in (2, 3):
        text, counts = _sharded_decode(tmp_path, world, gz_path, 'raw')
        assert text == single
        assert sorted(c['rank'] for c in counts) == list(range(world))
        for c in counts:
            assert 0 < c['inflated_members'] < c['members'], c
    # a keyed mix and a column-major pattern: whole tables are inflated, the text is the same
    small = synth.fastq(20261018, 6000, (30, 61), n_rate=2, dup='both', dup_templates=40)
    for tag, flags in (('keyed', ['--sort', 'DNA', '--raw', 'QUAL']), ('pattern', ['--raw', 'DNA', 'QNAME', '--pattern', '3.1', '0.2'])):
        d = tmp_path / tag; d.mkdir()
        enc, _ = _encode(ctx, d, small, flags, True)
        want, _ = _decode(ctx, enc)
        for world in (2, 3):
            assert _sharded_decode(d, world, enc, tag)[0] == want, (tag, world)


def test_table_past_4_gib_through_the_parts_entry_and_the_bgzf_source(ctx):
    """One part of 4.3 GB (noise: stored members, so compressed and inflated offsets both pass 2^32) behind a 128-byte prefix; a slice
    that straddles the 4 GiB offset of the inflated stream, read back through the BGZF source, is the input."""
    t = ctx.torch
    g = t.Generator(device=ctx.device)
    g.manual_seed(20261016)
    n = (1 << 32) + (40 << 20)
    src = t.randint(0, 256, (n,), dtype=t.uint8, device=ctx.device, generator=g)
    prefix = bytes(range(128))
    blob, sizes = ops.bgzf_compress_parts(ctx, [(prefix, src), (b'tail', src[:1000])], eof=True)
    assert sizes[0] > n and blob.numel() == sum(sizes) + 28
    host = blob.cpu().numpy()
    kind, m, total, _ = ops.gzip_scan(host)
    assert kind == ops.GZIP_BGZF and total == 128 + n + 4 + 1000
    source = container.BgzfSource(host, m, total, container.device_inflater(ops, ctx, lambda lo, k: blob[lo:lo + k], m))
    lo, k = (1 << 32) - (3 << 20) + 12345, 6 << 20
    got = source.to_device(lo, k)
    assert t.equal(got, src[lo - 128:lo - 128 + k])
    assert 0 < source.inflated_members <= k // BLOCK + 2 < len(m)
    assert source.read_host(0, 128) == prefix
    assert source.read_host(128 + n, 4) == b'tail' and t.equal(source.to_device(128 + n + 4, 1000), src[:1000])
    assert source.read_host((1 << 32) - 7, 14) == src[(1 << 32) - 7 - 128:(1 << 32) + 7 - 128].cpu().numpy().tobytes()
