"""BGZF-compressed containers, the parts that need no GPU: the CLI rules of --gz, the member-aligned layout built on the host from the golden
tars, the BGZF byte source against gzip.decompress, the tar walk under damage, and the refusals of other compressors."""
import argparse
import bz2
import gzip
import io
import lzma
import os
import random
import tarfile

import numpy as np
import pytest

from uq_amd import container, ops, uq

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GOLDEN = sorted(f[:-5] for f in os.listdir(GOLD) if f.endswith('.json'))
WRITTEN = [n for n in GOLDEN if not n.endswith('_refused')]          # the WRITTEN list of test_gpu_gzip.py
BLOCK = 65280
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(tmp_path, flags):
    inp = tmp_path / 'in.fastq'
    inp.write_bytes(b'@r\nACGT\n+\nIIII\n')
    return uq.build_parser().parse_args(['-i', str(inp)] + flags)


def test_validate_args_rules_for_gz(tmp_path):
    with pytest.raises(uq.UqError, match='--gz.*--decode'):
        uq.validate_args(_args(tmp_path, ['--gz', '--decode']))
    with pytest.raises(uq.UqError, match='--gz.*--peek'):
        uq.validate_args(_args(tmp_path, ['--gz', '--peek']))
    with pytest.raises(uq.UqError, match='--bgzf'):
        uq.validate_args(_args(tmp_path, ['--bgzf']))
    a = uq.validate_args(_args(tmp_path, ['--gz', '--test', '--device-compressor']))
    assert a.gz and a.test and a.device_compressor
    assert uq.validate_args(_args(tmp_path, ['--gz'])).gz
    with pytest.raises(uq.UqError, match='--device-compressor'):
        uq.validate_args(_args(tmp_path, ['--gz', '--device-compressor']))         # the existing rule: only with --test


def _tar_members(tar):
    with tarfile.open(fileobj=io.BytesIO(tar)) as t:
        return [(m.name, m.offset_data, m.size) for m in t.getmembers()]


@pytest.mark.parametrize('name', WRITTEN)
def test_member_aligned_host_twin_on_the_goldens(name):
    tar = open(os.path.join(GOLD, name + '.uQ'), 'rb').read()
    blob, layout, names = container.member_aligned_host(tar)
    assert gzip.decompress(blob) == tar
    kind, m, total, _ = ops.gzip_scan(np.frombuffer(blob, dtype=np.uint8))
    assert kind == ops.GZIP_BGZF and total == len(tar)
    assert int((m['isize'] == 0).sum()) == 1 and m['isize'][-1] == 0
    members = _tar_members(tar)
    assert names == [n for n, _, _ in members] and len(layout) == len(members) + 1
    pos = 0
    for (mname, offset, size), lay in zip(members, layout):
        whole = tar[offset:offset + size]
        f = io.BytesIO(whole)
        if mname == 'config.json': header = b''
        else:
            np.lib.format.read_magic(f); np.lib.format.read_array_header_1_0(f)
            header = whole[:f.tell()]
        assert lay['data'][1] == ops.deflate_size_host(whole[len(header):], prefix=header), mname
        assert lay['frame'][0] == pos and lay['data'][0] == pos + lay['frame'][1]
        # the data part inflates to the member, its blocks counted from the member's own start
        part = blob[lay['data'][0]:lay['data'][0] + lay['data'][1]]
        assert gzip.decompress(part) == whole if whole else part == b''
        _, pm, _, _ = ops.gzip_scan(np.frombuffer(part, dtype=np.uint8))
        assert [int(v) for v in pm['isize']] == [min(BLOCK, size - o) for o in range(0, size, BLOCK)]
        pos = lay['data'][0] + lay['data'][1]
    assert layout[-1]['data'] is None and layout[-1]['frame'][0] == pos
    assert pos + layout[-1]['frame'][1] + len(ops.BGZF_EOF) == len(blob) and blob.endswith(ops.BGZF_EOF)


def test_parts_host_twin_is_the_block_compressor_per_part():
    rng = np.random.RandomState(5)
    a = rng.randint(0, 4, 3 * BLOCK + 17).astype(np.uint8).tobytes()
    parts = [(b'H' * 128, a), (b'', b''), (b'xyz', b''), (b'', b'q'), (b'p' * 256, a[:BLOCK - 256])]
    blob, sizes = ops.bgzf_compress_parts_host(parts)
    assert sizes == [ops.deflate_size_host(d, prefix=p) for p, d in parts] and sum(sizes) == len(blob)
    assert gzip.decompress(blob) == b''.join(p + d for p, d in parts)
    assert ops.bgzf_compress_parts_host(parts, eof=True)[0] == blob + ops.BGZF_EOF
    assert ops.bgzf_compress_parts_host([]) == (b'', [])


def _whole_stream_bgzf(data):
    return b''.join(ops.bgzf_block_host(data[o:o + BLOCK]) for o in range(0, len(data), BLOCK)) + ops.BGZF_EOF


def _host_source(blob):
    """A BgzfSource over host bytes whose 'device' inflate is the device decoder's code on the CPU; it records what it was asked for."""
    comp = np.frombuffer(blob, dtype=np.uint8)
    kind, members, total, _ = ops.gzip_scan(comp)
    assert kind == ops.GZIP_BGZF
    asked = []

    def inflate(k0, k1):
        asked.append((k0, k1))
        out = []
        for k in range(k0, k1):
            m = members[k]
            st, b = ops.inflate_member_host(blob[int(m['data_offset']):int(m['data_offset']) + int(m['comp_bytes'])], int(m['isize']), int(m['crc32']))
            assert st == 0
            out.append(b)
        return np.frombuffer(b''.join(out), dtype=np.uint8)

    class Arr(container.BgzfSource):
        def to_device(self, offset, n):                      # numpy has no clone()
            k0, k1 = self.cover(offset, n)
            if k1 == k0: return np.zeros(0, np.uint8)
            self.inflated.update(k for k in range(k0, k1) if self.members[k]['isize'])
            skip = offset - int(self.out_offset[k0])
            return self.device_inflate(k0, k1)[skip:skip + n].copy()
    return Arr(comp, members, total, inflate), members, asked


@pytest.mark.parametrize('form', ['member_aligned', 'whole_stream'])
def test_bgzf_source_reads_equal_gzip_decompress(form):
    tar = open(os.path.join(GOLD, 'cfg1_10k_100bp.uQ'), 'rb').read()
    blob = container.member_aligned_host(tar)[0] if form == 'member_aligned' else _whole_stream_bgzf(tar)
    src, members, asked = _host_source(blob)
    plain = gzip.decompress(blob)
    assert plain == tar and src.total == len(tar)
    rng = random.Random(20261016)
    edges = sorted({int(v) for v in members['out_offset']} | {len(tar)})
    reads = []
    for _ in range(100):
        o = rng.randrange(len(tar)); reads.append((o, rng.randrange(0, min(300000, len(tar) - o) + 1)))
    for _ in range(40):                                      # start on a member boundary
        o = rng.choice(edges[:-1]); reads.append((o, rng.randrange(0, min(200000, len(tar) - o) + 1)))
    for _ in range(40):                                      # end on a member boundary
        e = rng.choice(edges[1:]); o = rng.randrange(0, e + 1); reads.append((o, e - o))
    reads += [(0, len(tar)), (len(tar), 0), (0, 0), (edges[1], edges[2] - edges[1])]
    past = [(len(tar), 1), (len(tar) - 5, 6), (len(tar) + 10, 0), (rng.randrange(len(tar)), len(tar))] + \
           [(rng.randrange(len(tar)), len(tar) + rng.randrange(1, 1000)) for _ in range(12)]
    assert len(reads) + len(past) >= 200
    for o, n in reads:
        del asked[:]
        got = src.to_device(o, n).tobytes()
        assert got == plain[o:o + n], (o, n)
        assert src.read_host(o, n) == plain[o:o + n], (o, n)
        sel = src.selected(o, n)
        if n == 0:
            assert sel == [] and asked == []
            continue
        # minimal: every selected member holds a byte of [o, o + n), and no member outside the selection does
        for k, m in enumerate(members):
            lo, hi = int(m['out_offset']), int(m['out_offset']) + int(m['isize'])
            inside = hi > lo and lo < o + n and hi > o
            assert inside == (k in sel), (o, n, k)
        k0, k1 = asked[0]
        assert len(asked) == 1 and k0 == sel[0] and k1 == sel[-1] + 1
    for o, n in past:
        with pytest.raises(uq.UqError):
            src.to_device(o, n)
        with pytest.raises(uq.UqError):
            src.read_host(o, n)


class _Bytes:
    def __init__(self, data):
        self.data, self.total, self.worst = data, len(data), 0

    def read_host(self, offset, n):
        assert 0 <= offset and n >= 0 and offset + n <= self.total, 'the walk addressed bytes outside the stream'
        return self.data[offset:offset + n]


def _golden_tar():
    return open(os.path.join(GOLD, 'cfg1_10k_100bp.uQ'), 'rb').read()


def test_tar_walk_equals_tarfile_and_rejects_damage():
    tar = _golden_tar()
    want = {n: (o, s) for n, o, s in _tar_members(tar)}
    assert container.walk_tar(_Bytes(tar)) == want
    # without the end-of-archive zeros, and with one zero block only
    last = max(o + s for o, s in want.values())
    body = tar[:last + (-last % 512)]
    assert container.walk_tar(_Bytes(body)) == want and container.walk_tar(_Bytes(body + b'\0' * 512)) == want
    # a size field that points past the inflated total
    name, (off, size) = max(want.items(), key=lambda kv: kv[1][0])
    hdr = bytearray(tar[off - 512:off])
    ti = tarfile.TarInfo.frombuf(bytes(hdr), tarfile.ENCODING, 'surrogateescape'); ti.size = len(tar)
    bad = tar[:off - 512] + ti.tobuf(tarfile.DEFAULT_FORMAT, tarfile.ENCODING, 'surrogateescape') + tar[off:]
    with pytest.raises(uq.UqError, match='damaged'):
        container.walk_tar(_Bytes(bad))
    # a truncated last member
    with pytest.raises(uq.UqError, match='damaged'):
        container.walk_tar(_Bytes(tar[:off + size // 2]))
    # cut inside a header block after the last whole member, and inside a member's padding
    for cut in [off - 512 + 100, off - 1] + ([off + size + 1] if size % 512 else []):
        with pytest.raises(uq.UqError, match='damaged'):
            container.walk_tar(_Bytes(tar[:cut]))
    # streams that are not a tar
    for junk in (b'', b'\0' * 2048, b'@r\nACGT\n+\nIIII\n' * 100, os.urandom(4096), tar[7:]):
        with pytest.raises(uq.UqError, match='not a tar file'):
            container.walk_tar(_Bytes(junk))
    with pytest.raises(uq.UqError, match='No config.json'):
        container.read_config(_Bytes(tar), {k: v for k, v in want.items() if k != 'config.json'})


def test_tar_walk_under_random_header_corruption():
    tar = _golden_tar()
    headers = [o - 512 for _, o, _ in _tar_members(tar)]
    outcomes = {'error': 0, 'table': 0}
    for seed in range(500):
        rng = random.Random(seed)
        data = bytearray(tar)
        h = rng.choice(headers)
        at = h + rng.randrange(512)
        data[at] = (data[at] + rng.randrange(1, 256)) & 255
        if seed % 5 == 0:                                    # and a checksum made right again, so the damaged field is believed
            blk = bytearray(data[h:h + 512]); blk[148:156] = b' ' * 8
            blk[148:156] = ('%06o\0 ' % sum(blk)).encode()
            data[h:h + 512] = blk
        src = _Bytes(bytes(data))
        try:
            members = container.walk_tar(src)
        except uq.UqError:
            outcomes['error'] += 1
            continue
        outcomes['table'] += 1
        for o, s in members.values():
            assert 0 <= o and 0 <= s and o + s <= src.total
    assert outcomes['error'] and outcomes['table']


def test_other_compressors_are_refused_by_name(tmp_path):
    tar = _golden_tar()[:20000]
    for fname, data, word in (('a.uQ.bz2', bz2.compress(tar), 'bzip2'), ('a.uQ.xz', lzma.compress(tar), 'xz'),
                              ('a.uQ.zst', b'\x28\xb5\x2f\xfd' + b'\0' * 64, 'zstd')):
        p = tmp_path / fname
        p.write_bytes(data)
        with pytest.raises(uq.UqError, match=word + '.*decompress it first'):
            container.sniff(str(p))
    p = tmp_path / 'plain.uQ'; p.write_bytes(tar)
    assert container.sniff(str(p)) == container.PLAIN
    p = tmp_path / 'g.uQ.gz'; p.write_bytes(gzip.compress(tar))
    assert container.sniff(str(p)) == container.GZIP


def test_sharded_cli_refuses_gz_encode_and_other_gzip_decode_before_any_set_up(tmp_path, capsys, monkeypatch):
    from uq_amd import dist_encode
    import torch.distributed as dist
    monkeypatch.setattr(dist, 'init_process_group', lambda *a, **k: pytest.fail('a process group was created'))
    fq = tmp_path / 'in.fastq'; fq.write_bytes(b'@r\nACGT\n+\nIIII\n')
    assert dist_encode.main(['-i', str(fq), '--gz']) == 1
    assert '--gz' in capsys.readouterr().out
    g = tmp_path / 'c.uQ.gz'; g.write_bytes(gzip.compress(_golden_tar()))
    assert dist_encode.main(['-i', str(g), '-o', str(tmp_path / 'o.fastq'), '--decode']) == 1
    assert 'BGZF' in capsys.readouterr().out
    z = tmp_path / 'c.uQ.xz'; z.write_bytes(lzma.compress(_golden_tar()[:5000]))
    assert dist_encode.main(['-i', str(z), '-o', str(tmp_path / 'o.fastq'), '--decode']) == 1
    assert 'decompress it first' in capsys.readouterr().out


def test_sharded_refusals_create_no_process_group(tmp_path):
    import subprocess
    import sys
    tar = open(os.path.join(GOLD, 'cfg1_10k_100bp.uQ'), 'rb').read()
    g = tmp_path / 'c.uQ.gz'; g.write_bytes(gzip.compress(tar))
    fq = tmp_path / 'in.fastq'; fq.write_bytes(open(os.path.join(GOLD, 'cfg1_10k_100bp.fastq'), 'rb').read())
    # no RANK / MASTER_* in the environment and a port nobody listens on: a process group could not come up; the refusal comes first
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(PYTHONPATH=REPO, WORLD_SIZE='2', RANK='1', MASTER_PORT='29999', UQ_DIST_BACKEND='gloo')
    for argv, word in ((['-i', str(g), '-o', str(tmp_path / 'o.fastq'), '--decode'], 'BGZF'), (['-i', str(fq), '--gz'], '--gz')):
        r = subprocess.run([sys.executable, '-m', 'uq_amd.dist_encode'] + argv, env=env, cwd=REPO, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=120)
        assert r.returncode == 1 and word in r.stdout.decode(), r.stdout.decode()[-2000:]
