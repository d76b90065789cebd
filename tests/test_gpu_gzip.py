"""gzip input on the MI355X: the CLI on gzip-compressed golden fixtures (BGZF inflated on the device, single-member gzip on the host)
against the .uQ files the reference wrote from the plain text, uq_inflate_members against zlib, the QNAME host fallback on compressed
input, empty and damaged members, and a BGZF stream whose output and compressed offsets pass 2^32."""
import gzip
import json
import os
import tarfile
import zlib

import numpy as np
import pytest

import uq_oracle as O
from test_gzip_cpu import BGZF_EOF, bgzf, corrupt_cases, crafted, fastq, member_matrix, raw_deflate
from uq_amd import ops, synth, uq

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GOLDEN = sorted(f[:-5] for f in os.listdir(GOLD) if f.endswith('.json'))
REFUSED = [n for n in GOLDEN if n.endswith('_refused')]
WRITTEN = [n for n in GOLDEN if n not in REFUSED]
FORMS = {'bgzf': lambda fq: bgzf(fq), 'bgzf_small_members': lambda fq: bgzf(fq, chunk=997), 'gzip': lambda fq: gzip.compress(fq, 6)}


def _encode(ctx, tmp_path, blob, flags, name='in.fastq.gz'):
    inp = tmp_path / name
    inp.write_bytes(blob)
    out = tmp_path / 'out.uQ'
    args = uq.build_parser().parse_args(['-i', str(inp), '-o', str(out), '--quiet'] + flags)
    uq.validate_args(args)
    s = uq.Session(args, ctx=ctx)
    s.encode()
    with tarfile.open(out) as t:
        members = {m.name: t.extractfile(m).read() for m in t.getmembers()}
    return json.loads(members.pop('config.json').decode()), members, s


@pytest.mark.parametrize('form', sorted(FORMS))
@pytest.mark.parametrize('name', WRITTEN)
def test_gzip_input_matches_reference_output(ctx, tmp_path, name, form):
    meta = json.load(open(os.path.join(GOLD, name + '.json')))
    fq = open(os.path.join(GOLD, name + '.fastq'), 'rb').read()
    ref_cfg, ref_members = O.read_tar(os.path.join(GOLD, name + '.uQ'))
    cfg, members, s = _encode(ctx, tmp_path, FORMS[form](fq), meta['flags'])
    assert s.path is None and s.gzip_path.startswith('BGZF' if form.startswith('bgzf') else 'gzip')
    assert set(members) == set(ref_members)
    for k in ref_cfg:
        if k in ('sort', 'raw', 'pattern'): continue
        assert json.loads(json.dumps(cfg[k])) == ref_cfg[k], k
    if meta['stable_patch'] or 'sort' not in ' '.join(meta['flags']) or '--sort None' in ' '.join(meta['flags']):
        for k in ref_members:
            assert members[k] == ref_members[k], k
    else:
        from test_oracle_golden import assert_equal_up_to_tie_order
        assert_equal_up_to_tie_order(cfg, members, ref_cfg, ref_members)
    # and the same bytes as the plain file gives
    cfg2, members2, _ = _encode(ctx, tmp_path, fq, meta['flags'], name='in.fastq')
    assert members2 == members and cfg2 == cfg


@pytest.mark.parametrize('form', sorted(FORMS))
@pytest.mark.parametrize('name', REFUSED)
def test_gzip_input_refused_like_plain(ctx, tmp_path, name, form):
    from uq_amd import qname
    meta = json.load(open(os.path.join(GOLD, name + '.json')))
    fq = open(os.path.join(GOLD, name + '.fastq'), 'rb').read()
    with pytest.raises((uq.UqError, qname.QnameError)) as plain:
        _encode(ctx, tmp_path, fq, meta['flags'], name='in.fastq')
    with pytest.raises((uq.UqError, qname.QnameError)) as comp:
        _encode(ctx, tmp_path, FORMS[form](fq), meta['flags'])
    assert type(comp.value) is type(plain.value) and str(comp.value) == str(plain.value)


def _table(streams):
    """One compressed buffer of raw deflate streams and its member table (what uq_gzip_scan returns for BGZF)."""
    comp, rows, out = bytearray(), [], 0
    for d, isize, crc in streams:
        rows.append((len(comp) + 7, len(d), out, isize, crc))
        comp += b'\x00' * 7 + d                      # unaligned data offsets
        out += isize
    return bytes(comp) + b'\x00' * 3, np.array(rows, dtype=ops.GZIP_MEMBER), out


def test_inflate_members_matches_zlib_on_the_matrix(ctx):
    mat = member_matrix()
    data = fastq(3000)
    streams, want = [], []
    for _, d, payload in mat:
        streams.append((d, len(payload), zlib.crc32(payload))); want.append(payload)
    for i in range(0, len(data), 4093):                # records straddle the members
        c = data[i:i + 4093]
        streams.append((raw_deflate(c, 6), len(c), zlib.crc32(c))); want.append(c)
    comp, table, total = _table(streams)
    ops.scribble_lds(ctx, 0x5A5A5A5A)
    out, bad = ops.inflate_members(ctx, ctx.bytes_to_device(comp), table, total)
    assert bad is None
    assert ctx.to_numpy(out).tobytes() == b''.join(want)


def test_inflate_members_status_matches_host_decoder_on_bad_streams(ctx):
    cases = [(s, isize, 0) for _, s, isize, _ in crafted()]
    cases += [(s, isize, crc) for s, isize, crc, _ in corrupt_cases(seed=31, count=48) if isize <= 65536]
    comp, table, total = _table(cases)
    t = ctx.torch
    d_st = t.zeros(len(table), dtype=t.int32, device=ctx.device)
    out = t.zeros(total + 64, dtype=t.uint8, device=ctx.device)
    d_members = ctx.to_device(table.view(np.uint8))
    d_comp = ctx.bytes_to_device(comp)
    from uq_amd._lib import call
    call('uq_inflate_members', ctx.h, ops._p(d_comp), d_comp.numel(), ops._p(d_members), len(table), ops._p(out), total, ops._p(d_st))
    got = ctx.to_numpy(d_st, np.int32)
    host = [ops.inflate_member_host(s, isize, crc)[0] for s, isize, crc in cases]
    assert list(got) == host
    assert int(out[total:].sum()) == 0                                    # nothing past the table's last member


def test_qname_host_fallback_reads_inflated_bytes(ctx, tmp_path):
    names = [b'@r:%d{%d' % (i, 7 * i) for i in range(300)]                 # '{': a regex metacharacter -> the sequential host QNAME path
    fq = b''.join(n + b'\nACGTACGTAC\n+\nIIIIIIIIII\n' for n in names)
    plain_cfg, plain, _ = _encode(ctx, tmp_path, fq, [], name='in.fastq')
    for blob in (bgzf(fq, chunk=1000), gzip.compress(fq)):
        cfg, members, s = _encode(ctx, tmp_path, blob, [])
        assert s.path is None and s._host is not None                     # the host copy was made, from the device buffer
        assert members == plain and cfg == plain_cfg


@pytest.mark.parametrize('blob', [BGZF_EOF, gzip.compress(b''), bgzf(b'') + BGZF_EOF], ids=['bgzf_eof', 'gzip', 'bgzf_two_eof'])
def test_empty_gzip_is_empty_input(ctx, tmp_path, blob):
    with pytest.raises(uq.UqError) as e:
        _encode(ctx, tmp_path, blob, [])
    assert str(e.value) == 'ERROR: empty input'


def test_trailer_mismatch_names_the_member(ctx, tmp_path):
    data = fastq(3000)
    blob = bytearray(bgzf(data))
    kind, m, _, _ = ops.gzip_scan(np.frombuffer(bytes(blob), dtype=np.uint8))
    k = 2
    crc_at = int(m[k]['data_offset'] + m[k]['comp_bytes'])
    bad = bytearray(blob); bad[crc_at] ^= 0x40                            # CRC of member 2
    with pytest.raises(uq.UqError) as e:
        _encode(ctx, tmp_path, bytes(bad), [])
    assert 'member 2 (deflate data at byte %d)' % int(m[k]['data_offset']) in str(e.value) and 'CRC-32' in str(e.value)
    bad = bytearray(blob); bad[crc_at + 4] ^= 0x01                         # ISIZE of member 2 (65280 -> 65281)
    with pytest.raises(uq.UqError) as e:
        _encode(ctx, tmp_path, bytes(bad), [])
    assert 'member 2 (deflate data at byte %d)' % int(m[k]['data_offset']) in str(e.value) and 'ISIZE' in str(e.value)
    bad = blob[:len(blob) // 2]                                           # truncated: BSIZE past the end, refused by the scan
    with pytest.raises(uq.UqError) as e:
        _encode(ctx, tmp_path, bytes(bad), [])
    assert 'not a readable gzip file' in str(e.value)
    with pytest.raises(uq.UqError):                                       # the host path on a truncated single member
        _encode(ctx, tmp_path, gzip.compress(data)[:-100], [])


def test_bgzf_past_4_gib_on_the_device(ctx):
    """Synthetic FASTQ of more than 4 GiB as BGZF: the first 4.3 GB as stored members (so that the compressed offsets cross 2^31 and 2^32
    as well), the rest at level 1; inflated on the device = the generator's bytes."""
    t = ctx.torch
    spec = synth.Spec(20261016, 150)
    n = 13_000_000
    d_ref = ops.synth_fastq(ctx, spec, 0, n)
    size = d_ref.numel()
    assert size > (1 << 32) + (64 << 20)
    host = d_ref.cpu().numpy()
    chunk = 65280
    stored = ((1 << 32) + (32 << 20)) // chunk * chunk
    nst = stored // chunk
    msize = 18 + 5 + chunk + 8
    head = np.empty(nst * msize, dtype=np.uint8).reshape(nst, msize)
    hdr = np.frombuffer(b'\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00' + (msize - 1).to_bytes(2, 'little') +
                        b'\x01' + chunk.to_bytes(2, 'little') + (chunk ^ 0xFFFF).to_bytes(2, 'little'), dtype=np.uint8)
    head[:, :23] = hdr
    head[:, 23:23 + chunk] = host[:stored].reshape(nst, chunk)
    crcs = np.array([zlib.crc32(host[i * chunk:(i + 1) * chunk]) for i in range(nst)], dtype='<u4')
    head[:, 23 + chunk:27 + chunk] = crcs.view(np.uint8).reshape(nst, 4)
    head[:, 27 + chunk:] = np.frombuffer(chunk.to_bytes(4, 'little'), dtype=np.uint8)
    tail = bgzf(host[stored:].tobytes(), level=1)
    kind, m, total, _ = ops.gzip_scan(head.reshape(-1))
    kind2, m2, total2, _ = ops.gzip_scan(np.frombuffer(tail, dtype=np.uint8))
    assert kind == kind2 == ops.GZIP_BGZF and total + total2 == size
    m2['data_offset'] += head.size
    m2['out_offset'] += total
    members = np.concatenate([m, m2])
    assert int(members['data_offset'][-1]) > 1 << 32 and int(members['out_offset'][-1]) > 1 << 32
    d_comp = t.empty(head.size + len(tail), dtype=t.uint8, device=ctx.device)
    d_comp[:head.size].copy_(t.from_numpy(head.reshape(-1)))
    d_comp[head.size:].copy_(t.from_numpy(np.frombuffer(tail, dtype=np.uint8).copy()))
    del head, host
    out, bad = ops.inflate_members(ctx, d_comp, members, size)
    assert bad is None
    assert t.equal(out, d_ref)
