"""The table-driven pack and decode kernels at every symbol width against the C oracle (which test_width_matrix_cpu.py holds to the
reference's own loops on the same cases, without a GPU).

Every input whose alphabet is not the benchmark's -- binned or scattered qualities, IUPAC or lower-case bases, --pad, 7- and 8-bit
qualities -- is packed by one of the 128 plain pack_tile_kernel<BD, BQ, NTRICK> instances or by pack_carry_kernel, and comes back
through the run-time-width decoders: unpack_pipe_kernel / unpack_kernel / unpack_long_kernel, the default emit_tile_kernel<true> with
direct_tiles_kernel<true>, row_lengths_kernel.  The matrix of width_matrix_inputs launches each of the 64 width pairs with fixed and
variable lengths, without an N-trick, with one that shares a code of the alphabet and with the reference's NEW code (Q9, which at
1 .. 3 bits carries: pack_carry_kernel), on alphabets the lookup-free forms take ('letters' at 2 and 3 bits of base) and on ones they
refuse ('scattered').  The parameters are built directly: decide() never yields width 1 and cannot be steered to most widths.

Excluded, as everywhere in the suite: the decode of a NEW N code (Q9), which the reference cannot decode either -- those 256 of the
768 cases are packed and compared, not decoded.

The kernel-selection ladder walks uq_unpack's two switches with few, long reads, and a 21 000-base read among short ones reaches
pack_carry_kernel with a sentinel, direct_tiles_kernel and row_lengths_kernel<64>.  The command-line subset holds decide() and the
JSON path to the wide alphabets."""
import json

import numpy as np
import pytest

import oracle_c
import uq_oracle as O
import width_matrix_inputs as W
from uq_amd import ops, qname

pytestmark = pytest.mark.gpu
GUARD = 256


def _dev(ctx, a):
    return ctx.to_device(np.ascontiguousarray(a))


@pytest.fixture(scope='module')
def refs():
    """The oracle's side of a case, computed once per case and shared by the tests of this module: index, rows, unpacked text."""
    cache = {}

    def get(key, c):
        if key not in cache:
            host = np.frombuffer(c['fastq'], dtype=np.uint8)
            hls = oracle_c.index_lines(host)
            n = c['n']
            assert len(hls) == 4 * n + 1
            rd, rq, bad = oracle_c.pack(host, hls, 0, n, c['bases'], c['qualities'], c['N_qual'], c['bits_per_base'], c['bits_per_quality'],
                                        c['variable_read_lengths'], c['dna_bytes_per_row'], c['quality_bytes_per_row'])
            assert bad is None
            un = oracle_c.unpack(rd, rq, c) if c['decodable'] else None
            rec = int((hls[4::4] - hls[:-1:4]).max())
            for a in (host, hls, rd, rq) + (un[:3] if un else ()): a.setflags(write=False)
            cache[key] = dict(host=host, hls=hls, rd=rd, rq=rq, un=un, max_record_bytes=rec)
        return cache[key]
    return get


def _guarded(ctx, nbytes):
    """A slice of nbytes inside a larger allocation of 0xA5 with GUARD bytes in front (the slice keeps the alignment the library always gets)
    and behind."""
    whole = ctx.empty(GUARD + nbytes + GUARD)
    whole.fill_(0xA5)
    return whole, whole[GUARD:GUARD + nbytes]


def _guards_intact(ctx, whole, nbytes):
    w = ctx.to_numpy(whole)
    return bool((w[:GUARD] == 0xA5).all() and (w[GUARD + nbytes:] == 0xA5).all())


def _pack_args(c, max_record_bytes):
    return (c['bases'], c['qualities'], c['N_qual'], c['bits_per_base'], c['bits_per_quality'], c['variable_read_lengths'],
            c['dna_bytes_per_row'], c['quality_bytes_per_row'], c['dna_max'], max_record_bytes)


def _check_pack(ctx, c, ref, tag, fused=True):
    n, Cd, Cq = c['n'], c['dna_bytes_per_row'], c['quality_bytes_per_row']
    p = ops.make_pack_params(*_pack_args(c, ref['max_record_bytes']))
    assert bytes(p) == bytes(ops.make_pack_params_py(*_pack_args(c, ref['max_record_bytes']))), tag + ': uq_make_pack_params differs from its numpy twin'
    d_buf = _dev(ctx, ref['host']); ls = _dev(ctx, ref['hls'])
    wd, dna = _guarded(ctx, n * Cd); wq, qual = _guarded(ctx, n * Cq)
    _, _, bad = ops.pack(ctx, d_buf, ls, 0, n, p, dna=dna, qual=qual)
    assert ops.bad_index(bad) is None, tag + ': uq_pack reports an uncoded symbol'
    got_d, got_q = ctx.to_numpy(dna).reshape(n, Cd), ctx.to_numpy(qual).reshape(n, Cq)
    assert np.array_equal(got_d, ref['rd']), '%s: DNA rows differ from the oracle (first at row %d)' % (tag, int(np.flatnonzero((got_d != ref['rd']).any(axis=1))[0]))
    assert np.array_equal(got_q, ref['rq']), '%s: QUAL rows differ from the oracle (first at row %d)' % (tag, int(np.flatnonzero((got_q != ref['rq']).any(axis=1))[0]))
    assert _guards_intact(ctx, wd, n * Cd) and _guards_intact(ctx, wq, n * Cq), tag + ': uq_pack wrote outside its tables'
    if fused:
        res = ops.pack_stats(ctx, d_buf, ls, 0, n, p)                    # (None: this geometry has no fused kernel)
        if res is not None:
            assert not ops.stats_fetch(ctx, res[3]).incomplete, tag + ': fused statistics incomplete under the true parameters'
            assert ops.bad_index(res[2]) is None, tag
            assert np.array_equal(ctx.to_numpy(res[0]).reshape(n, Cd), ref['rd']) and np.array_equal(ctx.to_numpy(res[1]).reshape(n, Cq), ref['rq']), \
                tag + ': rows of the fused kernel differ from the oracle'


def _check_decode(ctx, c, ref, tag, seed):
    """uq_unpack, uq_decode_fastq and uq_unpack + uq_emit_fastq on the oracle's rows."""
    n = c['n']
    host = ref['host']
    prefix, suffix, separators, columns, arrays = qname.analyse(qname.qname_lines(host, ref['hls'], n))
    cfg = dict(bases=c['bases'], qualities=c['qualities'], N_qual=c['N_qual'], bits_per_base=c['bits_per_base'],
               bits_per_quality=c['bits_per_quality'], variable_read_lengths=c['variable_read_lengths'], dna_max=c['dna_max'],
               QNAME_prefix=prefix, QNAME_suffix=suffix, QNAME_separators=separators, QNAME_columns=columns)
    cols = [_dev(ctx, np.ascontiguousarray(a)) for a in arrays]
    dna, qual = _dev(ctx, ref['rd'].ravel()), _dev(ctx, ref['rq'].ravel())
    up = ops.make_unpack_params(cfg)
    assert (up.dna_bytes_per_row, up.quality_bytes_per_row) == (c['dna_bytes_per_row'], c['quality_bytes_per_row'])
    ops.scribble_lds(ctx, 0x96969696 ^ seed)
    seq, qt, ln, bad = ops.unpack(ctx, dna, qual, n, up)
    rs, rqt, rln, rbad = ref['un']
    assert rbad is None and ops.bad_index(bad) is None, tag + ': uq_unpack reports a row without a sentinel'
    assert np.array_equal(ctx.to_numpy(ln, np.uint32), rln), tag + ': read lengths differ from the oracle'
    assert np.array_equal(ctx.to_numpy(seq).reshape(n, -1), rs), tag + ': unpacked bases differ from the oracle'
    assert np.array_equal(ctx.to_numpy(qt).reshape(n, -1), rqt), tag + ': unpacked qualities differ from the oracle'
    text = host.tobytes()
    ops.scribble_lds(ctx, 0x69696969 ^ seed)
    got, bad = ops.decode_fastq(ctx, cfg, cols, dna, qual, n)
    assert bad is None and ctx.to_numpy(got).tobytes() == text, tag + ': uq_decode_fastq is not the input text'
    two = ops.emit_fastq(ctx, cfg, cols, seq, qt, ln, n)
    assert ctx.to_numpy(two).tobytes() == text, tag + ': uq_unpack + uq_emit_fastq is not the input text'
    assert ops.decode_fastq(ctx, cfg, cols, dna, qual, n, size_only=True) == (len(text), None), tag + ': size pass'
    if c['variable_read_lengths'] and n > 7:
        rd2 = ref['rd'].copy(); rd2[7, :] = 0                            # a row without its sentinel is named
        assert ops.decode_fastq(ctx, cfg, cols, _dev(ctx, rd2.ravel()), qual, n) == (None, 7), tag + ': row 7 without a sentinel'


@pytest.mark.parametrize('bq', range(1, 9), ids=lambda v: 'q%d' % v)
@pytest.mark.parametrize('bd', range(1, 9), ids=lambda v: 'd%d' % v)
def test_width_pair_against_the_oracle(ctx, refs, bd, bq):
    """The twelve sub-cases of one width pair (fixed / variable x no N-trick / shared code / NEW code x letters / scattered): plain pack,
    the parameter builder, the fused form where there is one, unpack and both decoders, all against oracle_c and the input text."""
    decoded = 0
    for k, (variable, ntrick, alphabet) in enumerate((v, t, a) for v in (False, True) for t in W.NTRICKS for a in W.ALPHABETS):
        c = W.case(bd, bq, variable, ntrick, alphabet)
        tag = W.case_id(bd, bq, variable, ntrick, alphabet)
        ref = refs(tag, c)
        _check_pack(ctx, c, ref, tag)
        if c['decodable']:
            _check_decode(ctx, c, ref, tag, (bd * 8 + bq) * 12 + k)
            decoded += 1
        else:
            assert ntrick == 'new'                                       # Q9, the one exclusion
    assert decoded == 8


# ------------------------------------------------------------------ the kernel-selection ladder
def _unpack_route(bd, bq, dna_max, variable):
    """Which kernel uq_unpack launches (uq_amd/csrc/unpack.hip), restated: per_read = Cd + Cq + 2 dna_max + 4 bytes of LDS a read; the
    pipelined kernel while 31 KiB hold 16 reads (and its registers their rows), the wave-per-read kernel once a read with 256 bytes of
    slack passes 150 KiB, the tile kernel in between."""
    lv = dna_max + (1 if variable else 0)
    Cd, Cq = (bd * lv + 7) // 8, (bq * lv + 7) // 8
    per_read = Cd + Cq + 2 * dna_max + 4
    if per_read + 256 > 150 * 1024: return 'unpack_long_kernel'
    Rp = (31 * 1024) // per_read
    if Rp >= 16: Rp &= ~15
    Rp = min(Rp, 256)
    if Rp >= 16 and Rp * Cd + 48 <= 2 * 256 * 16 and Rp * Cq + 48 <= 4 * 256 * 16: return 'unpack_pipe_kernel'
    return 'unpack_kernel'


def _last_length_on(bd, bq, route):
    """The longest fixed read length that still takes `route` (the routes follow one another as the length grows)."""
    lo, hi = 1, 1 << 17
    order = ['unpack_pipe_kernel', 'unpack_kernel', 'unpack_long_kernel']
    assert _unpack_route(bd, bq, lo, False) == 'unpack_pipe_kernel' and _unpack_route(bd, bq, hi, False) == 'unpack_long_kernel'
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if order.index(_unpack_route(bd, bq, mid, False)) <= order.index(route): lo = mid
        else: hi = mid
    return lo


LADDER_PAIRS = [(8, 8), (5, 7), (2, 6)]


def test_ladder_switches_restated():
    """Where the restated formula puts the two switches at 8 + 8 bits: per_read = 4 L + 4, so 31 KiB / per_read is 16 up to L = 495
    and per_read + 256 passes 150 KiB from L = 38 336 on."""
    assert _last_length_on(8, 8, 'unpack_pipe_kernel') == 495 and _last_length_on(8, 8, 'unpack_kernel') == 38335
    assert (31 * 1024) // (4 * 495 + 4) == 16 and (31 * 1024) // (4 * 496 + 4) == 15
    assert 4 * 38335 + 4 + 256 == 150 * 1024 and 4 * 38336 + 4 + 256 > 150 * 1024


@pytest.mark.parametrize('step', [0, 1], ids=['below', 'above'])
@pytest.mark.parametrize('switch', ['pipe-to-tile', 'tile-to-long'])
@pytest.mark.parametrize('bd,bq', LADDER_PAIRS, ids=lambda v: str(v))
def test_ladder_fixed_lengths(ctx, refs, bd, bq, switch, step):
    """One step either side of each of uq_unpack's two switches: 40 reads around the length where the pipelined kernel's tile falls below
    16 reads, 6 reads around the length where a row no longer fits an LDS tile.  uq_unpack, uq_decode_fastq and uq_pack against oracle_c
    and the text."""
    first = switch == 'pipe-to-tile'
    L = _last_length_on(bd, bq, 'unpack_pipe_kernel' if first else 'unpack_kernel') + step
    want = (['unpack_pipe_kernel', 'unpack_kernel'] if first else ['unpack_kernel', 'unpack_long_kernel'])[step]
    assert _unpack_route(bd, bq, L, False) == want
    c = W.ladder_case(bd, bq, L, 40 if first else 6)
    assert c['dna_max'] == L and not c['variable_read_lengths'] and c['decodable']
    tag = 'ladder %d.%d L=%d (%s)' % (bd, bq, L, want)
    ref = refs(tag, c)
    _check_pack(ctx, c, ref, tag, fused=False)
    _check_decode(ctx, c, ref, tag, L)


@pytest.mark.parametrize('bd,bq', LADDER_PAIRS, ids=lambda v: str(v))
def test_ladder_one_long_read_among_short_ones(ctx, refs, bd, bq):
    """Variable lengths, one read of 21 000 bases among 30 of up to 60: its record passes the pack kernel's 20 KiB stage, so pack_carry_kernel
    packs the table -- with a sentinel --; its text passes the decode tile (direct_tiles_kernel), and rows beyond 512 bytes take
    row_lengths_kernel<64>."""
    c = W.ladder_case(bd, bq, 21000, 31, short=60)
    assert c['variable_read_lengths'] and c['decodable'] and max(c['lengths']) == 21000 and sorted(c['lengths'])[-2] <= 60
    tag = 'ladder %d.%d one long read' % (bd, bq)
    ref = refs(tag, c)
    assert ref['max_record_bytes'] + 64 > 20 * 1024 and c['dna_bytes_per_row'] > 512
    _check_pack(ctx, c, ref, tag, fused=False)
    _check_decode(ctx, c, ref, tag, 21000)


# ------------------------------------------------------------------ the command line on wide alphabets
# (bd, bq, variable, flags, quality symbols): the diagonal with variable lengths, four off-diagonal pairs with fixed lengths; 8 bits of
# quality from printable characters take --pad (17 .. symbols -> 8 bits)
CLI_CASES = [(k, k, True, [], None) for k in range(2, 8)] + [(7, 2, False, [], None), (2, 7, False, [], None), (2, 8, False, ['--pad'], 41), (4, 3, False, [], None)]


@pytest.mark.parametrize('bd,bq,variable,flags,nq', CLI_CASES, ids=['%d.%d-%s' % (c[0], c[1], 'variable' if c[2] else 'fixed') for c in CLI_CASES])
def test_cli_on_wide_alphabets(ctx, tmp_path, bd, bq, variable, flags, nq):
    """decide() and the container's JSON on scattered printable alphabets of every width: the encode through uq.Session equals O.encode
    member for member and key for key, the widths in config.json are the ones the case was built for, the decode equals O.decode."""
    from test_gpu_e2e import _run_decode, _run_encode
    c = W.printable_case(bd, bq, variable, nq=nq)
    fq = c['fastq']
    ocfg, omembers, _ = O.encode(fq, sort=None, raw=None, pattern=None, notricks=False, pad='--pad' in flags)
    cfg, members, names, path = _run_encode(ctx, tmp_path, fq, flags)
    assert (cfg['bits_per_base'], cfg['bits_per_quality']) == (ocfg['bits_per_base'], ocfg['bits_per_quality']) == (bd, bq)
    assert cfg['bases'] == c['bases'] and cfg['qualities'] == c['qualities'] and cfg['N_qual'] == {} and cfg['variable_read_lengths'] == variable
    assert set(members) == set(omembers)
    for k in omembers: assert members[k] == omembers[k], k
    for k in ocfg:
        if k in ('sort', 'raw', 'pattern'): continue
        assert json.loads(json.dumps(cfg[k])) == json.loads(json.dumps(ocfg[k])), k
    text = _run_decode(ctx, path)
    assert text.decode('latin-1') == O.decode(ocfg, omembers) and text == fq
