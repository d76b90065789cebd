"""The 64-read tile of the fused pack + statistics (+ QNAME) kernels (csrc/pack_geometry.h: a 22 KiB stage, 64 reads a tile, three lanes a
read beside a full parser wave, the tile's 257 line starts taken by 256 lanes) at the shapes where it can go wrong.  As
tests/test_gpu_pack_roles.py, whose `check` this file uses: the queued list forms with and without the QNAME phase, and the indexed fused
form, against ops.pack + ops.stats_accumulate + qname_device.analyse_device and oracle_c -- rows, the 256 x 256 counts, lengths, flags and
QNAME columns byte for byte.  Every case takes its tile from the library's query (ops.pack_tile_geometry) and asserts the geometry it was
built for.  (Without the QNAME phase a kernel has the 64-read tile only with an N-trick base -- the forms built for four workgroups per CU --
so the inputs of the plain list form carry Ns.)"""
import numpy as np
import pytest

import oracle_c
from test_gpu_pack_prefetch import digits, qnames, sim_name
from test_gpu_pack_roles import check, decide, fused
from test_gpu_pack_stores import fastq, group_zeroed
from uq_amd import ops, qname_device, synth

S = 20261022
gpu = pytest.mark.gpu
STAGE64 = 22 * 1024                                       # bytes of a 64-read tile's records, from the 16-byte boundary at or below the first
N_ENDS = dict(n_pos=lambda i, L: [[L - 1], [0], [0, L - 1], []][i % 4])       # an N as a read's last base, its first (the top group), both, none


def geometry(p, form):
    return ops.pack_tile_geometry(p, stats=True, qname=form.endswith('qname'), lists=form.startswith('lists'))


def assert_tile64(p, form, lanes):
    g = geometry(p, form)
    assert g.tile64 and (g.R, g.Rs, g.P, g.wg_per_cu, g.copies, g.stage_bytes) == (64, 64, min(lanes, g.G), 4, 4, STAGE64 + 32), g
    return g


def check_indexed_qname(ctx, host, n, guess=None, qname='exact'):
    """The indexed fused form WITH the QNAME phase (ops.pack_stats(fq=...): a record index, no lists) against the plain kernels, the exact
    QNAME passes and the oracle."""
    hls, ref, d, p = decide(host, n)
    if guess is not None: d, p = guess
    rd, rq, rbad = oracle_c.pack(host, hls, 0, n, d['bases'], d['qualities'], d['N_qual'], d['bits_per_base'], d['bits_per_quality'],
                                 d['variable_read_lengths'], d['dna_bytes_per_row'], d['quality_bytes_per_row'])
    assert rbad is None
    d_buf = ctx.to_device(host)
    ls = ops.index_lines(ctx, d_buf, ops.count_lines(ctx, d_buf))
    fq = ops.FusedQname(ctx, n + 7)
    ops.qname_guess(ctx, d_buf, ls, n, fq)
    sp = ops.pack_stats(ctx, d_buf, ls, 0, n, p, fq=fq)
    assert sp is not None, 'no fused kernel for this geometry'
    ops.qname_fused_finish(ctx, fq)
    hs = ops.stats_fetch(ctx, sp[3])
    assert not hs.incomplete and ops.bad_index(sp[2]) is None
    assert np.array_equal(ctx.to_numpy(sp[0]).reshape(n, -1), rd) and np.array_equal(ctx.to_numpy(sp[1]).reshape(n, -1), rq)
    assert np.array_equal(hs.counts, ref['counts'])
    assert (hs.len_min, hs.len_max, hs.max_record_bytes) == (ref['len_min'], ref['len_max'], ref['max_record_bytes'])
    from uq_amd.qname import QnameError
    got = qname_device.analyse_fused(ctx, fq, n)
    try: want = qname_device.analyse_device(ctx, d_buf, ls, n)
    except QnameError: want = None
    if (got is None or want is None) and qname == 'may-decline': return p      # (below 64 reads either analysis may decline: too few lines to tell a layout)
    assert got is not None and want is not None and got[:4] == want[:4]
    for a, b in zip(got[4], want[4]): assert ctx.torch.equal(a, b), 'a fused QNAME column differs from the exact passes\''
    return p


def run_form(ctx, host, n, form, **kw):
    if form == 'indexed-qname': return check_indexed_qname(ctx, host, n, **kw)
    return check(ctx, host, n, form == 'lists-qname', **kw)


FORMS = ['lists-qname', 'lists', 'indexed-qname']
LANES = {'lists-qname': 3, 'lists': 4, 'indexed-qname': 3}


def reads150(n, form, seed):
    """n reads of 150 bases; the plain list form's carry Ns (an N-trick base: see above)."""
    return fastq([sim_name(i) for i in range(n)], [150] * n, seed, **(N_ENDS if form == 'lists' else {}))


@gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('count', ['R-1', 'R', 'R+1', '2R+1', '3R'])
def test_read_counts_around_the_tile(ctx, count, form):
    """A tile short of one read, one full tile -- its last line start, the 257th, is the first one no lane had before --, a tile and a read,
    two tiles and a read, three full tiles."""
    R = 64
    n = {'R-1': R - 1, 'R': R, 'R+1': R + 1, '2R+1': 2 * R + 1, '3R': 3 * R}[count]
    host = reads150(n, form, S + 1)
    p = run_form(ctx, host, n, form, qname='may-decline' if n < 64 else 'exact')
    assert_tile64(p, form, LANES[form])


@gpu
@pytest.mark.parametrize('form', ['lists-qname', 'lists'])
@pytest.mark.parametrize('L', [8, 17, 24, 25, 48, 49, 150])
def test_fixed_lengths_at_three_lanes_a_read(ctx, L, form):
    """One group (8), as many groups as a read has lanes (17, 24: three), one more (25: four), the lanes' shares equal (48: six groups) and a
    top group of one symbol (17, 25, 49); 2R + 1 reads.  (The list form without the QNAME phase deals the same reads over four lanes.)"""
    n = 2 * 64 + 1
    host = fastq([sim_name(i) for i in range(n)], [L] * n, S + 2 + L, **(N_ENDS if form == 'lists' else {}))
    p = run_form(ctx, host, n, form)
    g = assert_tile64(p, form, LANES[form])
    assert g.G == (L + 7) // 8


def stage_end_input(width_of):
    """Names '@' + 30 x 'X' + ':' + a + ':' + b with b of five digits and a of width_of(read) digits: records of 343 + width bytes."""
    n = 4 * 64 + 1
    names = [b'@' + b'X' * 30 + b':' + digits(i, width_of(i)) + b':' + digits(i + 1, 5) for i in range(n)]
    return fastq(names, [150] * n, S + 3), n


@gpu
@pytest.mark.parametrize('form', ['lists-qname', 'indexed-qname'])
def test_records_that_end_with_the_stages_last_byte(ctx, form):
    """The guess comes from records of 351 bytes, the longest of which 64 fit the stage; the 64 records of tile 1 are 352 bytes each, and tile 0
    ends on a 16-byte boundary: tile 1 spans the stage to its last byte, its last read's windows are the stage's last bytes."""
    head, n = stage_end_input(lambda i: 8)
    _, _, d, p = decide(head, n)
    assert p.max_record_bytes == 351 and (64 * 351) % 16 == 0
    assert_tile64(p, form, 3)
    host, n = stage_end_input(lambda i: 9 if 64 <= i < 128 else 8)
    assert 64 * 352 == STAGE64
    run_form(ctx, host, n, form, guess=(d, p))


@gpu
@pytest.mark.parametrize('form', ['lists-qname', 'lists'])
def test_a_tile_one_byte_beyond_the_stage(ctx, form):
    """One record of tile 1 a byte longer still: the tile no longer fits the stage, is offered piece by piece (a piece of the 64-read tile is
    the tile itself: its records are longer than the guess allowed for) and left out -- *bad names its first read, the statistics come back
    incomplete -- and the tiles behind it are packed as ever."""
    kw = N_ENDS if form == 'lists' else {}
    n = 4 * 64 + 1
    def names(w): return [b'@' + b'X' * 30 + b':' + digits(i, w(i)) + b':' + digits(i + 1, 5) for i in range(n)]
    head = fastq(names(lambda i: 8), [150] * n, S + 4, **kw)
    hls, _, d, p = decide(head, n)
    assert_tile64(p, form, LANES[form])
    host = fastq(names(lambda i: 9 if 64 <= i < 127 else 10 if i == 127 else 8), [150] * n, S + 4, **kw)
    assert host.size == head.size + 63 + 2 and 63 * 352 + 353 == STAGE64 + 1
    hls = oracle_c.index_lines(host)
    rd, rq, rbad = oracle_c.pack(host, hls, 0, n, d['bases'], d['qualities'], d['N_qual'], d['bits_per_base'], d['bits_per_quality'],
                                 d['variable_read_lengths'], d['dna_bytes_per_row'], d['quality_bytes_per_row'])
    assert rbad is None
    q, hs, fq, (nl, ok) = fused(ctx, ctx.to_device(host), n, p, form == 'lists-qname')
    assert ok and nl == 4 * n and hs.incomplete and ops.bad_index(q[2]) == 64
    got_d, got_q = ctx.to_numpy(q[0][:n * rd.shape[1]]).reshape(n, -1), ctx.to_numpy(q[1][:n * rq.shape[1]]).reshape(n, -1)
    keep = np.r_[0:64, 128:n]
    assert np.array_equal(got_d[keep], rd[keep]) and np.array_equal(got_q[keep], rq[keep]), 'the tiles around the one left out'
    if fq is not None: assert qname_device.analyse_fused(ctx, fq, n) is None


@gpu
@pytest.mark.parametrize('form', ['lists-qname', 'lists'])
@pytest.mark.parametrize('mis', [1, 7, 15])
def test_buffers_off_a_16_byte_boundary(ctx, mis, form):
    n = 2 * 64 + 1
    p = check(ctx, reads150(n, form, S + 5), n, form == 'lists-qname', mis=mis)
    assert_tile64(p, form, LANES[form])


def parser_fields(n):
    W = [1, 4, 5, 8, 9]
    return [[digits(i, W[i % 5]), digits(i + 1, W[(i // 5) % 5]), digits(i + 2, W[(i // 25) % 5])] for i in range(n)]


@gpu
@pytest.mark.parametrize('form', ['lists-qname', 'indexed-qname'])
def test_parser_lanes_48_to_63_carry_the_column_extremes(ctx, form):
    """The parser wave's upper sixteen lanes had no read at 48 reads a tile: in every tile of this launch reads 48 .. 63 alone bear the
    smallest and largest values of the three columns, 0 and 999 999 999 among them."""
    n = 3 * 64 + 5
    f = parser_fields(n)
    for i in range(n): f[i] = [digits(i, 5), digits(i + 1, 5), digits(i + 2, 6)]
    for t in range(3):
        for k in range(48, 64):
            i = 64 * t + k
            f[i] = [b'%d' % (9999 - 600 * (k - 48) - t), b'%d' % (100000 + 50000000 * (k - 48) + t), b'%d' % ((1 - (k % 2)) * (999999999 - k - t) + (k % 2) * (k - 48 + t))]
    f[63] = [b'0', b'999999999', b'0']; f[64 + 48] = [b'999999999', b'0', b'999999999']
    host = fastq(qnames([tuple(x) for x in f]), [150] * n, S + 6)
    p = run_form(ctx, host, n, form)
    assert_tile64(p, form, 3)


@gpu
@pytest.mark.parametrize('bad', [b'007', b'', b'1234567890'], ids=['leading-zeros', 'empty', 'ten-digits'])
@pytest.mark.parametrize('k', [48, 63])
def test_parser_lanes_48_to_63_flag_what_they_must(ctx, k, bad):
    """A field the fused pass does not take, in read 48 or 63 of the second tile: the flag must arrive, the rows may not depend on it."""
    n = 3 * 64
    f = parser_fields(n)
    f[64 + k][k % 3] = bad
    host = fastq(qnames([tuple(x) for x in f]), [150] * n, S + 7)
    p = check(ctx, host, n, True, qname='flagged')
    assert_tile64(p, 'lists-qname', 3)
    fq = fused(ctx, ctx.to_device(host), n, p, True)[2]
    r = ops.qname_fused_fetch(ctx, fq)
    want = 4 if len(bad) > 9 else 16
    assert not r.ok or r.flags & want, 'flags %d: bit %d expected' % (r.flags, want)


@gpu
@pytest.mark.parametrize('what', ['quality', 'base'])
def test_symbol_outside_the_guess_in_read_63(ctx, what):
    """The last read of a full tile -- the last three lanes that pack -- bears a quality character beyond the guessed alphabet, or an N the
    guess has no code for, in its top group: incomplete statistics, *bad names the read, its rows are the oracle's with that group's bytes zero
    and every other row the oracle's."""
    n = 2 * 64 + 1
    clean = fastq([sim_name(i) for i in range(n)], [150] * n, S + 8)
    hls, _, d, p = decide(clean, n)
    assert_tile64(p, 'lists-qname', 3)
    k, host = 63, clean.copy()
    if what == 'quality': host[int(hls[4 * k + 3])] = ord('Z')
    else: host[int(hls[4 * k + 1])] = ord('N')
    rd, rq, rbad = oracle_c.pack(host, hls, 0, n, d['bases'], d['qualities'], d['N_qual'], d['bits_per_base'], d['bits_per_quality'],
                                 d['variable_read_lengths'], d['dna_bytes_per_row'], d['quality_bytes_per_row'])
    assert rbad == k
    rd, rq = rd.copy(), rq.copy()
    rd[k] = group_zeroed(rd[k], 2, 18); rq[k] = group_zeroed(rq[k], d['bits_per_quality'], 18)
    d_buf = ctx.to_device(host)
    ls = ops.index_lines(ctx, d_buf, ops.count_lines(ctx, d_buf))
    fq = ops.FusedQname(ctx, n + 7); ops.qname_guess(ctx, d_buf, ls, n, fq)
    results = {'lists-qname': fused(ctx, d_buf, n, p, True)[0], 'indexed-qname': ops.pack_stats(ctx, d_buf, ls, 0, n, p, fq=fq)}
    for form, res in results.items():
        assert res is not None and ops.bad_index(res[2]) == k, form
        assert np.array_equal(ctx.to_numpy(res[0][:n * rd.shape[1]]).reshape(n, -1), rd), 'DNA rows (%s)' % form
        assert np.array_equal(ctx.to_numpy(res[1][:n * rq.shape[1]]).reshape(n, -1), rq), 'QUAL rows (%s)' % form
        assert ops.stats_fetch(ctx, res[3]).incomplete, form


@gpu
@pytest.mark.parametrize('form', FORMS)
def test_n_trick_with_an_n_in_the_top_group(ctx, form):
    """150 bp, every second read with an N among its first six bases (group 18, the partial one, which the third lane of a read takes -- the
    fourth without the QNAME phase), read 63 of the first tile among them."""
    n = 2 * 64 + 1
    host = fastq([sim_name(i) for i in range(n)], [150] * n, S + 9, n_pos=lambda i, L: [i % 6] if i % 2 else [L - 1 - i % 7])
    p = run_form(ctx, host, n, form)
    assert any(v >= 0 for v in p.n_qual) and p.bits_per_base == 2
    assert_tile64(p, form, LANES[form])


@gpu
def test_three_bit_bases_keep_their_tile(ctx):
    """N kept as a fifth base: 512 bins a copy of the count table do not leave the LDS for the larger stage -- the geometry is the one from
    before (48 reads, four copies), and the query says so."""
    dk = dict(notricks=True)
    n = 2 * 48 + 1
    host = fastq([sim_name(i) for i in range(n)], [150] * n, S + 10, n_rate=5, nq=17)
    for qn in (True, False):
        p = check(ctx, host, n, qn, **dk)
        g = geometry(p, 'lists-qname' if qn else 'lists')
        assert p.bits_per_base == 3 and not g.tile64 and (g.R, g.copies, g.stage_bytes) == (48, 4, 16 * 1024 + 32), g


@gpu
@pytest.mark.parametrize('notricks', [False, True], ids=['var-ntrick', 'var-notricks'])
def test_36_to_301_bp_keeps_its_tile(ctx, notricks):
    """Rows of 303 bytes a read: 64 of them do not fit beside the larger stage, the query reports the geometry unchanged."""
    from test_gpu_pack_roles import tile_reads
    dk = dict(notricks=True) if notricks else {}
    head = synth.fastq_array(synth.Spec(S + 11, (36, 301), n_rate=1), 300)
    hls, _, d, p = decide(head, 300, **dk)
    g = geometry(p, 'lists-qname')
    assert not g.tile64 and g.R == tile_reads(p) and g.stage_bytes == 16 * 1024 + 32 and g.copies == (4 if notricks else 8), g
    n = 2 * g.R + 1
    check(ctx, head[:int(hls[4 * n])].copy(), n, True, guess=(d, p), **dk)
