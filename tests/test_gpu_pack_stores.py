"""The group loop of the pack kernels after DESIGN 29: a group's bytes go into the LDS image of the rows as byte stores (never a merged,
unaligned wide one), both windows of a group are requested together, and a lane's FULL groups run through a straight-line body that leaves
for the general code when any lane of the wave meets a symbol outside the guess.  What can go wrong there shows at the row widths (Cd / Cq
even, odd, mixed), at reads that are all partial group, all full groups or full groups and one symbol, where rows begin at every byte
residue of the out tile, and at a wrong guess inside a full group or inside the partial one.  As tests/test_gpu_pack_roles.py (whose `check`
this file uses): the queued list forms with and without the QNAME phase and the indexed fused form against ops.pack +
ops.stats_accumulate + qname_device.analyse_device and oracle_c -- rows, counts, lengths, flags and QNAME columns byte for byte."""
import numpy as np
import pytest

import oracle_c
from test_gpu_pack_prefetch import check_indexed, digits, qnames, sim_name
from test_gpu_pack_roles import FAMILIES, check, decide, device_buffer, fused, tile_reads
from uq_amd import ops, synth

S = 20261021
gpu = pytest.mark.gpu
ACGT = np.frombuffer(b'ACGT', dtype=np.uint8)
LENGTHS = [1, 7, 8, 9, 15, 16, 17, 24, 150]
FORMS = ['lists', 'lists-qname', 'indexed']


def fastq(names, lens, seed, nq=41, n_pos=None, n_rate=0):
    """name / bases / '+' / qualities per record; the qualities run through an alphabet of `nq` consecutive characters from '!' in turn.
    n_pos(i, L) -> positions of read i that bear an N, n_rate: per cent of random positions that do; an N bears '!' alone and the other
    bases the remaining nq - 1 characters, which is what makes N an N-trick base."""
    rng = np.random.default_rng(seed)
    with_n = n_pos is not None or n_rate > 0
    parts, k = [], 0
    for i, (nm, L) in enumerate(zip(names, lens)):
        seq = ACGT[rng.integers(0, 4, L)]
        if with_n:
            q = (34 + (k + np.arange(L)) % (nq - 1)).astype(np.uint8)
            isn = rng.integers(0, 100, L) < n_rate
            if n_pos is not None: isn[[p for p in n_pos(i, L) if 0 <= p < L]] = True
            seq = np.where(isn, 78, seq).astype(np.uint8); q = np.where(isn, 33, q).astype(np.uint8)
        else:
            q = (33 + (k + np.arange(L)) % nq).astype(np.uint8)
        k += L
        parts += [nm, b'\n', seq.tobytes(), b'\n+\n', q.tobytes(), b'\n']
    return np.frombuffer(b''.join(parts), dtype=np.uint8).copy()


def fixed_input(L, count, seed, **kw):
    """`count`(R) reads of L bases, R being the tile these reads give (short records: the largest tile, 56 reads)."""
    dk = kw.pop('dk', {})
    probe = fastq([sim_name(i) for i in range(127)], [L] * 127, seed, **kw)
    R = tile_reads(decide(probe, 127, **dk)[3])
    n = count(R)
    return fastq([sim_name(i) for i in range(n)], [L] * n, seed, **kw), n, R


def check_forms(ctx, host, n, forms=FORMS, **dk):
    p = None
    for form in forms:
        if form == 'indexed': check_indexed(ctx, host, n, **dk)
        else: p = check(ctx, host, n, form == 'lists-qname', qname='may-decline' if n < 64 else 'exact', **dk)
    return p


@gpu
@pytest.mark.parametrize('nq', [3, 5, 9, 17, 33, 64])
@pytest.mark.parametrize('L', LENGTHS)
def test_fixed_lengths_two_bit_bases_every_quality_width(ctx, L, nq):
    """2-bit bases, 2 - 6 bits of quality, 2R + 1 reads: rows of Cd = ceil(L / 4) and Cq = ceil(bits * L / 8) bytes -- both even, both odd
    and mixed -- made of a partial group alone (1, 7), of full groups alone (8, 16, 24), of full groups and one symbol (9, 17) or seven (15)."""
    host, n, R = fixed_input(L, lambda R: 2 * R + 1, S + 64 * L + nq, nq=nq)
    p = check_forms(ctx, host, n)
    assert p.bits_per_base == 2 and (1 << p.bits_per_quality) >= nq > (1 << (p.bits_per_quality - 1)) and not p.variable and tile_reads(p) == R


@gpu
@pytest.mark.parametrize('nq', [5, 17])
@pytest.mark.parametrize('L', LENGTHS)
def test_fixed_lengths_three_bit_bases(ctx, L, nq):
    """The same with N kept as a fifth base (3 bits): the instances that look their codes up with v_perm_b32 and count pair by pair."""
    dk = dict(notricks=True)
    host, n, R = fixed_input(L, lambda R: 2 * R + 1, S + 64 * L + nq + 1, nq=nq, n_rate=5, n_pos=lambda i, L: [i % L] if i % 5 == 0 else [], dk=dk)
    p = check_forms(ctx, host, n, **dk)
    assert p.bits_per_base == 3 and not p.variable and tile_reads(p) == R


@gpu
@pytest.mark.parametrize('nq', [3, 9, 64])
@pytest.mark.parametrize('L', [7, 9, 15, 17, 24, 150])
def test_n_trick_in_a_full_group_and_in_the_partial_one(ctx, L, nq):
    """The N-trick instances: reads with an N as their last base (group 0: a full group from 8 bases on), as their first (the top group: the
    partial one unless L is a multiple of 8), both, and none -- so that waves meet the N in the straight-line body and in the general code."""
    where = lambda i, L: [[L - 1], [0], [0, L - 1], []][i % 4]
    host, n, R = fixed_input(L, lambda R: 2 * R + 1, S + 64 * L + nq + 2, nq=nq, n_pos=where)
    p = check_forms(ctx, host, n)
    assert p.bits_per_base == 2 and tile_reads(p) == R


@gpu
@pytest.mark.parametrize('count', ['R-1', 'R', 'R+1', '2R+1'])
@pytest.mark.parametrize('L', [7, 9, 17, 150])
def test_rows_begin_at_every_residue_of_the_out_tile(ctx, L, count):
    """R - 1, R, R + 1 and 2R + 1 reads with odd row widths (Cd = 2, 3, 5, 38; Cq = 6, 7, 13, 113 at six bits): the rows of a tile begin at every
    residue modulo 4, and the QUAL image begins behind R, R - 1 or one DNA rows."""
    host, n, R = fixed_input(L, {'R-1': lambda R: R - 1, 'R': lambda R: R, 'R+1': lambda R: R + 1, '2R+1': lambda R: 2 * R + 1}[count], S + 7 * L)
    check_forms(ctx, host, n)


@gpu
@pytest.mark.parametrize('count', ['R-1', 'R', 'R+1', '2R+1'])
@pytest.mark.parametrize('family', ['var-notricks', 'var-ntrick'])
def test_variable_lengths(ctx, family, count):
    """36 - 301 bp with 1 % N (the instances that deal only the groups a read has): the lanes of a wave leave the straight-line body at
    different groups and all take the sentinel's group in the general code."""
    length, kw, dk = FAMILIES[family]
    head = synth.fastq_array(synth.Spec(S + 3, length, **kw), 400)
    hls, _, d, p = decide(head, 400, **dk)
    R = tile_reads(p)
    n = {'R-1': R - 1, 'R': R, 'R+1': R + 1, '2R+1': 2 * R + 1}[count]
    host = head[:int(hls[4 * n])].copy()
    for form in ('lists', 'lists-qname'):
        check(ctx, host, n, form == 'lists-qname', qname='may-decline' if n < 64 else 'exact', guess=(d, p), **dk)
    check_indexed(ctx, host, n, **dk)


@gpu
@pytest.mark.parametrize('mis', [1, 7, 15])
@pytest.mark.parametrize('kind', ['17bp', '150bp-ntrick', 'var-ntrick'])
def test_buffers_off_a_16_byte_boundary(ctx, kind, mis):
    """The stage then begins `mis` bytes into the tile's first 16-byte vector: every window's byte phase moves with it."""
    if kind == 'var-ntrick':
        length, kw, dk = FAMILIES[kind]
        head = synth.fastq_array(synth.Spec(S + 4, length, **kw), 300)
        hls, _, d, p = decide(head, 300, **dk)
        n = 2 * tile_reads(p) + 1
        check(ctx, head[:int(hls[4 * n])].copy(), n, True, mis=mis, guess=(d, p), **dk)
        return
    kw = dict(n_pos=lambda i, L: [[L - 1], [0], []][i % 3]) if kind == '150bp-ntrick' else {}
    host, n, _ = fixed_input(150 if kind == '150bp-ntrick' else 17, lambda R: 2 * R + 1, S + 5, **kw)
    for qn in (False, True): check(ctx, host, n, qn, mis=mis)


# ---- a symbol outside the guess
def group_zeroed(row, bits, gg):
    """The row with the bytes of group gg (eight symbols from the read's end: `bits` whole bytes from the row's end) zero."""
    out = row.copy()
    hi = row.size - bits * gg
    out[max(hi - bits, 0):hi] = 0
    return out


@gpu
@pytest.mark.parametrize('where', ['full-group', 'partial-group'])
@pytest.mark.parametrize('what', ['quality', 'base'])
@pytest.mark.parametrize('L', [17, 150])
def test_symbol_outside_the_guess(ctx, L, what, where):
    """The guess comes from the file without the symbol; one read of the second tile then bears a quality character beyond the alphabet, or an
    N the guess has no code for, in group 1 (a full one) or in its top, partial group.  As before: the statistics come back incomplete, *bad
    names the read (as the oracle does), every other row is the oracle's, and the read's own rows are the oracle's with that group's bytes zero --
    in the queued forms, the indexed fused form and the plain kernel alike."""
    clean, n, R = fixed_input(L, lambda R: 2 * R + 1, S + 11 * L)
    hls, _, d, p = decide(clean, n)
    k = R + 5
    pos = L - 1 - 8 - 3 if where == 'full-group' else 0
    gg = (L - 1 - pos) // 8
    assert (8 * gg + 8 <= L) == (where == 'full-group')
    host = clean.copy()
    if what == 'quality': host[int(hls[4 * k + 3]) + pos] = ord('Z')
    else: host[int(hls[4 * k + 1]) + pos] = ord('N')
    rd, rq, rbad = oracle_c.pack(host, hls, 0, n, d['bases'], d['qualities'], d['N_qual'], d['bits_per_base'], d['bits_per_quality'],
                                 d['variable_read_lengths'], d['dna_bytes_per_row'], d['quality_bytes_per_row'])
    assert rbad == k
    rd, rq = rd.copy(), rq.copy()
    rd[k] = group_zeroed(rd[k], d['bits_per_base'], gg); rq[k] = group_zeroed(rq[k], d['bits_per_quality'], gg)
    d_buf = ctx.to_device(host)
    ls = ops.index_lines(ctx, d_buf, ops.count_lines(ctx, d_buf))
    results = {'plain': ops.pack(ctx, d_buf, ls, 0, n, p) + (None,), 'indexed': ops.pack_stats(ctx, d_buf, ls, 0, n, p)}
    for qn in (False, True): results['lists-qname' if qn else 'lists'] = fused(ctx, d_buf, n, p, qn)[0]
    for form, res in results.items():
        assert res is not None, form
        assert ops.bad_index(res[2]) == k, form
        assert np.array_equal(ctx.to_numpy(res[0][:n * rd.shape[1]]).reshape(n, -1), rd), 'DNA rows (%s)' % form
        assert np.array_equal(ctx.to_numpy(res[1][:n * rq.shape[1]]).reshape(n, -1), rq), 'QUAL rows (%s)' % form
        if res[3] is not None: assert ops.stats_fetch(ctx, res[3]).incomplete, form


@gpu
@pytest.mark.parametrize('where', ['full-group', 'partial-group'])
@pytest.mark.parametrize('L', [17, 150])
def test_n_trick_base_with_a_second_quality(ctx, L, where):
    """An N-trick guess, and one N of the file bears another quality character than the guess says: the rows are the oracle's (the N's code
    does not depend on its character), nothing is bad, and the counts come back incomplete."""
    npos = lambda i, L: [[L - 1], [0], []][i % 3]
    clean, n, R = fixed_input(L, lambda R: 2 * R + 1, S + 13 * L, n_pos=npos)
    hls, _, d, p = decide(clean, n)
    assert d['N_qual']
    k = next(i for i in range(R + 3, n) if i % 3 == (0 if where == 'full-group' else 1))      # (i % 3 picks the read's N: its last base, or its first)
    pos = npos(k, L)[0]
    assert pos == (L - 1 if where == 'full-group' else 0)
    host = clean.copy()
    q_at = int(hls[4 * k + 3]) + pos
    assert host[q_at] == 33
    host[q_at] = 40
    rd, rq, rbad = oracle_c.pack(host, hls, 0, n, d['bases'], d['qualities'], d['N_qual'], d['bits_per_base'], d['bits_per_quality'],
                                 d['variable_read_lengths'], d['dna_bytes_per_row'], d['quality_bytes_per_row'])
    assert rbad is None
    d_buf = ctx.to_device(host)
    ls = ops.index_lines(ctx, d_buf, ops.count_lines(ctx, d_buf))
    results = {'indexed': ops.pack_stats(ctx, d_buf, ls, 0, n, p)}
    for qn in (False, True): results['lists-qname' if qn else 'lists'] = fused(ctx, d_buf, n, p, qn)[0]
    for form, res in results.items():
        assert res is not None and ops.bad_index(res[2]) is None, form
        assert np.array_equal(ctx.to_numpy(res[0][:n * rd.shape[1]]).reshape(n, -1), rd), 'DNA rows (%s)' % form
        assert np.array_equal(ctx.to_numpy(res[1][:n * rq.shape[1]]).reshape(n, -1), rq), 'QUAL rows (%s)' % form
        assert ops.stats_fetch(ctx, res[3]).incomplete, form


# ---- the parser: '@q' + a + ':' + b + '/' + c, three numeric fields
WIDTHS = [1, 4, 5, 8, 9]


@gpu
@pytest.mark.parametrize('edge', ['widths', 'min-max', 'moving-extremes'])
def test_qname_field_values(ctx, edge):
    """Fields of 1, 4, 5, 8 and 9 digits in every column, 0 and 999 999 999 as a column's smallest and largest value, and columns whose
    smallest (first column), largest (second) or both (third) values so far change in every tile of the launch."""
    n = 230
    f = [(digits(i, WIDTHS[i % 5]), digits(i + 1, WIDTHS[(i // 5) % 5]), digits(i + 2, WIDTHS[(i // 25) % 5])) for i in range(n)]
    if edge == 'min-max':
        f[3] = (b'0', b'999999999', b'0'); f[77] = (b'999999999', b'0', b'999999999'); f[n - 1] = (b'100000000', b'99999999', b'10')
    if edge == 'moving-extremes':
        f = [(b'%d' % (500000 - 1999 * i), b'%d' % (7 + 4000001 * i), b'%d' % (500000000 + (1 - 2 * (i % 2)) * 2000003 * i)) for i in range(n)]
    host = fastq(qnames(f), [150] * n, S + 20)
    p = check(ctx, host, n, True, qname='exact')
    assert n > 4 * tile_reads(p)


@gpu
@pytest.mark.parametrize('bad', [b'1234567890', b'007', b'', b'00'], ids=['ten-digits', 'leading-zeros', 'empty', 'two-zeros'])
@pytest.mark.parametrize('col', [0, 1, 2])
def test_qname_field_the_parser_must_flag(ctx, col, bad):
    """One name of 200 has a field the fused pass does not take -- ten digits (flag 4), '007', '00' or an empty field (flag 16): the flag must
    arrive, and the rows may not depend on it."""
    n = 200
    f = [[digits(i, WIDTHS[i % 5]), digits(i + 1, 4), digits(i + 2, WIDTHS[(i // 5) % 5])] for i in range(n)]
    f[101][col] = bad
    host = fastq(qnames([tuple(x) for x in f]), [150] * n, S + 21)
    p = check(ctx, host, n, True, qname='flagged')
    _, _, fq, _ = fused(ctx, device_buffer(ctx, host), n, p, True)
    r = ops.qname_fused_fetch(ctx, fq)
    want = 4 if len(bad) > 9 else 16
    assert not r.ok or r.flags & want, 'flags %d: bit %d expected' % (r.flags, want)
