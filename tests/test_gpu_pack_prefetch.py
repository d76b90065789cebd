"""The fused pack + statistics (+ QNAME) kernels at the inputs where a window of phase B taken a group early, a tile loop that swaps register
sets or a QNAME field built from partial sums could go wrong (those three changes were built, passed these tests, lost their A/B
and were taken out again; the parser wave's issue priority stayed, and so did the tests -- they hold whatever is tried next on the group
loop and the parser).  As tests/test_gpu_pack_roles.py (whose `check` this file uses): the queued list forms, with and without the QNAME
phase, and the indexed fused form against ops.pack + ops.stats_accumulate + qname_device.analyse_device and oracle_c -- rows, counts,
lengths, flags and QNAME columns byte for byte."""
import numpy as np
import pytest

import oracle_c
from test_gpu_pack_roles import FAMILIES, check, decide, fused, tile_reads
from uq_amd import ops, synth

S = 20261020
gpu = pytest.mark.gpu
ACGT = np.frombuffer(b'ACGT', dtype=np.uint8)
STAGE = 4 * 256 * 16                                      # what a tile of the fused kernels holds in flight


def sim_name(i):
    return b'@SIM001:42:FCX01:%d:%d:%d:%d' % (1 + i % 4, 1101 + i % 64, 1000 + (i * 7919) % 29000, 1000 + (i * 104729) % 29000)


def fastq(names, lens, seed, n_rate=0):
    """name / bases / '+' / qualities per record.  The qualities run through their whole alphabet in turn ('!' .. 'I'; with Ns: N bears '!'
    alone, the others '"' .. 'I'), so that a few hundred symbols already show a contiguous range -- the fused kernels are built for that."""
    rng = np.random.default_rng(seed)
    parts, k = [], 0
    for nm, L in zip(names, lens):
        seq = ACGT[rng.integers(0, 4, L)]
        if n_rate:
            q = (34 + (k + np.arange(L)) % 40).astype(np.uint8)
            isn = rng.integers(0, 100, L) < n_rate
            seq = np.where(isn, 78, seq).astype(np.uint8); q = np.where(isn, 33, q).astype(np.uint8)
        else:
            q = (33 + (k + np.arange(L)) % 41).astype(np.uint8)
        k += L
        parts += [nm, b'\n', seq.tobytes(), b'\n+\n', q.tobytes(), b'\n']
    return np.frombuffer(b''.join(parts), dtype=np.uint8).copy()


def check_indexed(ctx, host, n, **dk):
    """The indexed fused form (ops.pack_stats: a record index, no lists, no QNAME phase) against the plain kernels and the oracle."""
    hls, ref, d, p = decide(host, n, **dk)
    rd, rq, rbad = oracle_c.pack(host, hls, 0, n, d['bases'], d['qualities'], d['N_qual'], d['bits_per_base'], d['bits_per_quality'],
                                 d['variable_read_lengths'], d['dna_bytes_per_row'], d['quality_bytes_per_row'])
    assert rbad is None
    d_buf = ctx.to_device(host)
    ls = ops.index_lines(ctx, d_buf, ops.count_lines(ctx, d_buf))
    sp = ops.pack_stats(ctx, d_buf, ls, 0, n, p)
    assert sp is not None, 'no fused kernel for this geometry'
    hs = ops.stats_fetch(ctx, sp[3])
    assert not hs.incomplete and ops.bad_index(sp[2]) is None
    assert np.array_equal(ctx.to_numpy(sp[0]).reshape(n, -1), rd) and np.array_equal(ctx.to_numpy(sp[1]).reshape(n, -1), rq)
    assert np.array_equal(hs.counts, ref['counts'])
    assert (hs.len_min, hs.len_max, hs.max_record_bytes) == (ref['len_min'], ref['len_max'], ref['max_record_bytes'])


@gpu
@pytest.mark.parametrize('form', ['lists', 'lists-qname', 'indexed'])
@pytest.mark.parametrize('L', [1, 7, 8, 9, 24, 31, 32, 33])
def test_fixed_length_at_the_group_boundaries(ctx, L, form):
    """Every read L bases long, 2R + 1 of them: one group (1, 7, 8), a top group of one symbol (9, 33), as many groups as a read has lanes (24:
    three), one more than that (31, 32).  Short records make the tile as large as it gets (56 reads, three lanes a read)."""
    n = 2 * 56 + 1
    host = fastq([sim_name(i) for i in range(n)], [L] * n, S + L)
    if form == 'indexed': return check_indexed(ctx, host, n)
    p = check(ctx, host, n, form == 'lists-qname')
    assert tile_reads(p) == 56 and not p.variable


SPECIAL = [1, 7, 8, 9, 31, 32, 33, 301]


def variable_input(dk):
    """(bytes, reads, R): the special lengths placed by tiles of R reads, R being the tile these very reads give (it depends on their average)."""
    for R in (32, 36, 40):
        rng = np.random.default_rng(S + 7)
        lens = [int(x) for x in rng.integers(36, 302, 6 * R)]
        for k in range(3): lens[k * R] = SPECIAL[k]                              # tiles 0 - 2 begin with 1, 7, 8
        for k, L in enumerate(SPECIAL): lens[3 * R - 1 - 2 * k] = L              # tile 2 ends with 1 (its last read), the others further in
        for k, L in enumerate(SPECIAL): lens[3 * R + 5 + k] = L                  # side by side in the middle of tile 3
        lens[4 * R - 1] = 301; lens[4 * R] = 9                                   # a tile's last read the longest, the next one's first nearly the shortest
        lens += [36, 301] * R
        host = fastq([sim_name(i) for i in range(len(lens))], lens, S + 8, n_rate=1)
        if tile_reads(decide(host, len(lens), **dk)[3]) == R: return host, len(lens), R
    raise AssertionError('no tile size of 32, 36 or 40 reads reproduces itself')


@gpu
@pytest.mark.parametrize('form', ['lists', 'lists-qname', 'indexed'])
@pytest.mark.parametrize('family', ['var-notricks', 'var-ntrick'])
def test_variable_lengths_with_the_short_and_the_longest(ctx, family, form):
    """36 - 301 bp with 1 % N, and among them reads of 1, 7, 8 (the top group holds the sentinel alone: it takes no window), 9, 31, 32, 33 and
    301 = dna_max bases -- as the first read of a tile, as its last, and in its middle; then two tiles of 36 and 301 bp alternating (the
    lanes of a wave end their group loops at different groups)."""
    _, _, dk = FAMILIES[family]
    host, n, R = variable_input(dk)
    if form == 'indexed': return check_indexed(ctx, host, n, **dk)
    p = check(ctx, host, n, form == 'lists-qname', **dk)
    assert tile_reads(p) == R and p.variable and p.dna_max == 301


COUNTS = ['1', 'R-1', 'R', 'R+1', '2R+1']


@gpu
@pytest.mark.parametrize('qn', [False, True], ids=['plain', 'qname-phase'])
@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('family', list(FAMILIES))
def test_read_counts_around_one_and_two_tiles(ctx, family, count, qn):
    """One read, a tile short of one read, one tile, one tile and a read, two tiles and a read: the tile loop ends behind its first, its second
    and its third turn, and the last tile has lanes whose read does not exist."""
    length, kw, dk = FAMILIES[family]
    head = synth.fastq_array(synth.Spec(S + 1, length, **kw), 400)
    hls, _, d, p = decide(head, 400, **dk)
    R = tile_reads(p)
    assert 8 <= R <= 63
    n = {'1': 1, 'R-1': R - 1, 'R': R, 'R+1': R + 1, '2R+1': 2 * R + 1}[count]
    check(ctx, head[:int(hls[4 * n])].copy(), n, qn, qname='may-decline' if n < 64 else 'exact', guess=(d, p), **dk)


@gpu
@pytest.mark.parametrize('qn', [False, True], ids=['plain', 'qname-phase'])
def test_piece_path_first_then_normal_tiles(ctx, qn):
    """One record of the launch's first tile is longer than the tile allows: that tile goes piece by piece, the tiles behind it take the
    pipeline up again."""
    n = 203
    names = [sim_name(i) for i in range(n)]
    names[2] = b'@' + b'L' * 7000 + names[2][1:]
    host = fastq(names, [150] * n, S + 9)
    p = check(ctx, host, n, qn, qname='flagged')
    R = tile_reads(p)
    assert n > 4 * R and R * 330 + 7000 > STAGE


def stage_end_input(first_len, R, extra):
    n = 3 * R + 1
    names = [b'@%d' % (1 + i) for i in range(n)]
    lens = [150] * n
    lens[0] = first_len
    for i in range(R, 2 * R): names[i] = b'@' + b'0' * 100 + names[i][1:]       # tile 1's names: 100 more bytes each, the last one makes up the rest
    size = [len(nm) + 2 * L + 5 for nm, L in zip(names, lens)]
    start1 = sum(size[:R])
    more = STAGE - start1 % 16 - sum(size[R:2 * R]) + extra
    names[2 * R - 1] = b'@' + b'0' * more + names[2 * R - 1][1:]
    assert 0 <= more and len(names[2 * R - 1]) <= 255
    return fastq(names, lens, S + 10 + first_len)


@gpu
@pytest.mark.parametrize('qn', [False, True], ids=['plain', 'qname-phase'])
@pytest.mark.parametrize('first_len', [1, 9])
def test_windows_at_the_front_and_the_end_of_the_stage(ctx, first_len, qn):
    """The launch's first read has the shortest name there is ('@1') and `first_len` bases: its base window begins below the stage's first
    byte (the buffer is 16-byte aligned, the tile starts at stage offset 0).  The names of tile 1 are padded so that its records end with the
    stage's last byte (16 384 bytes from the 16-byte boundary at or below the tile's first record): its last read's windows are the stage's last bytes."""
    R = 40
    n = 3 * R + 1
    for extra in (0, 1):                                   # (one byte more: tile 1 no longer fits and goes piece by piece)
        host = stage_end_input(first_len, R, extra)
        p = check(ctx, host, n, qn, qname='may-decline')
        assert tile_reads(p) == R


@gpu
@pytest.mark.parametrize('mis', [1, 7, 15])
@pytest.mark.parametrize('family', ['var-ntrick', 'var-notricks'])
def test_variable_lengths_off_a_16_byte_boundary(ctx, family, mis):
    length, kw, dk = FAMILIES[family]
    head = synth.fastq_array(synth.Spec(S + 3, length, **kw), 300)
    hls, _, d, p = decide(head, 300, **dk)
    n = 2 * tile_reads(p) + 1
    check(ctx, head[:int(hls[4 * n])].copy(), n, True, mis=mis, guess=(d, p), **dk)


# ---- the parser: '@q' + a + ':' + b + '/' + c, three numeric fields
def qnames(fields):
    return [b'@q%s:%s/%s' % f for f in fields]


def digits(i, nd):
    """a number of exactly nd digits that depends on i"""
    lo = 10 ** (nd - 1) if nd > 1 else 0
    return b'%d' % (lo + (i * 2654435761) % (10 ** nd - lo))


WIDTHS = [1, 4, 5, 8, 9]


@gpu
@pytest.mark.parametrize('edge', ['widths', 'min-max'])
def test_qname_field_values(ctx, edge):
    """Fields of 1, 4, 5, 8 and 9 digits in every column (the three dwords of a field's window hold 1 + 4 + 4 digits), among them 0 and
    999 999 999 as a column's smallest and largest value: the columns must equal the exact passes', their types follow from vmin / vmax."""
    n = 200
    f = [(digits(i, WIDTHS[i % 5]), digits(i + 1, WIDTHS[(i // 5) % 5]), digits(i + 2, WIDTHS[(i // 25) % 5])) for i in range(n)]
    if edge == 'min-max':
        f[3] = (b'0', b'999999999', b'0'); f[77] = (b'999999999', b'0', b'999999999'); f[n - 1] = (b'100000000', b'99999999', b'10')
    host = fastq(qnames(f), [150] * n, S + 20)
    check(ctx, host, n, True, qname='exact')


@gpu
@pytest.mark.parametrize('bad', [b'1234567890', b'007', b'', b'00', b'12x4'], ids=['ten-digits', 'leading-zeros', 'empty', 'two-zeros', 'letter'])
@pytest.mark.parametrize('col', [0, 1, 2])
def test_qname_field_the_parser_must_flag(ctx, col, bad):
    """One name of 200 has a field the fused pass does not take -- ten digits (flag 4), '007' or '00' or a letter (flag 16), empty (flag 16) --
    in the first, the middle or the last column, in a tile's middle: the flag must arrive, and the rows may not depend on it."""
    n = 200
    f = [[digits(i, WIDTHS[i % 5]), digits(i + 1, 4), digits(i + 2, WIDTHS[(i // 5) % 5])] for i in range(n)]
    f[101][col] = bad
    host = fastq(qnames([tuple(x) for x in f]), [150] * n, S + 21)
    p = check(ctx, host, n, True, qname='flagged')
    d_buf = ctx.to_device(host)
    _, _, fq, _ = fused(ctx, d_buf, n, p, True)
    r = ops.qname_fused_fetch(ctx, fq)
    want = 4 if len(bad) > 9 else 16
    assert not r.ok or r.flags & want, 'flags %d: bit %d expected' % (r.flags, want)
