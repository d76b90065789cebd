"""GPU: the statistics pass (csrc/stats.hip) held to oracle_c.stats on inputs built for its paths: a workgroup's second and
third tile and the staged -> unstaged -> staged pipeline, both ends of the two LDS windows in every tier, the fill-pair
correction at every length, shards with differing window hints, both forms of the fetch, export / import without a process
group, and uq_first_occurrence with offsets and a read beyond 2^20 bases.  Integer work: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import oracle_c
import stats_inputs as SI
import uq_oracle as O
from uq_amd import analysis, ops
from uq_amd._lib import call

pytestmark = pytest.mark.gpu

FIELDS = ('len_min', 'len_max', 'max_record_bytes', 'bad_plus', 'bad_len')


def _device(ctx, host, misalign=0):
    """(device bytes at `misalign` bytes past an aligned address, the oracle's record index on the device and on the host)."""
    t = ctx.torch
    backing = t.zeros(host.size + misalign + 64, dtype=t.uint8, device=ctx.device)
    d_buf = backing[misalign:misalign + host.size]
    d_buf.copy_(t.from_numpy(host))
    hls = oracle_c.index_lines(host)
    return d_buf, ctx.to_device(hls), hls


def _same(hs, ref, what=''):
    for f in FIELDS:
        assert getattr(hs, f) == ref[f], (what, f, getattr(hs, f), ref[f])
    if not np.array_equal(hs.counts, ref['counts']):
        b, q = np.nonzero(hs.counts != ref['counts'])
        raise AssertionError('%s: %d counters differ, first (base %d, quality %d): %d, oracle %d'
                             % (what, len(b), b[0], q[0], hs.counts[b[0], q[0]], ref['counts'][b[0], q[0]]))


def _accumulate_and_compare(ctx, host, pieces=None, misalign=0, what=''):
    d_buf, ls, hls = _device(ctx, host, misalign)
    n = (len(hls) - 1) // 4
    st = ops.stats_new(ctx)
    for first, cnt in pieces or [(0, n)]:
        ops.stats_accumulate(ctx, st, d_buf, ls, first, cnt)
    hs = ops.stats_fetch(ctx, st)
    _same(hs, oracle_c.stats(host, hls, 0, n), what)
    return hs


# ------------------------------------------------------------------ the software pipeline
@pytest.fixture(scope='module')
def pipeline_file():
    """140 000 records of 1 .. 12 bases (about 20 bytes each: tiles of 64 records, 2 188 tiles over 1 024 workgroups, so workgroups
    0 .. 139 count three tiles); records 65 536 .. 65 663 -- tiles 1 024 and 1 025, the SECOND tile of workgroups 0 and 1 --
    have 480 bases, which does not fit the 20 KiB stage.  One record in sixteen ends with a pair outside the windows (tier 3)."""
    rng = np.random.default_rng(20261018)
    n = 140_000
    lens = rng.integers(1, 13, n)
    lens[65536:65536 + 128] = 480
    total = int(lens.sum())
    seq = rng.choice(np.frombuffer(b'ACGTACGTACGTNacgn', np.uint8), total)
    qual = rng.integers(33, 97, total).astype(np.uint8)
    odd_rec = np.flatnonzero(rng.random(n) < 1 / 16)
    odd = np.cumsum(lens)[odd_rec] - 1                         # the record's last pair
    seq[odd[::2]] = ord('*'); qual[odd[1::2]] = 126
    sb, qb = seq.tobytes(), qual.tobytes()
    recs, at = [], 0
    for L in lens.tolist():
        recs.append((b'@r', sb[at:at + L], qb[at:at + L])); at += L
    host = SI.fastq(recs)
    hls = oracle_c.index_lines(host)
    return host, hls, n, int((lens[odd_rec] == 5).sum()), oracle_c.stats(host, hls, 0, n)


@pytest.mark.parametrize('misalign', [0, 5])
def test_second_and_third_tile_staged_unstaged_staged(ctx, pipeline_file, misalign):
    host, hls, n, fives, ref = pipeline_file
    # the geometry is a precondition, not luck: the kernel's prologue must choose R = 64 records a tile ...
    avg = host.size // n + 1
    assert (20480 - 64) // (avg + avg // 8 + 1) >= 64
    # ... so that tiles 1 024 / 1 025 are the long records (unstaged: 64 records of 967 bytes > 20 KiB), counted by workgroups 0 / 1
    # between a staged tile before (0 / 1) and one after (2 048 / 2 049)
    assert 65536 == 1024 * 64 and n > 2050 * 64 and int(hls[4 * (65536 + 64)] - hls[4 * 65536]) == 64 * (2 * 480 + 7) > 20480
    # and the per-byte tier meets groups of exactly five pairs (the guard between a group's two halves)
    assert fives > 300
    d_buf, ls, _ = _device(ctx, host, misalign)
    st = ops.stats_new(ctx)
    ops.stats_accumulate(ctx, st, d_buf, ls, 0, n)
    _same(ops.stats_fetch(ctx, st), ref, 'misalign %d' % misalign)


# ------------------------------------------------------------------ window edges, tiers
def _window_file(qbase, bbase):
    inq = [qbase + k for k in (1, 5, 20, 40, 62, 63, 0)]
    fillers = [b'ACGTACG', b'ACGNTNA'] if bbase == 64 else [b'acgtacg', b'acgntna']
    probe_q = [q for q in (qbase - 1, qbase, qbase + 63, qbase + 64, 0x7F, 0x80, 0xFF) if q >= 0 and q != 10]
    probe_b = [bbase - 1, bbase, bbase + 31, bbase + 32] + list(b'ACGT@BUa')
    # record 0 sets the hints: its lowest quality picks qbase (>= 64: 59, < 33: 0, else 33), its first base bbase (>= 96: 96)
    q0 = {33: b'5I', 59: b'hi', 0: b'\x05I'}[qbase]
    recs = [(b'@w', b'AC' if bbase == 64 else b'ac', q0)]
    for fill in fillers:
        for pb in probe_b:
            for pq in probe_q:
                for pos in range(8):
                    s = bytearray(fill); q = bytearray(inq)
                    s.insert(pos, pb); q.insert(pos, pq)
                    recs.append((b'@w', bytes(s), bytes(q)))
    return recs


@pytest.mark.parametrize('qbase,bbase', [(33, 64), (59, 64), (0, 64), (33, 96), (59, 96), (0, 96)])
def test_window_edges_in_every_tier(ctx, qbase, bbase):
    """Seven in-window pairs + one probe pair at each of the eight positions of a group: qualities at both ends of [qbase, qbase + 64)
    and with the top bit set, bases at both ends of [bbase, bbase + 32) and the neighbours of A/C/G/T that the tier-1 test must refuse."""
    recs = _window_file(qbase, bbase)
    host = SI.fastq(recs)
    # the hints this file is built for (stats.hip's prologue, restated)
    q0, s0 = recs[0][2], recs[0][1]
    assert (59 if min(q0) >= 64 else 0 if min(q0) < 33 else 33) == qbase and (96 if s0[0] >= 96 else 64) == bbase
    hs = _accumulate_and_compare(ctx, host, what='window %d/%d' % (qbase, bbase))
    for q in (qbase, qbase + 63, qbase + 64, 0x80, 0xFF):
        assert hs.counts[:, q].sum() > 0
    for b in (bbase - 1, bbase, bbase + 31, bbase + 32):
        assert hs.counts[b].sum() > 0


# ------------------------------------------------------------------ fill pairs
@pytest.mark.parametrize('qbase', [33, 59, 0])
@pytest.mark.parametrize('kind', ['acgt', 'acgt_n', 'lower'])
def test_fill_pairs_at_every_length(ctx, kind, qbase):
    """A read's last group is padded to eight pairs with (window base + 1, quality slot 0) and the padding taken off that bin at the
    flush: every length 1 .. 24 (every residue of L mod 8, one to three groups) in tier 1 (A/C/G/T), tier 2 (an N in every group)
    and tier 2 of the lower-case window, with real counts at the fill bin -- 'A' or 'a' = bbase + 1 with quality qbase -- so that a
    wrong correction moves a counter that is in use."""
    lo = {33: 33, 59: 64, 0: 1}[qbase]                          # record 0's lowest quality places the quality window
    fill = ord('a' if kind == 'lower' else 'A')
    recs = [(b'@f', b'ac' if kind == 'lower' else b'AC', bytes([lo, lo + 1]))]
    for rep in range(3):
        for L in range(1, 25):
            s = bytearray((b'acgt' if kind == 'lower' else b'ACGT')[(i + rep + L) % 4] for i in range(L))
            own = bytearray([fill]) * L                        # a read of this length made of the fill pair itself
            if kind == 'acgt_n':
                s[0::8] = b'N' * len(s[0::8]); own[0::8] = b'N' * len(own[0::8])
            q = bytes(b if b != 10 else 12 for b in (qbase + (i * 7 + rep) % 40 for i in range(L)))
            recs += [(b'@f', bytes(s), q), (b'@f', bytes(own), bytes([qbase]) * L)]
    hs = _accumulate_and_compare(ctx, SI.fastq(recs), what='%s qbase %d' % (kind, qbase))
    assert hs.counts[fill, qbase] >= 3 * sum(L - (L + 7) // 8 for L in range(1, 25))


# ------------------------------------------------------------------ shards into one struct
def test_shards_with_other_windows_accumulate_into_one_struct(ctx):
    """(0, 1), (1, 1), (2, n - 2): the first record of each piece places other windows (Phred+33 upper case, Phred+64 lower case,
    quality below 33).  The windows are hints: no count may depend on them, and the bad records are file-wide numbers."""
    rng = np.random.default_rng(7)
    recs = [(b'@s', b'ACGTNACGT', b'5IIII!!5I'), (b'@s', b'acgtnacgtnn', b'hhhhiijjhhh'), (b'@s', b'NNACGT*', b'\x05\x06IIhh~')]
    for i in range(400):
        L = int(rng.integers(1, 40))
        recs.append((b'@s', bytes(rng.choice(np.frombuffer(b'ACGTNacgtn', np.uint8), L)), bytes(rng.integers(33, 127, L, dtype=np.uint8))))
    recs[300] = recs[300][:3] + (b'-',)
    recs[77] = recs[77][:3] + (b'x+',)
    recs[150] = (b'@s', b'ACGTACGT', b'IIIII')
    recs[9] = (b'@s', b'ACG', b'IIIIII')
    host = SI.fastq(recs)
    n = len(recs)
    hs = _accumulate_and_compare(ctx, host, pieces=[(0, 1), (1, 1), (2, n - 2)], what='shards')
    assert (hs.bad_plus, hs.bad_len) == (77, 9)
    _accumulate_and_compare(ctx, host, pieces=[(2, n - 2), (1, 1), (0, 1)], misalign=5, what='shards, reversed')


# ------------------------------------------------------------------ both forms of the fetch
PAIRS = [(b, q) for b in range(65, 105) for q in range(33, 127)]           # 3 760 distinct (base, quality) pairs, enumerated


@pytest.mark.parametrize('npairs', [2048, 2049, 3001])
def test_fetch_on_both_sides_of_the_compact_cap(ctx, npairs):
    """ops.stats_fetch (the list of non-zero counters, or the whole table beyond UQ_STATS_COMPACT_CAP = 2 048 of them) and
    uq_stats_fetch itself return the oracle's table with exactly 2 048, 2 049 and about 3 000 counters in use."""
    assert ops.STATS_COMPACT_CAP == 2048
    use = PAIRS[:npairs]
    recs = [(b'@p', bytes(b for b, _ in use[i:i + 2]), bytes(q for _, q in use[i:i + 2])) for i in range(0, npairs, 2)]
    host = SI.fastq(recs)
    d_buf, ls, hls = _device(ctx, host)
    ref = oracle_c.stats(host, hls, 0, len(recs))
    assert int(np.count_nonzero(ref['counts'])) == npairs
    st = ops.stats_new(ctx)
    ops.stats_accumulate(ctx, st, d_buf, ls, 0, len(recs))
    hs = ops.stats_fetch(ctx, st)
    assert (hs.nz_keys is not None) == (npairs <= 2048)
    _same(hs, ref, 'stats_fetch, %d pairs' % npairs)
    raw = np.empty(1, dtype=ops.STATS_DTYPE)
    call('uq_stats_fetch', ctx.h, ops._p(st), C.c_void_p(raw.ctypes.data))
    _same(ops.HostStats(raw[0]), ref, 'uq_stats_fetch, %d pairs' % npairs)


# ------------------------------------------------------------------ export / import
@pytest.mark.parametrize('bounds', [[0, None], [0, 1, None], [0, None, None], [0, 70, None], [0, 1, 1, 40, 77, None], [0, 0, 60, 61, 120, None]],
                         ids=['world1', 'world2_single_read', 'world2_empty_rank', 'world2_offenders_apart', 'world5', 'world5_empty_front'])
def test_export_sum_import_without_a_process_group(ctx, bounds):
    """Every rank's shard (its own buffer, its own record index from 0) exported with its read offset, the buffers summed as the
    all-reduce would, imported into a fresh struct: every field of the whole file's statistics.  A bad '+' line and a length
    mismatch lie in different shards; one shard holds a single read, one rank none."""
    rng = np.random.default_rng(11)
    recs = []
    for i in range(130):
        L = int(rng.integers(2, 60))
        recs.append((b'@e%d' % i, bytes(rng.choice(np.frombuffer(b'ACGTN', np.uint8), L)), bytes(rng.integers(33, 75, L, dtype=np.uint8))))
    recs[50] = recs[50][:3] + (b'*',)
    recs[125] = recs[125][:3] + (b'',)
    recs[90] = (b'@e90', b'ACGTACGTAC', b'IIIIIII')
    recs[100] = (b'@e100', b'ACG', b'IIIII')
    n = len(recs)
    bounds = [n if b is None else b for b in bounds]
    world = len(bounds) - 1
    host = SI.fastq(recs)
    hls = oracle_c.index_lines(host)
    ref = oracle_c.stats(host, hls, 0, n)
    assert (ref['bad_plus'], ref['bad_len']) == (50, 90)
    total = None
    for rank in range(world):
        lo, hi = bounds[rank], bounds[rank + 1]
        st = ops.stats_new(ctx)
        if hi > lo:
            part = host[int(hls[4 * lo]):int(hls[4 * hi])].copy()
            d_buf, ls, _ = _device(ctx, part)
            ops.stats_accumulate(ctx, st, d_buf, ls, 0, hi - lo)
        words = ops.stats_export(ctx, st, rank, world, lo)
        total = words if total is None else total + words
    out = ops.stats_new(ctx)
    ops.stats_import(ctx, total, world, out)
    _same(ops.stats_fetch(ctx, out), ref, 'world %d' % world)


# ------------------------------------------------------------------ first occurrence
def _small_records():
    return [(b'@o', b'GGGA', b'IIII'), (b'@o', b'AGTn', b'IIII'), (b'@o', b'NNNNNNNNC*', b'IIIIIIIIII'), (b'@o', b'c' * 70 + b'Ra', b'I' * 72),
            (b'@o', b'TTTT', b'IIII'), (b'@o', b'x', b'I'), (b'@o', b'ACGTYK', b'IIIIII')]


@pytest.mark.parametrize('first_read,nreads,index_base', [(0, 7, 0), (2, 5, 0), (2, 4, 1000), (1, 1, 1 << 31), (3, 4, (1 << 32) - 8)])
def test_first_occurrence_with_offsets(ctx, first_read, nreads, index_base):
    """uq_first_occurrence of reads [first_read, first_read + nreads) numbered from index_base, against a plain scan of the lines:
    the order of the bases and the absent ones."""
    recs = _small_records()
    d_buf, ls, _ = _device(ctx, SI.fastq(recs))
    fs = ops.first_occurrence(ctx, d_buf, ls, first_read, nreads, index_base=index_base)
    want = SI.first_appearance(recs, first_read, nreads)
    order, absent = SI.order_of_keys(fs)
    assert order == want and absent == set(range(256)) - set(want)


def test_first_occurrence_of_shards_combines_with_min(ctx):
    """Two shards with file-wide read numbers (index_base = the shard's first read): the element-wise minimum is the whole file's table."""
    recs = _small_records()
    d_buf, ls, _ = _device(ctx, SI.fastq(recs))
    whole = ops.first_occurrence(ctx, d_buf, ls, 0, 7)
    a = ops.first_occurrence(ctx, d_buf, ls, 0, 3, index_base=0)
    b = ops.first_occurrence(ctx, d_buf, ls, 3, 4, index_base=3)
    assert np.array_equal(np.minimum(a, b), whole)
    assert SI.order_of_keys(np.minimum(a, b))[0] == SI.first_appearance(recs)


def test_first_occurrence_in_a_read_beyond_2_pow_20_bases(ctx):
    """X first at position 6, Y first at position 2^20 + 5 of read 0, both N-trick candidates with a shared quality: the keys must
    sort X in front of Y, or the two N_qual codes come out swapped against the reference's dict order (O.pass1 -> O.decide)."""
    recs = SI.long_read_records()
    host = SI.fastq(recs)
    hs = _accumulate_and_compare(ctx, host, what='long read')
    d_buf, ls, _ = _device(ctx, host)
    fs = ops.first_occurrence(ctx, d_buf, ls, 0, len(recs))
    want = SI.first_appearance(recs)
    order, absent = SI.order_of_keys(fs)
    assert order == want and absent == set(range(256)) - set(want)
    p1 = O.pass1(O.read_lines(host.tobytes()))
    ref = O.decide(p1['static_qualities'], p1['dna_min'], p1['dna_max'])
    assert len(ref['N_qual']) == 2
    assert analysis.decide_from_stats(hs, first_seen=fs)['N_qual'] == ref['N_qual']
