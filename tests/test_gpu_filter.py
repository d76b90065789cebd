"""GPU: uq_filter_mark, uq_filter_plan and uq_compact_records against the pure-Python definition (tests/filter_ref.py).  Verdicts are compared
as the whole verdict buffer between two guards; every compaction comparison is the WHOLE output buffer between two guards of 64 bytes, with
the source and the output placed at chosen 16-byte phases.

The compaction (csrc/filter.hip) cuts the output into tiles of TILE = CP_TILE bytes at 16-byte-aligned addresses and keeps a tile's unit
starts in an LDS list of TILE / 4 + 3 entries; an item is one aligned output vector.  The inputs (tests/filter_inputs.py) are built from that:
records of 4 to 14 bytes at every output phase, a unit boundary on every byte from -17 to +17 around a tile's edge, more than 4 096 units in
one tile, kept units far apart in the source, a 70 000-base record kept and dropped."""
import os
import random
import re

import numpy as np
import pytest

import filter_inputs as I
import filter_ref as R
from uq_amd import ops, synth
from uq_amd._lib import UqHipError

pytestmark = pytest.mark.gpu

TILE = 16384
GUARD = 64
FILL = 0xA5
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_ON = dict(min_len=10, max_len=60000, max_n=3, min_mean_q=20, sample_threshold=3 << 62, seed=11, flags=1)
CRITERIA = [{}, ALL_ON, dict(min_len=1, max_n=0, min_mean_q=1), dict(max_len=10, min_mean_q=93), dict(min_mean_q=30, max_n=1)]


def test_the_tile_size_is_the_kernels():
    src = open(os.path.join(REPO, 'uq_amd', 'csrc', 'filter.hip')).read()
    threads = int(re.search(r'CP_THREADS = (\d+);', src).group(1))
    unroll = int(re.search(r'CP_UNROLL = (\d+);', src).group(1))
    assert re.search(r'CP_TILE = CP_THREADS \* CP_UNROLL \* 16;', src) and re.search(r'CP_NP = CP_TILE / 4 \+ 3;', src)
    assert threads * unroll * 16 == TILE


class Source:
    """A text in HBM at an address `phase` bytes past a 16-byte boundary, and its record index; tight: the allocation ends with the text."""

    def __init__(self, ctx, text, phase=0, tight=False):
        t = ctx.torch
        self.whole = t.full((len(text) + (phase % 16 if tight else 48),), FILL, dtype=t.uint8, device=ctx.device)
        start = (phase - self.whole.data_ptr()) % 16
        self.buf = self.whole[start:start + len(text)]
        if len(text): self.buf.copy_(ctx.to_device(np.frombuffer(text, dtype=np.uint8)))
        assert self.buf.data_ptr() % 16 == phase % 16 and self.buf.numel() == len(text)
        if tight: assert start + len(text) == self.whole.numel()
        self.ls = ctx.to_device(ops.host_line_starts(text).view(np.int64))
        self.reads = (self.ls.numel() - 1) // 4


class Output:
    """`size` bytes of FILL in HBM at a chosen phase, between two guards."""

    def __init__(self, ctx, size, phase=0):
        t = ctx.torch
        self.ctx, self.size = ctx, size
        self.whole = t.full((size + 2 * GUARD + 32,), FILL, dtype=t.uint8, device=ctx.device)
        start = GUARD + (phase - self.whole.data_ptr() - GUARD) % 16
        self.region = self.whole[start - GUARD:start + size + GUARD]
        self.buf = self.whole[start:start + size]
        assert size == 0 or self.buf.data_ptr() % 16 == phase % 16          # (an empty tensor has no address)

    def result(self):
        return self.ctx.to_numpy(self.region).tobytes()


def guarded(text, size=None):
    size = len(text) if size is None else size
    return bytes([FILL]) * GUARD + text + bytes([FILL]) * (size - len(text) + GUARD)


def u64s(ctx, tensor, n):
    return [int(x) for x in ctx.to_numpy(tensor[:n]).view(np.uint64)]


# ------------------------------------------------------------------ verdicts, report, plan
def check_mark(ctx, text, c, unit=1, phase=0, first=0, n=None, base=0, tight=False, vphase=5):
    c = R.criteria(**c)
    S = Source(ctx, text, phase, tight)
    n = S.reads - first if n is None else n
    want = R.run(text, c, unit, first, n, base)
    V = Output(ctx, n, vphase)
    d_rep = ops.filter_report_new(ctx)
    ops.filter_mark(ctx, d_rep, S.buf, S.ls, first, n, ops.filter_params(unit=unit, **c), base, verdict=V.buf)
    assert V.result() == guarded(bytes(want[0]))
    src, dst, kept, size = ops.filter_plan(ctx, d_rep, S.ls, first, n, unit, V.buf)
    assert ops.filter_report_fetch(ctx, d_rep) == want[4]
    assert kept == len(want[1]) and size == want[2][-1]
    assert u64s(ctx, src, kept) == want[1] and u64s(ctx, dst, kept + 1) == want[2]
    return want


@pytest.mark.parametrize('name,text', list(I.hand_inputs()), ids=[n for n, _ in I.hand_inputs()])
def test_hand_inputs(ctx, name, text):
    for c in CRITERIA + [dict(min_len=10), dict(max_len=10), dict(max_n=3), dict(min_mean_q=20)]:
        check_mark(ctx, text, c, phase=len(c) % 16)


def test_one_record_of_each_length_0_to_17(ctx):
    text = I.lengths(range(18), seed=8, n_rate=0.3)
    for c in CRITERIA + [dict(min_len=L) for L in (1, 8, 9, 16, 17)] + [dict(max_n=k) for k in (0, 1, 2)]:
        check_mark(ctx, text, c, phase=3)
    for L in range(18):
        check_mark(ctx, I.lengths([L], seed=L, n_rate=0.5), dict(max_n=L // 3, min_mean_q=19), phase=L)


@pytest.mark.parametrize('phase', [1, 3, 7])
def test_short_records_in_misaligned_buffers_that_end_with_the_text(ctx, phase):
    text = I.short_records(300)
    for c in CRITERIA:
        want = check_mark(ctx, text, c, phase=phase, tight=True)
    assert 0 < want[4]['reads_out'] < 300


def test_read_lengths_around_the_lane_groups(ctx):
    # the last two: tiles whose span passes the stage, with lines at and beyond what a half-wave takes there (4096) among short ones
    for ls in ([63, 64, 65] * 20, [255, 256, 257] * 12, [5000] * 7, [63, 5000, 64, 257, 65, 5000, 255, 256],
               [30] * 40 + [4096, 4097, 9000] + [30] * 21, [300] * 29 + [4095, 4096, 4097] + [300] * 40):
        text = I.lengths(ls, seed=len(ls), n_rate=0.01)
        nmax = max(s.count(b'N') + s.count(b'n') for _, s, _, _ in R.records(text))
        for c in (ALL_ON, dict(max_n=nmax), dict(max_n=nmax - 1), dict(min_mean_q=20), dict(min_mean_q=21), dict(min_len=ls[1]), dict(max_len=ls[1])):
            check_mark(ctx, text, c, phase=9)


@pytest.mark.parametrize('where', ['first', 'middle', 'last'])
def test_a_70000_base_read(ctx, where):
    text, at = I.long_record_text(where)
    _, s, _, u = R.records(text)[at]
    assert len(s) == 70000
    ncount, qsum = s.count(b'N'), sum(R.q(b) for b in u)
    assert qsum % 70000 != 0
    for c in (dict(max_n=ncount), dict(max_n=ncount - 1), dict(min_mean_q=qsum // 70000), dict(min_mean_q=qsum // 70000 + 1), dict(max_len=69999),
              dict(max_len=70000), dict(min_len=70000), ALL_ON):
        want = check_mark(ctx, text, c, phase=13)
    assert want[0][at] & 2


def test_the_lds_table_clamp_gives_the_same_verdicts(ctx, monkeypatch):
    """UQ_FILTER_CLAMP=lds: the quality clamp as a 256-byte LDS table instead of SWAR (DESIGN.md section 27 has the two timed)."""
    monkeypatch.setenv('UQ_FILTER_CLAMP', 'lds')
    for text in (I.odd_quality_bytes(), I.edges_q(), I.odd_shapes(), I.short_records(300), I.long_record_text('middle')[0],
                 I.lengths([30] * 40 + [4096, 4097, 9000] + [30] * 21, seed=3)):
        for c in (ALL_ON, dict(min_mean_q=1), dict(min_mean_q=20), dict(min_mean_q=93)):
            check_mark(ctx, text, c, phase=7)


def test_a_slice_a_base_and_no_reads(ctx):
    text = I.short_records(300)
    for first, n, base in ((0, 300, 0), (17, 100, 17), (17, 100, 1 << 40), (299, 1, 5), (100, 0, 0), (300, 0, 0)):
        check_mark(ctx, text, ALL_ON, first=first, n=n, base=base, phase=2)
    pairs = I.pairs_text()
    for first, n, base in ((0, 120, 0), (10, 50, 10), (10, 50, 4000), (118, 2, 0), (4, 0, 2)):
        check_mark(ctx, pairs, dict(min_len=12, max_n=2, sample_threshold=1 << 63, flags=1), unit=2, first=first, n=n, base=base, phase=6)


def test_reports_add_over_calls(ctx):
    text = I.short_records(300)
    c = R.criteria(**ALL_ON)
    S = Source(ctx, text, 4)
    d_rep = ops.filter_report_new(ctx)
    assert ops.filter_report_fetch(ctx, d_rep) == dict.fromkeys(R.FIELDS, 0)
    v = ctx.empty(300)
    for first, n in ((200, 100), (0, 200)):
        ops.filter_mark(ctx, d_rep, S.buf, S.ls, first, n, ops.filter_params(**c), first, verdict=v[first:first + n])
        ops.filter_plan(ctx, d_rep, S.ls, first, n, 1, v[first:first + n])
    want = R.run(text, c)
    assert ops.filter_report_fetch(ctx, d_rep) == want[4]
    assert ctx.to_numpy(v).tobytes() == bytes(want[0])


def test_bad_arguments_are_refused(ctx):
    text = I.pairs_text()
    S = Source(ctx, text)
    d_rep = ops.filter_report_new(ctx)
    v = ctx.zeros(120)
    for kw, n, base, words in ((dict(min_len=5, max_len=4), 120, 0, 'min_len'), (dict(min_mean_q=94), 120, 0, 'min_mean_q'), (dict(unit=3), 120, 0, 'unit'),
                               (dict(unit=0), 120, 0, 'unit'), (dict(unit=2), 119, 0, 'pairs'), (dict(unit=2), 118, 1, 'pairs')):
        with pytest.raises(UqHipError, match=words):
            ops.filter_mark(ctx, d_rep, S.buf, S.ls, 0, n, ops.filter_params(**kw), base, verdict=v)
    with pytest.raises(UqHipError, match='pairs'):
        ops.filter_plan(ctx, d_rep, S.ls, 0, 119, 2, v)
    with pytest.raises(UqHipError, match='unit'):
        ops.filter_plan(ctx, d_rep, S.ls, 0, 120, 3, v)
    assert ops.filter_report_fetch(ctx, d_rep) == dict.fromkeys(R.FIELDS, 0)


# ------------------------------------------------------------------ the compaction
def kept_text(text, keep, unit=1):
    """(filtered text, src, dst) of the units whose `keep` entry is true."""
    ls = [int(x) for x in ops.host_line_starts(text)]
    out, src, dst = bytearray(), [], [0]
    for w, k in enumerate(keep):
        if not k: continue
        lo, hi = ls[4 * w * unit], ls[4 * (w + 1) * unit]
        src.append(lo); out += text[lo:hi]; dst.append(len(out))
    return bytes(out), src, dst


def check_compact(ctx, text, keep, unit=1, out_phase=0, src_phase=0, room=0):
    """Hand-made verdicts (1 = dropped) through the plan and the compaction; the whole output between its guards."""
    S = Source(ctx, text, src_phase)
    keep = list(keep)
    assert len(keep) * unit == S.reads
    want, wsrc, wdst = kept_text(text, keep, unit)
    v = ctx.to_device(np.repeat(np.array([0 if k else 1 for k in keep], dtype=np.uint8), unit))
    d_rep = ops.filter_report_new(ctx)
    src, dst, kept, size = ops.filter_plan(ctx, d_rep, S.ls, 0, S.reads, unit, v)
    assert kept == len(wsrc) and size == len(want)
    assert u64s(ctx, src, kept) == wsrc and u64s(ctx, dst, kept + 1) == wdst
    out = Output(ctx, len(want) + room, out_phase)
    ops.compact_records(ctx, S.buf, src, dst, kept, out=out.buf)
    assert out.result() == guarded(want, len(want) + room)
    return want


def keep_patterns(n, seed=1):
    rnd = random.Random(seed)
    yield 'all', [True] * n
    yield 'none', [False] * n
    yield 'every other', [i % 2 == 0 for i in range(n)]
    yield 'first only', [i == 0 for i in range(n)]
    yield 'last only', [i == n - 1 for i in range(n)]
    yield 'random', [rnd.random() < 0.5 for _ in range(n)]


def test_one_kept_record(ctx):
    text = I.text([I.record(b'a', b'ACGT'), I.record(b'b', b'ACGTACGTACGTACGTACGTAC'), I.record(b'c', b'AC')])
    for phase in (0, 1, 15):
        assert check_compact(ctx, text, [False, True, False], out_phase=phase, src_phase=3) == I.record(b'b', b'ACGTACGTACGTACGTACGTAC')
        check_compact(ctx, text, [True, False, False], out_phase=phase, src_phase=7)
        check_compact(ctx, text, [False, False, True], out_phase=phase, src_phase=15, room=40)


TINY = I.tiny_records()


@pytest.mark.parametrize('out_phase', range(16))
def test_tiny_records_at_every_phase(ctx, out_phase):
    """Records of 4 to 14 bytes: a vector holds up to four units; every output phase, four source phases, six keep patterns."""
    sizes = [len(b''.join(l + b'\n' for l in r)) for r in R.records(TINY)]
    assert len(sizes) == 41 and min(sizes) == 4 and max(sizes) == 14
    for src_phase in (0, 5, 10, 15):
        for name, keep in keep_patterns(41, seed=out_phase):
            check_compact(ctx, TINY, keep, out_phase=out_phase, src_phase=src_phase)


def test_unit_boundaries_around_a_tile_edge(ctx):
    seen = set()
    for d in range(-17, 18):
        phase = (d * 7) % 16
        first = TILE - phase + d                                      # the first tile ends TILE - phase bytes into the output
        text = I.text([I.sized_record(first), I.record(b'dropped', b'NNNN'), I.sized_record(40, b'TGCA'), I.sized_record(9), I.sized_record(33)])
        want = check_compact(ctx, text, [True, False, True, False, True], out_phase=phase, src_phase=(d * 3) % 16)
        assert len(want) == first + 73
        seen.add(first - (TILE - phase))
        # the same boundary behind a run of short units, the long one last
        text = I.text([I.sized_record(20), I.record(b'dropped', b'NNNN'), I.sized_record(first - 20, b'TGCA'), I.sized_record(8), I.sized_record(24)])
        check_compact(ctx, text, [True, False, True, True, True], out_phase=phase, src_phase=(d * 5) % 16)
    assert seen == set(range(-17, 18))


def test_more_than_4096_units_in_one_tile(ctx):
    """Four empty lines are the smallest unit: a tile of them fills the LDS list to its bound."""
    n = 3 * TILE // 4
    text = I.four_byte_units(n)
    for phases in ((0, 0), (5, 9)):
        check_compact(ctx, text, [True] * n, out_phase=phases[0], src_phase=phases[1])
    # a unit that begins in front of every tile edge, then 4-byte units up to the next edge and beyond; dropped ones in between
    rnd = random.Random(7)
    for lead in (6, 7, 9):
        text = I.sized_record(lead) + I.four_byte_units(n)
        keep = [True] + [rnd.random() < 0.9 for _ in range(n)]
        assert sum(keep) > 2 * 4096 + 4
        check_compact(ctx, text, keep, out_phase=lead, src_phase=3)
        check_compact(ctx, text, [True] * (n + 1), out_phase=16 - lead, src_phase=11)


def test_one_in_a_thousand_of_20000_records(ctx):
    text = I.numbered_records(20000)
    rnd = random.Random(9)
    keep = [rnd.random() < 0.001 for _ in range(20000)]
    assert 8 <= sum(keep) <= 40
    want = check_compact(ctx, text, keep, out_phase=3, src_phase=6)
    assert 0 < len(want) < TILE
    keep = [i % 1000 == 999 for i in range(20000)]
    check_compact(ctx, text, keep, out_phase=12, src_phase=1)


@pytest.mark.parametrize('where', ['first', 'middle', 'last'])
def test_a_70000_base_record_kept_and_dropped(ctx, where):
    text, at = I.long_record_text(where)
    n = len(R.records(text))
    for phases in ((0, 0), (11, 3)):
        want = check_compact(ctx, text, [i == at for i in range(n)], out_phase=phases[0], src_phase=phases[1])
        assert len(want) > 140000
        check_compact(ctx, text, [i != at for i in range(n)], out_phase=phases[0], src_phase=phases[1])
        check_compact(ctx, text, [i == at or i % 3 == 0 for i in range(n)], out_phase=phases[1], src_phase=phases[0])


def test_pairs_are_units_of_two(ctx):
    text = I.pairs_text()
    for name, keep in keep_patterns(60, seed=3):
        check_compact(ctx, text, keep, unit=2, out_phase=7, src_phase=2)
    # and through the verdicts: a filter that fails one mate of some pairs drops both
    c = R.criteria(max_n=2, min_len=12)
    want = check_mark(ctx, text, c, unit=2)
    assert want[4]['fail_mate'] > 5
    S = Source(ctx, text, 9)
    d_rep = ops.filter_report_new(ctx)
    v = ops.filter_mark(ctx, d_rep, S.buf, S.ls, 0, S.reads, ops.filter_params(unit=2, **c))
    src, dst, kept, size = ops.filter_plan(ctx, d_rep, S.ls, 0, S.reads, 2, v)
    out = Output(ctx, size, 1)
    ops.compact_records(ctx, S.buf, src, dst, kept, out=out.buf)
    assert out.result() == guarded(want[3]) and len(R.records(want[3])) == 2 * kept


def test_a_capacity_one_byte_short_is_refused_and_nothing_kept_is_a_no_op(ctx):
    text = I.short_records(300)
    S = Source(ctx, text, 4)
    keep = [i % 3 != 1 for i in range(300)]
    want, _, _ = kept_text(text, keep)
    v = ctx.to_device(np.array([0 if k else 1 for k in keep], dtype=np.uint8))
    d_rep = ops.filter_report_new(ctx)
    src, dst, kept, size = ops.filter_plan(ctx, d_rep, S.ls, 0, 300, 1, v)
    out = Output(ctx, size, 2)
    with pytest.raises(UqHipError, match='out_capacity'):
        ops.compact_records(ctx, S.buf, src, dst, kept, out=out.buf, out_capacity=size - 1)
    assert out.result() == guarded(b'', size)
    ops.compact_records(ctx, S.buf, src, dst, 0, out=out.buf, out_capacity=0)                # kept = 0: nothing happens, whatever the capacity says
    assert out.result() == guarded(b'', size)
    ops.compact_records(ctx, S.buf, src, dst, kept, out=out.buf, out_capacity=size)
    assert out.result() == guarded(want)
    # nothing kept: the plan says so, dst[0] = 0
    src, dst, kept, size = ops.filter_plan(ctx, d_rep, S.ls, 0, 300, 1, ctx.to_device(np.ones(300, dtype=np.uint8)))
    assert (kept, size) == (0, 0) and u64s(ctx, dst, 1) == [0]


@pytest.mark.parametrize('length', [(36, 301), 150], ids=['36-301bp', '150bp'])
def test_device_against_the_host_twins(ctx, length):
    text = synth.fastq(20261020, 6000, length, n_rate=2)
    c = R.criteria(min_len=50, max_n=3, min_mean_q=19, sample_threshold=(1 << 64) // 10 * 9, seed=4, flags=1)
    ls = ops.host_line_starts(text)
    hv, hrep = ops.filter_mark_host(text, ops.filter_params(**c), ls)
    hsrc, hdst, hkept, hsize, hrep = ops.filter_plan_host(ls, hv, report=hrep)
    want = ops.compact_records_host(text, hsrc, hdst, hkept).tobytes()
    assert 1000 < hkept < 5900
    S = Source(ctx, text, 5)
    d_rep = ops.filter_report_new(ctx)
    v = ops.filter_mark(ctx, d_rep, S.buf, S.ls, 0, 6000, ops.filter_params(**c))
    assert ctx.to_numpy(v).tobytes() == hv.tobytes()
    src, dst, kept, size = ops.filter_plan(ctx, d_rep, S.ls, 0, 6000, 1, v)
    assert (kept, size) == (hkept, hsize) and ops.filter_report_fetch(ctx, d_rep) == hrep
    out = Output(ctx, size, 13)
    ops.compact_records(ctx, S.buf, src, dst, kept, out=out.buf)
    assert out.result() == guarded(want)


# ------------------------------------------------------------------ offsets beyond 2^31 and 2^32
def test_beyond_4_gib(ctx):
    """13 M reads of 36 .. 301 bases made on the device (4.8 GB): the source passes 2^32, the outputs 2^31 (keep-all: 2^32 as well).
    Keep-all gives the source back; min-len = L and max-len = L - 1 split it into two texts whose fingerprint sums add up to the source's
    (L = 211 halves the BYTES: the records of 36 .. 210 bases hold 48 825 of every 98 420 bytes)."""
    t = ctx.torch
    n, L = 13_000_000, 211
    src = ops.synth_fastq(ctx, synth.Spec(20261020, (36, 301), n_rate=1), 0, n)
    nl = ops.count_lines(ctx, src)
    ls = ops.index_lines(ctx, src, nl)
    assert nl == 4 * n and src.numel() > (1 << 32) + (1 << 20)
    before = ops.fingerprint(ctx, src, ls, n)
    parts = []
    for c in ({}, dict(min_len=L), dict(max_len=L - 1)):
        d_rep = ops.filter_report_new(ctx)
        v = ops.filter_mark(ctx, d_rep, src, ls, 0, n, ops.filter_params(**c))
        psrc, pdst, kept, size = ops.filter_plan(ctx, d_rep, ls, 0, n, 1, v)
        rep = ops.filter_report_fetch(ctx, d_rep)
        assert rep['reads_in'] == n and rep['bytes_in'] == src.numel() and rep['bases_in'] == before['bases']
        assert rep['reads_out'] == kept and rep['bytes_out'] == size > (1 << 31) + (1 << 20)
        out = ctx.empty(size)
        ops.compact_records(ctx, src, psrc, pdst, kept, out=out)
        if not c:
            assert kept == n and size == src.numel() and t.equal(out, src)
        else:
            assert ops.count_lines(ctx, out) == 4 * kept
            fp = ops.fingerprint(ctx, out, ops.index_lines(ctx, out, 4 * kept), kept)
            assert fp['reads'] == kept == n - rep['fail_min_len'] - rep['fail_max_len'] and fp['bases'] == rep['bases_out']
            parts.append(fp)
        del out, psrc, pdst, v
    for k in ('reads', 'bases', 'records'): assert (parts[0][k] + parts[1][k]) % (1 << 64) == before[k], k
