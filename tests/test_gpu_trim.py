"""GPU: uq_trim_mark, uq_trim_plan and uq_trim_records against the pure-Python definition (tests/trim_ref.py).  The windows, the report, the
plan, the trimmed text and its index are each compared as the WHOLE buffer between two guards of 64 bytes; source and output lie at chosen
16-byte phases, and the source allocation ends with the text.

The mark kernel (csrc/trim.hip) gives P lanes to a record and 8 bytes of a line to a lane per step; tiles beyond its 20 KiB stage are read
from HBM by half-waves, lines beyond 4096 bytes by the whole workgroup.  The copy cuts the output into tiles of TILE = TC_TILE bytes at
16-byte-aligned addresses and keeps TILE / 4 + 3 record starts in LDS; a record's output is five pieces of its source.  The inputs
(tests/trim_inputs.py) are built from that."""
import os
import random
import re

import numpy as np
import pytest

import filter_inputs as FI
import trim_inputs as I
import trim_ref as R
from uq_amd import _lib, ops, synth
from uq_amd._lib import UqHipError

pytestmark = pytest.mark.gpu

TILE = 16384
GUARD = 64
FILL = 0xA5
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_ON = dict(head=2, tail=1, crop=150, polyg=8, q5=18, q3=20, flags=1)
STEPS = [{}, ALL_ON, dict(q3=20), dict(q5=20), dict(q3=20, q5=20), dict(polyg=10), dict(flags=1), dict(head=3, tail=2, crop=20)]


def test_the_tile_size_is_the_kernels():
    src = open(os.path.join(REPO, 'uq_amd', 'csrc', 'trim.hip')).read()
    threads = int(re.search(r'TC_THREADS = (\d+);', src).group(1))
    unroll = int(re.search(r'TC_UNROLL = (\d+);', src).group(1))
    assert re.search(r'TC_TILE = TC_THREADS \* TC_UNROLL \* 16;', src) and re.search(r'TC_NP = TC_TILE / 4 \+ 3;', src)
    assert threads * unroll * 16 == TILE


class Source:
    """A text in HBM at an address `phase` bytes past a 16-byte boundary, and its record index; tight: the allocation ends with the text."""

    def __init__(self, ctx, text, phase=0, tight=True):
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


def guarded(data, size=None):
    size = len(data) if size is None else size
    return bytes([FILL]) * GUARD + data + bytes([FILL]) * (size - len(data) + GUARD)


def words(values, dtype):
    return np.array(values, dtype=dtype).tobytes()


def check(ctx, text, c, src_phase=0, out_phase=0, first=0, n=None, room=0):
    """Mark, plan and copy of the records [first, first + n): every buffer whole, between its guards -> what trim_ref.run returns."""
    c = R.steps(**c)
    S = Source(ctx, text, src_phase)
    n = S.reads - first if n is None else n
    want = R.run(text, c, first, n)
    wins, wdst, wtext, wrep = want
    W = Output(ctx, 8 * n, 4 * (src_phase % 4))                     # u32 pairs: any 4-byte phase
    Rp = Output(ctx, 8 * len(R.FIELDS), 8)
    _lib.call('uq_trim_report_init', ctx.h, ops._p(Rp.buf))
    ops.trim_mark(ctx, Rp.buf, S.buf, S.ls, first, n, ops.trim_params(**c), window=W.buf)
    assert W.result() == guarded(words([v for w in wins for v in w], np.uint32))
    assert Rp.result() == guarded(words([wrep[k] for k in R.FIELDS], np.uint64))
    D = Output(ctx, 8 * (n + 1), 8)
    _, size = ops.trim_plan(ctx, S.ls, first, n, W.buf, dst=D.buf)
    assert size == len(wtext) and D.result() == guarded(words(wdst, np.uint64))
    out = Output(ctx, len(wtext) + room, out_phase)
    L = Output(ctx, 8 * (4 * n + 1), 8)
    ops.trim_records(ctx, S.buf, S.ls, first, n, W.buf, D.buf, out=out.buf, index=True, line_start_out=L.buf)
    assert out.result() == guarded(wtext, len(wtext) + room)
    if n: assert L.result() == guarded(ops.host_line_starts(wtext).tobytes())
    else: assert L.result() == guarded(b'', 8)
    return want


# ------------------------------------------------------------------ windows and report
@pytest.mark.parametrize('name,text', list(I.hand_inputs()), ids=[n for n, _ in I.hand_inputs()])
def test_hand_inputs(ctx, name, text):
    """Lines of 0 .. 17 and 63 / 64 / 65 bases with the cut on every position of the last two chunks; sums of 0 and stops that must hold; G runs
    of G - 1, G, the whole window and across the chunk and lane-group boundaries; lower case; N ends and all-N reads; quality bytes outside
    33 .. 126; Ls != Lu, empty lines, +comment lines, CRLF."""
    for k, c in enumerate(STEPS + [dict(polyg=9), dict(polyg=11), dict(head=1000), dict(tail=1000), dict(crop=1), dict(q3=93, q5=93), dict(q3=1, q5=1)]):
        check(ctx, text, c, src_phase=k % 16, out_phase=(5 * k + 3) % 16)


def test_cuts_on_every_position_of_the_last_two_chunks(ctx):
    text = I.quality_cuts()                                           # ... and lines of 255 / 256 / 257
    want = check(ctx, text, dict(q3=I.T, q5=I.T), src_phase=7, out_phase=9)
    cuts = {(len(s), len(s) - (b - a)) for (_, s, _, _), (a, b) in zip(R.records(text), want[0])}
    assert all((L, c) in cuts for L in (17, 63, 64, 65, 255, 256, 257) for c in range(18))
    check(ctx, text, dict(q3=I.T), src_phase=1, out_phase=2)
    check(ctx, text, dict(q5=I.T, flags=1), src_phase=15, out_phase=0)


def test_reads_of_5000_bases_among_short_ones(ctx):
    """Tiles whose span passes the stage: half-waves from HBM, and lines at and beyond 4096 bytes, which the whole workgroup walks."""
    text = I.long_reads_among_short()
    for k, c in enumerate(STEPS):
        want = check(ctx, text, c, src_phase=3 + k, out_phase=11 - k)
    assert check(ctx, text, ALL_ON)[3]['cut_q3'] > 100
    for ls in ([5000] * 7, [30] * 40 + [4096, 4097, 9000] + [30] * 21, [300] * 29 + [4095, 4096, 4097] + [300] * 40):
        t = FI.lengths(ls, seed=len(ls), n_rate=0.02).replace(b'T', b'G')
        check(ctx, t, dict(polyg=2, q3=20, q5=18, flags=1), src_phase=9, out_phase=6)


@pytest.mark.parametrize('where', ['first', 'middle', 'last'])
def test_a_70000_base_read_cut_deep_inside(ctx, where):
    text, at = I.deep_text(where)
    want = check(ctx, text, dict(q3=I.T, q5=I.T), src_phase=13, out_phase=5)
    assert want[0][at] == (1700, 67000)                               # the highest sums lie steps away from their stops
    check(ctx, text, dict(q3=I.T), src_phase=2, out_phase=14)
    check(ctx, text, dict(head=5, tail=3, q5=I.T, polyg=3, flags=1), src_phase=6, out_phase=1)
    # poly-G and N runs that reach many steps into the long line
    qn, s, p, u = R.records(text)[at]
    s2 = b'n' * 5000 + s[5000:40000] + b'Gg' * 15000
    t2 = text.replace(s, s2)
    want = check(ctx, t2, dict(polyg=30000, flags=1), src_phase=4, out_phase=8)
    assert want[0][at] == (5000, 40000)
    assert check(ctx, t2, dict(polyg=30001), src_phase=4, out_phase=8)[0][at] == (0, 70000)


def test_a_slice_no_reads_and_reports_add(ctx):
    text = I.quality_shapes()
    n = len(R.records(text))
    for first, k in ((0, n), (17, 60), (n - 1, 1), (40, 0), (n, 0)):
        check(ctx, text, ALL_ON, src_phase=first % 16, out_phase=3, first=first, n=k)
    S = Source(ctx, text, 4)
    d_rep = ops.trim_report_new(ctx)
    assert ops.trim_report_fetch(ctx, d_rep) == dict.fromkeys(R.FIELDS, 0)
    for first, k in ((50, n - 50), (0, 50)):
        ops.trim_mark(ctx, d_rep, S.buf, S.ls, first, k, ops.trim_params(**ALL_ON))
    assert ops.trim_report_fetch(ctx, d_rep) == R.run(text, R.steps(**ALL_ON))[3]


def test_bad_arguments_are_refused(ctx):
    text = I.n_ends()
    S = Source(ctx, text)
    d_rep = ops.trim_report_new(ctx)
    w = ctx.torch.zeros(2 * S.reads, dtype=ctx.torch.int32, device=ctx.device)
    for kw, word in ((dict(q5=94), 'q5'), (dict(q3=94), 'q3'), (dict(crop=0), 'crop')):
        with pytest.raises(UqHipError, match=word):
            ops.trim_mark(ctx, d_rep, S.buf, S.ls, 0, S.reads, ops.trim_params(**kw), window=w)
    assert ops.trim_report_fetch(ctx, d_rep) == dict.fromkeys(R.FIELDS, 0) and int(w.abs().sum()) == 0


# ------------------------------------------------------------------ the copy
def sized(size, trim):
    """A record whose TRIMMED form (head = 1, tail = 2 when `trim`) holds exactly `size` bytes."""
    return FI.sized_record(size + (6 if trim else 0))


def test_piece_boundaries_around_a_tile_edge(ctx):
    """The end of the first record on every byte from -17 to +17 around the first tile's edge; the records behind it are a few bytes a piece, so
    the boundaries of all five pieces cross the edge byte by byte as well."""
    seen = set()
    small = [FI.record(b'ab', b'ACGTACG', b'IIIIIII', b'+x'), FI.record(b'', b'ACG', b'III'), FI.record(b'c', b'ACGT', b'II'),
             FI.record(b'dd', b'ACGTACGTACGTACGTACGTACGT', None), FI.record(b'e', b'NNNN', b'IIII')]
    for d in range(-17, 18):
        phase = (d * 7) % 16
        first = TILE - phase + d                                      # the first tile ends TILE - phase bytes into the output
        for trim in (True, False):
            c = dict(head=1, tail=2) if trim else {}
            text = FI.text([sized(first, trim)] + small)
            want = check(ctx, text, c, src_phase=(d * 3) % 16, out_phase=phase)
            assert want[1][1] == first
            # the same edge behind a run of short records, the long one last but two
            text = FI.text(small[:3] + [sized(first - (want[1][4] - want[1][1]), trim)] + small[3:])
            want = check(ctx, text, c, src_phase=(d * 5) % 16, out_phase=phase)
            assert want[1][4] == first
        seen.add(first - (TILE - phase))
    assert seen == set(range(-17, 18))


def test_more_than_4096_output_records_in_one_tile(ctx):
    """Records trimmed to their four newlines are the smallest output records: a tile of them fills the LDS list to its bound, and their
    entries are read from the index (the LDS entries hold the records of tiles with fewer of them)."""
    n = 3 * TILE // 4
    text = b'\nACGTACGT\n\nIIIIIIII\n' * n
    for phases in ((0, 0), (5, 9)):
        want = check(ctx, text, dict(head=100), src_phase=phases[1], out_phase=phases[0])
        assert want[2] == b'\n\n\n\n' * n and want[3]['emptied'] == n
    # a record that begins in front of every tile edge, then 4-byte records up to the next edge and beyond, a long one in between
    for lead in (6, 7, 9):
        text = FI.sized_record(lead + 16) + b'\nACGTACGT\n\nIIIIIIII\n' * (n // 2) + FI.sized_record(300) + b'\nACGT\n\nIIII\n' * (n // 2)
        check(ctx, text, dict(head=8, crop=140), src_phase=3, out_phase=lead)


def tiny_trimmable(n=48, seed=4):
    rnd = random.Random(seed)
    out = []
    for k in range(n):
        L = rnd.randrange(0, 6)
        out.append(b''.join(x + b'\n' for x in (b'@'[:rnd.randrange(0, 2)],bytes(rnd.choice(b'ACGTN') for _ in range(L)), b'+'[:rnd.randrange(0, 2)],
                                                  bytes(rnd.randrange(33, 75) for _ in range(L)))))
    return FI.text(out)


TINY = tiny_trimmable()


@pytest.mark.parametrize('out_phase', range(16))
def test_tiny_records_at_every_phase(ctx, out_phase):
    """Output records of 4 to 14 bytes: a vector holds up to four records and many pieces; every output phase, four source phases."""
    sizes = [b - a for a, b in zip(R.run(TINY, R.steps(head=1))[1], R.run(TINY, R.steps(head=1))[1][1:])]
    assert min(sizes) == 4 and max(sizes) <= 14
    for src_phase in (0, 5, 10, 15):
        check(ctx, TINY, dict(head=1), src_phase=src_phase, out_phase=out_phase)
        check(ctx, FI.tiny_records(), dict(tail=1, flags=1), src_phase=src_phase, out_phase=out_phase)      # (Ls != Lu in most: unchanged)


def test_the_identity_trim_gives_the_input_back(ctx):
    for text in (FI.short_records(300), I.long_reads_among_short(), FI.odd_shapes(), I.deep_text('middle')[0]):
        for c in ({}, dict(polyg=100000), dict(crop=R.U32 - 1)):
            assert check(ctx, text, c, src_phase=5, out_phase=12, room=40)[2] == text


def test_a_capacity_one_byte_short_is_refused_and_no_reads_is_a_no_op(ctx):
    text = I.n_ends()
    S = Source(ctx, text, 4)
    want = R.run(text, R.steps(flags=1))
    d_rep = ops.trim_report_new(ctx)
    w = ops.trim_mark(ctx, d_rep, S.buf, S.ls, 0, S.reads, ops.trim_params(flags=1))
    dst, size = ops.trim_plan(ctx, S.ls, 0, S.reads, w)
    out = Output(ctx, size, 2)
    with pytest.raises(UqHipError, match='out_capacity'):
        ops.trim_records(ctx, S.buf, S.ls, 0, S.reads, w, dst, out=out.buf, out_capacity=size - 1)
    assert out.result() == guarded(b'', size)
    ops.trim_records(ctx, S.buf, S.ls, 0, 0, w, dst, out=out.buf, out_capacity=0)                     # no reads: nothing happens, whatever the capacity says
    assert out.result() == guarded(b'', size)
    ops.trim_records(ctx, S.buf, S.ls, 0, S.reads, w, dst, out=out.buf)
    assert out.result() == guarded(want[2])


@pytest.mark.parametrize('length', [(36, 301), 150], ids=['36-301bp', '150bp'])
def test_device_against_the_host_twins_and_the_fingerprint(ctx, length):
    """6000 synthetic reads: the device against the sequential twins, and a cross-check through code that knows nothing of trimming -- the
    fingerprint of the trimmed text has the input's reads and QNAME sum, and bases_out bases."""
    text = synth.fastq(20261020, 6000, length, n_rate=2)
    c = dict(head=1, polyg=3, q5=14, q3=16, flags=1)
    ls = ops.host_line_starts(text)
    hw, hrep = ops.trim_mark_host(text, ops.trim_params(**c), ls)
    hdst, hsize = ops.trim_plan_host(ls, hw)
    want = ops.trim_records_host(text, ls, hw, hdst).tobytes()
    assert 1000 < hrep['reads_trimmed'] and hrep['cut_q3'] > 1000 and hrep['cut_q5'] > 100
    S = Source(ctx, text, 5)
    d_rep = ops.trim_report_new(ctx)
    w = ops.trim_mark(ctx, d_rep, S.buf, S.ls, 0, 6000, ops.trim_params(**c))
    assert ctx.to_numpy(w).tobytes() == hw.tobytes()
    dst, size = ops.trim_plan(ctx, S.ls, 0, 6000, w)
    rep = ops.trim_report_fetch(ctx, d_rep)
    assert size == hsize and rep == hrep
    out = Output(ctx, size, 13)
    _, lso = ops.trim_records(ctx, S.buf, S.ls, 0, 6000, w, dst, out=out.buf, index=True)
    assert out.result() == guarded(want)
    before, after = ops.fingerprint(ctx, S.buf, S.ls, 6000), ops.fingerprint(ctx, out.buf, lso, 6000)
    assert after['reads'] == before['reads'] == 6000 and after['qname'] == before['qname'] and after['bases'] == rep['bases_out'] < before['bases']


# ------------------------------------------------------------------ offsets beyond 2^32
def test_beyond_4_gib(ctx):
    """13 M reads of 36 .. 301 bases made on the device (4.8 GB): the source passes 2^32.  The identity trim gives the source back; tail = 50
    with q3 = 16 gives a text whose index is what uq_index_lines writes for it and whose fingerprint has the source's reads and QNAME sum."""
    t = ctx.torch
    n = 13_000_000
    free = t.cuda.mem_get_info(ctx.device)[0]
    if free < 14 << 30: pytest.skip('needs 14 GiB of free device memory, %.1f are free' % (free / 2 ** 30))
    src = ops.synth_fastq(ctx, synth.Spec(20261020, (36, 301), n_rate=1), 0, n)
    nl = ops.count_lines(ctx, src)
    ls = ops.index_lines(ctx, src, nl)
    assert nl == 4 * n and src.numel() > (1 << 32) + (1 << 20)
    before = ops.fingerprint(ctx, src, ls, n)
    for c in ({}, dict(tail=50, q3=16)):
        d_rep = ops.trim_report_new(ctx)
        w = ops.trim_mark(ctx, d_rep, src, ls, 0, n, ops.trim_params(**c))
        dst, size = ops.trim_plan(ctx, ls, 0, n, w)
        rep = ops.trim_report_fetch(ctx, d_rep)
        assert rep['reads_in'] == n and rep['bytes_in'] == src.numel() and rep['bases_in'] == before['bases'] and rep['bytes_out'] == size
        assert rep['bytes_in'] - rep['bytes_out'] == 2 * (rep['bases_in'] - rep['bases_out'])
        out, lso = ops.trim_records(ctx, src, ls, 0, n, w, dst, out_bytes=size, index=True)
        if not c:
            assert size == src.numel() and t.equal(out, src) and t.equal(lso, ls) and rep['reads_trimmed'] == 0
        else:
            assert (1 << 31) < size < src.numel() and rep['cut_fixed'] > 45 * n and rep['cut_q3'] > 0
            assert ops.count_lines(ctx, out) == 4 * n and t.equal(lso, ops.index_lines(ctx, out, 4 * n))
            fp = ops.fingerprint(ctx, out, lso, n)
            assert fp['reads'] == n and fp['qname'] == before['qname'] and fp['bases'] == rep['bases_out']
        del out, lso, dst, w
