"""GPU: uq_adapter_mark against the pure-Python definition (tests/adapter_ref.py).  The windows and the report are each compared as the WHOLE
buffer between two guards of 64 bytes; the source lies at chosen 16-byte phases and its allocation ends with the text.

The kernel (csrc/adapter.hip) stages tiles of at most 64 records in 20 KiB of LDS, packs a record's window to 2 bits a base (16 bases a
dword), and gives P lanes (4 .. 16) to a record: they test the positions a + lane, a + lane + P, ... and a ballot after every step finds the
first candidate.  A position reads 32 (adapters up to 32 bases) or 64 bases at its bit offset.  Tiles beyond the stage are read from HBM by
half-waves, lines beyond 4096 bytes by the whole workgroup in segments of 16384 positions.  The inputs are built from that."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import adapter_inputs as I
import adapter_ref as R
import filter_inputs as FI
import trim_ref as TR
from filter_inputs import record
from uq_amd import _lib, ops, synth
from uq_amd._lib import UqHipError

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP, RMAX, LONG, SEG = 20480, 64, 4096, 16384
LENGTHS = list(range(18)) + [31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]


def test_the_geometry_is_the_kernels():
    src = open(os.path.join(REPO, 'uq_amd', 'csrc', 'adapter.hip')).read()
    assert int(re.search(r'AD_NV = (\d+);', src).group(1)) * 256 * 16 == CAP and re.search(r'AD_CAP = AD_NV \* 256 \* 16;', src)
    assert int(re.search(r'AD_RMAX = (\d+);', src).group(1)) == RMAX and int(re.search(r'AD_LONG = (\d+);', src).group(1)) == LONG
    assert int(re.search(r'AD_SEG = (\d+);', src).group(1)) == SEG
    assert re.search(r'R = \(AD_CAP - 64\) / \(avg \+ avg / 8 \+ 1\);', src) and re.search(r'x\.staged = span \+ 16 <= AD_CAP;', src)


def geometry(text):
    """(R, P) the kernel works out for a text: records a tile, lanes a record."""
    n = len(TR.records(text))
    avg = len(text) // n + 1
    Rr = max(1, min(RMAX, (CAP - 64) // (avg + avg // 8 + 1)))
    P = 16
    while P > 1 and P * Rr > 256: P >>= 1
    return Rr, P


class Source:
    """A text in HBM at an address `phase` bytes past a 16-byte boundary, and its record index; tight: the allocation ends with the text."""

    def __init__(self, ctx, text, phase=0):
        t = ctx.torch
        self.whole = t.full((len(text) + phase % 16,), FILL, dtype=t.uint8, device=ctx.device)
        start = (phase - self.whole.data_ptr()) % 16
        self.buf = self.whole[start:start + len(text)]
        if len(text): self.buf.copy_(ctx.to_device(np.frombuffer(text, dtype=np.uint8)))
        assert self.buf.data_ptr() % 16 == phase % 16 and self.buf.numel() == len(text) and start + len(text) == self.whole.numel()
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

    def fill(self, data):
        if len(data): self.buf.copy_(self.ctx.to_device(np.frombuffer(data, dtype=np.uint8)))

    def result(self):
        return self.ctx.to_numpy(self.region).tobytes()


def guarded(data):
    return bytes([FILL]) * GUARD + data + bytes([FILL]) * GUARD


def words(values, dtype):
    return np.array(values, dtype=dtype).tobytes()


def lib_params(c):
    letters = lambda cl: None if cl is None else ''.join('ACGT'[k] for k in cl)
    return ops.adapter_params(letters(c['seq']), letters(c['seq2']), c['err'], c['overlap'], c['flags'])


def check(ctx, text, c, src_phase=0, first=0, n=None, windows=None, want=None):
    """uq_adapter_mark on the records [first, first + n): windows and report whole, between their guards -> what adapter_ref.run returns.
    `windows`: the ones handed in (FRESH: what the buffer holds before the call, which must not matter)."""
    S = Source(ctx, text, src_phase)
    n = S.reads - first if n is None else n
    if want is None: want = R.run(text, c, first, n, windows)
    W = Output(ctx, 8 * n, 4 * (src_phase % 4))                     # u32 pairs: any 4-byte phase
    if windows is not None: W.fill(words([v for w in windows for v in w], np.uint32))
    Rp = Output(ctx, 8 * len(R.FIELDS), 8)
    _lib.call('uq_adapter_report_init', ctx.h, ops._p(Rp.buf))
    ops.adapter_mark(ctx, Rp.buf, S.buf, S.ls, first, n, lib_params(c), window=W.buf)
    got = np.frombuffer(W.result()[GUARD:GUARD + 8 * n], np.uint32).reshape(-1, 2)
    bad = [(i, tuple(got[i]), want[0][i]) for i in range(n) if tuple(got[i]) != want[0][i]][:5]
    assert not bad, bad
    assert W.result() == guarded(words([v for w in want[0] for v in w], np.uint32))
    assert Rp.result() == guarded(words([want[1][k] for k in R.FIELDS], np.uint64))
    return want


# ------------------------------------------------------------------ every start, every overlap
@pytest.mark.parametrize('La', [1, 13, 32, 33, 64])
def test_the_adapter_at_every_position_and_every_overlap(ctx, La):
    """Lines of 0 .. 17, 31 .. 33, 63 .. 65, 127 .. 129 and 255 .. 257 bases; in each the adapter begins at every position (so it also overlaps
    the end by every length up to La); La = 1, 13, 32, 33, 64: the packed words' boundaries."""
    A = I.adapter(La)
    recs = []
    for L in LENGTHS:
        base = I.body(L, L)
        recs.append(record(b'plain%d' % L, base))
        for start in range(L):
            recs.append(record(b'L%d_s%d' % (L, start), I.implant(base, A, start)))
    text = FI.text(recs)
    cuts = set()
    for k, (err, overlap) in enumerate(((0, 1), (10, min(3, La)), (0, La))):
        want = check(ctx, text, R.params(A, err=err, overlap=overlap, flags=R.FRESH), src_phase=(5 * k + La) % 16)
        if k == 0:
            cuts = {(len(r[1]), b) for r, (a, b) in zip(TR.records(text), want[0]) if b < len(r[1])}
            assert want[1]['full'] > 100 and (La == 1 or want[1]['partial'] > 100) and want[1]['emptied'] >= len(LENGTHS) - 1
    if La > 1: assert all((L, s) in cuts for L in (65, 129, 257) for s in range(1, L - La + 1))     # every start of a full match is found


def test_threshold_edges(ctx):
    recs, expect = [], []
    for m in (9, 10, 19, 20):
        for A, full in ((I.adapter(m), True), (I.adapter(33), False)):
            for name, line, mm, wrong in I.threshold_edges(A, 10, (m,)):
                want = check(ctx, record(name, line), R.params(A, err=10, overlap=3, flags=R.FRESH), src_phase=m % 16)
                hit = want[0][0] == (0, 17 if full else 40 - m)
                assert hit == (len(wrong) <= (m * 10) // 100), (name, wrong, want[0])
                expect.append(hit)
    assert expect.count(True) >= 12 and expect.count(False) >= 12
    # err = 30 at 64 bases: 19 mismatches pass, 20 do not
    A = I.adapter(64)
    for nwrong, hit in ((19, True), (20, False)):
        line = b'N' * 9 + I.implant(A, A, 0, wrong=range(0, 3 * nwrong, 3)[:nwrong]) + b'N' * 4
        assert (check(ctx, record(b'w', line), R.params(A, err=30, overlap=3, flags=R.FRESH), src_phase=3)[0][0] == (0, 9)) == hit


def test_n_lower_case_and_cr(ctx):
    A = I.adapter(20)
    recs = []
    for bad in (b'N', b'n', b'\r', b'.', b'\xe1', None):
        for j in (0, 7, 8, 19):
            s = bytearray(b'N' * 10 + A + b'N' * 5)
            if bad: s[10 + j:11 + j] = bad
            recs.append(record(b'b%d' % j, bytes(s)))
    recs.append(record(b'lc', b'N' * 10 + A.lower() + b'NN'))
    recs.append(record(b'mixed', I.body(40, 1).lower() + A[:9].lower() + A[9:] + b'acgt'))
    text = FI.text(recs) + b'@r\r\n' + b'NNNN' + A[:6] + b'\r\n+\r\n' + b'I' * 10 + b'\r\n'
    for err in (0, 10, 20):
        want = check(ctx, text, R.params(A, err=err, flags=R.FRESH), src_phase=err % 16)
    assert check(ctx, text, R.params(A, err=0, flags=R.FRESH))[0][-1] == (0, 11)


@pytest.mark.parametrize('long_ones', [0, 16], ids=['P=4', 'P=16'])
def test_the_leftmost_candidate_across_the_ballot(ctx, long_ones):
    """Two candidates one position apart (a run of nine A under the adapter AAAAAAAA) beginning at every position 0 .. 70: in the last lane of a
    step and the first of the next, and both in one step; and a worse match left of a better one."""
    A = b'A' * 8
    recs = [record(b'p%d' % p, b'C' * p + b'A' * 9 + b'C' * (80 - p)) for p in range(71)]
    A20 = I.adapter(20)
    worse = I.implant(A20, A20, 0, wrong=(3, 11))
    recs += [record(b'long%d' % k, I.body(3000, k, b'CT')) for k in range(long_ones)]
    text = FI.text(recs)
    assert geometry(text)[1] == (16 if long_ones else 4)
    want = check(ctx, text, R.params(A, err=0, overlap=8, flags=R.FRESH), src_phase=long_ones)
    assert [w[1] for w in want[0][:71]] == list(range(71))
    two = FI.text([record(b't%d' % p, b'N' * p + worse + b'N' * 4 + A20 + b'N' * 3) for p in range(40)] + recs[71:])
    want = check(ctx, two, R.params(A20, err=10, flags=R.FRESH), src_phase=7)
    assert [w[1] for w in want[0][:40]] == list(range(40))
    assert [w[1] for w in check(ctx, two, R.params(A20, err=0, flags=R.FRESH), src_phase=8)[0][:40]] == [p + 24 for p in range(40)]


# ------------------------------------------------------------------ beyond the stage
def long_read(L, A, where, seed):
    """A read of L random C/T bases (the adapters hold A and G: nothing matches by chance) with the adapter at `where` (None: nowhere)."""
    s = I.body(L, seed, b'CT')
    return s if where is None else I.implant(s, A, where)


@pytest.mark.parametrize('La', [13, 33])
def test_reads_of_5000_and_70000_bases(ctx, La):
    """The adapter 3 bases from the start, across the 4096-byte boundary, across the workgroup's segment boundary, as a partial match of 3
    bases at the very end, and nowhere; the long reads among short ones, first, in the middle and last."""
    A = I.adapter(La)
    assert set(A) & set(b'AG')
    for L, places in ((5000, (3, LONG - 5, LONG, 4990, None)), (70000, (3, LONG - 5, SEG - La + 1, SEG - 1, SEG, 3 * SEG - 2, 4 * SEG + 7, None))):
        small = [record(b's%d' % k, I.implant(I.body(20 + 9 * k, k), A, 5 + k)) for k in range(10)]
        longs = [record(b'at%s' % str(w).encode(), long_read(L, A, w, i)) for i, w in enumerate(places)]
        longs.append(record(b'end3', long_read(L, A, L - 3, 99)))
        longs.append(record(b'end%d' % (La - 1), long_read(L, A, L - La + 1, 98)))
        text = FI.text(small[:3] + longs[:2] + small[3:7] + longs[2:] + small[7:])
        c = R.params(A, err=0, overlap=3, flags=R.FRESH)
        want = check(ctx, text, c, src_phase=La % 16)
        got = {r[0]: w for r, w in zip(TR.records(text), want[0])}
        for w in places:
            assert got[b'@at%s' % str(w).encode()] == (0, L if w is None else w)
        assert got[b'@end3'] == (0, L - 3) and got[b'@end%d' % (La - 1)] == (0, L - La + 1)
        # one long read first and one last; with mismatches allowed
        text = FI.text([longs[1]] + small + [longs[-1]])
        check(ctx, text, R.params(A, err=10, overlap=3, flags=R.FRESH), src_phase=2)
        # windows handed in: the adapter beyond b is not seen, a partial match is measured against b
        wins = [(0, len(r[1])) for r in TR.records(text)]
        wins[0] = (2, LONG - 5 + 4)
        wins[-1] = (L - 100, L - 1)
        w2 = check(ctx, text, R.params(A, err=0, overlap=3), src_phase=9, windows=wins)
        assert w2[0][0] == (2, LONG - 5) and w2[0][-1] == (L - 100, L - La + 1 if La - 2 >= 3 else L - 1)


def test_tiles_beyond_the_stage(ctx):
    """Runs of longer-than-average reads: tiles whose span passes the stage are read from HBM by half-waves, lines of 4095, 4096 and 4097
    bases on both sides of the whole-workgroup threshold."""
    A = I.A33
    rnd = random.Random(5)
    for k, ls in enumerate(([5000] * 7, [30] * 40 + [4096, 4097, 9000] + [30] * 21, [300] * 29 + [4095, 4096, 4097] + [300] * 40,
                            [100] * 200 + [900] * 40 + [100] * 200)):
        recs = []
        for i, L in enumerate(ls):
            s = I.body(L, i)
            if i % 2 == 0: s = I.implant(s, A, rnd.randrange(0, L))
            recs.append(record(b'r%d' % i, s, None if i % 11 else b'I' * (L + 1)))       # (and lines of different lengths among them)
        text = FI.text(recs)
        want = check(ctx, text, R.params(A, err=10, overlap=3, flags=R.FRESH), src_phase=3 + k)
        assert want[1]['reads_cut'] * 3 > len(ls) and want[1]['len_mismatch'] > 0
        check(ctx, text, R.params(A[:13], A, err=10, overlap=3, flags=R.FRESH | R.PAIRED), src_phase=11)


def edge_text(d):
    """32 records, 16 a tile: the first tile's span is CAP - 16 + d bytes with the source at phase 0 (staged for d <= 0, from HBM beyond), the
    whole text's size -- and with it the geometry -- the same for every d."""
    first = [FI.sized_record(1279)] * 14
    a, b = 1279 + (CAP - 16 - 16 * 1279) + d, 921 - d
    recs = [FI.sized_record(a)] + first + [FI.sized_record(1279)] + [FI.sized_record(b)] + [FI.sized_record(921)] * 15
    return recs


def test_a_record_boundary_on_every_byte_around_the_stage_edge(ctx):
    A = I.A33
    seen = set()
    for d in range(-20, 21):
        recs = edge_text(d)
        out = []
        for i, r in enumerate(recs):
            qn, s, p, u = r.split(b'\n')[:4]
            if len(s) == len(u) and len(s) > 40: s = I.implant(s, A, (37 * i + 5 * d) % (len(s) - 1) if i % 3 else len(s) - 1 - i)
            out.append(qn + b'\n' + s + b'\n' + p + b'\n' + u + b'\n')
        text = FI.text(out)
        assert geometry(text) == (16, 16) and sum(len(r) for r in out[:16]) == CAP - 16 + d
        for phase in (0, (3 * d) % 16):
            want = check(ctx, text, R.params(A, err=10, overlap=3, flags=R.FRESH), src_phase=phase)
        assert want[1]['reads_cut'] >= 20
        seen.add(d)
    assert seen == set(range(-20, 21))


def test_12288_records_of_4_to_14_bytes(ctx):
    rnd = random.Random(12)
    recs = []
    for k in range(12288):
        L = rnd.randrange(0, 5)
        recs.append(b''.join(x + b'\n' for x in (b'@'[:rnd.randrange(0, 2)], bytes(rnd.choice(b'ACGTN') for _ in range(L)), b'+'[:rnd.randrange(0, 2)],
                                                  bytes(rnd.randrange(33, 75) for _ in range(L if rnd.random() > 0.05 else 1)))))
    text = FI.text(recs)
    assert min(len(r) for r in recs) == 4 and max(len(r) for r in recs) <= 14
    for k, (A, overlap) in enumerate(((b'A', 1), (b'AC', 1), (b'ACG', 2), (b'GT', 2))):
        want = check(ctx, text, R.params(A, err=0, overlap=overlap, flags=R.FRESH), src_phase=5 * k)
        assert want[1]['reads_cut'] > 200 and want[1]['emptied'] > 50 and want[1]['len_mismatch'] > 100


# ------------------------------------------------------------------ windows handed in, mates, slices, sums
def test_windows_from_the_trimmer(ctx):
    A = I.A33
    recs = []
    for i, (qn, s, p, u) in enumerate(TR.records(I.seeded(600, A, lo=0, hi=130))):
        if i % 5 == 0: s, u = s + b'G' * 12, u + b'#' * 12
        recs.append(qn + b'\n' + s + b'\n' + p + b'\n' + u + b'\n')
    text = b''.join(recs)
    steps = TR.steps(polyg=8, q3=20)
    twins = TR.run(text, steps)[0]
    c = R.params(A, err=10, overlap=3)
    want = R.run(text, c, windows=twins)
    S = Source(ctx, text, 6)
    W = Output(ctx, 8 * S.reads, 4)
    d_trep = ops.trim_report_new(ctx)
    ops.trim_mark(ctx, d_trep, S.buf, S.ls, 0, S.reads, ops.trim_params(**steps), window=W.buf)
    assert W.result() == guarded(words([v for w in twins for v in w], np.uint32))
    d_rep = ops.adapter_report_new(ctx)
    ops.adapter_mark(ctx, d_rep, S.buf, S.ls, 0, S.reads, lib_params(c), window=W.buf)
    assert W.result() == guarded(words([v for w in want[0] for v in w], np.uint32))
    rep = ops.adapter_report_fetch(ctx, d_rep)
    assert rep == want[1] and rep['bases_in'] == ops.trim_report_fetch(ctx, d_trep)['bases_out'] and rep['reads_cut'] > 100
    # plan and copy take the narrowed windows as they are
    dst, size = ops.trim_plan(ctx, S.ls, 0, S.reads, W.buf)
    out = ops.trim_records(ctx, S.buf, S.ls, 0, S.reads, W.buf, dst, out_bytes=size)
    assert ctx.to_numpy(out).tobytes() == want[3] == R.after_trim(text, steps, c)
    # FRESH: what the window buffer holds does not matter; given identity windows: the same
    fresh = check(ctx, text, dict(c, flags=R.FRESH), src_phase=1, windows=[(77, 3)] * S.reads, want=R.run(text, dict(c, flags=R.FRESH)))
    ident = check(ctx, text, c, src_phase=1, windows=[(0, len(r[1])) for r in TR.records(text)])
    assert fresh[:2] == ident[:2]
    # windows with a > 0 and b < Ls
    wins = [(min(3, len(r[1])), max(len(r[1]) - 4, min(3, len(r[1])))) if len(r[1]) == len(r[3]) else (0, len(r[1])) for r in TR.records(text)]
    check(ctx, text, c, src_phase=13, windows=wins)


def test_mates_slices_and_reports_add(ctx):
    A1, A2 = I.adapter(33), I.adapter(20, seed=7)
    text = I.seeded(900, A1, lo=0, hi=150, A2=A2)
    c = R.params(A1, A2, err=10, overlap=3, flags=R.FRESH | R.PAIRED)
    whole = check(ctx, text, c, src_phase=2)
    assert whole[1]['mate2'] > 50 and whole[1]['reads_cut'] - whole[1]['mate2'] > 50
    for first, k in ((0, 900), (1, 301), (2, 300), (899, 1), (450, 0), (900, 0)):
        got = check(ctx, text, c, src_phase=first % 16, first=first, n=k)
        assert got[0] == whole[0][first:first + k]
    assert check(ctx, text, dict(c, flags=R.FRESH), src_phase=4)[1]['mate2'] == 0
    S = Source(ctx, text, 4)
    d_rep = ops.adapter_report_new(ctx)
    assert ops.adapter_report_fetch(ctx, d_rep) == dict.fromkeys(R.FIELDS, 0)
    for first, k in ((333, 567), (0, 333)):
        ops.adapter_mark(ctx, d_rep, S.buf, S.ls, first, k, lib_params(c))
    assert ops.adapter_report_fetch(ctx, d_rep) == whole[1]
    ops.adapter_mark(ctx, d_rep, S.buf, S.ls, 0, 900, lib_params(c))
    assert ops.adapter_report_fetch(ctx, d_rep) == {k: 2 * v for k, v in whole[1].items()}


@pytest.mark.parametrize('length', [(36, 301), 150], ids=['36-301bp', '150bp'])
def test_device_against_the_host_twin(ctx, length):
    """6000 synthetic reads with the adapter written into a third: the device against the sequential twin, through trim, adapter, plan, copy."""
    A = I.A33
    text = I.implant_text(synth.fastq(20261021, 6000, length, n_rate=2), A)
    ls = ops.host_line_starts(text)
    steps = dict(polyg=8, q3=20)
    hw, _ = ops.trim_mark_host(text, ops.trim_params(**steps), ls)
    for La, paired in ((13, False), (33, True)):
        p = ops.adapter_params(A[:La].decode(), A.decode() if paired else None, 10, 3, 2 if paired else 0)
        hw2, hrep = ops.adapter_mark_host(text, p, ls, window=hw)
        assert hrep['reads_cut'] > 1500 and hrep['full'] > 500 and hrep['partial'] > 100
        S = Source(ctx, text, 5)
        d_rep, d_trep = ops.adapter_report_new(ctx), ops.trim_report_new(ctx)
        w = ops.trim_mark(ctx, d_trep, S.buf, S.ls, 0, 6000, ops.trim_params(**steps))
        ops.adapter_mark(ctx, d_rep, S.buf, S.ls, 0, 6000, p, window=w)
        assert ctx.to_numpy(w).tobytes() == hw2.tobytes() and ops.adapter_report_fetch(ctx, d_rep) == hrep


# ------------------------------------------------------------------ errors
def test_bad_arguments_are_refused(ctx):
    text = I.seeded(50, I.ILLUMINA)
    S = Source(ctx, text)
    P = ops.adapter_params
    ok = dict(seq='ACGTACGT', err=10, overlap=3, flags=1)
    t = ctx.torch
    w = t.zeros(2 * S.reads + 2, dtype=t.int32, device=ctx.device)
    d_rep = ops.adapter_report_new(ctx)
    for kw, word in ((dict(ok, seq=''), 'len1'), (dict(ok, len1=65), 'len1'), (dict(ok, seq2='ACG', len2=65), 'len2'), (dict(ok, flags=3), 'len2'),
                     (dict(ok, seq=[0, 1, 4, 2]), r'seq1\[2\]'), (dict(ok, seq2=[0, 1, 2, 9]), r'seq2\[3\]'), (dict(ok, overlap=0), 'overlap'),
                     (dict(ok, overlap=9), 'overlap'), (dict(ok, seq2='ACGT', flags=3, overlap=5), 'overlap'), (dict(ok, err=31), 'err_pct'),
                     (dict(ok, flags=5), 'flag'), (dict(ok, reserved=(1, 0, 0)), 'reserved')):
        with pytest.raises(UqHipError, match=word):
            ops.adapter_mark(ctx, d_rep, S.buf, S.ls, 0, S.reads, P(**kw), window=w)
    p = P(**ok)
    args = [ctx.h, ops._p(S.buf), ops._p(S.ls), 0, S.reads, ctypes.byref(p), ops._p(w), ops._p(d_rep)]
    for k in (0, 1, 2, 5, 6, 7):
        bad = list(args); bad[k] = None
        with pytest.raises(UqHipError, match='null'):
            _lib.call('uq_adapter_mark', *bad)
    wb = w.view(t.uint8)
    with pytest.raises(UqHipError, match='4-byte'):
        _lib.call('uq_adapter_mark', *(args[:6] + [ops._p(wb[2:]), args[7]]))
    with pytest.raises(UqHipError, match='8-byte'):
        _lib.call('uq_adapter_mark', *(args[:7] + [ops._p(d_rep.view(t.uint8)[4:])]))
    with pytest.raises(UqHipError, match='null'):
        _lib.call('uq_adapter_report_init', ctx.h, None)
    with pytest.raises(ValueError):
        ops.adapter_mark(ctx, d_rep, S.buf, S.ls, 0, S.reads, P(**dict(ok, flags=0)))
    assert ops.adapter_report_fetch(ctx, d_rep) == dict.fromkeys(R.FIELDS, 0) and int(w.abs().sum()) == 0
    _lib.call('uq_adapter_mark', *args)
    assert ops.adapter_report_fetch(ctx, d_rep)['reads_in'] == S.reads


# ------------------------------------------------------------------ offsets beyond 2^32
def test_beyond_4_gib(ctx):
    """13 M reads of 36 .. 301 bases made on the device (4.8 GB): the source passes 2^32.  The report's sums against the fingerprint's, and the
    windows of the 4000 records around the 2^32 mark against the host twin on their bytes."""
    t = ctx.torch
    n = 13_000_000
    free = t.cuda.mem_get_info(ctx.device)[0]
    if free < 14 << 30: pytest.skip('needs 14 GiB of free device memory, %.1f are free' % (free / 2 ** 30))
    src = ops.synth_fastq(ctx, synth.Spec(20261021, (36, 301), n_rate=1), 0, n)
    nl = ops.count_lines(ctx, src)
    ls = ops.index_lines(ctx, src, nl)
    assert nl == 4 * n and src.numel() > (1 << 32) + (1 << 20)
    p = ops.adapter_params('GAT', None, 0, 3, ops.ADAPTER_FRESH)               # three bases: found in most reads, at any depth
    d_rep = ops.adapter_report_new(ctx)
    w = ops.adapter_mark(ctx, d_rep, src, ls, 0, n, p)
    rep = ops.adapter_report_fetch(ctx, d_rep)
    assert rep['reads_in'] == n and rep['bases_in'] == ops.fingerprint(ctx, src, ls, n)['bases'] and rep['len_mismatch'] == 0
    assert rep['reads_cut'] == rep['full'] + rep['partial'] > n // 2
    wv = w.view(t.int32).reshape(-1, 2).to(t.int64)
    assert int(wv[:, 1].sum()) == rep['bases_out'] and int(wv[:, 0].abs().sum()) == 0
    # the records around the 2^32 mark, on the host
    starts = ls[::4].contiguous()
    at = int(t.searchsorted(starts, 1 << 32))
    lo, hi = at - 2000, at + 2000
    o0, o1 = int(starts[lo]), int(starts[hi])
    assert o0 < (1 << 32) < o1
    piece = ctx.to_numpy(src[o0:o1]).tobytes()
    hw, _ = ops.adapter_mark_host(piece, p)
    assert ctx.to_numpy(w[2 * lo:2 * hi]).tobytes() == hw.tobytes()
