"""GPU: uq_interleave_records and uq_mate_check against the pure-Python definitions (tests/pairs_ref.py).  Every interleave comparison is
the WHOLE output buffer between two guards of 64 bytes, with the sources and the output placed at chosen 16-byte phases.

The kernel (csrc/pairs.hip) cuts the output into tiles of TILE = PR_TILE bytes at 16-byte-aligned addresses; an item is one aligned output
vector, copied by one load and one store when it lies inside one segment and byte by byte when it crosses a segment boundary.  The inputs
(tests/pairs_inputs.py) are built from that: records of 7 to 14 bytes at every output phase, a boundary on every byte from -17 to +17
around a tile's edge, more than 256 pairs in one tile, a 70 000-base record first, in the middle and last."""
import os
import re

import numpy as np
import pytest

import pairs_inputs as I
import pairs_ref as R
from uq_amd import ops, synth
from uq_amd._lib import UqHipError

pytestmark = pytest.mark.gpu

TILE = 16384
GUARD = 64
FILL = 0xA5
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_tile_size_is_the_kernels():
    src = open(os.path.join(REPO, 'uq_amd', 'csrc', 'pairs.hip')).read()
    threads = int(re.search(r'PR_THREADS = (\d+);', src).group(1))
    unroll = int(re.search(r'PR_UNROLL = (\d+);', src).group(1))
    assert re.search(r'PR_TILE = PR_THREADS \* PR_UNROLL \* 16;', src)
    assert threads * unroll * 16 == TILE


class Source:
    """A text in HBM at an address `phase` bytes past a 16-byte boundary, and its record index."""

    def __init__(self, ctx, text, phase=0):
        t = ctx.torch
        self.whole = t.full((len(text) + 48,), FILL, dtype=t.uint8, device=ctx.device)
        start = (phase - self.whole.data_ptr()) % 16
        self.buf = self.whole[start:start + len(text)]
        if len(text): self.buf.copy_(ctx.to_device(np.frombuffer(text, dtype=np.uint8)))
        assert self.buf.data_ptr() % 16 == phase % 16
        self.ls = ctx.to_device(ops.host_line_starts(text).view(np.int64))
        self.reads = (self.ls.numel() - 1) // 4


class Output:
    """`size` bytes of FILL in HBM at a chosen phase, between two guards; behind = bytes of the buffer past what the call should write."""

    def __init__(self, ctx, size, phase=0):
        t = ctx.torch
        self.ctx, self.size = ctx, size
        self.whole = t.full((size + 2 * GUARD + 32,), FILL, dtype=t.uint8, device=ctx.device)
        start = GUARD + (phase - self.whole.data_ptr() - GUARD) % 16
        self.region = self.whole[start - GUARD:start + size + GUARD]
        self.buf = self.whole[start:start + size]
        assert self.buf.data_ptr() % 16 == phase % 16

    def result(self):
        return self.ctx.to_numpy(self.region).tobytes()


def guarded(text, size=None):
    size = len(text) if size is None else size
    return bytes([FILL]) * GUARD + text + bytes([FILL]) * (size - len(text) + GUARD)


def check(ctx, a, b, out_phase=0, a_phase=0, b_phase=0, first=0, n=None, room=0):
    A, B = Source(ctx, a, a_phase), Source(ctx, b, b_phase)
    n = A.reads - first if n is None else n
    want = R.interleave(a, b, first, n)
    out = Output(ctx, len(want) + room, out_phase)
    ops.interleave_records(ctx, A.buf, A.ls, B.buf, B.ls, first, n, out=out.buf)
    assert out.result() == guarded(want, len(want) + room)
    return want


def test_one_pair(ctx):
    a, b = I.one_pair()
    for phase in (0, 1, 15):
        assert check(ctx, a, b, phase, 3, 7) == a + b


TINY = I.tiny_pairs()


@pytest.mark.parametrize('out_phase', range(16))
def test_tiny_records_at_every_phase(ctx, out_phase):
    """A vector holds up to three segments; every output phase, four source phases each."""
    a, b = TINY
    assert len(R.records(a)) >= 40
    for a_phase, b_phase in ((0, 0), (1, 5), (7, 2), (15, 11)):
        check(ctx, a, b, out_phase, a_phase, b_phase)


def test_unequal_and_variable_lengths(ctx):
    a, b = I.unequal_pairs()
    for phases in ((0, 0, 0), (9, 4, 13), (3, 15, 1)):
        check(ctx, a, b, *phases)


@pytest.mark.parametrize('which', [1, 2, 3], ids=['end-of-A0', 'end-of-B0', 'end-of-A1'])
def test_boundaries_around_a_tile_edge(ctx, which):
    seen = set()
    for d in range(-17, 18):
        phase = (d * 7) % 16
        a, b, at = I.edge_pairs(TILE, d, which, phase)
        la, lb = ops.host_line_starts(a), ops.host_line_starts(b)
        boundaries = {1: int(la[4]), 2: int(la[4] + lb[4]), 3: int(la[8] + lb[4])}
        assert boundaries[which] == at
        seen.add(at - (TILE - phase))                                # the first tile ends TILE - phase bytes into the output
        check(ctx, a, b, phase, (d * 3) % 16, (d * 5) % 16)
    assert seen == set(range(-17, 18))


def test_more_than_256_pairs_in_one_tile(ctx):
    a, b = I.many_pairs_in_a_tile()
    la, lb = ops.host_line_starts(a), ops.host_line_starts(b)
    starts = [int(la[4 * r] + lb[4 * r]) for r in range(len(R.records(a)))]
    assert sum(1 for s in starts if s < TILE) > 256
    for phases in ((0, 0, 0), (5, 6, 7)):
        check(ctx, a, b, *phases)


@pytest.mark.parametrize('where', ['first', 'middle', 'last'])
def test_a_record_longer_than_a_tile(ctx, where):
    a, b = I.long_record_pairs(where)
    for phases in ((0, 0, 0), (11, 3, 14)):
        check(ctx, a, b, *phases)


def test_subranges_start_at_byte_zero_and_leave_the_rest(ctx):
    a, b = I.unequal_pairs()
    n = len(R.records(a))
    for first, cnt in ((1, 1), (7, 50), (n - 3, 3), (60, 2)):
        want = check(ctx, a, b, 6, 1, 2, first=first, n=cnt, room=100)
        assert want.startswith(R.records(a)[first])
    # no pairs: nothing happens, whatever the capacity says
    A, B = Source(ctx, a, 1), Source(ctx, b, 2)
    out = Output(ctx, 200, 3)
    ops.interleave_records(ctx, A.buf, A.ls, B.buf, B.ls, 5, 0, out=out.buf)
    ops.interleave_records(ctx, A.buf, A.ls, B.buf, B.ls, n, 0, out=out.buf, out_capacity=0)
    assert out.result() == guarded(b'', 200)


def test_a_capacity_one_byte_short_is_refused(ctx):
    a, b = I.unequal_pairs()
    A, B = Source(ctx, a, 4), Source(ctx, b, 9)
    size = len(a) + len(b)
    assert ops.interleaved_size(ctx, A.ls, B.ls, 0, A.reads) == size
    out = Output(ctx, size, 2)
    with pytest.raises(UqHipError):
        ops.interleave_records(ctx, A.buf, A.ls, B.buf, B.ls, 0, A.reads, out=out.buf, out_capacity=size - 1)
    assert out.result() == guarded(b'', size)
    ops.interleave_records(ctx, A.buf, A.ls, B.buf, B.ls, 0, A.reads, out=out.buf, out_capacity=size)
    assert out.result() == guarded(R.interleave(a, b))


@pytest.mark.parametrize('length', [(36, 301), 150], ids=['36-301bp', '150bp'])
def test_device_against_the_host_twin(ctx, length):
    a = synth.fastq(20261020, 6000, length, n_rate=1)
    b = synth.fastq(20261021, 6000, length)
    want = R.interleave(a, b)
    assert ops.interleave_records_host(a, b).tobytes() == want
    check(ctx, a, b, 13, 5, 10)


# ------------------------------------------------------------------ the mate rule
def device_report(ctx, a, b, first_a=0, step_a=1, first_b=0, step_b=1, npairs=None, base=0, d_rep=None, phases=(3, 9)):
    A = Source(ctx, a, phases[0])
    B = A if b is a else Source(ctx, b, phases[1])
    if npairs is None: npairs = min(len(range(first_a, A.reads, step_a)), len(range(first_b, B.reads, step_b)))
    d_rep = ops.mate_report_new(ctx) if d_rep is None else d_rep
    ops.mate_check(ctx, d_rep, A.buf, A.ls, first_a, step_a, B.buf, B.ls, first_b, step_b, npairs, base)
    return ops.mate_report_fetch(ctx, d_rep)


def both_forms(ctx, a, b, want, base=0):
    """Two buffers, and one interleaved buffer given twice."""
    assert device_report(ctx, a, b, base=base) == want
    both = R.interleave(a, b)
    assert device_report(ctx, both, both, 0, 2, 1, 2, base=base) == want


def test_rule_cases_one_by_one(ctx):
    for x, y, ok, slash in I.RULE_CASES:
        a, b = I.name_pair(x, y)
        want = {'pairs': 1, 'mismatches': 0 if ok else 1, 'first_mismatch': None if ok else 0, 'slash_pairs': int(slash)}
        assert R.check_texts(a, b) == want
        both_forms(ctx, a, b, want)


def test_rule_cases_together(ctx):
    a = I.names_text([c[0] for c in I.RULE_CASES], 31)
    b = I.names_text([c[1] for c in I.RULE_CASES], 32)
    want = R.check_texts(a, b)
    assert want['mismatches'] == sum(1 for c in I.RULE_CASES if not c[2]) and want['slash_pairs'] == sum(1 for c in I.RULE_CASES if c[3])
    assert want['first_mismatch'] == [c[2] for c in I.RULE_CASES].index(False)
    both_forms(ctx, a, b, want)


@pytest.mark.parametrize('bad,first', [({0}, 0), ({299}, 299), ({3, 77}, 3), (set(), None)], ids=['first', 'last', '3-and-77', 'none'])
def test_where_the_mismatch_is(ctx, bad, first):
    a, b = I.mismatch_texts(300, bad)
    want = {'pairs': 300, 'mismatches': len(bad), 'first_mismatch': first, 'slash_pairs': 0}
    assert R.check_texts(a, b) == want
    both_forms(ctx, a, b, want)
    if bad:
        want['first_mismatch'] = first + (1 << 40)
        both_forms(ctx, a, b, want, base=1 << 40)


def test_two_calls_over_halves_sum_to_the_whole(ctx):
    a, b = I.mismatch_texts(300, {3, 77, 200})
    A, B = Source(ctx, a, 1), Source(ctx, b, 2)
    d_rep = ops.mate_report_new(ctx)
    assert ops.mate_report_fetch(ctx, d_rep) == {'pairs': 0, 'mismatches': 0, 'first_mismatch': None, 'slash_pairs': 0}
    ops.mate_check(ctx, d_rep, A.buf, A.ls, 150, 1, B.buf, B.ls, 150, 1, 150, 150)
    assert ops.mate_report_fetch(ctx, d_rep) == {'pairs': 150, 'mismatches': 1, 'first_mismatch': 200, 'slash_pairs': 0}
    ops.mate_check(ctx, d_rep, A.buf, A.ls, 0, 1, B.buf, B.ls, 0, 1, 150, 0)
    ops.mate_check(ctx, d_rep, A.buf, A.ls, 0, 1, B.buf, B.ls, 0, 1, 0, 0)          # no pairs: a no-op
    assert ops.mate_report_fetch(ctx, d_rep) == R.check_texts(a, b) == {'pairs': 300, 'mismatches': 3, 'first_mismatch': 3, 'slash_pairs': 0}


def test_random_pairs_against_the_reference(ctx):
    a, b = I.random_pairs()
    want = R.check_texts(a, b)
    assert 20 <= want['mismatches'] <= 90 and want['slash_pairs'] > 300
    assert ops.mate_check_host(a, b) == want
    both_forms(ctx, a, b, want)


# ------------------------------------------------------------------ offsets beyond 2^31 and 2^32
def test_beyond_4_gib(ctx):
    """~6.5 M x 150 bp made on the device (2.2 GB) as both mates: the sources pass 2^31, the output 2^31 and 2^32.  The output's fingerprint
    sums are twice the source's, its even and odd records are mates, and 1 MiB windows around 2^31, 2^32 and at the end equal the host
    interleave of the matching source windows."""
    t = ctx.torch
    n = 6_500_000
    try:
        src = ops.synth_fastq(ctx, synth.Spec(20261020, 150), 0, n)
        nl = ops.count_lines(ctx, src)
        ls = ops.index_lines(ctx, src, nl)
        out = ctx.empty(2 * src.numel())
    except (RuntimeError, MemoryError) as e:
        if 'out of memory' not in str(e).lower() and 'alloc' not in str(e).lower(): raise
        pytest.skip('no room for 6.6 GB of buffers and their indexes: %s' % e)
    assert nl == 4 * n and src.numel() > (1 << 31) + (1 << 20) and out.numel() > (1 << 32) + (1 << 20)
    before = ops.fingerprint(ctx, src, ls, n)
    ops.interleave_records(ctx, src, ls, src, ls, 0, n, out=out)
    assert ops.count_lines(ctx, out) == 8 * n
    ols = ops.index_lines(ctx, out, 8 * n)
    after = ops.fingerprint(ctx, out, ols, 2 * n)
    for k in ('reads', 'bases', 'qname', 'dna', 'qual', 'records'): assert after[k] == (2 * before[k]) % (1 << 64), k
    d_rep = ops.mate_report_new(ctx)
    ops.mate_check(ctx, d_rep, out, ols, 0, 2, out, ols, 1, 2, n)
    assert ops.mate_report_fetch(ctx, d_rep) == {'pairs': n, 'mismatches': 0, 'first_mismatch': None, 'slash_pairs': 0}
    rec_starts = ols[0:8 * n + 1:8].contiguous()                     # where the pairs begin in the output
    for centre in (1 << 31, 1 << 32, out.numel() - (1 << 19)):
        p0 = int(t.searchsorted(rec_starts, t.tensor([centre - (1 << 19)], dtype=t.int64, device=ctx.device))[0])
        p1 = min(int(t.searchsorted(rec_starts, t.tensor([centre + (1 << 19)], dtype=t.int64, device=ctx.device))[0]), n)
        o0, o1 = int(rec_starts[p0]), int(rec_starts[p1])
        s0, s1 = int(ls[4 * p0]), int(ls[4 * p1])
        assert o1 - o0 > (1 << 20) - 2000 and o1 - o0 == 2 * (s1 - s0) and (centre >= out.numel() - (1 << 19) or o0 < centre < o1)
        window = ctx.to_numpy(src[s0:s1]).tobytes()
        assert ctx.to_numpy(out[o0:o1]).tobytes() == ops.interleave_records_host(window, window).tobytes(), centre
        if centre > out.numel() - (1 << 20): assert o1 == out.numel()
