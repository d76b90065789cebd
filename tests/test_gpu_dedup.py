"""GPU: uq_dedup_keys and uq_dedup_mark against their host twins (which tests/test_dedup_cpu.py holds to the pure-Python definition,
tests/dedup_ref.py): key rows, verdicts and reports are equal exactly.  The key rows and the verdicts are each compared as a whole buffer
between two guards of 64 bytes; the text is placed at chosen 16-byte phases.  Before anything is compared, every input used with the full hash
is shown to have no collision at seed 0 under the Python reference, and every forced-collision case to have some: an exact case cannot pass
by being retried."""
import numpy as np
import pytest

import dedup_inputs as I
import dedup_ref as R
from uq_amd import ops

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5


class Source:
    """A text in HBM at an address `phase` bytes past a 16-byte boundary, and its record index; the allocation ends with the text."""

    def __init__(self, ctx, text, phase=0):
        t = ctx.torch
        self.whole = t.full((len(text) + 16 + phase % 16,), FILL, dtype=t.uint8, device=ctx.device)
        start = (phase - self.whole.data_ptr()) % 16
        self.buf = self.whole[start:start + len(text)]
        if len(text): self.buf.copy_(ctx.to_device(np.frombuffer(text, dtype=np.uint8)))
        assert self.buf.data_ptr() % 16 == phase % 16 and self.buf.numel() == len(text)
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
        assert self.buf.data_ptr() % 16 == phase % 16

    def result(self):
        return self.ctx.to_numpy(self.region).tobytes()


def guarded(payload):
    return bytes([FILL]) * GUARD + payload + bytes([FILL]) * GUARD


def host(text, p, first, n, base):
    ls = ops.host_line_starts(text)
    keys, rep = ops.dedup_keys_host(text, p, ls, first, n, base)
    v, rep = ops.dedup_mark_host(text, p, keys, ops.dedup_order_host(keys), ls, first, n, base, rep)
    return keys, v, rep


_NO_COLLISION = {}


def check(ctx, text, unit=1, prefix=0, best=False, seed=0, hash_bits=64, phase=0, first=0, n=None, base=0, collide=None):
    """Device keys, verdicts and report against the twins'; -> the report."""
    if hash_bits == 64 and seed == 0:                            # the condition on the inputs, on the CPU, before anything is compared
        k = (hash(text), unit, prefix, first, n)
        if k not in _NO_COLLISION: _NO_COLLISION[k] = R.rule(text, unit, prefix, False, 0, 64, first, n, base)[2]['collisions']
        assert _NO_COLLISION[k] == 0
    if collide: assert R.rule(text, unit, prefix, best, seed, hash_bits, first, n, base)[2]['collisions'] > 0
    S = Source(ctx, text, phase)
    n = S.reads - first if n is None else n
    p = ops.dedup_params(unit=unit, prefix=prefix, hash_bits=hash_bits, flags=ops.DEDUP_BEST if best else 0, seed=seed)
    want_keys, want_v, want_rep = host(text, p, first, n, base)
    units = n // unit
    KEYS, V = Output(ctx, 16 * units, 0), Output(ctx, n, 5)
    d_rep = ops.dedup_report_new(ctx)
    ops.dedup_keys(ctx, d_rep, S.buf, S.ls, first, n, p, base, keys=KEYS.buf)
    assert KEYS.result() == guarded(want_keys.tobytes())
    perm = ops.argsort_rows(ctx, KEYS.buf, units, 16)
    assert ctx.to_numpy(perm).view(np.uint32).tolist() == ops.dedup_order_host(want_keys).tolist()
    ops.dedup_mark(ctx, d_rep, S.buf, S.ls, first, n, p, KEYS.buf, perm, base, verdict=V.buf)
    assert V.result() == guarded(want_v.tobytes())
    assert KEYS.result() == guarded(want_keys.tobytes())          # (mark reads the keys only)
    rep = ops.dedup_report_fetch(ctx, d_rep)
    assert rep == want_rep
    if collide is not None: assert (rep['collisions'] > 0) == collide
    return rep, want_v


@pytest.mark.parametrize('name,text', list(I.hand_inputs()), ids=[n for n, _ in I.hand_inputs()])
def test_hand_inputs(ctx, name, text):
    nrec = len(R.records(text))
    for unit in (1, 2):
        if nrec % unit: continue
        for prefix, best in ((0, False), (0, True), (9, False), (8, True), (1000, False)):
            check(ctx, text, unit, prefix, best, phase=prefix % 16 + 1)
        check(ctx, text, unit, seed=1, phase=3)


def test_edge_lengths_and_near_misses_by_hand(ctx):
    text = I.near_misses()
    seqs = [r[1] for r in R.records(text)]
    _, v = check(ctx, text, phase=7)
    assert v.tolist() == [1 if s in seqs[:i] else 0 for i, s in enumerate(seqs)]
    text = I.edge_lengths()
    seqs = [r[1] for r in R.records(text)]
    rep, v = check(ctx, text, phase=9)
    assert v.tolist() == [1 if s in seqs[:i] else 0 for i, s in enumerate(seqs)] and rep['classes'] == len(set(seqs))


@pytest.mark.parametrize('phase', range(16))
def test_every_text_phase(ctx, phase):
    check(ctx, I.edge_lengths(), phase=phase, best=bool(phase & 1))
    check(ctx, I.counted(129, unit=2), unit=2, phase=phase)


def test_spread_duplicates(ctx):
    text = I.spread(20000)
    for unit, best in ((1, False), (1, True), (2, False), (2, True)):
        rep, _ = check(ctx, text, unit, best=best, phase=unit + 2 * best)
        assert rep['units_in'] == 20000 // unit
    rep, _ = check(ctx, text, phase=11)
    assert 1500 < rep['dup_units'] < 2500                        # about 10 % duplicates: in the same tile, the neighbouring one, anywhere
    check(ctx, text, prefix=40, phase=4)


def test_one_class_of_1000_copies(ctx):
    rep, _ = check(ctx, I.one_class(1000), phase=2)
    assert rep['dup_units'] == 999
    check(ctx, I.one_class(1000), best=True, phase=2)


def test_pairs(ctx):
    rep, v = check(ctx, I.pairs(), unit=2, phase=6)
    assert v.tolist() == [0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 1]


def test_tiles_beyond_the_stage(ctx):
    text = I.long_run()
    for unit, best in ((1, False), (1, True), (2, False), (2, True)):
        rep, _ = check(ctx, text, unit, best=best, phase=13)
    assert check(ctx, text, phase=1)[0]['dup_units'] >= 28


def test_a_line_of_70000_bases(ctx):
    for copies in (1, 2):
        for best in (False, True):
            rep, _ = check(ctx, I.huge_line(copies), best=best, phase=3 + copies)
            assert rep['dup_units'] == copies - 1 and rep['dup_bases'] == 70000 * (copies - 1)
    text = I.huge_line(2)
    check(ctx, text + text, unit=2, phase=8)
    check(ctx, I.huge_line(2), prefix=5000, phase=8)             # beyond the half-wave threshold by its prefix alone


def test_score_ties(ctx):
    _, v = check(ctx, I.score_ties(), best=True, phase=10)
    assert v.tolist() == [1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 1]


def test_first_read_and_base(ctx):
    text = I.spread(3000)
    for unit in (1, 2):
        check(ctx, text, unit, first=1000, n=500, base=1000, phase=5)
        check(ctx, text, unit, best=True, first=10, n=130, base=0, phase=5)
        check(ctx, text, unit, first=2998, n=2, base=(1 << 32) * unit - 2, phase=5)


def test_forced_collisions(ctx):
    for text in (I.counted(129), I.spread(3000), I.edge_lengths()):
        check(ctx, text, hash_bits=2, collide=True, phase=12)
        check(ctx, text, hash_bits=2, best=True, seed=1, collide=True, phase=12)
    check(ctx, I.counted(64, unit=2), unit=2, hash_bits=2, collide=True)
    check(ctx, I.spread(3000), hash_bits=1, collide=True)
    check(ctx, I.spread(3000), hash_bits=64, collide=False)


def test_plan_and_compaction_give_the_deduplicated_text(ctx):
    for text, unit, prefix, best in ((I.spread(20000), 1, 0, False), (I.spread(20000), 2, 0, True), (I.long_run(), 1, 30, False), (I.pairs(), 2, 0, False)):
        S = Source(ctx, text, 3)
        p = ops.dedup_params(unit=unit, prefix=prefix, flags=ops.DEDUP_BEST if best else 0)
        d_rep = ops.dedup_report_new(ctx)
        keys = ops.dedup_keys(ctx, d_rep, S.buf, S.ls, 0, S.reads, p)
        perm = ops.argsort_rows(ctx, keys, S.reads // unit, 16)
        verdict = ops.dedup_mark(ctx, d_rep, S.buf, S.ls, 0, S.reads, p, keys, perm)
        assert ops.dedup_report_fetch(ctx, d_rep)['collisions'] == 0
        src, dst, kept, size = ops.filter_plan(ctx, ops.filter_report_new(ctx), S.ls, 0, S.reads, unit, verdict)
        out = ops.compact_records(ctx, S.buf, src, dst, kept, out_bytes=size)
        assert ctx.to_numpy(out).tobytes() == R.deduped(text, unit, prefix, best)
