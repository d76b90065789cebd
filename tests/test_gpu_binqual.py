"""GPU: uq_requantise_qualities against the numpy reference (tests/binqual_ref.py).  Every test compares the WHOLE device buffer, with 64
guard bytes on either side, and the device counter of changed bytes.

The kernel (csrc/requant.hip) lists the 16-byte-aligned vectors that hold a byte of a quality line, per group of 256 records, and works the
list off in tiles of TILE = RQ_TILE bytes (1 024 vectors); a vector is stored whole, dword by dword or byte by byte, by what its line owns
of it.  The inputs below are built from that: quality lines 6 to 10 bytes apart at every buffer phase, line ends and line starts at every
byte from -17 to +17 around a tile's edge, a 70 000-base read between short ones, a line longer than a tile first and last."""
import os
import random
import re

import numpy as np
import pytest

import binqual_ref as R
from uq_amd import binqual, ops, synth

pytestmark = pytest.mark.gpu

TILE = 16384
GUARD = 64
FILL = 0xA5
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ILLUMINA8 = binqual.parse('illumina8')


def text_of(records):
    return b''.join(b'\n'.join(r) + b'\n' for r in records)


def line(rnd, L, alphabet=None):
    if alphabet: return bytes(rnd.choice(alphabet) for _ in range(L))
    return bytes(rnd.randrange(33, 127) for _ in range(L))


def read(rnd, name, L):
    return (name, line(rnd, L, b'ACGTN'), b'+', line(rnd, L))


class OnDevice:
    """The text in HBM at an address `phase` bytes past a 16-byte boundary, between two guards of 64 bytes; its record index from the host."""

    def __init__(self, ctx, text, phase=0):
        t = ctx.torch
        self.ctx, self.n = ctx, len(text)
        self.whole = t.full((len(text) + 2 * GUARD + 32,), FILL, dtype=t.uint8, device=ctx.device)
        start = GUARD + (phase - self.whole.data_ptr() - GUARD) % 16
        self.region = self.whole[start - GUARD:start + len(text) + GUARD]
        self.buf = self.whole[start:start + len(text)]
        if len(text): self.buf.copy_(ctx.to_device(np.frombuffer(text, dtype=np.uint8)))
        assert self.buf.data_ptr() % 16 == phase % 16
        self.ls = ctx.to_device(ops.host_line_starts(text).view(np.int64))
        self.reads = (self.ls.numel() - 1) // 4
        self.changed = ops.changed_new(ctx)

    def apply(self, lut, first=0, n=None):
        ops.requantise_qualities(self.ctx, self.buf, self.ls, first, self.reads - first if n is None else n, lut, self.changed)

    def result(self):
        return self.ctx.to_numpy(self.region).tobytes(), int(self.ctx.to_numpy(self.changed).view(np.uint64)[0])


def guarded(text):
    return bytes([FILL]) * GUARD + text + bytes([FILL]) * GUARD


def check(ctx, text, lut, phase=0):
    d = OnDevice(ctx, text, phase)
    d.apply(lut)
    want, changed = R.apply(text, lut)
    got, cnt = d.result()
    assert got == guarded(want)
    assert cnt == changed
    return changed


def test_the_tile_size_is_the_kernels():
    src = open(os.path.join(REPO, 'uq_amd', 'csrc', 'requant.hip')).read()
    threads = int(re.search(r'RQ_THREADS = (\d+);', src).group(1))
    unroll = int(re.search(r'RQ_UNROLL = (\d+);', src).group(1))
    assert re.search(r'RQ_TILE = RQ_THREADS \* RQ_UNROLL \* 16;', src)
    assert threads * unroll * 16 == TILE


def close_lines_text():
    """Quality (= sequence) lengths 0..33 under names of 1 to 3 characters: with 0 and 1 bases the quality lines sit 6 to 10 bytes apart."""
    rnd = random.Random(21)
    recs = []
    for k in (1, 2, 3):
        name = b'@ab'[:k]
        recs += [read(rnd, name, L) for L in (0, 1, 1, 0, 0, 1, 1, 1, 0, 1) * 4]
        recs += [read(rnd, name, L) for L in range(34)]
        recs += [read(rnd, name, 1) for _ in range(40)]
    return text_of(recs)


CLOSE = close_lines_text()


@pytest.mark.parametrize('phase', range(16))
def test_lengths_and_alignment(ctx, phase):
    """Where an edge handled wider than the line owns, or a write outside line 4, shows: every other byte is a neighbour's."""
    starts = ops.host_line_starts(CLOSE)
    gaps = {int(starts[4 * i + 7] - starts[4 * i + 3]) for i in range(len(starts) // 4 - 1)}
    assert {6, 7, 8, 9, 10} <= gaps
    assert check(ctx, CLOSE, R.ALL_I, phase) > 0
    assert check(ctx, CLOSE, ILLUMINA8, phase) > 0


def edge_text(rnd, d, phase, gap):
    """A first record whose quality line ends (gap 0) -- or whose successor's quality line starts (gap 8: '\\n@b\\nC\\n+\\n') -- d bytes
    behind the edge of the group's first tile: the tile's vectors are counted from the aligned vector that holds the line's first byte."""
    for namelen in (1, 2, 3, 4):
        for L in range(TILE + d - gap - 15, TILE + d - gap + 1):
            p = (phase + namelen + 1 + L + 1 + 2) % 16                      # the quality line's first byte within its vector
            if p + L + gap == TILE + d:
                recs = [read(rnd, b'@abc'[:namelen], L)] + [read(rnd, b'@b', 1) for _ in range(30)] + [read(rnd, b'@r%d' % i, 20 + i) for i in range(20)]
                return text_of(recs), p
    raise AssertionError('no such record')


@pytest.mark.parametrize('gap', [0, 8], ids=['line-ends', 'line-starts'])
def test_lines_around_a_tile_edge(ctx, gap):
    rnd = random.Random(22)
    seen = set()
    for d in range(-17, 18):
        phase = (d * 7) % 16
        text, p = edge_text(rnd, d, phase, gap)
        starts = ops.host_line_starts(text)
        first_vector = int(starts[3]) - p
        at = int(starts[4] - 1) if gap == 0 else int(starts[7])             # the line's end / the next line's first byte
        seen.add(at - first_vector - TILE)
        check(ctx, text, R.ALL_I, phase)
        check(ctx, text, ILLUMINA8, phase)
    assert seen == set(range(-17, 18))


def test_long_lines_first_last_and_between(ctx):
    rnd = random.Random(23)
    recs = [read(rnd, b'@first', TILE + 100)] + [read(rnd, b'@s%d' % i, 3 + i % 40) for i in range(300)]
    recs += [read(rnd, b'@long', 70000)] + [read(rnd, b'@t%d' % i, 1 + i % 50) for i in range(300)] + [read(rnd, b'@last', 2 * TILE + 37)]
    text = text_of(recs)
    for phase in (0, 5, 15):
        check(ctx, text, R.ALL_I, phase)
        check(ctx, text, ILLUMINA8, phase)


def test_pieces(ctx):
    rnd = random.Random(24)
    recs = [read(rnd, b'@p%d' % i, rnd.choice((0, 1, 2, 17, 36, 150, 301))) for i in range(700)]
    text = text_of(recs)
    n = len(recs)
    whole, changed = R.apply(text, ILLUMINA8)
    # two calls over halves = one call; the counter accumulates
    d = OnDevice(ctx, text, 3)
    d.apply(ILLUMINA8, 0, n // 2)
    half, c_half = R.apply(text, ILLUMINA8, 0, n // 2)
    assert d.result() == (guarded(half), c_half)
    d.apply(ILLUMINA8, n // 2, n - n // 2)
    assert d.result() == (guarded(whole), changed)
    # a subrange leaves the other records alone
    for first, cnt in ((0, 1), (255, 2), (256, 256), (n - 1, 1), (100, 313)):
        d = OnDevice(ctx, text, 9)
        d.apply(R.ALL_I, first, cnt)
        want, c = R.apply(text, R.ALL_I, first, cnt)
        assert d.result() == (guarded(want), c), (first, cnt)
    # no reads: nothing happens, with and without a counter
    d = OnDevice(ctx, text, 1)
    d.apply(R.ALL_I, 5, 0)
    d.apply(R.ALL_I, n, 0)
    ops.requantise_qualities(ctx, d.buf, d.ls, 0, 0, R.ALL_I, None)
    assert d.result() == (guarded(text), 0)
    # without a counter the text is the same
    d = OnDevice(ctx, text, 1)
    ops.requantise_qualities(ctx, d.buf, d.ls, 0, n, ILLUMINA8, None)
    assert d.result() == (guarded(whole), 0)
    # the identity changes nothing; a second pass of the bins changes nothing more
    d = OnDevice(ctx, text, 0)
    d.apply(R.IDENTITY)
    assert d.result() == (guarded(text), 0)
    d.apply(ILLUMINA8); d.apply(ILLUMINA8)
    assert d.result() == (guarded(whole), changed)


def test_a_table_with_a_newline_is_refused(ctx):
    from uq_amd._lib import UqHipError
    d = OnDevice(ctx, b'@a\nA\n+\nI\n')
    bad = bytearray(range(256)); bad[ord('I')] = 10
    with pytest.raises(UqHipError):
        d.apply(bytes(bad))
    assert d.result() == (guarded(b'@a\nA\n+\nI\n'), 0)


@pytest.mark.parametrize('length', [(36, 301), 150], ids=['36-301bp', '150bp'])
def test_device_against_the_host_twin(ctx, length):
    text = synth.fastq(20261019, 20000, length, n_rate=1)
    d = OnDevice(ctx, text, 11)
    d.apply(ILLUMINA8)
    twin, c = ops.requantise_qualities_host(text, ILLUMINA8)
    want, changed = R.apply(text, ILLUMINA8)
    assert twin.tobytes() == want and c == changed and changed > 0
    assert d.result() == (guarded(want), changed)


def test_beyond_4_gib(ctx):
    """~13.5 M x 150 bp made on the device (4.6 GB): offsets pass 2^31 and 2^32.  Windows of whole records around both, and at the end of the
    buffer, against the reference on the same windows taken before the call; the sums of the lines that binning leaves alone stay."""
    t = ctx.torch
    n = 13_500_000
    try:
        buf = ops.synth_fastq(ctx, synth.Spec(20261019, 150), 0, n)
        nl = ops.count_lines(ctx, buf)
        ls = ops.index_lines(ctx, buf, nl)
    except (RuntimeError, MemoryError) as e:
        if 'out of memory' not in str(e).lower() and 'alloc' not in str(e).lower(): raise
        pytest.skip('no room for a 4.6 GB buffer and its index: %s' % e)
    assert nl == 4 * n and buf.numel() > (1 << 32) + (1 << 20)
    rec_starts = ls[0:nl + 1:4].contiguous()
    windows = []
    for centre in (1 << 31, 1 << 32, buf.numel() - (1 << 19)):
        r0 = int(t.searchsorted(rec_starts, t.tensor([centre - (1 << 19)], dtype=t.int64, device=ctx.device))[0])
        r1 = min(int(t.searchsorted(rec_starts, t.tensor([centre + (1 << 19)], dtype=t.int64, device=ctx.device))[0]), n)
        a, b = int(rec_starts[r0]), int(rec_starts[r1])
        assert b - a > (1 << 20) - 1000 and (centre >= buf.numel() - (1 << 19) or a < centre < b)
        windows.append((a, b, ctx.to_numpy(buf[a:b]).tobytes()))
    assert windows[-1][1] == buf.numel()
    before = ops.fingerprint(ctx, buf, ls, n)
    changed = ops.changed_new(ctx)
    ops.requantise_qualities(ctx, buf, ls, 0, n, ILLUMINA8, changed)
    after = ops.fingerprint(ctx, buf, ls, n)
    for k in ('reads', 'bases', 'qname', 'dna'): assert after[k] == before[k], k
    assert after['qual'] != before['qual']
    inside = 0
    for a, b, old in windows:
        want, c = R.apply(old, ILLUMINA8)
        assert ctx.to_numpy(buf[a:b]).tobytes() == want, a
        assert c > 0
        inside += c
    total = int(ctx.to_numpy(changed).view(np.uint64)[0])
    assert inside < total <= 150 * n
    # the bins are idempotent: a second pass over everything changes nothing, so every byte was binned the first time
    ops.requantise_qualities(ctx, buf, ls, 0, n, ILLUMINA8, changed)
    assert int(ctx.to_numpy(changed).view(np.uint64)[0]) == total
    assert ops.fingerprint(ctx, buf, ls, n) == after
