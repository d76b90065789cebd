"""GPU: uq_qc_accumulate against the numpy statement of the per-cycle tables (tests/qc_ref.py), exactly, on every word.

The kernel (csrc/qc.hip) counts the exact cycles below QC_LDS_CYCLES in a table in LDS and the others straight in the object; the tail row
(positions >= cycles) lies inside that table's range, at its edge or beyond it depending on the cycles asked for.  It stages the stream in
tiles of QC_TILE bytes and deals 64 consecutive positions of a line to a wave.  The inputs below are built from those numbers: read lengths
around the wave, the table's edge and the largest cycle count, one 70 000-base read between short ones, a line longer than a tile at either
end of the buffer, buffers misaligned by 1, 3 and 7 bytes that end with the text."""
import os
import random
import re

import numpy as np
import pytest

import qc_ref as Q
from uq_amd import ops

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(REPO, 'uq_amd', 'csrc', 'qc.hip')).read()
LDS_CYCLES = int(re.search(r'QC_LDS_CYCLES = (\d+);', SRC).group(1))
TILE = int(re.search(r'QC_TILE = (\d+);', SRC).group(1))
BASES = b'ACGTACGTACGTNacgtnRY.'
QUALS = bytes(range(33, 127)) + b' \t\x7f\x80\xff'


def text_of(records):
    return b''.join(b'\n'.join(r) + b'\n' for r in records)


def line(rnd, L, alphabet):
    return bytes(rnd.choices(alphabet, k=L))


def record(rnd, i, Ls, Lu=None):
    return (b'@r:%d' % i, line(rnd, Ls, BASES), b'+', line(rnd, Ls if Lu is None else Lu, QUALS))


def on_device(ctx, text, mis=0):
    """(the text as a device tensor whose address is `mis` bytes past a 16-byte boundary and whose last byte is the last byte of its
    allocation, its record index built on the host)"""
    a = np.frombuffer(text, dtype=np.uint8)
    whole = ctx.torch.zeros(len(a) + mis, dtype=ctx.torch.uint8, device=ctx.device)
    assert whole.data_ptr() % 16 == 0
    buf = whole[mis:]
    buf.copy_(ctx.to_device(a))
    assert buf.data_ptr() % 16 == mis % 16 and buf.numel() == len(a)
    ls = ctx.to_device(ops.host_line_starts(text).view(np.int64))
    return buf, ls


def device_qc(ctx, text, cycles=1024, pieces=None, mis=0):
    buf, ls = on_device(ctx, text, mis)
    n = (ls.numel() - 1) // 4
    d = ops.qc_new(ctx, cycles)
    for first, cnt in (pieces if pieces is not None else [(0, n)]):
        ops.qc_accumulate(ctx, d, buf, ls, first, cnt, cycles)
    return ops.qc_fetch(ctx, d)


def same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint64
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, '%d words differ, the first is word %d: %d != %d' % (len(bad), bad[0], got[bad[0]], want[bad[0]])


def test_the_table_size_is_the_kernels():
    assert LDS_CYCLES >= 301 and LDS_CYCLES < 1024 and TILE >= 4096


def test_the_hand_example(ctx):
    from test_qc_cpu import HAND
    for cycles in (3, 1024, 1):
        same(device_qc(ctx, HAND, cycles), Q.qc(HAND, cycles))
    f = Q.fields(device_qc(ctx, HAND, 3))
    assert f['base_by_cycle'].tolist() == [[1, 0, 1, 0, 0, 0], [0, 1, 1, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 1, 0]]


def test_every_length_from_0_to_17(ctx):
    rnd = random.Random(31)
    for L in range(18):
        one = text_of([record(rnd, L, L, (L * 5) % 18)])
        same(device_qc(ctx, one, 1024), Q.qc(one, 1024))
        same(device_qc(ctx, one, 8), Q.qc(one, 8))
    recs = [record(rnd, i, i % 18, (i // 18) % 18) for i in range(18 * 18)]
    text = text_of(recs)
    same(device_qc(ctx, text, 1024), Q.qc(text, 1024))


@pytest.mark.parametrize('mis', [1, 3, 7])
def test_misaligned_buffer_that_ends_with_the_text(ctx, mis):
    """The buffer starts 1, 3 or 7 bytes past a 16-byte boundary and its allocation ends with the text: the first tile begins before the
    buffer, the last vector reaches beyond it, and nothing outside the text's vectors may be read."""
    rnd = random.Random(mis)
    recs = [record(rnd, i, rnd.randint(0, 60), rnd.randint(0, 60) if i % 5 == 0 else None) for i in range(300)]
    text = text_of(recs)
    same(device_qc(ctx, text, 1024, mis=mis), Q.qc(text, 1024))
    same(device_qc(ctx, text, 16, mis=mis, pieces=[(0, 111), (111, 189)]), Q.qc(text, 16))


EDGE_LENGTHS = [63, 64, 65, 255, 256, 257] + list(range(LDS_CYCLES - 2, LDS_CYCLES + 3)) + [1023, 1024, 1025, 5000]
_EDGE = {}


def edge_text():
    if not _EDGE:
        rnd = random.Random(32)
        _EDGE['text'] = text_of([record(rnd, i, L, L + 1 if i % 4 == 3 else None) for i, L in enumerate(EDGE_LENGTHS)])
        _EDGE['want'] = {c: Q.qc(_EDGE['text'], c) for c in (1024, LDS_CYCLES, 4)}
    return _EDGE['text'], _EDGE['want']


@pytest.mark.parametrize('cycles', [1024, LDS_CYCLES, 4], ids=['tail-beyond-the-table', 'tail-at-its-edge', 'tail-inside'])
def test_lengths_around_the_wave_and_the_table_edge(ctx, cycles):
    text, want = edge_text()
    same(device_qc(ctx, text, cycles), want[cycles])
    # record by record (each call sizes its groups from its own record), added up in one object
    same(device_qc(ctx, text, cycles, pieces=[(i, 1) for i in range(len(EDGE_LENGTHS))]), want[cycles])
    f = Q.fields(want[cycles])
    assert int(f['length_hist'][cycles]) == sum(L >= cycles for L in EDGE_LENGTHS) and int(f['base_by_cycle'][cycles].sum()) == sum(max(L - cycles, 0) for L in EDGE_LENGTHS)


def test_long_read_between_short_ones(ctx):
    rnd = random.Random(33)
    recs = [record(rnd, i, 100 + i % 50) for i in range(40)]
    recs.insert(20, record(rnd, 99, 70000))
    text = text_of(recs)
    for cycles in (1024, 150):
        same(device_qc(ctx, text, cycles), Q.qc(text, cycles))


def test_long_lines_first_and_last_in_the_buffer(ctx):
    rnd = random.Random(34)
    recs = [(b'@' + line(rnd, TILE + 100, QUALS[:94]), b'ACGT', b'+', b'IIII')] + [record(rnd, i, 100 + i) for i in range(5)]
    recs += [(b'@end', b'AC', b'+', line(rnd, TILE + 100, QUALS))]
    text = text_of(recs)
    want = Q.qc(text, 1024)
    for mis in (0, 5):
        same(device_qc(ctx, text, 1024, mis=mis), want)
    recs = [record(rnd, 0, 2 * TILE + 7)] + recs + [record(rnd, 1, TILE + 1, 3)]
    text = text_of(recs)
    same(device_qc(ctx, text, LDS_CYCLES + 5, mis=3), Q.qc(text, LDS_CYCLES + 5))


def test_identical_records_hit_the_same_cells(ctx):
    """20 000 copies of one 150 bp record: every read adds to the same 300 cells of every workgroup's table, and every workgroup walks
    over several groups.  Two calls into one object: the second flush adds to counters that are no longer zero."""
    rnd = random.Random(35)
    one = text_of([record(rnd, 7, 150)])
    text = one * 20000
    want = Q.qc(text, 1024)
    same(device_qc(ctx, text, 1024), want)
    same(device_qc(ctx, text, 1024, pieces=[(0, 20000), (0, 20000)]), 2 * want)
    same(device_qc(ctx, text, 100, pieces=[(0, 12345), (12345, 7655)]), Q.qc(text, 100))


def test_pieces_add_and_a_slice_is_that_slice(ctx):
    rnd = random.Random(36)
    recs = [record(rnd, i, rnd.randint(1, 330), None if i % 7 else rnd.randint(0, 330)) for i in range(2000)]
    text = text_of(recs)
    want = Q.qc(text, 1024)
    cuts = [0, 1, 2, 65, 700, 701, 1999, 2000]
    pieces = [(a, b - a) for a, b in zip(cuts, cuts[1:])]
    rnd.shuffle(pieces)
    same(device_qc(ctx, text, 1024, pieces=pieces), want)
    same(device_qc(ctx, text, 1024), want)
    same(device_qc(ctx, text, 1024, pieces=[(700, 600)]), Q.qc(text, 1024, 700, 600))
    same(device_qc(ctx, text, 200, pieces=[(1999, 1)]), Q.qc(text, 200, 1999, 1))
    same(ops.qc(ctx, on_device(ctx, text)[0], ncycles=77), Q.qc(text, 77))       # the index built on the device


def test_no_reads_leave_the_object_untouched(ctx):
    from test_qc_cpu import HAND
    buf, ls = on_device(ctx, HAND)
    d = ops.qc_new(ctx, 16)
    d.copy_(ctx.torch.arange(d.numel(), dtype=ctx.torch.int64, device=ctx.device) * 3 + 1)
    before = ops.qc_fetch(ctx, d)
    ops.qc_accumulate(ctx, d, buf, ls, 1, 0, 16)
    same(ops.qc_fetch(ctx, d), before)
    with pytest.raises(Exception): ops.qc_accumulate(ctx, d, buf, ls, 0, 2, 17)          # an object of another size
    with pytest.raises(Exception): ops.call('uq_qc_accumulate', ctx.h, ops._p(buf), ops._p(ls), 0, 2, 0, ops._p(d))
    with pytest.raises(Exception): ops.call('uq_qc_init', ctx.h, ops._p(d), 1025)
    same(ops.qc_fetch(ctx, d), before)
