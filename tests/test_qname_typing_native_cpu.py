"""CPU: the QNAME column typing that moved into the library (uq_qname_fused_columns, csrc/decide.hip) against the Python rules
analyse_fused applied before (qname_device.fused_columns_py): hand-built uq_qname_fused structures at every edge of the rules -- the
`distinct > T // 10` rule at, one below and one above the limit at every checkpoint, value ranges on both sides of every dtype, the
offset, and every way to decline or to ask for the sort.  The native answer must be the Python one, field for field."""
import itertools

import pytest

from uq_amd import qname_device as Q
from uq_amd._lib import QnameFused

N_BIG = 5_000_000            # checkpoints 10 000 ... 2 560 000 and the last read; those below 2^21 are the head
U32 = 2 ** 32 - 1


def fused(n, cols, **over):
    """A structure as a clean fused pass over n reads leaves it; cols = [(vmin, vmax, counts per checkpoint or a callable T -> count, undetermined)]."""
    r = QnameFused()
    r.ok = 1; r.plen = 2; r.slen = 0; r.nsep = len(cols) - 1; r.l1len = 8; r.nreads = n
    line = b'@r1:2:3x'
    for i, b in enumerate(line): r.line1[i] = b
    for i in range(len(cols) - 1): r.seps[i] = ord(':')
    ths = Q._thresholds(n) if n else []
    r.nth = len(ths)
    for k, T in enumerate(ths): r.thresholds[k] = T
    for c, (vmin, vmax, counts, und) in enumerate(cols):
        r.vmin[c] = vmin; r.vmax[c] = vmax; r.undetermined[c] = und
        for k, T in enumerate(ths):
            r.counts[c][k] = counts(T) if callable(counts) else counts[k] if k < len(counts) else 0
    for k, v in over.items(): setattr(r, k, v)
    return r


def same(r, n):
    want = Q.fused_columns_py(r, n)
    got = Q.fused_columns(r, n)
    assert got == want
    if isinstance(want, list):
        assert [list(c.items()) for c in got] == [list(c.items()) for c in want]        # key order too: the layout is written as JSON
        assert [[type(v) for v in c.values()] for c in got] == [[type(v) for v in c.values()] for c in want]
    return want


@pytest.mark.parametrize('n', [1, 2, 9999, 10000, 10001, 10002, 20001, 40001, 50000, (1 << 21), (1 << 21) + 1, (1 << 21) + 2, N_BIG])
def test_checkpoint_rule_at_every_checkpoint(n):
    ths = Q._thresholds(n)
    for k, delta in itertools.product(range(len(ths)), (-1, 0, 1)):
        counts = [0] * len(ths)
        counts[k] = max(ths[k] // 10 + delta, 0)
        counts[-1] = max(counts[-1], 3)
        for vmin, vmax in ((0, 4095), (0, 4096), (7, 7), (1000, 1 << 20), (0, U32)):
            res = same(fused(n, [(vmin, vmax, counts, 0), (1, 4, [2] * len(ths), 0)]), n)
            small = vmax - vmin + 1 <= Q.INT_RANGE_SMALL
            fires = counts[k] > ths[k] // 10 and (small or ths[k] < Q.INT_PREFIX)
            if small or fires or all(T < Q.INT_PREFIX for T in ths):
                assert res != Q.NEEDS_SORT
            else:
                assert res == Q.NEEDS_SORT
            if fires:
                assert res[0]['format'] == 'integers' and list(res[0])[2] == 'min'      # demoted by the rule: min, max, dtype by the range


@pytest.mark.parametrize('n', [100, 50000, N_BIG])
@pytest.mark.parametrize('span', [0, 1, 254, 255, 256, 65534, 65535, 65536, U32 - 1, U32])
def test_ranges_at_every_dtype_edge(n, span):
    ths = Q._thresholds(n)
    always = lambda T: T                                       # more distinct values than T // 10 at the first checkpoint: `integers`
    for vmin in (0, 1, 300, U32 - span):
        vmax = vmin + span
        if vmax > U32: continue
        res = same(fused(n, [(vmin, vmax, always, 0)]), n)
        assert res[0]['dtype'] == Q._ladder(span)[1] and res[0]['offset'] == (vmax > Q._ladder(span)[0])
    # a column that stays a mapping through every checkpoint: the dtype follows the distinct count, the range must fit it
    for nu in (1, 255, 256, 65535, 65536):
        if nu > ths[0] // 10 or span + 1 > Q.INT_RANGE_SMALL: continue
        res = same(fused(n, [(5, 5 + span, [min(nu, T // 10) for T in ths[:-1]] + [nu], 0)]), n)
        lim = Q._ladder(nu)[0]
        assert res == Q.DECLINE if span > lim else (res[0]['dtype'] == Q._ladder(nu)[1] and list(res[0])[2] == 'dtype')


def test_mapping_that_stays_a_mapping_declines_and_offset_follows_vmax():
    n = 200000
    ths = Q._thresholds(n)
    quiet = [min(200, T // 10) for T in ths]                   # never fires; 200 distinct values: uint8
    assert same(fused(n, [(0, 255, quiet, 0)]), n)[0] == {'name': 'QNAME_1', 'format': 'integers', 'dtype': 'uint8', 'max': 255, 'min': 0, 'offset': False}
    assert same(fused(n, [(0, 256, quiet, 0)]), n) == Q.DECLINE                   # range beyond the dtype of its distinct count: a mapping of strings
    assert same(fused(n, [(1000, 1255, quiet, 0)]), n)[0]['offset'] is True        # vmax > lim: stored minus min
    assert same(fused(n, [(1, 4, quiet, 0), (0, 256, quiet, 0)]), n) == Q.DECLINE  # the second column decides


def test_declines_and_sort_requests():
    n = 50000
    ths = Q._thresholds(n)
    ok = [(1, 4, [4] * len(ths), 0), (0, 3000, lambda T: T, 0)]
    assert isinstance(same(fused(n, ok), n), list)
    assert same(fused(n, ok, ok=0), n) == Q.DECLINE
    for flags in (1, 2, 0x80000000):
        assert same(fused(n, ok, flags=flags), n) == Q.DECLINE
    assert same(fused(n, ok, nreads=n - 1), n) == Q.DECLINE and same(fused(n, ok, nreads=n + 1), n) == Q.DECLINE
    assert same(fused(n, ok), n - 1) == Q.DECLINE and same(fused(n, ok), n + 1) == Q.DECLINE       # the caller's count differs
    assert same(fused(0, ok[:1]), 0) == Q.DECLINE and same(fused(n, ok), 0) == Q.DECLINE
    assert same(fused(n, ok, nth=len(ths) - 1), n) == Q.DECLINE and same(fused(n, ok, nth=len(ths) + 1), n) == Q.DECLINE
    for k in range(len(ths)):
        r = fused(n, ok); r.thresholds[k] += 1
        assert same(r, n) == Q.DECLINE
    # undetermined: the sort, whatever the counts say -- unless an earlier column has declined by then
    assert same(fused(n, [(1, 4, [4] * len(ths), 1)]), n) == Q.NEEDS_SORT
    assert same(fused(n, [(0, 1 << 20, lambda T: T, 1)]), n) == Q.NEEDS_SORT
    assert same(fused(n, [(0, 256, [9] * len(ths), 0), (1, 4, [4] * len(ths), 1)]), n) == Q.DECLINE
    assert same(fused(n, [(1, 4, [4] * len(ths), 1), (0, 256, [9] * len(ths), 0)]), n) == Q.NEEDS_SORT
    # a wide range that no checkpoint below 2^21 settles, on a file with checkpoints beyond
    big = Q._thresholds(N_BIG)
    assert same(fused(N_BIG, [(0, 1 << 20, [5] * len(big), 0)]), N_BIG) == Q.NEEDS_SORT
    # an empty value range as the kernel leaves it for a column it never saw (vmin = 2^32 - 1, vmax = 0)
    same(fused(n, [(U32, 0, [0] * len(ths), 0)]), n)


def test_every_column_count():
    n = 30000
    ths = Q._thresholds(n)
    for ncols in range(1, 9):
        cols = [(c, c + 10 ** c, lambda T: T, 0) if c % 2 else (1, 4, [4] * len(ths), 0) for c in range(ncols)]
        res = same(fused(n, cols), n)
        assert len(res) == ncols and [c['name'] for c in res] == ['QNAME_%d' % (c + 1) for c in range(ncols)]
