"""GPU: every helper kernel against the numpy restatement of its contract, output for output: the routing arithmetic of
csrc/route.hip (tests/numpy_rows.py), the QNAME kernels of csrc/qname_dev.hip and csrc/qname_fused.hip (tests/fake_qname_ops.py, or
plain numpy / a dict scan) and uq_check_index_range (tests/fake_decode_ops.py).  The pipelines that use these kernels mostly see
well-behaved inputs, and a wrong raw output often ends there as "declined"; here the inputs are the edges: more than one sweep of the
grid, the switch between the LDS-private and the global first-seen table, lines beyond the 64-byte LDS row and a last line whose
16-byte fetch would cross the end of the buffer, splitters that share their first eight bytes, empty shards.  Integer work: every comparison is exact."""
import os
import re

import numpy as np
import pytest
import torch

import fake_qname_ops as F
import oracle_c
import qname_raw_inputs as R
from fake_decode_ops import FakeOps
from numpy_rows import NumpyRows
from uq_amd import ops
from uq_amd.dist import HipRows

pytestmark = pytest.mark.gpu

_SIGNED = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
# grid_for() of csrc/qname_dev.hip and uq_check_index_range launch at most 8 * UQ_NUM_CU workgroups of 256 lanes: that many elements are
# one sweep of the grid-stride loops.  UQ_NUM_CU is not exposed through the ABI; it is read from the header the kernels are built with.
with open(os.path.join(os.path.dirname(ops.__file__), 'csrc', 'common.h')) as _f:
    UQ_NUM_CU = int(re.search(r'^#define UQ_NUM_CU (\d+)\s*$', _f.read(), re.M).group(1))
ONE_SWEEP = 8 * UQ_NUM_CU * 256
INT64_MAX = (1 << 63) - 1


def _both(ctx, a):
    """numpy array -> (CPU tensor for the restatement, device tensor for the kernel), unsigned types as their signed bit patterns."""
    a = np.ascontiguousarray(a)
    if a.dtype in _SIGNED: a = a.view(_SIGNED[a.dtype])
    tc = torch.from_numpy(a.copy())
    return tc, tc.to(ctx.device)


def _np(t, dtype=None):
    a = t.detach().cpu().numpy()
    return a.view(dtype) if dtype is not None else a


# ================================================================== route.hip
def _pool(C, rng):
    """Distinct rows in memcmp order to draw splitters from.  C > 8: most share their first eight bytes and differ at byte 8 or at the
    last byte only (the kernel's 8-byte prefix keys tie there and whole rows decide)."""
    if C == 1:
        rows = {bytes([v]) for v in range(256)}
    elif C <= 8:
        rows = {bytes(r) for r in rng.integers(0, 256, (400, C), dtype=np.uint8)}
    else:
        head = bytes(rng.integers(1, 255, 8, dtype=np.uint8))
        rows = {head + bytes([v]) + bytes(C - 9) for v in range(256)}
        rows |= {head + bytes(C - 9) + bytes([v]) for v in range(1, 256)}
        rows |= {bytes(r) for r in rng.integers(0, 256, (60, C), dtype=np.uint8)}
    return sorted(rows)


def _splitter_sets(C, nsplit, pool, rng):
    """(label, sorted splitter rows, the repeated row): all distinct, and a value repeated 2, 3 and nsplit times."""
    out = []
    for rep in sorted({1, 2, 3, nsplit} - {0}):
        if rep > nsplit: continue
        vals = [pool[i] for i in rng.choice(len(pool), nsplit - rep + 1, replace=False)]
        heavy = sorted(vals)[len(vals) // 2]
        out.append(('one value x%d' % rep, sorted(vals + [heavy] * (rep - 1)), heavy))
    return out or [('no splitters', [], bytes(C))]


@pytest.mark.parametrize('C', [1, 3, 7, 8, 9, 38, 113])
def test_partition_rows(ctx, C):
    """700 rows (three workgroups) against 0, 1, 2, 7 and 255 splitters: rows equal to a splitter, to one that 2, 3 or all splitters
    share (dealt to those ranks by file position), between, below and above them; for C > 8 splitters and rows that tie on the
    8-byte prefix key."""
    rng = np.random.default_rng(100 + C)
    rows, hip, ref = 700, HipRows(ctx), NumpyRows()
    pool = _pool(C, rng)
    for nsplit in (0, 1, 2, 7, 255):
        for label, split, heavy in _splitter_sets(C, nsplit, pool, rng):
            table = [heavy] * 150                                                   # many rows equal to the repeated value
            table += [split[i] for i in rng.integers(0, max(len(split), 1), 150 if split else 0)]     # rows equal to a splitter
            table += [pool[i] for i in rng.integers(0, len(pool), 150)]             # rows between them (C > 8: ties on the first eight bytes)
            table += [bytes(C), b'\xff' * C]                                        # below and above all splitters
            table += [bytes(r) for r in rng.integers(0, 256, (rows - len(table), C), dtype=np.uint8)]
            table = [table[i] for i in rng.permutation(rows)]
            tc, td = _both(ctx, np.frombuffer(b''.join(table), np.uint8))
            sc, sd = _both(ctx, np.frombuffer(b''.join(split) or bytes(C), np.uint8))
            for index_base, total in ((0, rows), (12345, 12345 + rows + 55)):       # the dealt ranks span the whole tie group / its upper end
                got = _np(hip.partition_rows(sd[:nsplit * C], nsplit, C, td, rows, index_base, total))
                want = ref.partition_rows(sc[:nsplit * C], nsplit, C, tc, rows, index_base, total).numpy()
                assert np.array_equal(got, want), (C, nsplit, label, index_base, np.flatnonzero(got != want)[:5])
                if index_base == 0 and split.count(heavy) >= 2:                     # the input does deal: the tie group's rows go to several ranks
                    assert len({int(want[r]) for r in range(rows) if table[r] == heavy}) >= 2


@pytest.mark.parametrize('world', [1, 2, 3, 16, 256])
def test_owner_of_rows(ctx, world):
    """Empty shards at the front, in the middle (two in a row) and at the end; probes at every start, start - 1 and the last row."""
    rng = np.random.default_rng(world)
    hip, ref = HipRows(ctx), NumpyRows()
    layouts = []
    sizes = rng.integers(1, 1000, world)
    layouts.append(sizes.copy())
    if world >= 2:
        a = sizes.copy(); a[0] = 0; layouts.append(a)                              # front
        a = sizes.copy(); a[-1] = 0; layouts.append(a)                             # end
    if world >= 3:
        a = sizes.copy(); a[0] = 0; a[-1] = 0; layouts.append(a)
    if world >= 16:
        a = sizes.copy(); a[0] = a[1] = 0; a[world // 2] = a[world // 2 + 1] = 0; a[-2] = a[-1] = 0; layouts.append(a)
    for sz in layouts:
        starts = [0] + np.cumsum(sz).tolist()
        total = starts[-1]
        probes = sorted({g for s in starts for g in (s, s - 1) if 0 <= g < total} | {total - 1})
        probes = np.array(probes + rng.integers(0, total, 600).tolist(), dtype=np.int64)    # three workgroups
        gc, gd = _both(ctx, probes)
        got = _np(hip.owner_of_rows(gd, starts))
        want = ref.owner_of_rows(gc, starts).numpy()
        assert np.array_equal(got, want), (world, starts[:8], np.flatnonzero(got != want)[:5])
        assert all(starts[o] <= g < starts[o + 1] for g, o in zip(probes.tolist(), got.tolist()))     # and the contract itself


@pytest.mark.parametrize('n', [0, 1, 257])
@pytest.mark.parametrize('in_dtype,out_itemsize', [(np.uint32, 4), (np.uint32, 8), (np.int64, 4), (np.int64, 8)])
def test_index_affine(ctx, in_dtype, out_itemsize, n):
    rng = np.random.default_rng(n + out_itemsize)
    hip, ref = HipRows(ctx), NumpyRows()
    if in_dtype is np.uint32:
        a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        a[:2] = [0xFFFFFFFF, 0x80000000][:n]                                       # unsigned 32-bit positions from 2^31 on
    else:
        a = rng.integers(0, 1 << 40, n, dtype=np.int64)
        a[:1] = [(1 << 32) + 5][:n]
    for add in (0, -3, -(1 << 31), (1 << 33) + 7, -(1 << 36)):                    # negative; 64-bit results beyond 2^32
        ac, ad = _both(ctx, a)
        got = _np(hip.index_affine(ad, add, out_itemsize))
        want = ref.index_affine(ac, add, out_itemsize).numpy()
        assert got.dtype == want.dtype and np.array_equal(got, want), (add, got[:4], want[:4])


@pytest.mark.parametrize('n', [1, 256, 257, 5000])
@pytest.mark.parametrize('dtype,base', [(np.uint32, 0), (np.uint32, (1 << 31) + 5), (np.int64, 77), (np.int64, (1 << 40) + 3)])
def test_invert_permutation(ctx, dtype, base, n):
    rng = np.random.default_rng(n)
    hip, ref = HipRows(ctx), NumpyRows()
    perm = (rng.permutation(n).astype(np.int64) + base).astype(dtype)
    pc, pd = _both(ctx, perm)
    assert np.array_equal(_np(hip.invert_permutation(pd, base)), ref.invert_permutation(pc, base).numpy())
    if n >= 256:                                                                   # two entries out of range: the lower one is named
        bad = perm.copy()
        bad[n - 1] = base + n
        bad[17] = (base - 1) if base else n + 5
        with pytest.raises(RuntimeError, match=r'\(entry 17\)'):
            hip.invert_permutation(_both(ctx, bad)[1], base)


# ================================================================== qname_dev.hip: the distinct counts
def _sorted_groups(keys):
    perm = np.argsort(keys, kind='stable')
    sk = keys[perm]
    head = np.ones(len(keys), dtype=bool); head[1:] = sk[1:] != sk[:-1]
    return perm, (np.cumsum(head) - 1).astype(np.int32)


def _thresholds(rng, n, count, offset=0):
    th = [0, n - 1] + rng.integers(0, n, max(count - 2, 0)).tolist()
    return [offset + int(x) for x in th[:count]]


@pytest.mark.parametrize('case', ['one', 'all_equal', 'all_distinct', 'groups', 'past_one_sweep'])
def test_prefix_distinct(ctx, case):
    """The stable order as 4-byte local positions and as 8-byte file-wide ones (from 2^32 on, thresholds there), 1 and 64 thresholds
    with 0 and n - 1 among them; the last case is one element group past the grid's first sweep."""
    rng = np.random.default_rng(3)
    n = {'one': 1, 'all_equal': 3000, 'all_distinct': 3000, 'groups': 70001, 'past_one_sweep': ONE_SWEEP + 300}[case]
    if case in ('one', 'all_equal'): keys = np.full(n, 9, np.int64)
    elif case == 'all_distinct': keys = rng.permutation(n).astype(np.int64)
    else:
        keys = rng.integers(0, n // 3, n)
        keys[n - 1] = n                                                            # a group whose only member is the last read
    perm, skey = _sorted_groups(keys)
    kc, kd = _both(ctx, skey)
    for base, single in ((0, n - 1), ((1 << 32) + 7, 0)):
        pc, pd = _both(ctx, perm.astype(np.int32) if base == 0 else perm.astype(np.int64) + base)
        for th in ([base + single], _thresholds(rng, n, 64, base)):
            assert ops.prefix_distinct(ctx, pd, kd, n, th) == F.prefix_distinct(F.FakeCtx(), pc, kc, n, th), (case, base, len(th))
        assert ops.prefix_distinct(ctx, pd, kd, n, [base + n - 1]) == [len(np.unique(keys))]


@pytest.mark.parametrize('value_range', [1, 4096, 4097, 1 << 20])
@pytest.mark.parametrize('n', [5, 300, 600_000])
def test_int_prefix_distinct(ctx, n, value_range):
    """The LDS-private table (range <= 4 096) and the global one; a workgroup's slice of the reads shorter than the workgroup and, at
    600 000 reads, longer (the grid is capped); values outside [vmin, vmin + range) ignored; file-wide read numbers."""
    rng = np.random.default_rng(n + value_range)
    vmin = -1234567
    val = vmin + rng.integers(-3, value_range + 3, n)                              # some below vmin, some beyond the range
    val[n // 2] = vmin + value_range - 1
    val[n - 1] = vmin
    vc, vd = _both(ctx, val.astype(np.int64))
    for index_base, count in ((0, 2), ((1 << 33) + 11, 64)):                       # (two thresholds: 0 and n - 1)
        th = _thresholds(rng, n, count, index_base)
        got = ops.int_prefix_distinct(ctx, vd, n, vmin, value_range, th, index_base=index_base)
        assert got == F.int_prefix_distinct(F.FakeCtx(), vc, n, vmin, value_range, th, index_base=index_base), (n, value_range, index_base)
    assert ops.int_prefix_distinct(ctx, vd, n, vmin, value_range, [n - 1]) == [got[1]]      # one threshold


@pytest.mark.parametrize('n', [1, 257])
@pytest.mark.parametrize('itemsize', [1, 2, 4, 8])
def test_encode_int(ctx, itemsize, n):
    rng = np.random.default_rng(itemsize * n)
    big = 10 ** 18 - 1                 # the widest value the tokeniser produces: val - sub stays inside int64, no signed overflow is asked for
    val = rng.integers(-big, big, n)
    val[:1] = big
    if n > 3: val[1:4] = [-big, 0, -1]
    vc, vd = _both(ctx, val.astype(np.int64))
    for sub in (-77, 0, 5, -big, big):
        got = _np(ops.encode_int(ctx, vd, sub, itemsize))
        want = F.encode_int(F.FakeCtx(), vc, sub, itemsize).numpy()
        assert got.dtype == want.dtype and np.array_equal(got, want), (itemsize, sub)


# ================================================================== qname_fused.hip
def _fused(ctx, cols, capacity):
    """A FusedQname whose value columns are written directly: cols[c] = uint32 values of column c."""
    fq = ops.FusedQname(ctx, capacity)
    host = np.full(ops.QF_MAXC * fq.pitch, 0xDEADBEEF, dtype=np.uint32)           # what lies between n and the pitch is nobody's
    for c, v in enumerate(cols): host[c * fq.pitch:c * fq.pitch + len(v)] = v
    fq.vals.copy_(torch.from_numpy(host.view(np.int32)))
    return fq


@pytest.mark.parametrize('n,capacity', [(1, 1), (3, 50), (1001, 1001), (1024, 1030), (5000, 7001)])
def test_encode_u32_and_columns(ctx, n, capacity):
    rng = np.random.default_rng(n)
    cols = [rng.integers(lo, hi, n, dtype=np.uint64).astype(np.uint32) for lo, hi in
            ((0, 256), (1000, 1256), (0, 1 << 16), (70000, 70000 + (1 << 16)), (0, 1 << 32), (1 << 31, 1 << 32), (5, 6), (0, 1 << 32))]
    assert len(cols) == ops.QF_MAXC
    fq = _fused(ctx, cols, capacity)
    assert fq.pitch >= n and (capacity == n or fq.pitch > n)
    dt = {1: np.uint8, 2: np.uint16, 4: np.uint32}
    sizes = [1, 1, 2, 2, 4, 4, 1, 2]
    for subs in ([0] * 8, [int(c.min()) for c in cols]):                           # sub = 0 and the column minimum
        for ncols in (1, ops.QF_MAXC):                                             # one column and as many as the structure holds
            outs = ops.encode_u32_columns(ctx, fq, n, subs[:ncols], sizes[:ncols])
            for c in range(ncols):
                want = (cols[c] - np.uint32(subs[c])).astype(dt[sizes[c]])
                assert np.array_equal(_np(outs[c], dt[sizes[c]]), want), ('columns', c, subs[c], ncols)
        for c in range(ops.QF_MAXC):
            for isz in (1, 2, 4):
                got = _np(ops.encode_u32(ctx, fq.column(c, n), n, subs[c], isz), dt[isz])
                assert np.array_equal(got, (cols[c] - np.uint32(subs[c])).astype(dt[isz])), ('single', c, subs[c], isz)


def _first_seen_scan(cols, read_offset, vmins, ranges):
    """A dict scan: table[c][v - vmin] = read_offset + the lowest read holding v, INT64_MAX where v does not occur or the column is skipped."""
    out = np.full((ops.QF_MAXC, 4096), INT64_MAX, dtype=np.int64)
    for c, (vmin, rg) in enumerate(zip(vmins, ranges)):
        first = {}
        for i, v in enumerate(cols[c].tolist()):
            if vmin <= v < vmin + rg and v not in first: first[v] = read_offset + i
        for v, i in first.items(): out[c, v - vmin] = i
    return out.reshape(-1)


def test_qname_fused_first_seen(ctx):
    """Ranges 1, 4 096 and 0 (column skipped), values outside the range ignored, read_offset != 0, and two shards whose element-wise
    minimum is the table of the whole file."""
    rng = np.random.default_rng(8)
    n, offset = 5000, (1 << 33) + 5
    vmins, ranges = [7, 1000, 3, 0xFFFFF000], [1, 4096, 0, 4096]
    cols = [np.where(rng.random(n) < 0.5, 7, rng.integers(0, 20, n)).astype(np.uint32),
            (1000 + rng.integers(-2, 4099, n) // 3 * 3).astype(np.uint32),             # a third of the range occurs; some values outside it
            rng.integers(0, 9, n).astype(np.uint32),
            (0xFFFFF000 + rng.integers(0, 4096, n)).astype(np.uint32)]                 # the top of the uint32 range
    cols[0][:3] = [9, 8, 6]                                                            # the range's one value is not in read 0
    whole = ops.qname_fused_first_seen(ctx, _fused(ctx, cols, n), n, offset, vmins, ranges)
    want = _first_seen_scan(cols, offset, vmins, ranges)
    assert np.array_equal(_np(whole), want)
    assert (want == INT64_MAX).sum() > 4096 * 5 and want[0] == offset + int(np.flatnonzero(cols[0] == 7)[0])
    lo = 1999
    a = ops.qname_fused_first_seen(ctx, _fused(ctx, [c[:lo] for c in cols], lo + 9), lo, offset, vmins, ranges)
    b = ops.qname_fused_first_seen(ctx, _fused(ctx, [c[lo:] for c in cols], n - lo), n - lo, offset + lo, vmins, ranges)
    assert np.array_equal(_np(a), _first_seen_scan([c[:lo] for c in cols], offset, vmins, ranges))
    assert np.array_equal(np.minimum(_np(a), _np(b)), want)
    none = ops.qname_fused_first_seen(ctx, _fused(ctx, cols, n), 0, offset, vmins, ranges)      # a rank without reads
    assert (_np(none) == INT64_MAX).all()


# ================================================================== gather.hip
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.uint32, np.uint64])
def test_check_index_range(ctx, dtype):
    rng = np.random.default_rng(np.dtype(dtype).itemsize)
    bits = 8 * np.dtype(dtype).itemsize
    top = (1 << bits) - 1
    for n in (0, 1, 700, ONE_SWEEP + 300):
        a = rng.integers(0, 200, n, dtype=np.uint64).astype(dtype)
        cases = [('none', a)]
        if n:
            b = a.copy(); b[n - 1] = top; cases.append(('last, top bit set', b))                   # unsigned: the largest value there is
            b = a.copy(); b[[n // 3, n // 2, n - 1]] = [1 << (bits - 1), top, 255]; cases.append(('several', b))
        for label, arr in cases:
            ic, idev = _both(ctx, arr)
            for limit in (0, 1, 256, 1 << 32):
                got = ops.check_index_range(ctx, idev, limit)
                assert got == FakeOps.check_index_range(None, ic, limit), (label, n, limit, got)


# ================================================================== qname_dev.hip: layout and tokeniser, raw outputs
def _index(ctx, names):
    host = R.fastq(names)
    ls = oracle_c.index_lines(host)
    bc, bd = _both(ctx, host)
    lc, ld = _both(ctx, ls)
    return bc, bd, lc, ld


@pytest.mark.parametrize('label,names', R.layout_files(), ids=[f[0] for f in R.layout_files()])
def test_qname_layout_raw_outputs(ctx, label, names):
    bc, bd, lc, ld = _index(ctx, names)
    n, line1 = len(names), names[0]
    if label in ('lengths', 'long_lines_last'):
        assert R.byte_tail_lines(names) == [n - 1]            # the last line is staged byte by byte: its 16-byte fetch would cross the buffer's end
    for base in (0, 1000):
        got = ops.qname_layout(ctx, bd, ld, n, line1, read_index_base=base)
        want = F.qname_layout(F.FakeCtx(), bc, lc, n, line1, read_index_base=base)
        for f in ('min_lcp', 'min_lcs', 'flags', 'nch'):
            assert getattr(got, f) == getattr(want, f), (label, base, f, getattr(got, f), getattr(want, f))
        for f in ('ch', 'entry', 'lastviol'):
            assert list(getattr(got, f)) == list(getattr(want, f)), (label, base, f)
    assert want.flags == {'proper_prefixes': 1, 'proper_suffixes': 1, 'a_name_of_256': 2}.get(label, 0)


def _tokenise_both(ctx, f):
    bc, bd, lc, ld = _index(ctx, f[4])
    n = len(f[4])
    got = ops.qname_tokenise(ctx, bd, ld, n, f[1], f[2], f[3])
    want = F.qname_tokenise(F.FakeCtx(), bc, lc, n, f[1], f[2], f[3])
    return got, want


@pytest.mark.parametrize('f', R.clean_files(), ids=[f[0] for f in R.clean_files()])
def test_qname_tokenise_clean_files_every_output(ctx, f):
    if f[0] == 'no_prefix_no_suffix':
        assert R.byte_tail_lines(f[4]) == [len(f[4]) - 1]      # the last line is staged byte by byte: its 16-byte fetch would cross the buffer's end
    (vals, strs, res), (wvals, wstrs, want) = _tokenise_both(ctx, f)
    assert want.flags == 0 and res.flags == 0
    for c in range(len(f[3]) + 1):
        gv, wv = _np(vals[c]), wvals[c].numpy()
        assert np.array_equal(gv, wv), (f[0], 'vals', c, np.flatnonzero(gv != wv)[:5])
        gs, ws = _np(strs[c]), wstrs[c].numpy()
        assert np.array_equal(gs, ws), (f[0], 'strs', c, np.flatnonzero(gs != ws)[:5])
    for field in ('first_nonint', 'vmin', 'vmax', 'any_long'):
        assert list(getattr(res, field)) == list(getattr(want, field)), (f[0], field)


@pytest.mark.parametrize('f', R.flagged_files(), ids=[f[0] for f in R.flagged_files()])
def test_qname_tokenise_flagged_files_flags_only(ctx, f):
    """One defect a file.  The contract sends the caller to the host on any flag, and kernel and restatement legitimately differ in
    what they leave behind there (the kernel folds a 19-digit field into vmin / vmax as 0, the restatement leaves it out; a name
    shorter than prefix + suffix gets no values at all): only the flags are compared, and each file raises its flag on both sides."""
    (_, _, res), (_, _, want) = _tokenise_both(ctx, f)
    assert res.flags == want.flags == f[5]
