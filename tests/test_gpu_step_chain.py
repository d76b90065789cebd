"""GPU: the launch chains around the census and the pack kernel of the encode step (the closing scan from bucket totals of 1 024 census
tiles, the clears moved out of the chain, the self-restoring first-occurrence tables, the decisions and the QNAME typing in the
library) -- the queued census at the sizes where the bucket scan can go wrong, the step's call order on small files against the
oracles, repeated on one context, and every fetch on its own."""
import numpy as np
import pytest

import oracle_c
import uq_oracle as O
from uq_amd import analysis, ops, qname, qname_device, synth

pytestmark = pytest.mark.gpu

TILE = 16384          # census tile (csrc/index.hip)
BUCKET = 1024         # census tiles per bucket total


def _text(nbytes, seed, mean_line=40):
    """nbytes of 'A'..'Z' with newlines at random places (about one per mean_line bytes); the last byte is a newline."""
    rng = np.random.default_rng(seed)
    a = (65 + (np.arange(nbytes, dtype=np.uint32) % 26)).astype(np.uint8)
    a[rng.integers(0, nbytes, size=max(nbytes // mean_line, 1))] = 10
    a[-1] = 10
    return a


def _queued_census(ctx, host, mis=0, chunks=1):
    """ChunkedCensus -> end_async -> index_lines_async -> wait on a device copy of `host` that starts `mis` bytes behind a 16-byte boundary
    -> (lines, ok, index)."""
    t = ctx.torch
    base = t.empty(host.size + 32, dtype=t.uint8, device=ctx.device)
    off = (-base.data_ptr()) % 16 + mis
    buf = base[off:off + host.size]
    buf.copy_(t.from_numpy(host))
    assert buf.data_ptr() % 16 == mis
    want = oracle_c.index_lines(host)
    cap = len(want) - 1 + 7
    cen = ops.ChunkedCensus(ctx, buf)
    ntiles = (host.size + mis + TILE - 1) // TILE
    cuts = sorted({min(max(k * ntiles // chunks, 1) * TILE - mis, host.size) for k in range(1, chunks)} | {host.size})
    lo = 0
    for hi in cuts:                                  # whole tiles of the aligned address space; the last chunk ends with the buffer
        cen.chunk(lo, hi - lo); lo = hi
    cen.end_async()
    ls = ops.index_lines_async(ctx, buf, cap)
    nl, ok = cen.wait()
    return nl, ok, ls, want


@pytest.mark.parametrize('tiles', [1, 2, 1023, 1024, 1025, 2049])
def test_queued_census_at_bucket_edges(ctx, tiles):
    for nbytes, chunks in ((tiles * TILE, 1), (tiles * TILE - 5, 3)) if tiles > 2 else ((tiles * TILE, 1), (tiles * TILE - TILE + 1, 1), (tiles * TILE - 5, 2)):
        host = _text(nbytes, 1000 + tiles)
        nl, ok, ls, want = _queued_census(ctx, host, chunks=chunks)
        assert ok and nl == len(want) - 1
        assert np.array_equal(ctx.to_numpy(ls[:nl + 1], np.uint64), want)


def test_queued_census_misaligned_buffers(ctx):
    host = _text(BUCKET * TILE + 3 * TILE + 77, 7)           # the misalignment moves the last bytes of a bucket's tiles into the next
    for mis in range(1, 16):
        nl, ok, ls, want = _queued_census(ctx, host, mis=mis, chunks=1 + mis % 3)
        assert ok and nl == len(want) - 1, mis
        assert np.array_equal(ctx.to_numpy(ls[:nl + 1], np.uint64), want), mis


def test_queued_census_tiles_without_newlines_at_a_bucket_boundary(ctx):
    host = _text((BUCKET + 3) * TILE, 11)
    for lo, hi in (((BUCKET - 1) * TILE, BUCKET * TILE), (BUCKET * TILE, (BUCKET + 1) * TILE), ((BUCKET - 2) * TILE + 5, (BUCKET + 2) * TILE - 5), (0, TILE)):
        h = host.copy()
        h[lo:hi] = 66                                       # one long line over the boundary
        nl, ok, ls, want = _queued_census(ctx, h, chunks=2)
        assert ok and nl == len(want) - 1
        assert np.array_equal(ctx.to_numpy(ls[:nl + 1], np.uint64), want)
    h = np.full(3 * TILE, 66, dtype=np.uint8)               # no newline at all
    nl, ok, ls, want = _queued_census(ctx, h)
    assert ok and nl == 0 and len(want) == 1


def test_queued_census_list_overflow_stands_down(ctx):
    host = _text(5 * TILE, 13)
    host[2 * TILE + 100:2 * TILE + 100 + 1500] = 10         # more than 1024 newlines in one tile
    nl, ok, ls, want = _queued_census(ctx, host)
    assert not ok and nl == len(want) - 1
    buf = ctx.to_device(host)                                # and the pack kernel behind such a census stands down too
    fastq = synth.fastq_array(synth.Spec(5, 50), 64)
    guess = ops.head_guess(ctx, ctx.to_device(fastq))[0]
    cen = ops.ChunkedCensus(ctx, buf); cen.chunk(0, buf.numel()); cen.end_async()
    q = ops.pack_stats_async(ctx, buf, None, 4096, guess)
    assert q is not None
    hs = ops.stats_fetch(ctx, q[3])
    assert cen.wait() == (len(want) - 1, False)
    assert ops.count_lines(ctx, buf) == len(want) - 1        # the bitmap form takes over
    assert np.array_equal(ctx.to_numpy(ops.index_lines(ctx, buf, len(want) - 1), np.uint64), want)
    assert hs.incomplete or int(hs.counts.sum()) == 0


# ------------------------------------------------------------------ the step's call order
INPUTS = {'1 read': (synth.Spec(31, 150), 1), '3 reads': (synth.Spec(32, 150), 3), '4097 reads': (synth.Spec(33, 150), 4097),
          '50000 reads': (synth.Spec(34, 150), 50000), '20000 var N': (synth.Spec(35, (36, 301), n_rate=1), 20000)}
_REF = {}


def _reference(name):
    """The oracles' answers for an input, computed once: index, statistics, decisions, rows, QNAME analysis."""
    if name not in _REF:
        spec, n = INPUTS[name]
        host = synth.fastq_array(spec, n)
        hls = oracle_c.index_lines(host)
        st = oracle_c.stats(host, hls, 0, n)
        od = O.decide(O.histogram_to_static_qualities(st['counts'], st['first_seen']), st['len_min'], st['len_max'])
        rd, rq, _ = oracle_c.pack(host, hls, 0, n, od['bases'], od['qualities'], od['N_qual'], od['bits_per_base'], od['bits_per_quality'],
                                  od['variable_read_lengths'], od['dna_bytes_per_row'], od['quality_bytes_per_row'])
        try:
            qn = qname.analyse(qname.qname_lines(host, hls, n))
        except qname.QnameError:                             # a file of one record: no separator has a constant count, the reference refuses it
            qn = None
        if qn is not None and n <= 5000:                                        # the faithful Python loops of the reference on the small ones
            lines = O.read_lines(host.tobytes())
            p1 = O.pass1(lines)
            assert (p1['prefix'], p1['suffix'], p1['separators']) == tuple(qn[:3])
            assert O.qname_columns(lines, p1['prefix'], p1['suffix'], p1['separators']) == qn[3]
        _REF[name] = dict(host=host, hls=hls, st=st, od=od, rd=rd, rq=rq, qn=qn, n=n)
    return _REF[name]


_SIDE = []


def _side(ctx):
    if not _SIDE:
        from uq_amd.device import SideContext
        _SIDE.append(SideContext(ctx))
    return _SIDE[0]


def _step(ctx, name, d_buf=None):
    """bench.py's step: stats_new -> ChunkedCensus -> head_guess -> FusedQname + qname_guess_async -> pack_stats_async ->
    qname_fused_finish -> stats_fetch -> wait -> analyse_fused -> decide; everything against the oracles."""
    ref = _reference(name)
    n, host = ref['n'], ref['host']
    if d_buf is None: d_buf = ctx.to_device(host)
    ctx.sync()                                               # (the side stream does not wait for the main one: the input is complete)
    st_q = ops.stats_new(ctx)
    cen = ops.ChunkedCensus(ctx, d_buf); cen.chunk(0, d_buf.numel()); cen.end_async()
    g = ops.head_guess(_side(ctx), d_buf, head_bytes=ops.HEAD_BYTES_SMALL, head_reads=ops.HEAD_READS_INDEXED)      # meanwhile, on a second stream
    assert g is not None
    guess, rpb = g
    cap = int(d_buf.numel() * rpb * 1.02) + 1024
    fq = ops.FusedQname(ctx, cap)
    ops.qname_guess_async(ctx, d_buf, None, fq)
    sp = ops.pack_stats_async(ctx, d_buf, None, cap, guess, st=st_q, fq=fq)
    if sp is not None:
        ops.qname_fused_finish(ctx, fq)
        hs = ops.stats_fetch(ctx, sp[3])
    nlines, ok = cen.wait()
    assert ok and nlines == 4 * n
    if sp is None:                                           # no fused kernel for the head's alphabets (a single read's): the step's plain passes
        assert n < 4
        st = ops.stats_new(ctx)
        ops.stats_accumulate(ctx, st, d_buf, ops.index_lines(ctx, d_buf, ops.count_lines(ctx, d_buf)), 0, n)
        hs = ops.stats_fetch(ctx, st)
    assert not hs.incomplete and hs.bad_plus is None and hs.bad_len is None
    assert np.array_equal(hs.counts, ref['st']['counts']) and (hs.len_min, hs.len_max) == (ref['st']['len_min'], ref['st']['len_max'])
    assert sp is None or ops.bad_index(sp[2]) is None
    qres = qname_device.analyse_fused(ctx, fq, n) if sp is not None else None
    d = analysis.decide_from_stats(hs)
    for k in ('bases', 'qualities', 'N_qual', 'bits_per_base', 'bits_per_quality', 'variable_read_lengths', 'dna_max', 'dna_bytes_per_row', 'quality_bytes_per_row'):
        assert d[k] == ref['od'][k], k
    p = ops.make_pack_params(d['bases'], d['qualities'], d['N_qual'], d['bits_per_base'], d['bits_per_quality'], d['variable_read_lengths'],
                             d['dna_bytes_per_row'], d['quality_bytes_per_row'], d['dna_max'], hs.max_record_bytes)
    assert ops.same_pack_params(p, guess) == ops.same_pack_params_py(p, guess)
    if sp is not None and ops.same_pack_params(p, guess):
        dna, qual = sp[0], sp[1]
    else:                                                    # the head of the file decided otherwise than the whole: the step packs again
        dna, qual, bad = ops.pack(ctx, d_buf, ops.index_lines(ctx, d_buf, ops.count_lines(ctx, d_buf)), 0, n, p)
        assert ops.bad_index(bad) is None
    assert np.array_equal(ctx.to_numpy(dna[:n * d['dna_bytes_per_row']]).reshape(n, -1), ref['rd'])
    assert np.array_equal(ctx.to_numpy(qual[:n * d['quality_bytes_per_row']]).reshape(n, -1), ref['rq'])
    want = ref['qn']
    if want is None:                                         # the reference refuses the QNAMEs: the fused pass must not answer
        assert qres is None
        return fq
    if qres is None:                                         # (a sample of two reads may not settle the layout: the exact kernels)
        assert n < 4
        qres = qname_device.analyse_device(ctx, d_buf, ops.index_lines(ctx, d_buf, ops.count_lines(ctx, d_buf)), n)
        if qres is None: return fq                           # (nor they: such a file is the host path's)
    assert list(qres[:4]) == list(want[:4])
    for a, b, c in zip(qres[4], want[4], want[3]):
        assert np.array_equal(ctx.to_numpy(a, np.dtype(c['dtype'])), np.asarray(b))
    return fq


@pytest.mark.parametrize('name', list(INPUTS))
def test_step_call_order_against_the_oracles(ctx, name):
    _step(ctx, name)


def test_step_repeated_on_one_context(ctx):
    # the same input twice in a row, another one in between, the first again: the first-occurrence tables restore themselves and the
    # clears that moved out of the chain still happen once per step
    for name in ('4097 reads', '4097 reads', '20000 var N', '4097 reads', '3 reads', '50000 reads', '4097 reads'):
        _step(ctx, name)


# ------------------------------------------------------------------ every fetch on its own
def test_stats_fetch_without_a_qname_pass(ctx):
    ref = _reference('4097 reads')
    d_buf = ctx.to_device(ref['host'])
    guess = ops.head_guess(ctx, d_buf)[0]
    cen = ops.ChunkedCensus(ctx, d_buf); cen.chunk(0, d_buf.numel()); cen.end_async()
    sp = ops.pack_stats_async(ctx, d_buf, None, ref['n'] + 9, guess)
    hs = ops.stats_fetch(ctx, sp[3])
    assert cen.wait() == (4 * ref['n'], True)
    assert not hs.incomplete and np.array_equal(hs.counts, ref['st']['counts'])
    # and of a table that no pack kernel filled: the plain statistics pass
    ls = ops.index_lines(ctx, d_buf, ops.count_lines(ctx, d_buf))
    st = ops.stats_new(ctx)
    ops.stats_accumulate(ctx, st, d_buf, ls, 0, ref['n'])
    assert np.array_equal(ops.stats_fetch(ctx, st).counts, ref['st']['counts'])


def test_qname_fused_fetch_without_a_finish(ctx):
    ref = _reference('4097 reads')
    d_buf = ctx.to_device(ref['host'])
    full = ops.qname_fused_fetch(ctx, _step(ctx, '4097 reads', d_buf))     # after a whole step (the finish has sent it)
    ls = ops.index_lines(ctx, d_buf, ops.count_lines(ctx, d_buf))
    fq = ops.FusedQname(ctx, ref['n'])
    ops.qname_guess(ctx, d_buf, ls, ref['n'], fq)
    r = ops.qname_fused_fetch(ctx, fq)                                      # the guess alone: nothing counted yet
    assert r.ok == 1 and (r.plen, r.slen, r.nsep, r.l1len) == (full.plen, full.slen, full.nsep, full.l1len)
    assert bytes(r.line1[:r.l1len]) == bytes(full.line1[:full.l1len]) and bytes(r.seps[:r.nsep]) == bytes(full.seps[:full.nsep])
    assert r.nreads == 0 and r.nth == 0 and r.flags == 0
    assert qname_device.fused_columns(r, ref['n']) == qname_device.DECLINE


def test_count_lines_wait_without_a_pack(ctx):
    for name in ('3 reads', '50000 reads'):
        ref = _reference(name)
        d_buf = ctx.to_device(ref['host'])
        for _ in range(2):
            cen = ops.ChunkedCensus(ctx, d_buf); cen.chunk(0, d_buf.numel()); cen.end_async()
            assert cen.wait() == (4 * ref['n'], True)
        cen = ops.ChunkedCensus(ctx, d_buf); cen.chunk(0, d_buf.numel())
        assert cen.end() == 4 * ref['n']                                    # the synchronous end of a census whose begin prepared the queued form
        assert np.array_equal(ctx.to_numpy(ops.index_lines(ctx, d_buf, 4 * ref['n']), np.uint64), ref['hls'])


def test_epilogue_and_read_back_in_other_orders(ctx):
    """The finish's one read-back serves the three fetches in any order, once each; what it did not send they send themselves."""
    ref = _reference('4097 reads')
    n = ref['n']
    d_buf = ctx.to_device(ref['host'])
    ctx.sync()
    guess = ops.head_guess(_side(ctx), d_buf)[0]
    for order in ('wait stats qname', 'qname wait stats', 'stats stats qname wait'):
        cen = ops.ChunkedCensus(ctx, d_buf); cen.chunk(0, d_buf.numel()); cen.end_async()
        fq = ops.FusedQname(ctx, n + 8)
        ops.qname_guess_async(ctx, d_buf, None, fq)
        sp = ops.pack_stats_async(ctx, d_buf, None, n + 8, guess, fq=fq)
        ops.qname_fused_finish(ctx, fq)
        for what in order.split():
            if what == 'wait': assert cen.wait() == (4 * n, True)
            elif what == 'stats':                            # (the second fetch finds nothing sent and compacts the statistics itself)
                hs = ops.stats_fetch(ctx, sp[3])
                assert not hs.incomplete and np.array_equal(hs.counts, ref['st']['counts']) and (hs.len_min, hs.len_max) == (150, 150)
            else:
                r = ops.qname_fused_fetch(ctx, fq)
                assert r.ok == 1 and r.flags == 0 and r.nreads == n and list(r.thresholds[:r.nth]) == qname_device._thresholds(n)
    # statistics changed after they were sent: the fetch must not hand out the copy on its way
    cen = ops.ChunkedCensus(ctx, d_buf); cen.chunk(0, d_buf.numel()); cen.end_async()
    fq = ops.FusedQname(ctx, n + 8)
    ops.qname_guess_async(ctx, d_buf, None, fq)
    sp = ops.pack_stats_async(ctx, d_buf, None, n + 8, guess, fq=fq)
    ops.qname_fused_finish(ctx, fq)
    assert cen.wait() == (4 * n, True)
    ls = ops.index_lines(ctx, d_buf, ops.count_lines(ctx, d_buf))
    ops.stats_accumulate(ctx, sp[3], d_buf, ls, 0, n)                        # every read counted a second time
    assert np.array_equal(ops.stats_fetch(ctx, sp[3]).counts, 2 * ref['st']['counts'])
    # a finish whose pack kernel was not the queued one: no statistics ride along, the fetch compacts them
    fq2 = ops.FusedQname(ctx, n)
    ops.qname_guess(ctx, d_buf, ls, n, fq2)
    sp2 = ops.pack_stats(ctx, d_buf, ls, 0, n, guess, fq=fq2)
    ops.qname_fused_finish(ctx, fq2)
    assert np.array_equal(ops.stats_fetch(ctx, sp2[3]).counts, ref['st']['counts'])
    assert qname_device.analyse_fused(ctx, fq2, n) is not None
