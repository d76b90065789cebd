"""The per-tile part of the fused pack + statistics (+ QNAME) kernel -- reads and tiles counted in 32 bits, the LDS carve with everything
but the out tile at constant offsets, the epilogue's addresses parked in LDS -- at the shapes where that code can go wrong:
the queued form that takes its line starts from the census's lists (ops.pack_stats_async, with and without a FusedQname) against what the
suite already trusts on the same buffer: ops.pack + ops.stats_accumulate + qname_device.analyse_device, and oracle_c for the rows.
Rows, the 256 x 256 counts, lengths, flags and QNAME columns byte for byte."""
import ctypes as C

import numpy as np
import pytest

import oracle_c
import uq_oracle as O
from uq_amd import ops, synth

S = 20261019
gpu = pytest.mark.gpu


def tile_reads(p, qn_or_ntrick=True):
    """Reads per tile of the fused kernels for these parameters: pack_impl's arithmetic (pack.hip: Rs from the longest record, R from the
    average one, what the out tile holds, a multiple of 16 / 8 / 4)."""
    stage_cap = 4 * 256 * 16
    rec, avg = int(p.max_record_bytes), int(p.avg_record_bytes)
    Rs = max(1, min((stage_cap - 64) // rec, 63))
    R = Rs
    if 4 <= avg < rec: R = max(Rs, min((stage_cap - 64) // (avg + avg * 15 // 100 + 1), 63))
    fit = (stage_cap * 3 // 4) // (p.dna_bytes_per_row + p.quality_bytes_per_row)
    if R > fit: R = max(fit, Rs)
    if R >= 4:
        r16, r8, r4 = R & ~15, R & ~7, R & ~3
        R = r16 if r16 * 100 >= R * 85 else (r8 if r8 * 100 >= R * 85 else r4)
    return max(R, 1)


def decide(host, n, **dk):
    hls = oracle_c.index_lines(host)
    ref = oracle_c.stats(host, hls, 0, n)
    d = O.decide(O.histogram_to_static_qualities(ref['counts'], None), ref['len_min'], ref['len_max'], dk.get('notricks', False), False)
    p = ops.make_pack_params(d['bases'], d['qualities'], d['N_qual'], d['bits_per_base'], d['bits_per_quality'], d['variable_read_lengths'],
                             d['dna_bytes_per_row'], d['quality_bytes_per_row'], d['dna_max'], ref['max_record_bytes'],
                             avg_record_bytes=max(host.size // max(n, 1), 4))
    return hls, ref, d, p


def device_buffer(ctx, host, mis=0):
    if not mis: return ctx.to_device(host)
    back = ctx.empty(host.size + 32)
    base = (-back.data_ptr()) % 16                       # the view starts `mis` bytes behind a 16-byte boundary
    d_buf = back[base + mis:base + mis + host.size]
    d_buf.copy_(ctx.torch.from_numpy(host))
    assert d_buf.data_ptr() % 16 == mis
    return d_buf


def fused(ctx, d_buf, n, p, qn):
    """The queued form from the census's lists: (dna, qual, bad, statistics, FusedQname or None, the census's answer)."""
    cen = ops.ChunkedCensus(ctx, d_buf); cen.chunk(0, d_buf.numel()); cen.end_async()
    fq = None
    if qn:
        fq = ops.FusedQname(ctx, n + 7)
        ops.qname_guess_async(ctx, d_buf, None, fq)
    q = ops.pack_stats_async(ctx, d_buf, None, n + 7, p, fq=fq)
    assert q is not None, 'no fused kernel for this geometry'
    if qn: ops.qname_fused_finish(ctx, fq)
    hs = ops.stats_fetch(ctx, q[3])
    return q, hs, fq, cen.wait()


def check(ctx, host, n, qn, mis=0, qname='exact', guess=None, **dk):
    """`guess`: (decisions, parameters) made from MORE reads of the same stream (what a head guess is); else from these reads.
    qname: 'exact' = both analyses must stand and agree; 'may-decline' = compared when both stand; 'flagged' = the fused pass must raise a flag."""
    from uq_amd import qname_device
    t = ctx.torch
    hls, ref, d, p = decide(host, n, **dk)
    if guess is not None: d, p = guess
    rd, rq, rbad = oracle_c.pack(host, hls, 0, n, d['bases'], d['qualities'], d['N_qual'], d['bits_per_base'], d['bits_per_quality'],
                                 d['variable_read_lengths'], d['dna_bytes_per_row'], d['quality_bytes_per_row'])
    assert rbad is None
    d_buf = device_buffer(ctx, host, mis)
    # what the suite trusts: the indexed plain kernels
    nl = ops.count_lines(ctx, d_buf)
    assert nl == 4 * n
    ls = ops.index_lines(ctx, d_buf, nl)
    dna, qual, bad = ops.pack(ctx, d_buf, ls, 0, n, p)
    assert ops.bad_index(bad) is None
    st = ops.stats_new(ctx)
    ops.stats_accumulate(ctx, st, d_buf, ls, 0, n)
    hp = ops.stats_fetch(ctx, st)
    assert np.array_equal(ctx.to_numpy(dna).reshape(n, -1), rd) and np.array_equal(ctx.to_numpy(qual).reshape(n, -1), rq)
    # the fused form
    q, hs, fq, (nl2, ok) = fused(ctx, d_buf, n, p, qn)
    assert ok and nl2 == nl and not hs.incomplete and ops.bad_index(q[2]) is None
    Cd, Cq = d['dna_bytes_per_row'], d['quality_bytes_per_row']
    assert t.equal(q[0][:n * Cd], dna), 'DNA rows differ from the plain pack kernel'
    assert t.equal(q[1][:n * Cq], qual), 'QUAL rows differ from the plain pack kernel'
    assert np.array_equal(hs.counts, hp.counts) and np.array_equal(hs.counts, ref['counts'])
    assert (hs.len_min, hs.len_max, hs.max_record_bytes) == (hp.len_min, hp.len_max, hp.max_record_bytes) == (ref['len_min'], ref['len_max'], ref['max_record_bytes'])
    assert (hs.bad_plus, hs.bad_len) == (hp.bad_plus, hp.bad_len)
    if qn:
        if qname == 'flagged':
            r = ops.qname_fused_fetch(ctx, fq)
            assert not r.ok or r.flags != 0
            assert qname_device.analyse_fused(ctx, fq, n) is None
            return p
        from uq_amd.qname import QnameError
        got = qname_device.analyse_fused(ctx, fq, n)
        try: want = qname_device.analyse_device(ctx, d_buf, ls, n)
        except QnameError: want = None                     # (a handful of reads may share no separator: the exact passes refuse like the reference)
        if (got is None or want is None) and qname == 'may-decline': return p
        assert got is not None and want is not None, 'a QNAME analysis declined names it is built for'
        assert got[:4] == want[:4]
        for a, b in zip(got[4], want[4]): assert t.equal(a, b), 'a fused QNAME column differs from the exact passes\''
    return p


def fixed150(n, first=0):
    return synth.fastq_array(synth.Spec(S, 150), n, first=first)


COUNTS = ['1', 'R-1', 'R', 'R+1', '4R+1']
FAMILIES = {'150bp': (150, {}, {}), 'var-notricks': ((36, 301), dict(n_rate=1), dict(notricks=True)), 'var-ntrick': ((36, 301), dict(n_rate=1), {})}


@gpu
@pytest.mark.parametrize('qn', [False, True], ids=['plain', 'qname-phase'])
@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('family', list(FAMILIES))
def test_reads_per_launch_around_the_tile(ctx, family, count, qn):
    """Fewer reads than the parser wave has lanes, one tile, several tiles, a last short tile; fixed 150 bp and the variable-length
    instances (36 - 301 bp, 1 % N, with and without the N-trick), which share the tile loop.  (Below 64 reads either QNAME analysis may
    decline -- too few lines to tell a layout -- and the columns are compared when both stand; rows and counts always.)"""
    length, kw, dk = FAMILIES[family]
    spec = synth.Spec(S + 1, length, **kw)
    head = synth.fastq_array(spec, 400)                   # the guess comes from 400 reads, the launch packs the first n of them
    hls, _, d, p = decide(head, 400, **dk)
    R = tile_reads(p)
    assert 8 <= R <= 63
    n = {'1': 1, 'R-1': R - 1, 'R': R, 'R+1': R + 1, '4R+1': 4 * R + 1}[count]
    check(ctx, head[:int(hls[4 * n])].copy(), n, qn, qname='may-decline' if n < 64 else 'exact', guess=(d, p), **dk)


@gpu
@pytest.mark.parametrize('family', list(FAMILIES))
def test_every_workgroup_takes_several_tiles(ctx, family):
    """One launch of ~ 250 000 reads (85 MB at 150 bp): every persistent workgroup of a 256-CU card takes at least two tiles, the software
    pipeline runs its steady state.  Then the same launch with ONE read of the last tiles made
    non-conforming in its QNAME line: the flag must still arrive."""
    length, kw, dk = FAMILIES[family]
    n = 250_000
    spec = synth.Spec(S + 2, length, **kw)
    host = ctx.to_numpy(ops.synth_fastq(ctx, spec, 0, n))
    p = check(ctx, host, n, True, **dk)
    hls = oracle_c.index_lines(host)
    R = tile_reads(p)
    assert (n + R - 1) // R >= 2 * 4 * 256
    bad_read = n - R - 3                                   # in the last tile of the workgroup that owns the last but one tile
    q0 = int(hls[4 * bad_read])
    field = host[q0:int(hls[4 * bad_read + 1])].tobytes()
    digit = max(i for i, c in enumerate(field[:-1]) if 48 <= c <= 57)
    host2 = host.copy(); host2[q0 + digit] = ord('x')      # a letter in a numeric field
    d_buf = ctx.to_device(host2)
    q, hs, fq, (nl, ok) = fused(ctx, d_buf, n, p, True)
    assert ok and nl == 4 * n and not hs.incomplete
    r = ops.qname_fused_fetch(ctx, fq)
    assert r.ok and r.flags != 0, 'a non-conforming QNAME line in a workgroup\'s last tile went unnoticed'
    from uq_amd import qname_device
    assert qname_device.analyse_fused(ctx, fq, n) is None
    plain = fused(ctx, ctx.to_device(host), n, p, False)[0]
    Cd, Cq = p.dna_bytes_per_row, p.quality_bytes_per_row
    assert ctx.torch.equal(q[0][:n * Cd], plain[0][:n * Cd]) and ctx.torch.equal(q[1][:n * Cq], plain[1][:n * Cq]), 'the rows depend on the QNAME lines'


@gpu
@pytest.mark.parametrize('qn', [False, True], ids=['plain', 'qname-phase'])
def test_record_longer_than_the_tile_allows(ctx, qn):
    """Tiles are sized from the average record: three reads with QNAME lines of 7 000 bytes make their tiles' records exceed the stage,
    and those tiles are packed piece by piece (the path that reads what the tile loop parked in LDS) -- the first tile of the launch,
    which no barrier precedes, among them.  The QNAME pass may stand down (lines beyond 255 bytes); rows and counts may not differ."""
    n = 300
    base = fixed150(n)
    hls = oracle_c.index_lines(base)
    parts = []
    for r in range(n):
        rec = base[int(hls[4 * r]):int(hls[4 * r + 4])].tobytes()
        if r in (2, 130, n - 1): rec = rec[:1] + b'L' * 7000 + rec[1:]
        parts.append(rec)
    host = np.frombuffer(b''.join(parts), dtype=np.uint8).copy()
    p = check(ctx, host, n, qn, qname='flagged')
    R = tile_reads(p)
    assert R > 16 and R * (base.size // n) + 7000 > 4 * 256 * 16, 'the long records no longer overflow a tile: the piece path is not run'


@gpu
@pytest.mark.parametrize('mis', [1, 7, 15])
def test_buffer_off_a_16_byte_boundary(ctx, mis):
    """mis != 0: the census's tiles and the pack kernel's 16-byte loads start in front of the buffer's first byte."""
    spec = synth.Spec(S + 3, 150)
    head = synth.fastq_array(spec, 300)
    hls, _, d, p = decide(head, 300)
    n = 4 * tile_reads(p) + 1
    check(ctx, head[:int(hls[4 * n])].copy(), n, True, mis=mis, guess=(d, p))


def test_more_reads_than_32_bits_count_is_refused_without_a_launch():
    """The kernels count reads and tiles in 32 bits: uq_pack refuses more than 2^31 reads in one call before it touches its other
    arguments (no context, no buffers here: nothing can have been queued)."""
    from uq_amd import _lib
    lib = _lib.load()
    assert lib.uq_pack(None, None, None, 0, (1 << 31) + 1, None, None, None, None) != 0
    assert b'reads in one call' in lib.uq_last_error()
    st, fused_flag = C.c_void_p(16), C.c_int(7)
    assert lib.uq_pack_stats(None, None, None, 0, 1 << 32, None, None, None, None, st, C.byref(fused_flag)) != 0
    assert b'reads in one call' in lib.uq_last_error()
