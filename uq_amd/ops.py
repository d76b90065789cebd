"""Thin typed wrappers over the C ABI: torch tensors in, torch tensors out.  One function per
entry point of include/uqhip.h; the reference site each one replaces is cited there."""
import ctypes as C

import numpy as np

from ._lib import call, Stats, PackParams, PackTileGeom, UnpackParams, SynthSpec, GzipStreamInfo, BgzfPart, Fingerprint, MateReport, FilterParams, FilterReport, TrimParams, TrimReport, AdapterParams, AdapterReport, DedupParams, DedupReport, UQ_NONE, load

PATTERN_IDS = {'0.1': 0, '0.2': 1, '1.1': 2, '1.2': 3, '2.1': 4, '2.2': 5, '3.1': 6, '3.2': 7}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# ------------------------------------------------------------------ record index
def count_lines(ctx, buf):
    n = C.c_uint64()
    call('uq_count_lines', ctx.h, _p(buf), buf.numel(), C.byref(n))
    return n.value


class ChunkedCensus:
    """uq_count_lines over a buffer that is still being filled: `chunk(lo, n)` as each piece lands, `end()` = the line count."""

    def __init__(self, ctx, buf):
        self.ctx, self.buf = ctx, buf
        call('uq_count_lines_begin', ctx.h, _p(buf), buf.numel())

    def chunk(self, lo, n):
        call('uq_count_lines_chunk', self.ctx.h, _p(self.buf), self.buf.numel(), int(lo), int(n))

    def end(self):
        out = C.c_uint64()
        call('uq_count_lines_end', self.ctx.h, _p(self.buf), self.buf.numel(), C.byref(out))
        return out.value

    # the queued form: end_async() -> index_lines_async / pack_stats_async (they take the line count on the device) -> wait()
    def end_async(self):
        call('uq_count_lines_end_async', self.ctx.h, _p(self.buf), self.buf.numel())

    def wait(self):
        """(line count, ok): ok False = the index made meanwhile is not usable (list or capacity overflow)."""
        out, ok = C.c_uint64(), C.c_int(0)
        call('uq_count_lines_wait', self.ctx.h, _p(self.buf), self.buf.numel(), C.byref(out), C.byref(ok))
        return out.value, bool(ok.value)


def index_lines(ctx, buf, nlines):
    """int64 tensor [nlines + 1] of line start offsets (bit pattern of uint64)."""
    t = ctx.torch
    ls = t.empty(nlines + 1, dtype=t.int64, device=ctx.device)
    call('uq_index_lines', ctx.h, _p(buf), buf.numel(), nlines, _p(ls))
    return ls


def index_lines_async(ctx, buf, capacity_lines):
    """The record index behind ChunkedCensus.end_async(): int64 tensor [capacity_lines + 1]; entries [0, lines] are written."""
    t = ctx.torch
    ls = t.empty(capacity_lines + 1, dtype=t.int64, device=ctx.device)
    call('uq_index_lines_async', ctx.h, _p(buf), buf.numel(), capacity_lines, _p(ls))
    return ls


# ------------------------------------------------------------------ pass-1 statistics
STATS_DTYPE = np.dtype([('counts', np.uint64, (65536,)), ('bad_plus', np.uint64), ('bad_len', np.uint64), ('len_min', np.uint32),
                        ('len_max', np.uint32), ('max_record_bytes', np.uint32), ('reserved', np.uint32)])    # struct uq_stats
assert STATS_DTYPE.itemsize == C.sizeof(Stats)


STATS_COMPACT_CAP = 2048
STATS_COMPACT_DTYPE = np.dtype([('n', np.uint32), ('len_min', np.uint32), ('len_max', np.uint32), ('max_record_bytes', np.uint32), ('reserved', np.uint32),
                                ('pad', np.uint32), ('bad_plus', np.uint64), ('bad_len', np.uint64), ('key', np.uint32, (STATS_COMPACT_CAP,)),
                                ('count', np.uint64, (STATS_COMPACT_CAP,))])                              # struct uq_stats_compact


class HostStats:
    """Host copy of uq_stats: counts[256][256] + ranges + first bad records.  From uq_stats_fetch_compact it holds the non-zero
    counters as a list (nz_keys = base * 256 + quality, nz_counts) and builds the dense table only when somebody asks for it."""

    def __init__(self, s):
        """`s`: a ctypes `Stats`, a numpy record of STATS_DTYPE (same layout) or one of STATS_COMPACT_DTYPE -- or the one-element array of
        STATS_COMPACT_DTYPE that holds it, which is then kept as it is (no copy)."""
        own = None
        if isinstance(s, np.ndarray) and s.dtype == STATS_COMPACT_DTYPE and s.shape == (1,):
            own, s = s, s[0]
        if isinstance(s, Stats):
            s = np.frombuffer(s, dtype=STATS_DTYPE, count=1)[0]
        self.compact = None                           # the uq_stats_compact itself (a one-element array): what uq_decide_from_stats reads
        self._nz = None
        if 'key' in s.dtype.names:
            self.compact = own
            if self.compact is None:
                self.compact = np.empty(1, dtype=STATS_COMPACT_DTYPE)
                self.compact[0] = s
            self._counts = None
        else:
            self._counts = s['counts'].reshape(256, 256).copy()
        bad_plus, bad_len = int(s['bad_plus']), int(s['bad_len'])
        self.bad_plus = None if bad_plus == UQ_NONE else bad_plus
        self.bad_len = None if bad_len == UQ_NONE else bad_len
        self.len_min, self.len_max = int(s['len_min']), int(s['len_max'])
        self.max_record_bytes = int(s['max_record_bytes'])
        self.incomplete = bool(s['reserved'])         # set by uq_pack_stats only: counts not usable

    def _pairs(self):
        if self._nz is None:
            c = self.compact[0]
            n = int(c['n'])
            self._nz = (c['key'][:n].astype(np.int64), c['count'][:n].astype(np.int64))
        return self._nz

    @property
    def nz_keys(self):
        return None if self.compact is None else self._pairs()[0]

    @property
    def nz_counts(self):
        return None if self.compact is None else self._pairs()[1]

    @property
    def counts(self):
        if self._counts is None:
            c = np.zeros(65536, dtype=np.uint64)
            c[self.nz_keys] = self.nz_counts.astype(np.uint64)
            self._counts = c.reshape(256, 256)
        return self._counts


def stats_new(ctx):
    t = ctx.torch
    d = t.empty(C.sizeof(Stats), dtype=t.uint8, device=ctx.device)
    call('uq_stats_init', ctx.h, _p(d))
    return d


def stats_accumulate(ctx, d_stats, buf, line_start, first_read, nreads):
    call('uq_stats_accumulate', ctx.h, _p(buf), _p(line_start), first_read, nreads, _p(d_stats))


def index_and_stats(ctx, buf, nlines):
    """Record index + pass-1 statistics of the whole buffer (uq_index_lines + uq_stats_accumulate).
    Returns (line_start tensor, device uq_stats)."""
    ls = index_lines(ctx, buf, nlines)
    st = stats_new(ctx)
    if nlines >= 4:
        stats_accumulate(ctx, st, buf, ls, 0, nlines // 4)
    return ls, st


def stats_fetch(ctx, d_stats):
    raw = np.empty(1, dtype=STATS_COMPACT_DTYPE)
    call('uq_stats_fetch_compact', ctx.h, _p(d_stats), C.c_void_p(raw.ctypes.data))
    if int(raw[0]['n']) <= STATS_COMPACT_CAP:
        return HostStats(raw)
    raw = np.empty(1, dtype=STATS_DTYPE)              # more non-zero counters than the list holds: the whole table
    call('uq_stats_fetch', ctx.h, _p(d_stats), C.c_void_p(raw.ctypes.data))
    return HostStats(raw[0])


def stats_export(ctx, d_stats, rank, world, read_offset=0):
    """A device uq_stats as ONE summable buffer (uq_stats_export): int64[65536 + 6 * world] on the device, this rank's scalars in its own
    six slots (bad records made file-wide with read_offset), zeros in the others."""
    t = ctx.torch
    words = t.empty(65536 + 6 * world, dtype=t.int64, device=ctx.device)
    call('uq_stats_export', ctx.h, _p(d_stats), int(rank), int(world), int(read_offset), _p(words))
    return words


def stats_import(ctx, words, world, d_stats):
    """The SUM of every rank's stats_export folded back into d_stats (uq_stats_import)."""
    call('uq_stats_import', ctx.h, _p(words), int(world), _p(d_stats))


def first_occurrence(ctx, buf, line_start, first_read, nreads, index_base=0):
    t = ctx.torch
    d = t.full((256,), -1, dtype=t.int64, device=ctx.device)
    call('uq_first_occurrence', ctx.h, _p(buf), _p(line_start), first_read, nreads, index_base, _p(d))
    return d.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------ the record fingerprint uqfp1 (include/uqhip.h)
FINGERPRINT_FIELDS = tuple(k for k, _ in Fingerprint._fields_)


def fingerprint_new(ctx):
    """A zeroed device uq_fingerprint (int64[9]: the bit patterns of its nine u64 sums)."""
    t = ctx.torch
    d = t.empty(len(FINGERPRINT_FIELDS), dtype=t.int64, device=ctx.device)
    call('uq_fingerprint_init', ctx.h, _p(d))
    return d


def fingerprint_accumulate(ctx, d_fp, buf, line_start, first_read, nreads, index_base=0):
    """Adds the records [first_read, first_read + nreads) of buf into d_fp (queued, nothing read back); record first_read + i counts as the
    global record index_base + i."""
    call('uq_fingerprint_accumulate', ctx.h, _p(buf), _p(line_start), int(first_read), int(nreads), int(index_base), _p(d_fp))


def fingerprint_fetch(ctx, d_fp):
    """The device sums as a dict of Python integers (synchronises)."""
    return dict(zip(FINGERPRINT_FIELDS, (int(v) for v in ctx.to_numpy(d_fp).view(np.uint64))))


def _indexed(ctx, buf, who):
    """(record index, reads) of a FASTQ text in HBM whose caller brought no index: census + uq_index_lines (no reads: no index)."""
    nlines = count_lines(ctx, buf) if buf.numel() else 0
    if nlines % 4: raise ValueError('%s: %d lines are not whole FASTQ records' % (who, nlines))
    return (index_lines(ctx, buf, nlines) if nlines else None), nlines // 4


def fingerprint(ctx, buf, line_start=None, nreads=None):
    """The fingerprint of a FASTQ text in HBM (uint8 tensor); without an index it is built here (census + uq_index_lines)."""
    if line_start is None: line_start, nreads = _indexed(ctx, buf, 'fingerprint')
    d = fingerprint_new(ctx)
    if nreads: fingerprint_accumulate(ctx, d, buf, line_start, 0, nreads)
    return fingerprint_fetch(ctx, d)


def host_line_starts(data):
    """What uq_index_lines writes, for host bytes: uint64[lines + 1]."""
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    return np.concatenate(([0], np.flatnonzero(a == 10) + 1)).astype(np.uint64)


def _host_indexed(data, line_start):
    """A host twin's text and index as it passes them on: (contiguous uint8 array, contiguous uint64 line starts -- the caller's, or made here)."""
    a = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data)
    return a, np.ascontiguousarray(host_line_starts(a) if line_start is None else line_start, dtype=np.uint64)


def _host_records(data, line_start, first_read, nreads, who):
    """_host_indexed and the records [first_read, first_read + nreads) checked against the index (nreads None: all from first_read on, of
    a text of whole records) -> (bytes, line starts, nreads)."""
    a, ls = _host_indexed(data, line_start)
    if nreads is None:
        if (len(ls) - 1) % 4: raise ValueError('%s: %d lines are not whole FASTQ records' % (who, len(ls) - 1))
        nreads = (len(ls) - 1) // 4 - first_read
    if first_read < 0 or nreads < 0 or 4 * (first_read + nreads) + 1 > len(ls): raise ValueError('%s: records beyond the index' % who)
    return a, ls, nreads


def fingerprint_host(data, line_start=None, first_read=0, nreads=None, index_base=0):
    """uq_fingerprint_host: the same sums on the CPU, sequentially, over host bytes (needs no GPU)."""
    a, ls, nreads = _host_records(data, line_start, first_read, nreads, 'fingerprint')
    fp = Fingerprint()
    call('uq_fingerprint_host', C.c_void_p(a.ctypes.data if a.size else 0), C.c_void_p(ls.ctypes.data), int(first_read), int(nreads),
         int(index_base), C.byref(fp))
    return {k: int(getattr(fp, k)) for k in FINGERPRINT_FIELDS}


def fingerprint_json(fp):
    """The one line --fingerprint prints: counts as numbers, the six sums as 16 hex digits."""
    import json
    d = {'uqfp': 1}
    for i, k in enumerate(FINGERPRINT_FIELDS): d[k] = fp[k] if i < 3 else '%016x' % fp[k]
    return json.dumps(d)


# ------------------------------------------------------------------ the per-cycle tables uqqc1 (include/uqhip.h)
QC_MAX_CYCLES, QC_NBASE, QC_NQUAL, QC_NGC = 1024, 6, 94, 101
QC_SCALARS = ('reads', 'bases', 'qual_chars', 'qual_out_of_range', 'len_mismatch')


def qc_words(ncycles):
    """uq_qc_words: the number of u64 words of the object for ncycles exact cycles."""
    n = int(ncycles)
    if not 1 <= n <= QC_MAX_CYCLES: raise ValueError('qc: ncycles = %d is outside 1 .. %d' % (n, QC_MAX_CYCLES))
    return int(load().uq_qc_words(n))


def qc_new(ctx, ncycles=QC_MAX_CYCLES):
    """A zeroed device uqqc1 object (int64[uq_qc_words]: the bit patterns of its u64 counters)."""
    t = ctx.torch
    d = t.empty(qc_words(ncycles), dtype=t.int64, device=ctx.device)
    call('uq_qc_init', ctx.h, _p(d), int(ncycles))
    return d


def qc_accumulate(ctx, d_qc, buf, line_start, first_read, nreads, ncycles=QC_MAX_CYCLES):
    """Adds the records [first_read, first_read + nreads) of buf into d_qc (queued, nothing read back)."""
    if d_qc.numel() != qc_words(ncycles): raise ValueError('qc: the object holds %d words, ncycles = %d needs %d' % (d_qc.numel(), ncycles, qc_words(ncycles)))
    call('uq_qc_accumulate', ctx.h, _p(buf), _p(line_start), int(first_read), int(nreads), int(ncycles), _p(d_qc))


def qc_fetch(ctx, d_qc):
    """The device object as a flat uint64 array (synchronises)."""
    return ctx.to_numpy(d_qc).view(np.uint64).copy()


def qc(ctx, buf, line_start=None, nreads=None, ncycles=QC_MAX_CYCLES):
    """The uqqc1 object of a FASTQ text in HBM (uint8 tensor); without an index it is built here (census + uq_index_lines)."""
    if line_start is None: line_start, nreads = _indexed(ctx, buf, 'qc')
    d = qc_new(ctx, ncycles)
    if nreads: qc_accumulate(ctx, d, buf, line_start, 0, nreads, ncycles)
    return qc_fetch(ctx, d)


def qc_host(data, ncycles=QC_MAX_CYCLES, line_start=None, first_read=0, nreads=None):
    """uq_qc_host: the same object on the CPU, sequentially, over host bytes (needs no GPU)."""
    a, ls, nreads = _host_records(data, line_start, first_read, nreads, 'qc')
    out = np.zeros(qc_words(ncycles), dtype=np.uint64)
    call('uq_qc_host', C.c_void_p(a.ctypes.data if a.size else 0), C.c_void_p(ls.ctypes.data), int(first_read), int(nreads), int(ncycles),
         C.c_void_p(out.ctypes.data))
    return out


def qc_cycles(flat):
    """The number of exact cycles of a flat uqqc1 array, from its length."""
    c, r = divmod(len(flat) - 8 - QC_NQUAL - QC_NGC, QC_NBASE + QC_NQUAL + 1)
    if r or not 1 <= c - 1 <= QC_MAX_CYCLES: raise ValueError('qc: %d words are no uqqc1 object' % len(flat))
    return c - 1


def qc_fields(flat):
    """A flat uqqc1 array as a dict of its parts: the scalars as integers, the tables as uint64 views of `flat`."""
    flat = np.asarray(flat, dtype=np.uint64)
    c = qc_cycles(flat)
    d = {k: int(flat[i]) for i, k in enumerate(QC_SCALARS)}
    o = 8
    for name, rows, cols in (('base_by_cycle', c + 1, QC_NBASE), ('qual_by_cycle', c + 1, QC_NQUAL), ('length_hist', c + 1, 0),
                             ('mean_qual_hist', QC_NQUAL, 0), ('gc_hist', QC_NGC, 0)):
        n = rows * max(cols, 1)
        d[name] = flat[o:o + n].reshape(rows, cols) if cols else flat[o:o + n]
        o += n
    return d


def qc_json(flat):
    """The one line --qc prints.  Plain integers throughout.  The per-cycle tables and length_hist are cut after their last non-zero exact
    cycle and qual_by_cycle's rows after the highest Phred value in use; the tail row (positions and lengths >= cycles) stands under
    "beyond".  qc_from_json gives the flat array back exactly."""
    import json
    f = qc_fields(flat)
    c = qc_cycles(flat)
    base, qual, length = f['base_by_cycle'], f['qual_by_cycle'], f['length_hist']

    def used(rows):
        nz = np.flatnonzero(rows.reshape(len(rows), -1).any(axis=1))
        return int(nz[-1]) + 1 if len(nz) else 0

    nq = used(qual.T)
    d = {'format': 'uqqc1', 'cycles': c}
    for k in QC_SCALARS: d[k] = f[k]
    d['base_classes'] = 'ACGTN*'
    d['base_by_cycle'] = base[:used(base[:c])].tolist()
    d['qual_by_cycle'] = qual[:used(qual[:c]), :nq].tolist()
    d['length_hist'] = length[:used(length[:c])].tolist()
    d['beyond'] = {'base': base[c].tolist(), 'qual': qual[c, :nq].tolist(), 'length': int(length[c])}
    d['mean_qual_hist'] = f['mean_qual_hist'].tolist()
    d['gc_hist'] = f['gc_hist'].tolist()
    return json.dumps(d)


def qc_from_json(line):
    """The flat uqqc1 array of a line qc_json wrote."""
    import json
    d = json.loads(line)
    if d.get('format') != 'uqqc1': raise ValueError('qc: not a uqqc1 line')
    c = int(d['cycles'])
    flat = np.zeros(qc_words(c), dtype=np.uint64)
    f = qc_fields(flat)
    for i, k in enumerate(QC_SCALARS): flat[i] = int(d[k])
    for i, row in enumerate(d['base_by_cycle']): f['base_by_cycle'][i, :len(row)] = row
    for i, row in enumerate(d['qual_by_cycle']): f['qual_by_cycle'][i, :len(row)] = row
    f['length_hist'][:len(d['length_hist'])] = d['length_hist']
    f['base_by_cycle'][c, :] = d['beyond']['base']
    f['qual_by_cycle'][c, :len(d['beyond']['qual'])] = d['beyond']['qual']
    f['length_hist'][c] = int(d['beyond']['length'])
    f['mean_qual_hist'][:] = d['mean_qual_hist']
    f['gc_hist'][:] = d['gc_hist']
    return flat


# ------------------------------------------------------------------ quality binning (include/uqhip.h)
def _lut_arg(lut):
    a = np.ascontiguousarray(np.frombuffer(bytes(lut), dtype=np.uint8))
    if a.size != 256: raise ValueError('a quality table has 256 entries, not %d' % a.size)
    return a


def changed_new(ctx):
    """A zeroed device u64 (int64[1]) for uq_requantise_qualities to add its count of changed bytes to."""
    t = ctx.torch
    return t.zeros(1, dtype=t.int64, device=ctx.device)


def requantise_qualities(ctx, buf, line_start, first_read, nreads, lut, d_changed=None):
    """lut[] applied in place to the quality lines of the records [first_read, first_read + nreads) of buf (queued, nothing read back); the
    number of bytes that changed is added to d_changed (changed_new) when given."""
    a = _lut_arg(lut)
    call('uq_requantise_qualities', ctx.h, _p(buf), _p(line_start), int(first_read), int(nreads), C.c_void_p(a.ctypes.data), _p(d_changed))


def requantise_qualities_host(data, lut, line_start=None, first_read=0, nreads=None):
    """uq_requantise_qualities_host: the same on the CPU over host bytes (needs no GPU).  Returns (a new uint8 array, bytes changed)."""
    out, ls, nreads = _host_records(data, line_start, first_read, nreads, 'requantise')
    out = np.array(out, dtype=np.uint8, order='C')      # (a copy: the caller's text stays as it is)
    a, changed = _lut_arg(lut), C.c_uint64(0)
    call('uq_requantise_qualities_host', C.c_void_p(out.ctypes.data if out.size else 0), C.c_void_p(ls.ctypes.data), int(first_read), int(nreads),
         C.c_void_p(a.ctypes.data), C.byref(changed))
    return out, changed.value


# ------------------------------------------------------------------ paired-end input (include/uqhip.h)
MATE_REPORT_FIELDS = tuple(k for k, _ in MateReport._fields_)


def interleaved_size(ctx, ls_a, ls_b, first_pair, npairs):
    """The bytes uq_interleave_records writes for these pairs (four record starts brought down)."""
    if npairs == 0: return 0
    ends = [int(ctx.to_numpy(ls[4 * k:4 * k + 1], np.uint64)[0]) for ls in (ls_a, ls_b) for k in (first_pair, first_pair + npairs)]
    return (ends[1] - ends[0]) + (ends[3] - ends[2])


def interleave_records(ctx, buf_a, ls_a, buf_b, ls_b, first_pair, npairs, out=None, out_capacity=None):
    """Records first_pair .. first_pair + npairs of buf_a and buf_b, alternating, from byte 0 of `out` on (queued; a new uint8 tensor of
    exactly the size when `out` is None).  out_capacity: what the library is told `out` holds (its numel by default)."""
    if out is None:
        out = ctx.empty(interleaved_size(ctx, ls_a, ls_b, first_pair, npairs))
    call('uq_interleave_records', ctx.h, _p(buf_a), _p(ls_a), _p(buf_b), _p(ls_b), int(first_pair), int(npairs), _p(out),
         int(out.numel() if out_capacity is None else out_capacity))
    return out


def interleave_records_host(a, b, ls_a=None, ls_b=None, first_pair=0, npairs=None):
    """uq_interleave_records_host: the same on the CPU over host bytes (needs no GPU).  Returns a new uint8 array."""
    if npairs is None:
        (a, ls_a), (b, ls_b) = _host_indexed(a, ls_a), _host_indexed(b, ls_b)
        if (len(ls_a) - 1) % 4 or len(ls_a) != len(ls_b): raise ValueError('interleave: the two texts are not the same number of whole FASTQ records')
        npairs = (len(ls_a) - 1) // 4 - first_pair
    a, ls_a, _ = _host_records(a, ls_a, first_pair, npairs, 'interleave')
    b, ls_b, _ = _host_records(b, ls_b, first_pair, npairs, 'interleave')
    size = 0 if npairs == 0 else int(ls_a[4 * (first_pair + npairs)] - ls_a[4 * first_pair]) + int(ls_b[4 * (first_pair + npairs)] - ls_b[4 * first_pair])
    out = np.empty(size, dtype=np.uint8)
    call('uq_interleave_records_host', C.c_void_p(a.ctypes.data if a.size else 0), C.c_void_p(ls_a.ctypes.data), C.c_void_p(b.ctypes.data if b.size else 0),
         C.c_void_p(ls_b.ctypes.data), int(first_pair), int(npairs), C.c_void_p(out.ctypes.data if out.size else 0), size)
    return out


def mate_report_new(ctx):
    """A device uq_mate_report (int64[4]) with its counts at 0 and first_mismatch at UINT64_MAX."""
    t = ctx.torch
    d = t.empty(len(MATE_REPORT_FIELDS), dtype=t.int64, device=ctx.device)
    call('uq_mate_report_init', ctx.h, _p(d))
    return d


def mate_check(ctx, d_report, buf_a, ls_a, first_a, step_a, buf_b, ls_b, first_b, step_b, npairs, pair_index_base=0):
    """Adds the pairs (record first_a + i step_a of buf_a, record first_b + i step_b of buf_b), i < npairs, into d_report (queued)."""
    call('uq_mate_check', ctx.h, _p(buf_a), _p(ls_a), int(first_a), int(step_a), _p(buf_b), _p(ls_b), int(first_b), int(step_b), int(npairs),
         int(pair_index_base), _p(d_report))


def mate_report_fetch(ctx, d_report):
    """The device report as a dict of Python integers (synchronises); first_mismatch is None when every pair matched."""
    d = dict(zip(MATE_REPORT_FIELDS, (int(v) for v in ctx.to_numpy(d_report).view(np.uint64))))
    if d['first_mismatch'] == UQ_NONE: d['first_mismatch'] = None
    return d


def mate_check_host(a, b, first_a=0, step_a=1, first_b=0, step_b=1, npairs=None, pair_index_base=0, ls_a=None, ls_b=None, report=None):
    """uq_mate_check_host: the same on the CPU over host bytes (needs no GPU); `report`: a dict of an earlier call to add to."""
    (a, ls_a), (b, ls_b) = _host_indexed(a, ls_a), _host_indexed(b, ls_b)      # (the pairs its strides reach: the arithmetic below is its own)
    if npairs is None: npairs = min(((len(ls_a) - 1) // 4 - first_a + step_a - 1) // step_a, ((len(ls_b) - 1) // 4 - first_b + step_b - 1) // step_b)
    if npairs < 0 or first_a < 0 or first_b < 0 or step_a < 0 or step_b < 0: raise ValueError('mate check: negative argument')
    if npairs and (4 * (first_a + (npairs - 1) * step_a) + 5 > len(ls_a) or 4 * (first_b + (npairs - 1) * step_b) + 5 > len(ls_b)):
        raise ValueError('mate check: records beyond the index')
    r = MateReport(0, 0, UQ_NONE, 0)
    if report is not None:
        r = MateReport(report['pairs'], report['mismatches'], UQ_NONE if report['first_mismatch'] is None else report['first_mismatch'], report['slash_pairs'])
    call('uq_mate_check_host', C.c_void_p(a.ctypes.data if a.size else 0), C.c_void_p(ls_a.ctypes.data), int(first_a), int(step_a),
         C.c_void_p(b.ctypes.data if b.size else 0), C.c_void_p(ls_b.ctypes.data), int(first_b), int(step_b), int(npairs), int(pair_index_base), C.byref(r))
    d = {k: int(getattr(r, k)) for k in MATE_REPORT_FIELDS}
    if d['first_mismatch'] == UQ_NONE: d['first_mismatch'] = None
    return d


# ------------------------------------------------------------------ read filtering (include/uqhip.h)
FILTER_REPORT_FIELDS = tuple(k for k, _ in FilterReport._fields_)
FILTER_SAMPLE = 1
FILTER_OFF = {'min_len': 0, 'max_len': 0xFFFFFFFF, 'max_n': 0xFFFFFFFF, 'min_mean_q': 0, 'sample_threshold': 0, 'seed': 0, 'flags': 0}


def filter_params(unit=1, **criteria):
    """A uq_filter_params: every criterion off but the ones given (min_len, max_len, max_n, min_mean_q; sample_threshold + seed + flags)."""
    unknown = set(criteria) - set(FILTER_OFF)
    if unknown: raise ValueError('filter: unknown criteria %s' % sorted(unknown))
    d = dict(FILTER_OFF, **criteria)
    return FilterParams(d['min_len'], d['max_len'], d['max_n'], d['min_mean_q'], d['sample_threshold'], d['seed'], unit, d['flags'])


def filter_report_new(ctx):
    """A zeroed device uq_filter_report (int64[12])."""
    t = ctx.torch
    d = t.empty(len(FILTER_REPORT_FIELDS), dtype=t.int64, device=ctx.device)
    call('uq_filter_report_init', ctx.h, _p(d))
    return d


def filter_report_fetch(ctx, d_report):
    """The device report as a dict of Python integers (synchronises)."""
    return dict(zip(FILTER_REPORT_FIELDS, (int(v) for v in ctx.to_numpy(d_report).view(np.uint64))))


def filter_mark(ctx, d_report, buf, line_start, first_read, nreads, params, index_base=0, verdict=None):
    """The verdict bytes of the records [first_read, first_read + nreads) of buf (a new uint8 tensor when `verdict` is None), their counts
    added into d_report (queued, nothing read back)."""
    if verdict is None: verdict = ctx.empty(nreads)
    call('uq_filter_mark', ctx.h, _p(buf), _p(line_start), int(first_read), int(nreads), int(index_base), C.byref(params), _p(verdict), _p(d_report))
    return verdict


def filter_plan(ctx, d_report, line_start, first_read, nreads, unit, verdict):
    """The kept units of the records as (src, dst, kept units, output bytes): src[j] / dst[j] the unit's offsets in the source and in the
    output, dst[kept] the output's size (int64 tensors holding u64 of nreads / unit and one more entries; synchronises)."""
    t = ctx.torch
    src = t.empty(nreads // unit, dtype=t.int64, device=ctx.device)
    dst = t.empty(nreads // unit + 1, dtype=t.int64, device=ctx.device)
    kept, size = C.c_uint64(0), C.c_uint64(0)
    call('uq_filter_plan', ctx.h, _p(line_start), int(first_read), int(nreads), int(unit), _p(verdict), _p(src), _p(dst), _p(d_report),
         C.byref(kept), C.byref(size))
    return src, dst, kept.value, size.value


def compact_records(ctx, buf, src, dst, kept_units, out=None, out_capacity=None, out_bytes=None):
    """The kept units of buf back to back from byte 0 of `out` on (queued; a new uint8 tensor of out_bytes when `out` is None).
    out_capacity: what the library is told `out` holds (its numel by default)."""
    if out is None: out = ctx.empty(out_bytes)
    call('uq_compact_records', ctx.h, _p(buf), int(buf.numel()), _p(src), _p(dst), int(kept_units), _p(out),
         int(out.numel() if out_capacity is None else out_capacity))
    return out


def filter_mark_host(data, params, line_start=None, first_read=0, nreads=None, index_base=0, report=None):
    """uq_filter_mark_host: the same on the CPU over host bytes (needs no GPU) -> (uint8 verdicts, report dict; `report`: an earlier one to add to)."""
    a, ls, nreads = _host_records(data, line_start, first_read, nreads, 'filter')
    r = FilterReport(*[report[k] for k in FILTER_REPORT_FIELDS]) if report is not None else FilterReport()
    verdict = np.empty(nreads, dtype=np.uint8)
    call('uq_filter_mark_host', C.c_void_p(a.ctypes.data if a.size else 0), C.c_void_p(ls.ctypes.data), int(first_read), int(nreads), int(index_base),
         C.byref(params), C.c_void_p(verdict.ctypes.data if nreads else 0), C.byref(r))
    return verdict, {k: int(getattr(r, k)) for k in FILTER_REPORT_FIELDS}


def filter_plan_host(line_start, verdict, unit=1, first_read=0, report=None):
    """uq_filter_plan_host -> (src, dst, kept units, output bytes, report dict); src / dst are uint64 arrays cut to kept and kept + 1 entries."""
    ls = np.ascontiguousarray(line_start, dtype=np.uint64)
    verdict = np.ascontiguousarray(verdict, dtype=np.uint8)
    nreads = len(verdict)
    if first_read < 0 or 4 * (first_read + nreads) + 1 > len(ls): raise ValueError('filter: records beyond the index')
    r = FilterReport(*[report[k] for k in FILTER_REPORT_FIELDS]) if report is not None else FilterReport()
    src, dst = np.zeros(nreads // unit if unit in (1, 2) else 0, dtype=np.uint64), np.zeros((nreads // unit if unit in (1, 2) else 0) + 1, dtype=np.uint64)
    kept, size = C.c_uint64(0), C.c_uint64(0)
    call('uq_filter_plan_host', C.c_void_p(ls.ctypes.data), int(first_read), int(nreads), int(unit), C.c_void_p(verdict.ctypes.data if nreads else 0),
         C.c_void_p(src.ctypes.data if src.size else 0), C.c_void_p(dst.ctypes.data), C.byref(r), C.byref(kept), C.byref(size))
    return src[:kept.value], dst[:kept.value + 1], kept.value, size.value, {k: int(getattr(r, k)) for k in FILTER_REPORT_FIELDS}


def compact_records_host(data, src, dst, kept_units, out_capacity=None):
    """uq_compact_records_host: the kept units of host bytes as a new uint8 array (needs no GPU)."""
    a = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data)
    src, dst = np.ascontiguousarray(src, dtype=np.uint64), np.ascontiguousarray(dst, dtype=np.uint64)
    size = int(dst[kept_units]) if kept_units else 0
    out = np.empty(size, dtype=np.uint8)
    call('uq_compact_records_host', C.c_void_p(a.ctypes.data if a.size else 0), int(a.size), C.c_void_p(src.ctypes.data if src.size else 0),
         C.c_void_p(dst.ctypes.data), int(kept_units), C.c_void_p(out.ctypes.data if out.size else 0), size if out_capacity is None else int(out_capacity))
    return out


# ------------------------------------------------------------------ duplicate removal (include/uqhip.h)
DEDUP_REPORT_FIELDS = tuple(k for k, _ in DedupReport._fields_)
DEDUP_BEST = 1


def dedup_params(unit=1, prefix=0, hash_bits=64, flags=0, seed=0):
    """A uq_dedup_params: whole sequence lines, the full hash, the first of a class kept, seed 0 -- unless told otherwise."""
    return DedupParams(unit, prefix, hash_bits, flags, seed)


def dedup_report_new(ctx):
    """A zeroed device uq_dedup_report (int64[8])."""
    t = ctx.torch
    d = t.empty(len(DEDUP_REPORT_FIELDS), dtype=t.int64, device=ctx.device)
    call('uq_dedup_report_init', ctx.h, _p(d))
    return d


def dedup_report_fetch(ctx, d_report):
    """The device report as a dict of Python integers (synchronises)."""
    return dict(zip(DEDUP_REPORT_FIELDS, (int(v) for v in ctx.to_numpy(d_report).view(np.uint64))))


def dedup_keys(ctx, d_report, buf, line_start, first_read, nreads, params, index_base=0, keys=None):
    """The 16-byte key rows of the units of the records [first_read, first_read + nreads) of buf (a new uint8 tensor when `keys` is None),
    their counts added into d_report (queued, nothing read back)."""
    if keys is None: keys = ctx.empty(16 * (nreads // params.unit if params.unit in (1, 2) else nreads))
    call('uq_dedup_keys', ctx.h, _p(buf), _p(line_start), int(first_read), int(nreads), int(index_base), C.byref(params), _p(keys), _p(d_report))
    return keys


def dedup_mark(ctx, d_report, buf, line_start, first_read, nreads, params, keys, perm, index_base=0, verdict=None):
    """The verdict bytes (1 = duplicate) of those records from their keys and the keys' sorted order (a new uint8 tensor when `verdict` is
    None), the counts added into d_report (queued, nothing read back)."""
    if verdict is None: verdict = ctx.empty(nreads)
    call('uq_dedup_mark', ctx.h, _p(buf), _p(line_start), int(first_read), int(nreads), int(index_base), C.byref(params), _p(keys), _p(perm),
         _p(verdict), _p(d_report))
    return verdict


def _dedup_report_in(report):
    return DedupReport(*[report[k] for k in DEDUP_REPORT_FIELDS]) if report is not None else DedupReport()


def dedup_keys_host(data, params, line_start=None, first_read=0, nreads=None, index_base=0, report=None):
    """uq_dedup_keys_host: the same on the CPU over host bytes (needs no GPU) -> (uint8 keys [units, 16], report dict; `report`: an earlier one to add to)."""
    a, ls, nreads = _host_records(data, line_start, first_read, nreads, 'dedup')
    r = _dedup_report_in(report)
    keys = np.zeros((nreads // params.unit if params.unit in (1, 2) else nreads, 16), dtype=np.uint8)
    call('uq_dedup_keys_host', C.c_void_p(a.ctypes.data if a.size else 0), C.c_void_p(ls.ctypes.data), int(first_read), int(nreads), int(index_base),
         C.byref(params), C.c_void_p(keys.ctypes.data if keys.size else 0), C.byref(r))
    return keys, {k: int(getattr(r, k)) for k in DEDUP_REPORT_FIELDS}


def dedup_order_host(keys):
    """The memcmp-ascending order of host key rows, as uq_argsort_rows gives it on the device (uint32)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 16)
    return np.argsort(keys.view('V16').ravel(), kind='stable').astype(np.uint32)


def dedup_mark_host(data, params, keys, perm, line_start=None, first_read=0, nreads=None, index_base=0, report=None):
    """uq_dedup_mark_host -> (uint8 verdicts, report dict)."""
    a, ls, nreads = _host_records(data, line_start, first_read, nreads, 'dedup')
    r = _dedup_report_in(report)
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    perm = np.ascontiguousarray(perm, dtype=np.uint32)
    verdict = np.full(nreads, 0xEE, dtype=np.uint8)
    call('uq_dedup_mark_host', C.c_void_p(a.ctypes.data if a.size else 0), C.c_void_p(ls.ctypes.data), int(first_read), int(nreads), int(index_base),
         C.byref(params), C.c_void_p(keys.ctypes.data if keys.size else 0), C.c_void_p(perm.ctypes.data if perm.size else 0),
         C.c_void_p(verdict.ctypes.data if nreads else 0), C.byref(r))
    return verdict, {k: int(getattr(r, k)) for k in DEDUP_REPORT_FIELDS}


DEDUP_SEEDS = 8


def dedup_verdicts(run_seed):
    """The driver loop of --dedup: run_seed(seed) -> (verdict, report) of one keys / sort / mark round; while the round's hashes collided it is
    repeated with seed + 1.  -> (verdict, report, the seed that held); DEDUP_SEEDS collisions in a row are a UqError."""
    from .errors import UqError
    for seed in range(DEDUP_SEEDS):
        verdict, report = run_seed(seed)
        if report['collisions'] == 0: return verdict, report, seed
    raise UqError('ERROR: --dedup: %d hash seeds in a row collided' % DEDUP_SEEDS)


# ------------------------------------------------------------------ read trimming (include/uqhip.h)
TRIM_REPORT_FIELDS = tuple(k for k, _ in TrimReport._fields_)
TRIM_N = 1
TRIM_OFF = {'head': 0, 'tail': 0, 'crop': 0xFFFFFFFF, 'polyg': 0, 'q5': 0, 'q3': 0, 'flags': 0}


def trim_params(**steps):
    """A uq_trim_params: every step off but the ones given (head, tail, crop, polyg, q5, q3, flags)."""
    unknown = set(steps) - set(TRIM_OFF)
    if unknown: raise ValueError('trim: unknown steps %s' % sorted(unknown))
    d = dict(TRIM_OFF, **steps)
    return TrimParams(d['head'], d['tail'], d['crop'], d['polyg'], d['q5'], d['q3'], d['flags'], 0)


def trim_report_new(ctx):
    """A zeroed device uq_trim_report (int64[13])."""
    t = ctx.torch
    d = t.empty(len(TRIM_REPORT_FIELDS), dtype=t.int64, device=ctx.device)
    call('uq_trim_report_init', ctx.h, _p(d))
    return d


def trim_report_fetch(ctx, d_report):
    """The device report as a dict of Python integers (synchronises)."""
    return dict(zip(TRIM_REPORT_FIELDS, (int(v) for v in ctx.to_numpy(d_report).view(np.uint64))))


def trim_mark(ctx, d_report, buf, line_start, first_read, nreads, params, window=None):
    """The windows (a, b) of the records [first_read, first_read + nreads) of buf (a new int32 tensor of 2 nreads u32 when `window` is None),
    their counts added into d_report (queued, nothing read back)."""
    t = ctx.torch
    if window is None: window = t.empty(2 * nreads, dtype=t.int32, device=ctx.device)
    call('uq_trim_mark', ctx.h, _p(buf), _p(line_start), int(first_read), int(nreads), C.byref(params), _p(window), _p(d_report))
    return window


def trim_plan(ctx, line_start, first_read, nreads, window, dst=None):
    """(dst, output bytes): dst[i] the output offset of record first_read + i, dst[nreads] the output's size (an int64 tensor holding u64;
    synchronises)."""
    t = ctx.torch
    if dst is None: dst = t.empty(nreads + 1, dtype=t.int64, device=ctx.device)
    size = C.c_uint64(0)
    call('uq_trim_plan', ctx.h, _p(line_start), int(first_read), int(nreads), _p(window), _p(dst), C.byref(size))
    return dst, size.value


def trim_records(ctx, buf, line_start, first_read, nreads, window, dst, out=None, out_capacity=None, out_bytes=None, index=False, line_start_out=None):
    """The trimmed records back to back from byte 0 of `out` on (queued; a new uint8 tensor of out_bytes when `out` is None).  index=True: also the
    record index of the trimmed text (int64[4 nreads + 1]) -> (out, index).  out_capacity: what the library is told `out` holds."""
    t = ctx.torch
    if out is None: out = ctx.empty(out_bytes)
    if index and line_start_out is None: line_start_out = t.empty(4 * nreads + 1, dtype=t.int64, device=ctx.device)
    call('uq_trim_records', ctx.h, _p(buf), int(buf.numel()), _p(line_start), int(first_read), int(nreads), _p(window), _p(dst), _p(out),
         int(out.numel() if out_capacity is None else out_capacity), _p(line_start_out))
    return (out, line_start_out) if index else out


def trim_mark_host(data, params, line_start=None, first_read=0, nreads=None, report=None):
    """uq_trim_mark_host: the same on the CPU over host bytes (needs no GPU) -> (uint32[nreads, 2] windows, report dict; `report`: an earlier
    one to add to)."""
    a, ls, nreads = _host_records(data, line_start, first_read, nreads, 'trim')
    r = TrimReport(*[report[k] for k in TRIM_REPORT_FIELDS]) if report is not None else TrimReport()
    window = np.zeros((nreads, 2), dtype=np.uint32)
    call('uq_trim_mark_host', C.c_void_p(a.ctypes.data if a.size else 0), C.c_void_p(ls.ctypes.data), int(first_read), int(nreads),
         C.byref(params), C.c_void_p(window.ctypes.data if nreads else 0), C.byref(r))
    return window, {k: int(getattr(r, k)) for k in TRIM_REPORT_FIELDS}


def trim_plan_host(line_start, window, first_read=0):
    """uq_trim_plan_host -> (dst uint64[nreads + 1], output bytes)."""
    ls = np.ascontiguousarray(line_start, dtype=np.uint64)
    window = np.ascontiguousarray(window, dtype=np.uint32).reshape(-1, 2)
    nreads = len(window)
    if first_read < 0 or 4 * (first_read + nreads) + 1 > len(ls): raise ValueError('trim: records beyond the index')
    dst = np.zeros(nreads + 1, dtype=np.uint64)
    size = C.c_uint64(0)
    call('uq_trim_plan_host', C.c_void_p(ls.ctypes.data), int(first_read), int(nreads), C.c_void_p(window.ctypes.data if nreads else 0),
         C.c_void_p(dst.ctypes.data), C.byref(size))
    return dst, size.value


def trim_records_host(data, line_start, window, dst, first_read=0, out_capacity=None, index=False):
    """uq_trim_records_host: the trimmed records of host bytes as a new uint8 array (needs no GPU); index=True: -> (array, its record index)."""
    a, ls = _host_indexed(data, line_start)
    window = np.ascontiguousarray(window, dtype=np.uint32).reshape(-1, 2)
    dst = np.ascontiguousarray(dst, dtype=np.uint64)
    nreads = len(window)
    if first_read < 0 or 4 * (first_read + nreads) + 1 > len(ls) or len(dst) != nreads + 1: raise ValueError('trim: records beyond the index')
    size = int(dst[nreads])
    out = np.empty(size, dtype=np.uint8)
    lso = np.zeros(4 * nreads + 1, dtype=np.uint64) if index else None
    call('uq_trim_records_host', C.c_void_p(a.ctypes.data if a.size else 0), int(a.size), C.c_void_p(ls.ctypes.data), int(first_read), int(nreads),
         C.c_void_p(window.ctypes.data if nreads else 0), C.c_void_p(dst.ctypes.data), C.c_void_p(out.ctypes.data if out.size else 0),
         size if out_capacity is None else int(out_capacity), C.c_void_p(lso.ctypes.data) if index else C.c_void_p(0))
    return (out, lso) if index else out


# ------------------------------------------------------------------ 3' adapters (include/uqhip.h)
ADAPTER_REPORT_FIELDS = tuple(k for k, _ in AdapterReport._fields_)
ADAPTER_MAX = 64
ADAPTER_FRESH = 1
ADAPTER_PAIRED = 2
_ADAPTER_CLASS = {'A': 0, 'C': 1, 'G': 2, 'T': 3}


def _adapter_classes(seq, what):
    """A sequence as the library takes it: classes 0..3.  Letters of either case, or integers handed through as they are (the tests' way to
    reach the library's own checks)."""
    if isinstance(seq, str):
        try: return [_ADAPTER_CLASS[c] for c in seq.upper()]
        except KeyError: raise ValueError('adapter: %s %r holds letters other than A, C, G, T' % (what, seq))
    return [int(c) for c in seq]


def adapter_params(seq, seq2=None, err=10, overlap=3, flags=0, len1=None, len2=None, reserved=(0, 0, 0)):
    """A uq_adapter_params.  seq / seq2: letters or classes (at most 64 are stored); len1 / len2 override the lengths."""
    p = AdapterParams()
    for name, s, n in (('seq1', seq, len1), ('seq2', seq2, len2)):
        cls = _adapter_classes(s, name) if s is not None else []
        for j, c in enumerate(cls[:ADAPTER_MAX]): getattr(p, name)[j] = c
        setattr(p, 'len1' if name == 'seq1' else 'len2', len(cls) if n is None else int(n))
    p.overlap, p.err_pct, p.flags = int(overlap), int(err), int(flags)
    for j in range(3): p.reserved[j] = int(reserved[j])
    return p


def adapter_report_new(ctx):
    """A zeroed device uq_adapter_report (int64[9])."""
    t = ctx.torch
    d = t.empty(len(ADAPTER_REPORT_FIELDS), dtype=t.int64, device=ctx.device)
    call('uq_adapter_report_init', ctx.h, _p(d))
    return d


def adapter_report_fetch(ctx, d_report):
    """The device report as a dict of Python integers (synchronises)."""
    return dict(zip(ADAPTER_REPORT_FIELDS, (int(v) for v in ctx.to_numpy(d_report).view(np.uint64))))


def adapter_mark(ctx, d_report, buf, line_start, first_read, nreads, params, window=None):
    """Narrows the windows of the records [first_read, first_read + nreads) of buf to the leftmost adapter candidate (`window`: the int32
    tensor uq_trim_mark filled; None: a new one, which needs ADAPTER_FRESH in params.flags), the counts added into d_report (queued)."""
    t = ctx.torch
    if window is None:
        if not params.flags & ADAPTER_FRESH: raise ValueError('adapter: no windows given and ADAPTER_FRESH is not set')
        window = t.empty(2 * nreads, dtype=t.int32, device=ctx.device)
    call('uq_adapter_mark', ctx.h, _p(buf), _p(line_start), int(first_read), int(nreads), C.byref(params), _p(window), _p(d_report))
    return window


def adapter_mark_host(data, params, line_start=None, first_read=0, nreads=None, window=None, report=None):
    """uq_adapter_mark_host: the same on the CPU over host bytes (needs no GPU) -> (uint32[nreads, 2] windows, report dict).  `window`: the
    windows to narrow (copied; not needed with ADAPTER_FRESH); `report`: an earlier one to add to."""
    a, ls, nreads = _host_records(data, line_start, first_read, nreads, 'adapter')
    r = AdapterReport(*[report[k] for k in ADAPTER_REPORT_FIELDS]) if report is not None else AdapterReport()
    if window is None:
        if not params.flags & ADAPTER_FRESH: raise ValueError('adapter: no windows given and ADAPTER_FRESH is not set')
        window = np.zeros((nreads, 2), dtype=np.uint32)
    else:
        window = np.array(window, dtype=np.uint32).reshape(-1, 2)
        if len(window) != nreads: raise ValueError('adapter: %d windows for %d records' % (len(window), nreads))
    call('uq_adapter_mark_host', C.c_void_p(a.ctypes.data if a.size else 0), C.c_void_p(ls.ctypes.data), int(first_read), int(nreads),
         C.byref(params), C.c_void_p(window.ctypes.data if nreads else 0), C.byref(r))
    return window, {k: int(getattr(r, k)) for k in ADAPTER_REPORT_FIELDS}


# ------------------------------------------------------------------ pack
def make_pack_params(bases, qualities, N_qual, bits_per_base, bits_per_quality, variable,
                     dna_bytes_per_row, quality_bytes_per_row, dna_max, max_record_bytes, avg_record_bytes=0):
    """uq_pack_params from the decisions (uq_make_pack_params: the tables are filled in the library)."""
    p = PackParams()
    k = len(N_qual)
    call('uq_make_pack_params', bases.encode('latin-1'), len(bases), qualities.encode('latin-1'), len(qualities),
         ''.join(N_qual).encode('latin-1'), (C.c_int32 * max(k, 1))(*[int(v) for v in N_qual.values()]), k,
         int(bits_per_base), int(bits_per_quality), 1 if variable else 0, int(dna_bytes_per_row), int(quality_bytes_per_row), int(dna_max),
         int(max_record_bytes), int(avg_record_bytes), C.byref(p))
    return p


def make_pack_params_py(bases, qualities, N_qual, bits_per_base, bits_per_quality, variable,
                        dna_bytes_per_row, quality_bytes_per_row, dna_max, max_record_bytes, avg_record_bytes=0):
    """The numpy twin of uq_make_pack_params (what make_pack_params ran before; the tests compare the two byte for byte)."""
    p = PackParams()
    dna_code = np.full(256, -1, dtype=np.int16); qual_code = np.full(256, -1, dtype=np.int16); n_qual = np.full(256, -1, dtype=np.int32)
    dna_code[np.frombuffer(bases.encode('latin-1'), dtype=np.uint8)] = np.arange(len(bases), dtype=np.int16)
    qual_code[np.frombuffer(qualities.encode('latin-1'), dtype=np.uint8)] = np.arange(len(qualities), dtype=np.int16)
    for ch, code in N_qual.items(): n_qual[ord(ch)] = int(code)
    C.memmove(p.dna_code, dna_code.ctypes.data, 512); C.memmove(p.qual_code, qual_code.ctypes.data, 512)
    C.memmove(p.n_qual, n_qual.ctypes.data, 1024)
    p.bits_per_base = bits_per_base; p.bits_per_quality = bits_per_quality
    p.variable = 1 if variable else 0
    p.dna_bytes_per_row = dna_bytes_per_row; p.quality_bytes_per_row = quality_bytes_per_row
    p.max_record_bytes = max_record_bytes; p.dna_max = dna_max; p.avg_record_bytes = int(avg_record_bytes)
    return p


def pack(ctx, buf, line_start, first_read, nreads, params, dna=None, qual=None):
    """Returns (dna uint8[nreads * C_dna], qual uint8[nreads * C_qual], bad read index or None)."""
    t = ctx.torch
    if dna is None: dna = t.empty(nreads * params.dna_bytes_per_row, dtype=t.uint8, device=ctx.device)
    if qual is None: qual = t.empty(nreads * params.quality_bytes_per_row, dtype=t.uint8, device=ctx.device)
    bad = t.empty(1, dtype=t.int64, device=ctx.device)
    call('uq_pack', ctx.h, _p(buf), _p(line_start), first_read, nreads, C.byref(params), _p(dna), _p(qual), _p(bad))
    return dna, qual, bad


def pack_stats(ctx, buf, line_start, first_read, nreads, guess, fq=None):
    """One pass: pack with the GUESSED parameters and accumulate uq_stats of the same reads (uq_pack_stats).
    Returns (dna, qual, bad, d_stats) or None when there is no fused kernel for this geometry.
    `fq`: a FusedQname whose guess has been queued (qname_guess): the kernel also tokenises the QNAME lines (uq_pack_stats_qname)."""
    t = ctx.torch
    dna = t.empty(nreads * guess.dna_bytes_per_row, dtype=t.uint8, device=ctx.device)
    qual = t.empty(nreads * guess.quality_bytes_per_row, dtype=t.uint8, device=ctx.device)
    bad = t.empty(1, dtype=t.int64, device=ctx.device)
    st = stats_new(ctx)
    fused = C.c_int(0)
    if fq is None:
        call('uq_pack_stats', ctx.h, _p(buf), _p(line_start), first_read, nreads, C.byref(guess), _p(dna), _p(qual), _p(bad), _p(st), C.byref(fused))
    else:
        call('uq_pack_stats_qname', ctx.h, _p(buf), _p(line_start), first_read, nreads, C.byref(guess), _p(dna), _p(qual), _p(bad), _p(st),
             _p(fq.q), _p(fq.vals), fq.pitch, C.byref(fused))
    return (dna, qual, bad, st) if fused.value else None


def pack_stats_async(ctx, buf, line_start, capacity_reads, guess, st=None, fq=None):
    """pack_stats of every read of `buf` behind ChunkedCensus.end_async() + index_lines_async: tables of capacity_reads rows (the
    caller narrows them once wait() has told it the count; `st`: a stats_new() made earlier, so that its initialisation is not queued
    between the index and the pack kernel).  line_start may be None: no index is expanded, the kernel takes the line starts
    from the census's newline lists (include/uqhip.h).  Returns (dna, qual, bad, d_stats) or None (no fused kernel)."""
    t = ctx.torch
    dna = t.empty(capacity_reads * guess.dna_bytes_per_row, dtype=t.uint8, device=ctx.device)
    qual = t.empty(capacity_reads * guess.quality_bytes_per_row, dtype=t.uint8, device=ctx.device)
    bad = t.empty(1, dtype=t.int64, device=ctx.device)
    if st is None: st = stats_new(ctx)
    fused = C.c_int(0)
    if fq is None:
        call('uq_pack_stats_async', ctx.h, _p(buf), _p(line_start), capacity_reads, C.byref(guess), _p(dna), _p(qual), _p(bad), _p(st), C.byref(fused))
    else:
        call('uq_pack_stats_qname_async', ctx.h, _p(buf), _p(line_start), capacity_reads, C.byref(guess), _p(dna), _p(qual), _p(bad), _p(st),
             _p(fq.q), _p(fq.vals), fq.pitch, C.byref(fused))
    return (dna, qual, bad, st) if fused.value else None


# ------------------------------------------------------------------ the QNAME passes inside the pack kernel
QF_MAXC = 8


class FusedQname:
    """Device side of the fused QNAME pass (include/uqhip.h, uq_qname_fused): `q` = the structure in HBM, `vals` = QF_MAXC columns
    of `pitch` uint32 field values.  Order of calls: qname_guess[_async] -> pack_stats[_async](fq=...) -> qname_fused_finish ->
    qname_fused_fetch (the only one that waits for the device)."""

    def __init__(self, ctx, capacity_reads):
        from ._lib import QnameFused
        t = ctx.torch
        self.pitch = (int(capacity_reads) + 3) & ~3        # columns start 16-byte aligned
        self.q = t.empty(C.sizeof(QnameFused), dtype=t.uint8, device=ctx.device)
        self.vals = t.empty(QF_MAXC * self.pitch, dtype=t.int32, device=ctx.device)

    def column(self, c, n):
        return self.vals[c * self.pitch:c * self.pitch + n]


def qname_guess(ctx, buf, line_start, nreads, fq):
    call('uq_qname_guess', ctx.h, _p(buf), _p(line_start), int(nreads), _p(fq.q))


def qname_guess_async(ctx, buf, line_start, fq):
    """The layout guess behind ChunkedCensus.end_async() [+ index_lines_async] (the read count is taken on the device; line_start None:
    the sample is drawn through the census's newline lists)."""
    call('uq_qname_guess_async', ctx.h, _p(buf), _p(line_start), _p(fq.q))


def qname_fused_finish(ctx, fq):
    """Queue the distinct-value counts of the columns behind the pack kernel (no host wait)."""
    call('uq_qname_fused_finish', ctx.h, _p(fq.q), _p(fq.vals), fq.pitch)


def qname_fused_fetch(ctx, fq):
    from ._lib import QnameFused
    out = QnameFused()
    call('uq_qname_fused_fetch', ctx.h, _p(fq.q), C.byref(out))
    return out


def qname_fused_first_seen(ctx, fq, n, read_offset, vmins, ranges):
    """First occurrences of the small-range columns of a shard as file-wide read numbers (uq_qname_fused_first_seen): int64[QF_MAXC * 4096]
    on the device, INT64_MAX = absent; ranges[c] = 0 skips column c."""
    t = ctx.torch
    k = len(vmins)
    first = t.empty(QF_MAXC * 4096, dtype=t.int64, device=ctx.device)
    call('uq_qname_fused_first_seen', ctx.h, _p(fq.vals), fq.pitch, int(n), int(read_offset), (C.c_uint32 * k)(*[int(x) for x in vmins]),
         (C.c_uint32 * k)(*[int(x) for x in ranges]), k, _p(first))
    return first


def encode_u32_columns(ctx, fq, n, subs, itemsizes):
    """The first len(subs) columns of a fused pass narrowed to their dtypes in one launch (uq_encode_u32_columns)."""
    t = ctx.torch
    k = len(subs)
    outs = [t.empty(n, dtype=getattr(t, _NARROW_DT[isz]), device=ctx.device) for isz in itemsizes]
    call('uq_encode_u32_columns', ctx.h, _p(fq.vals), fq.pitch, int(n), k, (C.c_uint32 * k)(*[int(x) for x in subs]),
         (C.c_int * k)(*[int(x) for x in itemsizes]), (C.c_void_p * k)(*[o.data_ptr() for o in outs]))
    return outs


def encode_u32(ctx, val, n, sub, itemsize):
    t = ctx.torch
    out = t.empty(n, dtype=getattr(t, _NARROW_DT[itemsize]), device=ctx.device)
    call('uq_encode_u32', ctx.h, _p(val), int(n), int(sub), itemsize, _p(out))
    return out


HEAD_BYTES_SMALL = 4 << 20     # the slice of the file the pack-and-count encoder's guess is taken from (8192 reads of <= 512 bytes)
HEAD_READS_INDEXED = 8192


def head_guess(ctx, buf, notricks=False, pad=False, head_bytes=None, head_reads=None):
    """uq_pack_params guessed from the head of the file itself: the multi-pass statistics (uq.py:366-425) of its first
    HEAD_READS reads -> the decisions of uq.py:448-545 on that sample.  Returns (params, reads per byte estimate) or None when
    the head holds no complete record.  A guess is only ever used speculatively: the caller verifies it against the
    statistics of the WHOLE file (uq_pack_stats counts them in the same pass)."""
    from . import analysis
    with ctx.scope():                 # a SideContext: its tensors are allocated on ITS stream; `buf` (complete on the main one) is adopted
        head = ctx.adopt(buf)[:head_bytes or HEAD_BYTES_SMALL]
        nl = count_lines(ctx, head)
        n = min(nl // 4, head_reads or HEAD_READS_INDEXED)
        if n == 0:
            return None
        ls = index_lines(ctx, head, nl)
        st = stats_new(ctx)
        stats_accumulate(ctx, st, head, ls, 0, n)
        hs = stats_fetch(ctx, st)
    if hs.bad_plus is not None or hs.bad_len is not None:
        return None
    d = analysis.decide_from_stats(hs, notricks=notricks, pad=pad)
    if d['N_qual'] and max(d['N_qual'].values()) >= len(d['qualities']): return None       # Q9 new-code files: exact kernel only
    # bytes of the n reads, from the head's own byte and line counts (a read-back of ls[4 n] through torch would queue behind
    # whatever runs on torch's stream -- the caller's census of the whole file -- and hold the host until that is done)
    span = max(int(head.numel() * (4 * n) // max(nl, 1)), 4 * n)
    p = make_pack_params(d['bases'], d['qualities'], d['N_qual'], d['bits_per_base'], d['bits_per_quality'], d['variable_read_lengths'],
                         d['dna_bytes_per_row'], d['quality_bytes_per_row'], d['dna_max'], hs.max_record_bytes, avg_record_bytes=span // n)
    return p, n / span


def head_guess_indexed(ctx, buf, line_start, nreads, notricks=False, pad=False):
    """head_guess for a buffer whose record index exists already: the statistics of its first HEAD_READS_INDEXED reads -> decisions ->
    uq_pack_params, or None (malformed head, Q9 new-code alphabets: no speculative kernel)."""
    from . import analysis
    # 8192 reads: the statistics kernel flushes its tables once per workgroup, and a sample of 150 tiles keeps that to 150
    # workgroups (65 536 reads: 1024 workgroups, 0.15 ms of contended flushes for 22 MB of input)
    n = min(int(nreads), HEAD_READS_INDEXED)
    if n == 0:
        return None
    st = stats_new(ctx)
    stats_accumulate(ctx, st, buf, line_start, 0, n)
    hs = stats_fetch(ctx, st)
    if hs.bad_plus is not None or hs.bad_len is not None:
        return None
    d = analysis.decide_from_stats(hs, notricks=notricks, pad=pad)
    if d['N_qual'] and max(d['N_qual'].values()) >= len(d['qualities']): return None
    return make_pack_params(d['bases'], d['qualities'], d['N_qual'], d['bits_per_base'], d['bits_per_quality'], d['variable_read_lengths'],
                            d['dna_bytes_per_row'], d['quality_bytes_per_row'], d['dna_max'], hs.max_record_bytes,
                            avg_record_bytes=buf.numel() // max(int(nreads), 1))


def same_pack_params(a, b):
    """Do two uq_pack_params describe the same encoding (everything but the tile-sizing hints)?  (uq_same_pack_params)"""
    same = C.c_int(0)
    call('uq_same_pack_params', C.byref(a), C.byref(b), C.byref(same))
    return bool(same.value)


def pack_tile_geometry(params, stats=True, qname=False, lists=False):
    """The tile geometry the pack kernels run `params` at (uq_pack_tile_geometry; host only): a PackTileGeom -- tiled, tile64, R, Rs, P, G,
    stage_bytes, out_bytes, copies, lds_bytes, wg_per_cu.  stats / qname / lists name the kernel: the fused pack + statistics form, its
    QNAME phase, the line starts from the census's lists."""
    g = PackTileGeom()
    call('uq_pack_tile_geometry', C.byref(params), (1 if stats else 0) | (2 if qname else 0) | (4 if lists else 0), C.byref(g))
    return g


def same_pack_params_py(a, b):
    """The Python twin of uq_same_pack_params."""
    if (a.bits_per_base, a.bits_per_quality, a.variable, a.dna_bytes_per_row, a.quality_bytes_per_row, a.dna_max) != \
       (b.bits_per_base, b.bits_per_quality, b.variable, b.dna_bytes_per_row, b.quality_bytes_per_row, b.dna_max):
        return False
    return bytes(a.dna_code) == bytes(b.dna_code) and bytes(a.qual_code) == bytes(b.qual_code) and bytes(a.n_qual) == bytes(b.n_qual)


def scribble_lds(ctx, pattern=0xA5A5A5A5):
    """Test aid (uq_debug_scribble_lds): overwrite every CU's LDS so that reads of never-written LDS show."""
    call('uq_debug_scribble_lds', ctx.h, pattern & 0xFFFFFFFF)


def bad_index(bad_tensor):
    v = int(bad_tensor.cpu().numpy().view(np.uint64)[0])
    return None if v == UQ_NONE else v


# ------------------------------------------------------------------ patterns
def pattern(ctx, table, rows, cols, pattern_id, out=None):
    t = ctx.torch
    if isinstance(pattern_id, str): pattern_id = PATTERN_IDS[pattern_id]
    if out is None: out = t.empty(rows * cols, dtype=t.uint8, device=ctx.device)
    call('uq_pattern', ctx.h, _p(table), rows, cols, pattern_id, _p(out))
    return out


def unpattern(ctx, payload, rows, cols, pattern_id, out=None):
    t = ctx.torch
    if isinstance(pattern_id, str): pattern_id = PATTERN_IDS[pattern_id]
    if out is None: out = t.empty(rows * cols, dtype=t.uint8, device=ctx.device)
    call('uq_unpattern', ctx.h, _p(payload), rows, cols, pattern_id, _p(out))
    return out


# ------------------------------------------------------------------ sort / gather / unique
def sort_config(ctx, msd_min_rows=0, level_bits=None):
    """uq_sort_config: from how many rows a sort's round 0 runs as the MSD partition (0 = default, < 0 = never) and, optionally, its levels' digits."""
    bits = list(level_bits or [])
    call('uq_sort_config', ctx.h, int(msd_min_rows), (C.c_int * max(1, len(bits)))(*bits) if bits else None, len(bits))


def sort_counters(ctx):
    """(sorts whose round 0 ran as the MSD partition, sorts that took the LSD passes) since the context was created."""
    a, b = C.c_uint64(), C.c_uint64()
    call('uq_sort_counters', ctx.h, C.byref(a), C.byref(b))
    return a.value, b.value


def argsort_rows(ctx, table, rows, cols):
    t = ctx.torch
    perm = t.empty(rows, dtype=t.int32, device=ctx.device)
    call('uq_argsort_rows', ctx.h, _p(table), rows, cols, _p(perm))
    return perm


def lower_bound_rows(ctx, sorted_table, rows, cols, probes, nprobes):
    """int64 tensor [nprobes]: first row index of the sorted table that is >= each probe row."""
    t = ctx.torch
    pos = t.empty(nprobes, dtype=t.int64, device=ctx.device)
    call('uq_lower_bound_rows', ctx.h, _p(sorted_table), rows, cols, _p(probes), nprobes, _p(pos))
    return pos


def gather_rows(ctx, table, table_rows, cols, index, n_out=None, out=None):
    t = ctx.torch
    if n_out is None: n_out = index.numel()
    if out is None: out = t.empty(n_out * cols, dtype=t.uint8, device=ctx.device)
    call('uq_gather_rows', ctx.h, _p(table), table_rows, cols, _p(index), index.element_size(), n_out, _p(out))
    return out


def check_index_range(ctx, index, limit):
    """Lowest position whose value is >= limit, or None (uq_check_index_range): stored keys / mapping columns are
    checked before they index a table."""
    bad = C.c_uint64()
    call('uq_check_index_range', ctx.h, _p(index), index.element_size(), index.numel(), int(limit), C.byref(bad))
    return None if bad.value == UQ_NONE else int(bad.value)


def unique_rows(ctx, table, rows, cols, want_key=True, want_sorted_key=True, want_unique=True):
    """Returns (perm i32[rows], key or None, sorted_key or None, unique rows or None, nunique)."""
    t = ctx.torch
    perm = t.empty(rows, dtype=t.int32, device=ctx.device)
    key = t.empty(rows, dtype=t.int32, device=ctx.device) if want_key else None
    skey = t.empty(rows, dtype=t.int32, device=ctx.device) if want_sorted_key else None
    uniq = t.empty(rows * cols, dtype=t.uint8, device=ctx.device) if want_unique else None
    nu = C.c_uint64()
    call('uq_unique_rows', ctx.h, _p(table), rows, cols, _p(perm), _p(key), _p(skey), _p(uniq), C.byref(nu))
    if uniq is not None: uniq = uniq[:nu.value * cols]
    return perm, key, skey, uniq, nu.value


def unique_sorted_rows(ctx, sorted_table, rows, cols, want_unique=True):
    """unique of a table that is already in memcmp order (uq_unique_sorted_rows): (group id per row i32[rows], unique rows or None, nunique)."""
    t = ctx.torch
    group = t.empty(rows, dtype=t.int32, device=ctx.device)
    uniq = t.empty(rows * cols, dtype=t.uint8, device=ctx.device) if want_unique else None
    nu = C.c_uint64()
    call('uq_unique_sorted_rows', ctx.h, _p(sorted_table), rows, cols, _p(group), _p(uniq), C.byref(nu))
    if uniq is not None: uniq = uniq[:nu.value * cols]
    return group, uniq, nu.value


def unique_rows_of_groups(ctx, table, rows, cols, group, nunique, perm=None):
    """The distinct rows of a table from what its sort left (uq_unique_rows_of_groups): uint8[nunique * cols].  perm = the sort's order when
    the table has not been moved into it (only the distinct rows are gathered), None for a table in sorted order."""
    uniq = ctx.torch.empty(nunique * cols, dtype=ctx.torch.uint8, device=ctx.device)
    call('uq_unique_rows_of_groups', ctx.h, _p(table), rows, cols, _p(perm), _p(group), nunique, _p(uniq))
    return uniq


def partition_order(ctx, dest, n, ndest):
    """Stable partition of positions 0 .. n - 1 by dest[position] (uq_partition_order): (order i32[n], counts int64[ndest] ON THE DEVICE)."""
    t = ctx.torch
    order = t.empty(n, dtype=t.int32, device=ctx.device)
    counts = t.empty(ndest, dtype=t.int64, device=ctx.device)
    call('uq_partition_order', ctx.h, _p(dest), n, ndest, _p(order), _p(counts), None)
    return order, counts


def key_itemsize(max_key):
    return load().uq_key_itemsize(int(max_key))


_NARROW_DT = {1: 'uint8', 2: 'int16', 4: 'int32', 8: 'int64'}


def narrow(ctx, key, itemsize):
    t = ctx.torch
    out = t.empty(key.numel(), dtype=getattr(t, _NARROW_DT[itemsize]), device=ctx.device)
    call('uq_narrow', ctx.h, _p(key), key.numel(), itemsize, _p(out))
    return out


def stack_columns(ctx, cols, common_itemsize):
    t = ctx.torch
    n = cols[0].numel()
    ptrs = (C.c_void_p * len(cols))(*[c.data_ptr() for c in cols])
    sizes = (C.c_int * len(cols))(*[c.element_size() for c in cols])
    rows = t.empty(n * len(cols) * common_itemsize, dtype=t.uint8, device=ctx.device)
    call('uq_stack_columns', ctx.h, ptrs, sizes, len(cols), n, common_itemsize, _p(rows))
    return rows


def unstack_column(ctx, rows, n, ncols, common_itemsize, col, out_itemsize):
    t = ctx.torch
    out = t.empty(n, dtype=getattr(t, _NARROW_DT[out_itemsize]), device=ctx.device)
    call('uq_unstack_column', ctx.h, _p(rows), n, ncols, common_itemsize, col, out_itemsize, _p(out))
    return out


# ------------------------------------------------------------------ QNAME passes on the device
def qname_layout(ctx, buf, line_start, nreads, line1, read_index_base=0):
    """`line1`: bytes of the first QNAME line of the whole file; `read_index_base`: file-wide number of this
    shard's first read.  Returns the QnameLayoutResult structure."""
    from ._lib import QnameLayoutResult
    res = QnameLayoutResult()
    l1 = (C.c_uint8 * len(line1)).from_buffer_copy(line1)
    call('uq_qname_layout', ctx.h, _p(buf), _p(line_start), nreads, int(read_index_base), l1, len(line1), C.byref(res))
    return res


def qname_tokenise(ctx, buf, line_start, nreads, prefix_len, suffix_len, separators):
    """Returns (vals [ncols int64 tensors], strs [ncols int64 tensors holding 8 text bytes], QnameColsResult)."""
    from ._lib import QnameColsResult
    t = ctx.torch
    ncols = len(separators) + 1
    vals = [t.empty(nreads, dtype=t.int64, device=ctx.device) for _ in range(ncols)]
    strs = [t.empty(nreads, dtype=t.int64, device=ctx.device) for _ in range(ncols)]
    pv = (C.c_void_p * ncols)(*[v.data_ptr() for v in vals])
    ps = (C.c_void_p * ncols)(*[s.data_ptr() for s in strs])
    seps = (C.c_uint8 * len(separators)).from_buffer_copy(separators)
    res = QnameColsResult()
    call('uq_qname_tokenise', ctx.h, _p(buf), _p(line_start), nreads, prefix_len, suffix_len, seps, len(separators), pv, ps, C.byref(res))
    return vals, strs, res


def prefix_distinct(ctx, perm, sorted_key, n, thresholds):
    """`perm`: int32 (local argsort) or int64 (file-wide indices) tensor, one entry per sorted position."""
    th = (C.c_uint64 * len(thresholds))(*thresholds)
    out = (C.c_uint64 * len(thresholds))()
    call('uq_prefix_distinct', ctx.h, _p(perm), perm.element_size(), _p(sorted_key), n, th, len(thresholds), out)
    return list(out)


def int_prefix_distinct(ctx, val, n, vmin, value_range, thresholds, index_base=0):
    """Distinct values among reads [0, T] of the first n entries of an int64 column, per threshold T (uq_int_prefix_distinct)."""
    th = (C.c_uint64 * len(thresholds))(*thresholds)
    out = (C.c_uint64 * len(thresholds))()
    call('uq_int_prefix_distinct', ctx.h, _p(val), int(n), int(vmin), int(value_range), int(index_base), th, len(thresholds), out)
    return list(out)


def encode_int(ctx, val, sub, itemsize):
    t = ctx.torch
    out = t.empty(val.numel(), dtype=getattr(t, _NARROW_DT[itemsize]), device=ctx.device)
    call('uq_encode_int', ctx.h, _p(val), val.numel(), int(sub), itemsize, _p(out))
    return out


# ------------------------------------------------------------------ unpack
def make_unpack_params(config):
    p = UnpackParams()
    bases, quals = config['bases'], config['qualities']
    for i, ch in enumerate(bases): p.base_char[i] = ord(ch)
    for i, ch in enumerate(quals): p.qual_char[i] = ord(ch)
    for ch, code in config['N_qual'].items():
        if 0 <= int(code) < 256: p.qual_n_base[int(code)] = ord(ch)
    variable = bool(config['variable_read_lengths'])
    lv = config['dna_max'] + (1 if variable else 0)
    p.bits_per_base = config['bits_per_base']; p.bits_per_quality = config['bits_per_quality']
    p.variable = 1 if variable else 0
    p.dna_bytes_per_row = -(-p.bits_per_base * lv // 8)
    p.quality_bytes_per_row = -(-p.bits_per_quality * lv // 8)
    p.dna_max = config['dna_max']
    return p


def unpack(ctx, dna, qual, nreads, params):
    t = ctx.torch
    seq = t.empty(nreads * params.dna_max, dtype=t.uint8, device=ctx.device)
    qtxt = t.empty(nreads * params.dna_max, dtype=t.uint8, device=ctx.device)
    ln = t.empty(nreads, dtype=t.int32, device=ctx.device)
    bad = t.empty(1, dtype=t.int64, device=ctx.device)
    call('uq_unpack', ctx.h, _p(dna), _p(qual), nreads, C.byref(params), _p(seq), _p(qtxt), _p(ln), _p(bad))
    return seq, qtxt, ln, bad


# ------------------------------------------------------------------ FASTQ text emit (decode)
def _emit_params(ctx, config, column_tensors):
    """config.json's QNAME layout -> (uq_emit_params, column / string-table pointer arrays, tensors to keep alive)."""
    from ._lib import EmitParams
    cols = config['QNAME_columns']
    if len(cols) > 32: raise ValueError('more than 32 QNAME columns')
    p = EmitParams()
    pre = config['QNAME_prefix'].encode('latin-1'); suf = config['QNAME_suffix'].encode('latin-1')
    seps = config['QNAME_separators'].encode('latin-1')
    if len(pre) > 256 or len(suf) > 256: raise ValueError('QNAME prefix / suffix longer than 256 bytes')
    for i, b in enumerate(pre): p.prefix[i] = b
    for i, b in enumerate(suf): p.suffix[i] = b
    for i, b in enumerate(seps[:32]): p.separators[i] = b
    p.prefix_len = len(pre); p.suffix_len = len(suf); p.ncols = len(cols); p.dna_max = config['dna_max']
    keep = []
    d_cols = (C.c_void_p * 32)(); d_chars = (C.c_void_p * 32)(); d_offs = (C.c_void_p * 32)()
    for i, c in enumerate(cols):
        p.itemsize[i] = column_tensors[i].element_size()
        add = int(c['min']) if (c['format'] != 'mapping' and c.get('offset')) else 0
        if not -2 ** 63 <= add < 2 ** 63:                          # (ctypes would wrap it silently; Session.device_text_possible keeps such files on the host path)
            raise ValueError('QNAME column %d: the offset %d does not fit the int64 the device adds' % (i + 1, add))
        p.add[i] = add
        d_cols[i] = column_tensors[i].data_ptr()
        if c['format'] == 'mapping':
            strs = [s.encode('latin-1') for s in c['map']]
            offs = np.zeros(len(strs) + 1, dtype=np.uint32)
            offs[1:] = np.cumsum([len(s) for s in strs])
            chars = ctx.to_device(np.frombuffer(b''.join(strs) + b'\0', dtype=np.uint8))
            offt = ctx.to_device(offs)
            keep += [chars, offt]
            d_chars[i] = chars.data_ptr(); d_offs[i] = offt.data_ptr()
            p.add[i] = len(strs)                                 # mapping columns: the table's length (codes are clamped to it on the device)
    return p, d_cols, d_chars, d_offs, keep


def emit_fastq(ctx, config, column_tensors, seq, qual, ln, nreads, size_only=False):
    """Device-side FASTQ text: returns a uint8 tensor with the whole decoded file.
    `column_tensors`: one device tensor per QNAME column (values per read, the column's dtype).
    size_only: the size pass alone -- returns the text's length in bytes, writes nothing."""
    t = ctx.torch
    p, d_cols, d_chars, d_offs, keep = _emit_params(ctx, config, column_tensors)
    offsets = t.empty(nreads + 1, dtype=t.int64, device=ctx.device)
    total = C.c_uint64()
    call('uq_emit_fastq', ctx.h, C.byref(p), d_cols, d_chars, d_offs, _p(seq), _p(qual), _p(ln), nreads, _p(offsets), None, 0, C.byref(total))
    if size_only: return total.value
    out = t.empty(total.value, dtype=t.uint8, device=ctx.device)
    call('uq_emit_fastq', ctx.h, C.byref(p), d_cols, d_chars, d_offs, _p(seq), _p(qual), _p(ln), nreads, _p(offsets), _p(out), total.value, C.byref(total))
    del keep
    return out


def decode_fastq(ctx, config, column_tensors, dna, qual, nreads, size_only=False):
    """Packed DNA / QUAL tables + QNAME columns -> the FASTQ text (uint8 device tensor), in one pass over the rows
    (uq_decode_fastq).  Returns (text, bad): bad = lowest row without a length sentinel, or None.
    size_only: the first call alone (lengths, record sizes) -- returns (the text's length in bytes, bad), writes no text."""
    t = ctx.torch
    p, d_cols, d_chars, d_offs, keep = _emit_params(ctx, config, column_tensors)
    up = make_unpack_params(config)
    offsets = t.empty(nreads + 1, dtype=t.int64, device=ctx.device)
    ln = t.empty(nreads if up.variable else 0, dtype=t.int32, device=ctx.device)
    d_bad = t.empty(1, dtype=t.int64, device=ctx.device)
    total = C.c_uint64(); bad = C.c_uint64()
    args = (ctx.h, C.byref(p), C.byref(up), d_cols, d_chars, d_offs, _p(dna), _p(qual), nreads, _p(ln) if up.variable else None, _p(offsets), _p(d_bad))
    call('uq_decode_fastq', *args, None, 0, C.byref(total), C.byref(bad))
    if bad.value != 2 ** 64 - 1: return None, int(bad.value)
    if size_only: return total.value, None
    out = t.empty(total.value, dtype=t.uint8, device=ctx.device)
    call('uq_decode_fastq', *args, _p(out), total.value, C.byref(total), C.byref(bad))
    del keep
    return out, None


# ------------------------------------------------------------------ synthetic input
def synth_spec(spec):
    """uq_amd.synth.Spec -> C struct."""
    s = SynthSpec()
    s.seed = spec.seed; s.len_lo = spec.len_lo; s.len_hi = spec.len_hi; s.n_rate = spec.n_rate
    s.n_qual_exclusive = 1 if spec.n_qual_exclusive else 0
    s.dup = spec.dup; s.dup_templates = spec.dup_templates; s.skip_len_mod4 = 1 if spec.skip_len_mod4 else 0
    return s


def synth_fastq(ctx, spec, first, n):
    t = ctx.torch
    cs = synth_spec(spec)
    nbytes = C.c_uint64()
    call('uq_synth_size', ctx.h, C.byref(cs), first, n, C.byref(nbytes))
    out = t.empty(nbytes.value, dtype=t.uint8, device=ctx.device)
    call('uq_synth_fastq', ctx.h, C.byref(cs), first, n, _p(out), nbytes.value)
    return out


# ------------------------------------------------------------------ gzip input (an extension: BGZF members inflate on the device)
GZIP_BGZF, GZIP_OTHER, GZIP_MALFORMED = 1, 2, 3
GZIP_MEMBER = np.dtype([('data_offset', '<u8'), ('comp_bytes', '<u8'), ('out_offset', '<u8'), ('isize', '<u4'), ('crc32', '<u4')])
INFLATE_STATUS = {1: 'deflate data runs past the end of the member', 2: 'invalid block type', 3: 'stored block length check failed',
                  4: 'invalid code lengths set', 5: 'invalid code length repeat', 6: 'invalid Huffman code', 7: 'distance too far back',
                  8: 'more output than the trailer\'s ISIZE', 9: 'less output than the trailer\'s ISIZE', 10: 'CRC-32 mismatch',
                  11: 'too many length or distance symbols', 12: 'member larger than 64 KiB or outside the input',
                  13: 'bytes that are not a gzip member header', 15: 'distance too far back'}


def is_gzip(path):
    """Content sniff: gzip files start with 1f 8b (plain FASTQ starts with '@')."""
    with open(path, 'rb') as f:
        return f.read(2) == b'\x1f\x8b'


def gzip_scan(buf):
    """uq_gzip_scan over a host uint8 array (a memmap will do: only the headers are touched).  Returns (kind, members, total_out, error):
    members a GZIP_MEMBER array; error = (message, member offset) when kind is GZIP_MALFORMED, else None."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) or buf.dtype != np.uint8 else buf
    n, total, kind, bad = C.c_uint64(), C.c_uint64(), C.c_int(), C.c_uint64()
    ptr = C.c_void_p(buf.ctypes.data if buf.size else 0)
    call('uq_gzip_scan', ptr, buf.size, None, 0, C.byref(n), C.byref(total), C.byref(kind), C.byref(bad))
    if kind.value == GZIP_MALFORMED:
        return kind.value, np.zeros(0, GZIP_MEMBER), total.value, (load().uq_last_error().decode('utf-8', 'replace'), bad.value)
    members = np.zeros(n.value, GZIP_MEMBER)
    call('uq_gzip_scan', ptr, buf.size, C.c_void_p(members.ctypes.data), n.value, C.byref(n), C.byref(total), C.byref(kind), C.byref(bad))
    return kind.value, members, total.value, None


def inflate_members(ctx, d_comp, members, total_out, d_members=None):
    """uq_inflate_members: the members (a GZIP_MEMBER array from gzip_scan) of the compressed bytes d_comp inflated into a fresh uint8 device
    tensor of total_out bytes.  Returns (d_out, None), or (d_out, (member index, status)) for the first member that failed."""
    t = ctx.torch
    out = t.empty(int(total_out), dtype=t.uint8, device=ctx.device)
    n = len(members)
    if n == 0:
        return out, None
    if d_members is None:
        d_members = ctx.to_device(np.ascontiguousarray(members).view(np.uint8))
    st = t.zeros(n, dtype=t.int32, device=ctx.device)
    call('uq_inflate_members', ctx.h, _p(d_comp), d_comp.numel(), _p(d_members), n, _p(out), out.numel(), _p(st))
    bad = t.nonzero(st).flatten()[:1].cpu()
    if bad.numel():
        k = int(bad[0])
        return out, (k, int(st[k]))
    return out, None


def inflate_member_host(data, isize, crc32):
    """uq_inflate_member_host: one member's raw deflate bytes through the device decoder's code on the CPU.  Returns (status, bytes)."""
    data = bytes(data)
    src = np.frombuffer(data, dtype=np.uint8)
    out = np.zeros(max(int(isize), 1), dtype=np.uint8)
    st = C.c_uint32()
    call('uq_inflate_member_host', C.c_void_p(src.ctypes.data if src.size else 0), len(data), C.c_void_p(out.ctypes.data), int(isize),
         int(crc32) & 0xFFFFFFFF, C.byref(st))
    return st.value, out[:int(isize)].tobytes()


# ------------------------------------------------------------------ other gzip: chunks inflated on the device in parallel
GZS_MEMBER, GZS_UNCOMPRESSED, GZS_DYNAMIC = 0, 1, 2


class GzipStreamError(ValueError):
    """A damaged gzip stream: .status (UQ_INF_* / UQ_GZS_* code), .offset (the byte offset the message names)."""

    def __init__(self, message, status, offset):
        ValueError.__init__(self, message)
        self.status, self.offset = status, offset


def _starts_arg(starts):
    if starts is None:
        return None, C.c_void_p(0), 0
    arr = np.ascontiguousarray(np.asarray(starts, dtype=np.uint64).reshape(-1))
    return arr, C.c_void_p(arr.ctypes.data if arr.size else 0), arr.size


def _info_dict(info):
    return {k: getattr(info, k) for k, _ in GzipStreamInfo._fields_}


def gzip_stream_to_device(ctx, d_comp, chunk_bytes, starts=None):
    """uq_gzip_stream_begin / _finish: the gzip file d_comp (a uint8 device tensor, not BGZF or BGZF, any members) inflated on the device in
    parallel chunks of chunk_bytes compressed bytes.  starts: the caller's chunk starts instead of the finder's ((bit << 2) | kind).
    Returns (uint8 device tensor of the output, info dict); a damaged stream raises GzipStreamError."""
    t = ctx.torch
    keep, sp, ns = _starts_arg(starts)
    h, nout, st, bad = C.c_void_p(), C.c_uint64(), C.c_uint32(), C.c_uint64()
    n = d_comp.numel()
    call('uq_gzip_stream_begin', ctx.h, _p(d_comp) if n else C.c_void_p(0), n, int(chunk_bytes), sp, ns, C.byref(h), C.byref(nout),
         C.byref(st), C.byref(bad))
    if st.value:
        raise GzipStreamError(load().uq_last_error().decode('utf-8', 'replace'), st.value, bad.value)
    try:
        out = t.empty(nout.value, dtype=t.uint8, device=ctx.device)
        call('uq_gzip_stream_finish', h, _p(out) if nout.value else C.c_void_p(0), nout.value, C.byref(st), C.byref(bad))
        if st.value:
            raise GzipStreamError(load().uq_last_error().decode('utf-8', 'replace'), st.value, bad.value)
        info = GzipStreamInfo()
        call('uq_gzip_stream_get_info', h, C.byref(info))
    finally:
        call('uq_gzip_stream_free', h)
    return out, _info_dict(info)


def gzip_stream_host(data, chunk_bytes, starts=None):
    """uq_gzip_stream_host: the same finder, chunk decoder, chain check and resolution on the CPU.  Returns (bytes, info dict); a damaged
    stream raises GzipStreamError."""
    data = bytes(data)
    src = np.frombuffer(data, dtype=np.uint8)
    keep, sp, ns = _starts_arg(starts)
    nout, st, bad, info = C.c_uint64(), C.c_uint32(), C.c_uint64(), GzipStreamInfo()
    cap = 4 * len(data) + 4096
    while True:
        out = np.empty(max(cap, 1), dtype=np.uint8)
        call('uq_gzip_stream_host', C.c_void_p(src.ctypes.data if src.size else 0), len(data), int(chunk_bytes), sp, ns,
             C.c_void_p(out.ctypes.data), cap, C.byref(nout), C.byref(st), C.byref(bad), C.byref(info))
        if st.value:
            raise GzipStreamError(load().uq_last_error().decode('utf-8', 'replace'), st.value, bad.value)
        if nout.value <= cap:
            return out[:nout.value].tobytes(), _info_dict(info)
        cap = nout.value


# ------------------------------------------------------------------ BGZF output (an extension: members deflated on the device)
BGZF_BLOCK = 65280
BGZF_EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')
DEFLATE_STATUS = {1: 'the member needs more than the output capacity', 2: 'more than 65 280 input bytes'}
BGZF_LEVELS = (1, 2)
UQ_BGZF_EOF, UQ_BGZF_LEVEL2 = 1, 2


def bgzf_level_flags(level):
    """The flag bits of a compressor level: 1 (the default: one candidate per position, greedy) or 2 (more candidates, lazy)."""
    if level not in BGZF_LEVELS: raise ValueError('the BGZF compressor has levels 1 and 2, not %r' % (level,))
    return UQ_BGZF_LEVEL2 if level == 2 else 0


def bgzf_bound(nbytes):
    """uq_bgzf_bound: the output capacity bgzf_compress needs for nbytes of input."""
    out = C.c_uint64()
    call('uq_bgzf_bound', int(nbytes), C.byref(out))
    return out.value


def bgzf_compress(ctx, d_text, eof=True, level=1):
    """uq_bgzf_compress: the uint8 device tensor d_text as a BGZF stream (one member per 65 280 bytes, deflated on the device, plus the EOF
    member when `eof`) at compressor level `level`.  Returns a uint8 device tensor of exactly the stream's bytes."""
    flags = bgzf_level_flags(level) | (UQ_BGZF_EOF if eof else 0)
    t = ctx.torch
    n = d_text.numel()
    out = t.empty(bgzf_bound(n), dtype=t.uint8, device=ctx.device)
    nout = C.c_uint64()
    call('uq_bgzf_compress', ctx.h, _p(d_text) if n else C.c_void_p(0), n, _p(out), out.numel(), C.byref(nout), flags)
    return out[:nout.value]


def _bgzf_parts_arg(parts):
    """[(prefix bytes, uint8 device tensor or None)] -> (the uq_bgzf_part array, what must stay alive while it is used)."""
    arr = (BgzfPart * max(len(parts), 1))()
    keep = []
    for k, (prefix, d_data) in enumerate(parts):
        prefix = bytes(prefix)
        pre = np.frombuffer(prefix, dtype=np.uint8)
        nbytes = 0 if d_data is None else d_data.numel() * d_data.element_size()
        keep.append((pre, d_data))
        arr[k].h_prefix = pre.ctypes.data if pre.size else None
        arr[k].prefix_bytes = len(prefix)
        arr[k].d_data = d_data.data_ptr() if nbytes else None
        arr[k].nbytes = nbytes
    return arr, keep


def bgzf_parts_bound(parts):
    """uq_bgzf_parts_bound: the output capacity bgzf_compress_parts needs."""
    arr, keep = _bgzf_parts_arg(parts)
    out = C.c_uint64()
    call('uq_bgzf_parts_bound', arr, len(parts), C.byref(out))
    return out.value


def bgzf_compress_parts(ctx, parts, eof=False, capacity=None, level=1):
    """uq_bgzf_compress_parts: parts = [(prefix bytes (<= 256), device tensor)]; every part's prefix + data as BGZF members, the block cuts
    restarting at each part, all parts compressed in one run.  Returns (uint8 device tensor of the members of all parts in order, [bytes
    of each part]).  `capacity`: the output buffer's size instead of bgzf_parts_bound's; `level`: the compressor level."""
    flags = bgzf_level_flags(level) | (UQ_BGZF_EOF if eof else 0)
    t = ctx.torch
    arr, keep = _bgzf_parts_arg(parts)
    cap = bgzf_parts_bound(parts) if capacity is None else int(capacity)
    out = t.empty(cap, dtype=t.uint8, device=ctx.device)
    sizes = (C.c_uint64 * max(len(parts), 1))()
    nout = C.c_uint64()
    call('uq_bgzf_compress_parts', ctx.h, arr, len(parts), _p(out) if cap else C.c_void_p(0), cap, sizes, C.byref(nout), flags)
    return out[:nout.value], [int(sizes[k]) for k in range(len(parts))]


def bgzf_compress_parts_host(parts, eof=False, level=1):
    """The host twin of bgzf_compress_parts over host bytes: parts = [(prefix bytes, data bytes)].  Returns (bytes, [bytes of each part])."""
    out, sizes = [], []
    for prefix, data in parts:
        whole = bytes(prefix) + bytes(data)
        members = [bgzf_block_host(whole[o:o + BGZF_BLOCK], level=level) for o in range(0, len(whole), BGZF_BLOCK)]
        sizes.append(sum(len(m) for m in members))
        out.extend(members)
    if eof: out.append(BGZF_EOF)
    return b''.join(out), sizes


def bgzf_block_host(data, capacity=None, level=1):
    """uq_bgzf_compress_block_host: one block (<= 65 280 bytes) through the device compressor's code on the CPU.  Returns the member's
    bytes; with `capacity`, returns (status, member size, the capacity's bytes) instead.  `level` 2: uq_bgzf_compress_block_host_l with
    UQ_BGZF_LEVEL2."""
    flags = bgzf_level_flags(level)
    data = bytes(data)
    src = np.frombuffer(data, dtype=np.uint8)
    cap = 65536 if capacity is None else int(capacity)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    nout, st = C.c_uint64(), C.c_uint32()
    args = (C.c_void_p(src.ctypes.data if src.size else 0), len(data), C.c_void_p(out.ctypes.data), cap, C.byref(nout), C.byref(st))
    if flags: call('uq_bgzf_compress_block_host_l', *args, flags)
    else: call('uq_bgzf_compress_block_host', *args)
    if capacity is not None:
        return st.value, nout.value, out[:cap].tobytes()
    if st.value:
        raise ValueError('bgzf_block_host: %s' % DEFLATE_STATUS.get(st.value, 'status %d' % st.value))
    return out[:nout.value].tobytes()


# ------------------------------------------------------------------ the size of a buffer as BGZF (the --test sizer)
def deflate_size_host(data, prefix=b'', level=1):
    """uq_deflate_size_host: S(prefix + data) on the CPU -- the bytes ops.bgzf_compress(prefix + data, eof=False) would have at that level."""
    flags = bgzf_level_flags(level)
    data, prefix = bytes(data), bytes(prefix)
    src = np.frombuffer(data, dtype=np.uint8)
    pre = np.frombuffer(prefix, dtype=np.uint8)
    out = C.c_uint64()
    args = (C.c_void_p(pre.ctypes.data if pre.size else 0), len(prefix), C.c_void_p(src.ctypes.data if src.size else 0), len(data),
            C.byref(out))
    if flags: call('uq_deflate_size_host_l', *args, flags)
    else: call('uq_deflate_size_host', *args)
    return out.value


class DeflateSizes:
    """uq_deflate_size for up to `capacity` buffers: add() queues one (nothing is read back, the stream is not synchronised), fetch()
    reads all the totals back at once.  A buffer passed to add() may be overwritten by work queued behind it on the context's stream."""

    def __init__(self, ctx, capacity, level=1):
        self.ctx, self.capacity, self.n = ctx, int(capacity), 0
        self.flags = bgzf_level_flags(level)
        self.slots = ctx.torch.zeros(2 * self.capacity, dtype=ctx.torch.int64, device=ctx.device)      # totals, then one status each

    def add(self, prefix, d_data):
        """Queues S(prefix + the bytes of the device tensor d_data); returns its index in fetch()'s list."""
        if self.n >= self.capacity: raise ValueError('DeflateSizes: more than %d buffers' % self.capacity)
        prefix = bytes(prefix)
        nbytes = d_data.numel() * d_data.element_size()
        args = (self.ctx.h, prefix, len(prefix), _p(d_data) if nbytes else C.c_void_p(0), nbytes, _p(self.slots[self.n:]),
                _p(self.slots[self.capacity + self.n:]))
        if self.flags: call('uq_deflate_size_l', *args, self.flags)
        else: call('uq_deflate_size', *args)
        self.n += 1
        return self.n - 1

    def fetch(self):
        host = self.ctx.to_numpy(self.slots)
        bad = [k for k in range(self.n) if host[self.capacity + k]]
        if bad: raise ValueError('deflate_size: buffer %d: %s' % (bad[0], DEFLATE_STATUS.get(int(host[self.capacity + bad[0]]), 'failed')))
        return [int(v) for v in host[:self.n]]


def deflate_size(ctx, prefix, d_data, level=1):
    """S(prefix + the bytes of d_data) for one buffer (queue, then read back)."""
    q = DeflateSizes(ctx, 1, level=level)
    q.add(prefix, d_data)
    return q.fetch()[0]
