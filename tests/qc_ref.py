"""The per-cycle tables `uqqc1` (include/uqhip.h) in plain numpy, independent of the library: bytes and the number of
exact cycles in, the flat array of u64 counters out.  What the host twin and the kernel are held to, word for word."""
import numpy as np

NBASE, NQUAL, NGC = 6, 94, 101
SCALARS = ('reads', 'bases', 'qual_chars', 'qual_out_of_range', 'len_mismatch')

CLS = np.full(256, 5, dtype=np.int64)
for _i, _pair in enumerate((b'Aa', b'Cc', b'Gg', b'Tt', b'Nn')):
    for _b in _pair: CLS[_b] = _i
PHRED = np.clip(np.arange(256, dtype=np.int64) - 33, 0, 93)
OUT_OF_RANGE = (np.arange(256) < 33) | (np.arange(256) > 126)


def words(C):
    return 8 + (NBASE + NQUAL) * (C + 1) + (C + 1) + NQUAL + NGC


def offsets(C):
    """name -> (first word, rows, columns) of the object's tables."""
    o, out = 8, {}
    for name, rows, cols in (('base_by_cycle', C + 1, NBASE), ('qual_by_cycle', C + 1, NQUAL), ('length_hist', C + 1, 1),
                             ('mean_qual_hist', NQUAL, 1), ('gc_hist', NGC, 1)):
        out[name] = (o, rows, cols)
        o += rows * cols
    assert o == words(C)
    return out


def fields(flat):
    """The flat array as a dict: scalars as integers, tables as arrays (two-dimensional where the definition says so)."""
    flat = np.asarray(flat, dtype=np.uint64)
    C = (len(flat) - 8 - NQUAL - NGC) // (NBASE + NQUAL + 1) - 1
    assert len(flat) == words(C)
    d = {k: int(flat[i]) for i, k in enumerate(SCALARS)}
    d['reserved'] = [int(v) for v in flat[5:8]]
    for name, (o, rows, cols) in offsets(C).items():
        t = flat[o:o + rows * cols]
        d[name] = t.reshape(rows, cols) if cols > 1 else t
    return d


def line_starts(a):
    return np.concatenate(([0], np.flatnonzero(a == 10) + 1)).astype(np.int64)


def _positions(a, start, length):
    """For lines at `start` with `length` bytes: (record number, position in the line, byte) of every byte of every line."""
    total = int(length.sum())
    rec = np.repeat(np.arange(len(length), dtype=np.int64), length)
    pos = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(length) - length, length)
    return rec, pos, a[np.repeat(start, length) + pos] if total else np.zeros(0, dtype=np.uint8)


def qc(data, C=1024, first=0, n=None):
    """The flat uqqc1 array of the records [first, first + n) of a FASTQ text (bytes or a uint8 array)."""
    assert 1 <= C <= 1024
    a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    ls = line_starts(a)
    assert (len(ls) - 1) % 4 == 0, 'whole records'
    if n is None: n = (len(ls) - 1) // 4 - first
    ls = ls[4 * first:4 * (first + n) + 1]
    s0, Ls = ls[1:-1:4], ls[2::4] - ls[1:-1:4] - 1
    u0, Lu = ls[3::4], ls[4::4] - ls[3::4] - 1
    out = np.zeros(words(C), dtype=np.uint64)
    off = offsets(C)
    out[0], out[1], out[2], out[4] = n, int(Ls.sum()), int(Lu.sum()), int((Ls != Lu).sum())

    rec, pos, byte = _positions(a, s0, Ls)
    cls = CLS[byte]
    o, rows, cols = off['base_by_cycle']
    out[o:o + rows * cols] = np.bincount(np.minimum(pos, C) * NBASE + cls, minlength=rows * cols).astype(np.uint64)
    gc = np.bincount(rec[(cls == 1) | (cls == 2)], minlength=n).astype(np.int64)

    rec, pos, byte = _positions(a, u0, Lu)
    q = PHRED[byte]
    out[3] = int(OUT_OF_RANGE[byte].sum())
    o, rows, cols = off['qual_by_cycle']
    out[o:o + rows * cols] = np.bincount(np.minimum(pos, C) * NQUAL + q, minlength=rows * cols).astype(np.uint64)
    sq = np.zeros(n, dtype=np.int64)
    np.add.at(sq, rec, q)

    o, rows, _ = off['length_hist']
    out[o:o + rows] = np.bincount(np.minimum(Ls, C), minlength=rows).astype(np.uint64)
    o, rows, _ = off['mean_qual_hist']
    out[o:o + rows] = np.bincount(sq[Lu > 0] // Lu[Lu > 0], minlength=rows).astype(np.uint64)
    o, rows, _ = off['gc_hist']
    out[o:o + rows] = np.bincount(100 * gc[Ls > 0] // Ls[Ls > 0], minlength=rows).astype(np.uint64)
    return out
