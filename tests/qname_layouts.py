"""Hand-built QNAME layouts for the decoder tests (test_gpu_emit_qname.py on the device, test_emit_qname_cpu.py on the host path).

A layout is what config.json says about the QNAME lines -- prefix, suffix, separators, one entry per column -- plus the stored column
arrays.  It is written down here directly, not inferred from names: the encoders' prefix detection would swallow constant leading
digits, and no FASTQ of a few hundred reads makes a uint64 column hold 2**64 - 1.  `craft` puts a layout on top of the DNA / QUAL
tables the oracle packed from a small synthetic FASTQ; `O.decode(config, members)` -- Python integers, `str(int(v) + min)` -- is then
the expected text at any magnitude.

The printed numbers the integer columns aim at (TARGETS): -1, 0, 1, both sides of every digit-count boundary up to 10**19, of 2**32
and of 2**63, and 2**64 - 1; every column also stores 0 (prints `min`) and the largest value its dtype and the device's contract
[-2**63, 2**64) allow."""
import random

import numpy as np

import uq_oracle as O

DTYPES = ['uint8', 'uint16', 'uint32', 'uint64']
OFFSETS = [None, -1, -25, -2 ** 31, -2 ** 63, 1, 10 ** 9, 2 ** 32, 2 ** 63 - 1]       # None: a column without offset
TARGETS = sorted({-1, 0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1} | {10 ** k - 1 for k in range(1, 20)} | {10 ** k for k in range(1, 20)})
BEYOND = [2 ** 64, 2 ** 64 + 1, 10 ** 20 - 1, 10 ** 20]                              # host path only: results from 2**64 on
SEPS = ':/ _;,#|=.~!%^&*'
RAW = ['DNA', 'QUAL', 'QNAME']

# ---- the tables under the layouts: id -> (reads, lengths, bases, qualities, notricks).  What uq_decode_fastq makes of each is said
# (and the geometry asserted) in test_gpu_emit_qname.py.
Q31 = ''.join(chr(c) for c in range(40, 71))      # one contiguous quality range, 5 bits
GAPPED = '#+5AFI'                                  # qualities with gaps: the alphabets go through the tables
GEOMETRIES = {
    'S': (389, [1, 2, 7, 8, 9, 15, 16, 17, 40, 63, 64, 65, 90], 'ACGT', Q31, False),
    'T40': (197, [40], 'ACGT', Q31, False),
    'T100': (197, [100], 'ACGT', Q31, False),
    'Gfixed': (197, [50], 'ACGTN', GAPPED, True),
    'Gvar': (197, [1, 7, 8, 9, 33, 64, 65, 77], 'ACGTN', GAPPED, True),
    'D': (97, None, 'ACGTN', GAPPED, True),        # read 30 holds 6 000 bases, the others 15 - 25
}
_tables = {}


def tables(geom):
    """(config, {'DNA.raw', 'QUAL.raw'}, reads) of a geometry, packed by the oracle; computed once."""
    if geom not in _tables:
        n, lengths, bases, quals, notricks = GEOMETRIES[geom]
        rnd = random.Random(20261018 + sorted(GEOMETRIES).index(geom))
        recs = []
        for i in range(n):
            L = rnd.choice(lengths) if lengths else (6000 if i == 30 else rnd.randint(15, 25))
            recs.append('@g:%d:%d\n%s\n+\n%s\n' % (i % 7, i, ''.join(rnd.choice(bases) for _ in range(L)), ''.join(rnd.choice(quals) for _ in range(L))))
        cfg, members, _ = O.encode(''.join(recs).encode(), raw=RAW, notricks=notricks)
        _tables[geom] = (cfg, {k: members[k] for k in ('DNA.raw', 'QUAL.raw')}, n)
    return _tables[geom]


def contiguous(qualities):
    return all(ord(q) == ord(qualities[0]) + i for i, q in enumerate(qualities))


# ---- columns: (config entry without its name, stored array)
def int_column(dtype, offset, n, rnd, beyond=False, extra=()):
    """An integer column of n stored values.  Printed = stored + offset; the stored values are 0, the largest allowed, whatever prints
    one of TARGETS (+ `extra`), then random ones.  beyond: the results may pass 2**64 (the host path's tests)."""
    lim = 2 ** (8 * np.dtype(dtype).itemsize) - 1
    add = offset or 0
    hi = lim if beyond else min(lim, 2 ** 64 - 1 - add)
    assert hi >= 0
    stored = [0, hi] + [t - add for t in list(TARGETS) + list(extra) if 0 <= t - add <= hi]
    stored = list(dict.fromkeys(stored))
    assert len(stored) <= n, (dtype, offset, len(stored), n)
    while len(stored) < n:
        # random magnitudes, not random values: a uniform draw from a uint64 never has fewer than 17 digits
        stored.append(min(hi, rnd.getrandbits(rnd.randint(1, 8 * np.dtype(dtype).itemsize))))
    rnd.shuffle(stored)
    col = {'format': 'integers', 'dtype': dtype, 'offset': offset is not None, 'min': add + min(stored), 'max': add + max(stored)}
    return col, np.array(stored, dtype=dtype)


def map_column(dtype, strings, n, rnd):
    """A mapping column: codes below len(strings), every code at least once where n allows, the first and last always."""
    codes = list(range(len(strings))) if len(strings) <= n else [0, len(strings) - 1] + [c for c in (255, 256) if c < len(strings)]
    while len(codes) < n: codes.append(rnd.randrange(len(strings)))
    rnd.shuffle(codes)
    return {'format': 'mapping', 'dtype': dtype, 'map': list(strings)}, np.array(codes, dtype=dtype)


def layout(prefix, suffix, columns, seps=SEPS):
    cols = []
    for i, (c, a) in enumerate(columns):
        cols.append((dict(c, name='QNAME_%d' % (i + 1)), a))
    return {'prefix': prefix, 'suffix': suffix, 'separators': ''.join(seps[i % len(seps)] for i in range(max(len(cols) - 1, 0))), 'columns': cols}


def craft(geom, lay):
    """(config, members) of geometry `geom` with the QNAME layout `lay`: what O.decode and O.write_tar take."""
    cfg, members, n = tables(geom)
    cfg = dict(cfg, QNAME_prefix=lay['prefix'], QNAME_suffix=lay['suffix'], QNAME_separators=lay['separators'], QNAME_columns=[c for c, _ in lay['columns']])
    members = dict(members)
    for c, a in lay['columns']:
        assert len(a) == n
        members[c['name'] + '.raw'] = O.npy_bytes(a)
    return cfg, members


def qname_lines(text):
    return text.split('\n')[:-1][0::4]


# ---- the layouts of each part of the issue, for n reads
def integer_layouts(n, beyond=False):
    """1(a): per offset, the four dtypes side by side (four columns: a lane per field); per dtype, the nine offsets side by side
    (nine columns: more fields in a tile than lanes, the looped field passes).  Every layout starts with a prefix, so a field whose
    length is off by one moves bytes of its own line only."""
    rnd = random.Random(97)
    extra = BEYOND if beyond else ()
    out = {}
    for off in OFFSETS:
        out['offset=%s' % off] = layout('@a', '', [int_column(dt, off, n, rnd, beyond, extra) for dt in DTYPES])
    for dt in DTYPES:
        out[dt] = layout('@b.', '/1', [int_column(dt, off, n, rnd, beyond, extra) for off in OFFSETS])
    return out


def _ramp(j, length):
    return ''.join(chr(97 + (7 * j + k) % 26) for k in range(length))


def mapping_layouts(n):
    """1(b): the empty string, strings of 1 / 16 / 17 / 300 bytes, a table of one string, uint8 and uint16 codes (300 entries)."""
    rnd = random.Random(98)
    five = ['', 'k', _ramp(1, 16), _ramp(2, 17), _ramp(3, 300)]
    many = [_ramp(j, j % 19) for j in range(300)]                  # lengths 0 .. 18; many[0] and many[19] are empty
    return {
        'five-strings-alone': layout('@m', '', [map_column('uint8', five, n, rnd)]),
        'five-strings-between': layout('@m ', ' z', [int_column('uint8', None, n, rnd), map_column('uint8', five, n, rnd), map_column('uint8', ['solo'], n, rnd),
                                                      int_column('uint32', -25, n, rnd)]),
        'three-hundred-u16': layout('@w', '', [map_column('uint16', many, n, rnd), int_column('uint16', None, n, rnd), map_column('uint16', [''], n, rnd)]),
    }


def edge_layouts(n):
    """1(c): prefix 0 / 1 / 255 / 256 bytes, suffix 0 / 256, 0 / 1 / 5 / 32 columns (small numbers and short strings: what is tested is
    where the pieces of a line land)."""
    rnd = random.Random(99)
    kinds = [lambda: int_column('uint8', None, n, rnd), lambda: int_column('uint16', None, n, rnd), lambda: map_column('uint8', ['', 'ab', 'c'], n, rnd),
             lambda: int_column('uint32', -25, n, rnd), lambda: int_column('uint8', 1, n, rnd)]
    cols = lambda k: [kinds[i % len(kinds)]() for i in range(k)]
    text = lambda k: ''.join(chr(33 + (11 * i) % 90) for i in range(k))
    out = {}
    for p, s, k in [(0, 0, 0), (1, 0, 0), (256, 256, 0), (0, 0, 1), (1, 0, 1), (0, 256, 1), (255, 0, 5), (0, 0, 5), (255, 256, 5), (256, 0, 32), (0, 0, 32), (1, 256, 32)]:
        out['prefix%d-suffix%d-columns%d' % (p, s, k)] = layout(text(p), text(s)[::-1], cols(k))
    return out


def sweep_layout(n, length):
    """1(d): one mapping column whose three strings all have `length` bytes."""
    return layout('@', '', [map_column('uint8', [_ramp(j, length) for j in range(3)], n, random.Random(length))])
