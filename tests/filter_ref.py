"""The read filter's definition (include/uqhip.h) in plain Python, for the tests: nothing here comes from the product."""
M64 = (1 << 64) - 1
K = 0x9E3779B97F4A7C15
U32 = 0xFFFFFFFF
SAMPLE = 1
OFF = {'min_len': 0, 'max_len': U32, 'max_n': U32, 'min_mean_q': 0, 'sample_threshold': 0, 'seed': 0, 'flags': 0}
FIELDS = ('reads_in', 'bases_in', 'bytes_in', 'reads_out', 'bases_out', 'bytes_out',
          'fail_min_len', 'fail_max_len', 'fail_max_n', 'fail_mean_q', 'fail_sample', 'fail_mate')
BITS = (('fail_min_len', 1), ('fail_max_len', 2), ('fail_max_n', 4), ('fail_mean_q', 8), ('fail_sample', 16))


def mix(x):
    x &= M64
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def criteria(**kw):
    return dict(OFF, **kw)


def q(b):
    return min(max(b - 33, 0), 93)


def records(text):
    """The records of a text as lists of their four lines, each without its '\\n'."""
    lines = bytes(text).split(b'\n')
    assert lines[-1] == b'' and (len(lines) - 1) % 4 == 0
    return [lines[4 * r:4 * r + 4] for r in range((len(lines) - 1) // 4)]


def sample_bit(c, w):
    return bool(c['flags'] & SAMPLE) and mix(c['seed'] + K * (w + 1)) >= c['sample_threshold']


QTAB = bytes(q(b) for b in range(256))


def verdict(c, unit, g, s, u):
    v = 0
    if len(s) < c['min_len']: v |= 1
    if len(s) > c['max_len']: v |= 2
    if s.count(b'N') + s.count(b'n') > c['max_n']: v |= 4
    if sum(u.translate(QTAB)) < c['min_mean_q'] * len(u): v |= 8      # SUM_p q(u[p])
    if sample_bit(c, g // unit): v |= 16
    return v


def verdicts(text, c, unit=1, first=0, n=None, index_base=0):
    recs = records(text)
    if n is None: n = len(recs) - first
    return [verdict(c, unit, index_base + i, recs[first + i][1], recs[first + i][3]) for i in range(n)]


def run(text, c, unit=1, first=0, n=None, index_base=0):
    """-> (verdicts, src, dst, filtered text, report) of the records [first, first + n)."""
    recs = records(text)
    if n is None: n = len(recs) - first
    assert n % unit == 0
    v = verdicts(text, c, unit, first, n, index_base)
    size = [sum(len(l) + 1 for l in r) for r in recs]
    start = [0]
    for s in size: start.append(start[-1] + s)
    rep = dict.fromkeys(FIELDS, 0)
    rep['reads_in'] = n
    rep['bases_in'] = sum(len(recs[first + i][1]) for i in range(n))
    rep['bytes_in'] = start[first + n] - start[first]
    for name, bit in BITS: rep[name] = sum(1 for x in v if x & bit)
    src, dst, out = [], [0], bytearray()
    for w in range(n // unit):
        mine = range(w * unit, (w + 1) * unit)
        if all(v[i] == 0 for i in mine):
            r0 = first + w * unit
            src.append(start[r0])
            out += bytes(text)[start[r0]:start[r0 + unit]]
            dst.append(len(out))
            rep['reads_out'] += unit
            rep['bases_out'] += sum(len(recs[first + i][1]) for i in mine)
        else:
            rep['fail_mate'] += sum(1 for i in mine if v[i] == 0)
    rep['bytes_out'] = len(out)
    return v, src, dst, bytes(out), rep


def filtered(text, c, unit=1):
    return run(text, c, unit)[3]
