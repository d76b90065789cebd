"""The 3' adapter step's definition (include/uqhip.h) in plain Python, for the tests: nothing here comes from the product."""
import trim_ref

FRESH, PAIRED = 1, 2
FIELDS = ('reads_in', 'bases_in', 'bases_out', 'reads_cut', 'full', 'partial', 'mate2', 'emptied', 'len_mismatch')
PRESETS = {'illumina': 'AGATCGGAAGAGC', 'nextera': 'CTGTCTCTTATA', 'smallrna': 'TGGAATTCTCGG'}


def cls(b):
    """The QC tables' class of a byte: A 0, C 1, G 2, T 3 in either case, N 4, anything else 5."""
    return {ord('a'): 0, ord('c'): 1, ord('g'): 2, ord('t'): 3, ord('n'): 4}.get(b | 0x20, 5) if b < 128 else 5


def params(seq, seq2=None, err=10, overlap=3, flags=0):
    """seq / seq2: upper-case letters of ACGT (str or bytes)."""
    as_cls = lambda s: None if s is None else ['ACGT'.index(c) for c in (s.decode() if isinstance(s, bytes) else s)]
    return {'seq': as_cls(seq), 'seq2': as_cls(seq2), 'err': err, 'overlap': overlap, 'flags': flags}


def mismatches(s, p, A, m):
    return sum(1 for j in range(m) if cls(s[p + j]) != A[j])


def window(c, s, a, b, odd=False):
    """-> (b', kind) of a record whose two lines hold the same number of bytes: kind is None, 'full' or 'partial'."""
    A = c['seq2'] if (c['flags'] & PAIRED) and odd else c['seq']
    for p in range(a, b):
        m = min(len(A), b - p)
        if m < c['overlap']: continue
        k, bad = (m * c['err']) // 100, 0
        for j in range(m):                       # (mismatches(s, p, A, m) <= k, left as soon as it is decided)
            if cls(s[p + j]) != A[j]:
                bad += 1
                if bad > k: break
        if bad <= k:
            return p, 'full' if m == len(A) else 'partial'
    return b, None


def run(text, c, first=0, n=None, windows=None):
    """-> (windows [(a, b)], report, dst, cut text) of the records [first, first + n).  `windows`: the n windows received (needed unless FRESH
    is set, ignored when it is).  The text is made as trim_ref.run makes it: qn, s[a:b], p, u[a:b], the record as it is where Ls != Lu."""
    recs = trim_ref.records(text)
    if n is None: n = len(recs) - first
    rep = dict.fromkeys(FIELDS, 0)
    wins, dst, out = [], [0], bytearray()
    for i, (qn, s, p, u) in enumerate(recs[first:first + n]):
        rep['reads_in'] += 1
        if len(s) != len(u):
            rep['len_mismatch'] += 1; rep['bases_in'] += len(s); rep['bases_out'] += len(s)
            wins.append((0, len(s)))
            out += qn + b'\n' + s + b'\n' + p + b'\n' + u + b'\n'
        else:
            a, b = (0, len(s)) if c['flags'] & FRESH else windows[i]
            assert a <= b <= len(s)
            odd = (first + i) % 2 == 1
            b2, kind = window(c, s, a, b, odd)
            rep['bases_in'] += b - a; rep['bases_out'] += b2 - a
            if kind:
                rep['reads_cut'] += 1; rep[kind] += 1
                rep['mate2'] += bool(c['flags'] & PAIRED) and odd
                rep['emptied'] += b2 == a
            wins.append((a, b2))
            out += qn + b'\n' + s[a:b2] + b'\n' + p + b'\n' + u[a:b2] + b'\n'
        dst.append(len(out))
    return wins, rep, dst, bytes(out)


def cut(text, c, paired=False):
    """The text `--adapter` makes of `text` (no --trim in front: FRESH)."""
    return run(text, dict(c, flags=FRESH | (PAIRED if paired else 0)))[3]


def after_trim(text, steps, c, paired=False):
    """The text `--trim STEPS --adapter SPEC` makes: the trimmer's windows, narrowed."""
    wins = trim_ref.run(text, steps)[0]
    return run(text, dict(c, flags=PAIRED if paired else 0), windows=wins)[3]
