"""The read trimmer's definition (include/uqhip.h) in plain Python, for the tests: nothing here comes from the product."""
U32 = 0xFFFFFFFF
TRIM_N = 1
OFF = {'head': 0, 'tail': 0, 'crop': U32, 'polyg': 0, 'q5': 0, 'q3': 0, 'flags': 0}
FIELDS = ('reads_in', 'bases_in', 'bytes_in', 'reads_trimmed', 'bases_out', 'bytes_out',
          'cut_fixed', 'cut_polyg', 'cut_q5', 'cut_q3', 'cut_n', 'emptied', 'len_mismatch')


def steps(**kw):
    return dict(OFF, **kw)


def q(b):
    return min(max(b - 33, 0), 93)


def records(text):
    """The records of a text as lists of their four lines, each without its '\\n'."""
    lines = bytes(text).split(b'\n')
    assert lines[-1] == b'' and (len(lines) - 1) % 4 == 0
    return [lines[4 * r:4 * r + 4] for r in range((len(lines) - 1) // 4)]


def is_g(b): return b in b'Gg'
def is_n(b): return b in b'Nn'


def quality_sequential(u, a, b, t3, t5):
    """(a', b') of step 3: the two running sums as the definition writes them (0 switches an end off)."""
    a2, b2 = a, b
    if t3:
        acc = best = 0
        for i in range(b - 1, a - 1, -1):
            acc += t3 - q(u[i])
            if acc < 0: break
            if acc > best: best, b2 = acc, i
    if t5:
        acc = best = 0
        for i in range(a, b):
            acc += t5 - q(u[i])
            if acc < 0: break
            if acc > best: best, a2 = acc, i + 1
    return a2, b2


def quality_closed(u, a, b, t3, t5):
    """The same in closed form: suffix (prefix) sums, the last (first) negative one, the highest positive one beyond it."""
    a2, b2 = a, b
    if t3:
        S, acc = {}, 0
        for i in range(b - 1, a - 1, -1):
            acc += t3 - q(u[i]); S[i] = acc
        stop = max([i for i in range(a, b) if S[i] < 0], default=a - 1)
        cand = [i for i in range(stop + 1, b) if S[i] > 0]
        if cand:
            top = max(S[i] for i in cand)
            b2 = max(i for i in cand if S[i] == top)
    if t5:
        S, acc = {}, 0
        for i in range(a, b):
            acc += t5 - q(u[i]); S[i] = acc
        stop = min([i for i in range(a, b) if S[i] < 0], default=b)
        cand = [i for i in range(a, stop) if S[i] > 0]
        if cand:
            top = max(S[i] for i in cand)
            a2 = min(i for i in cand if S[i] == top) + 1
    return a2, b2


def window(c, s, u, quality=quality_sequential):
    """-> (a, b, cuts) of one record; cuts is None where the two lines differ in length (the record stays as it is)."""
    if len(s) != len(u): return 0, len(s), None
    L = len(s)
    cut = dict.fromkeys(('fixed', 'polyg', 'q5', 'q3', 'n'), 0)
    a = min(c['head'], L)
    b = L - min(c['tail'], L - a)
    if c['crop'] != U32: b = min(b, a + c['crop'])
    cut['fixed'] = L - (b - a)
    g = 0
    while g < b - a and is_g(s[b - 1 - g]): g += 1
    if c['polyg'] > 0 and g >= c['polyg']:
        b -= g; cut['polyg'] = g
    a1, b1 = quality(u, a, b, c['q3'], c['q5'])
    cut['q3'] = b - b1
    a1 = min(a1, b1)
    cut['q5'] = a1 - a
    a, b = a1, b1
    if c['flags'] & TRIM_N:
        while a < b and is_n(s[a]): a += 1; cut['n'] += 1
        while b > a and is_n(s[b - 1]): b -= 1; cut['n'] += 1
    return a, b, cut


def run(text, c, first=0, n=None, quality=quality_sequential):
    """-> (windows [(a, b)], dst, trimmed text, report) of the records [first, first + n)."""
    recs = records(text)
    if n is None: n = len(recs) - first
    rep = dict.fromkeys(FIELDS, 0)
    wins, dst, out = [], [0], bytearray()
    for qn, s, p, u in recs[first:first + n]:
        a, b, cut = window(c, s, u, quality)
        wins.append((a, b))
        rep['reads_in'] += 1; rep['bases_in'] += len(s); rep['bytes_in'] += len(qn) + len(s) + len(p) + len(u) + 4
        if cut is None:
            rep['len_mismatch'] += 1
            out += qn + b'\n' + s + b'\n' + p + b'\n' + u + b'\n'
            rep['bases_out'] += len(s)
        else:
            for k, v in cut.items(): rep['cut_' + k] += v
            rep['reads_trimmed'] += (a, b) != (0, len(s))
            rep['emptied'] += a == b and len(s) > 0
            rep['bases_out'] += b - a
            out += qn + b'\n' + s[a:b] + b'\n' + p + b'\n' + u[a:b] + b'\n'
        dst.append(len(out))
    rep['bytes_out'] = len(out)
    return wins, dst, bytes(out), rep


def trimmed(text, c):
    return run(text, c)[2]
