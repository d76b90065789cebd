"""FASTQ texts with adapters written into their reads, for the adapter step's tests (tests/test_adapter_cpu.py, tests/test_gpu_adapter.py,
tests/test_gpu_adapter_cli.py).  An adapter is put at a chosen start, so that it overlaps the line's end by a chosen length, with mismatches
at chosen places of the adapter."""
import glob
import os
import random

from filter_inputs import record, text

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(REPO, 'tests', 'golden', '*.fastq')))
ILLUMINA = b'AGATCGGAAGAGC'
A33 = b'AGATCGGAAGAGCACACGTCTGAACTCCAGTCA'       # TruSeq read 1, 33 bases
OTHER = {65: 67, 67: 71, 71: 84, 84: 65}          # a base that differs: A -> C -> G -> T -> A


def adapter(La, seed=0):
    """La letters: TruSeq's first bases, carried on at random (seed 0); another seed: random letters throughout."""
    rnd = random.Random(1000 + La + seed)
    return ((A33 if seed == 0 else b'') + bytes(rnd.choice(b'ACGT') for _ in range(64)))[:La]


def body(L, seed=0, alphabet=b'ACGT'):
    rnd = random.Random(seed * 7919 + L)
    return bytes(rnd.choice(alphabet) for _ in range(L))


def implant(seq, A, start, wrong=(), tail=None):
    """seq with the adapter A written at `start` (cut where the line ends: start > len(seq) - len(A) makes a partial match) and, where the line
    goes on behind it, `tail` or the bases that were there.  wrong: places j of the adapter that get another base."""
    a = bytearray(A)
    for j in wrong: a[j] = OTHER[a[j]]
    out = bytearray(seq)
    end = min(len(seq), start + len(a))
    out[start:end] = a[:end - start]
    if tail is not None: out[end:] = tail[:len(seq) - end]
    return bytes(out)


def at_end(L, A, overlap, wrong=(), seed=0, alphabet=b'CT'):
    """A line of L bases whose last `overlap` bases are the adapter's first (overlap <= len(A): partial unless equal)."""
    return implant(body(L, seed, alphabet), A, L - overlap, wrong)


def records_of(text_):
    lines = bytes(text_).split(b'\n')
    return [lines[4 * r:4 * r + 4] for r in range((len(lines) - 1) // 4)]


def implant_text(text_, A, every=3, seed=5, limit=None, partial=True, wrong=True, dimers=True, placed=None):
    """The records of a text (the first `limit`), the adapter written into every `every`-th one whose lines agree in length: in turn in full
    somewhere inside, over the line's end (partial=False: inside, for parameters under which no partial match exists), at the very start (an
    emptied read; dimers=False: inside), and in full with one wrong base (wrong=False: with none, for parameters that allow no mismatch).
    placed: a list that receives (record, kind, line length, start, wrong places) of every adapter written."""
    rnd = random.Random(seed)
    out, k = [], 0
    for i, (qn, s, p, u) in enumerate(records_of(text_)[:limit]):
        L = len(s)
        if i % every == 0 and len(s) == len(u) and L >= 1:
            kind = k % 4; k += 1
            if kind == 1 and not partial: kind = 0
            if kind == 3 and not wrong: kind = 0
            if kind == 2 and not dimers: kind = 0
            if kind == 0 or kind == 3:
                start = rnd.randrange(1, max(L - len(A), 1) + 1) if L > 1 else 0
                bad = (rnd.randrange(len(A)),) if kind == 3 and len(A) >= 10 else ()
            elif kind == 1:
                start, bad = max(L - rnd.randrange(1, len(A) + 1), 0), ()
            else:
                start, bad = 0, ()
            s = implant(s, A, start, wrong=bad)
            if placed is not None: placed.append((i, kind, L, start, bad))
        out.append(qn + b'\n' + s + b'\n' + p + b'\n' + u + b'\n')
    return b''.join(out)


def seeded(n, A, seed=30, lo=0, hi=120, every=3, A2=None, **kinds):
    """n random records of lo .. hi bases (N and lower case among them), the adapter written into every `every`-th one (A2, when given, into
    those of odd index: the second mates of an interleaved file)."""
    rnd = random.Random(seed)
    recs = []
    for i in range(n):
        L = rnd.randrange(lo, hi + 1)
        seq = bytes(rnd.choice(b'ACGT') if rnd.random() > 0.02 else rnd.choice(b'Nnacgt') for _ in range(L))
        qual = bytes(rnd.randrange(35, 75) for _ in range(L))
        recs.append(record(b'r%d' % i, seq, qual))
    t = text(recs)
    if A2 is None: return implant_text(t, A, every, seed, **kinds)
    even = implant_text(t, A, every, seed)
    odd = implant_text(t, A2, every, seed + 1)
    re_, ro = records_of(even), records_of(odd)
    return b''.join(b'\n'.join(re_[i] if i % 2 == 0 else ro[i]) + b'\n' for i in range(n))


def threshold_edges(A, err=10, ms=(9, 10, 19, 20)):
    """For m in ms (where (m * err) / 100 steps) and k = (m * err) // 100: lines of 40 N (which match nothing: no candidate in front of the adapter) with m adapter bases at the end (a partial
    match of m, when m < len(A)) or, for m = len(A), with the whole adapter inside, with exactly k and k + 1 wrong bases, the wrong ones
    including the first adapter base or the last compared one.  -> (name, line, m, wrong places)."""
    out = []
    for m in ms:
        if m > len(A): continue
        k = (m * err) // 100
        for nwrong in (k, k + 1):
            for first in (True, False):
                if nwrong == 0 and not first: continue
                places = ([0] if first else [m - 1]) + [j for j in range(2, m - 1)][:max(nwrong - 1, 0)]
                places = sorted(places[:nwrong])
                Am = A[:m]
                if m == len(A): line = implant(body(40 + m, m, b'N'), A, 17, places, tail=body(64, m + 1, b'N'))
                else: line = at_end(40, Am, m, places, seed=m, alphabet=b'N')
                out.append((b'e%d_%d_%d' % (m, nwrong, first), line, m, places))
    return out
