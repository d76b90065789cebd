"""CPU: the record fingerprint uqfp1.  The plain-Python statement (tests/fingerprint_ref.py) against the known answers
of the definition, uq_fingerprint_host (the sequential C++ twin in libuqhip.so) against the statement, the properties the CLI's diagnosis
rests on, and what the fingerprint says about the reference-written containers of tests/golden."""
import glob
import os
import random

import numpy as np
import pytest

import fingerprint_ref as F
import uq_oracle as O
from uq_amd import ops

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

V1 = b'@r1\nACGT\n+\nIIII\n'
V2 = b'@r1\nACGT\n+r1\nIIII\n@r2\nACGTACGTA\n+\nIIIIIIII#\n'
V3 = b'@r2\nACGTACGTA\n+\nIIIIIIII#\n'
KNOWN1 = dict(reads=1, bases=4, plus_text=0, qname=0x4d50a18b5486266b, dna=0x2e1638cb2c229290, qual=0x57cbd55ef507bb3e,
              pairs=0x1912c09dcdb40199, records=0xfd984cb49b884bef, ordered=0x629d30cdb7d2a328)
KNOWN2 = dict(reads=2, bases=13, plus_text=1, qname=0xf9a7da680c1e2af9, dna=0xbd3b6caf213cf20e, qual=0x50894e16f3a4d990,
              pairs=0xc6459321874d0f2b, records=0xe69785bca92f2b3a, ordered=0x564dd5e0e14645ac)
KNOWN3_ORDERED = 0xf3b0a5132973a284


def text_of(records):
    return b''.join(b'\n'.join(r) + b'\n' for r in records)


def differing(a, b):
    return {k for k in F.FIELDS if a[k] != b[k]}


@pytest.mark.parametrize('fingerprint', [F.fingerprint, lambda t, **kw: ops.fingerprint_host(t, index_base=kw.get('read_index_base', 0))],
                         ids=['python', 'uq_fingerprint_host'])
def test_known_answers(fingerprint):
    assert fingerprint(V1) == KNOWN1
    assert fingerprint(V2) == KNOWN2
    v3 = fingerprint(V3, read_index_base=1)
    assert v3['ordered'] == KNOWN3_ORDERED
    assert (v3['ordered'] + KNOWN1['ordered']) % 2 ** 64 == KNOWN2['ordered']


def test_mix_is_synths_splitmix_without_the_increment():
    from uq_amd import synth
    for x in (0, 1, 2 ** 64 - 1, 0x0123456789ABCDEF):
        assert synth.splitmix64(x) == F.mix(x + F.K)


def random_records(rnd, n, lo, hi):
    line = lambda: bytes(rnd.randrange(32, 127) for _ in range(rnd.randint(lo, hi)))
    return [(b'@' + line(), line(), b'+' + (line() if rnd.random() < 0.3 else b''), line()) for _ in range(n)]


def test_host_twin_equals_the_statement_on_random_records():
    rnd = random.Random(20261019)
    text = text_of(random_records(rnd, 300, 0, 40))
    assert ops.fingerprint_host(text) == F.fingerprint(text)


def test_host_twin_on_every_length_around_the_word_size():
    lengths = (0, 1, 7, 8, 9, 15, 16, 17)
    rnd = random.Random(3)
    line = lambda L: bytes(rnd.randrange(33, 127) for _ in range(L))
    recs = [(line(a), line(b), b'+', line(c)) for a in lengths for b in lengths for c in lengths]     # (a QNAME line of length 0 has no '@': the hash does not care)
    text = text_of(recs)
    assert ops.fingerprint_host(text) == F.fingerprint(text)
    for L in lengths:                                               # and one at a time, so that a wrong length cannot hide in the sum
        one = text_of([(line(L), line(L), b'+', line(L))])
        assert ops.fingerprint_host(one) == F.fingerprint(one), L


def test_host_twin_on_one_long_read():
    rnd = random.Random(4)
    seq = bytes(rnd.choice(b'ACGTN') for _ in range(70000)); qual = bytes(rnd.randrange(33, 75) for _ in range(70000))
    text = text_of([(b'@ont:1', seq, b'+', qual)])
    assert ops.fingerprint_host(text) == F.fingerprint(text)


def test_pieces_add_up_to_the_whole():
    rnd = random.Random(6)
    text = text_of(random_records(rnd, 50, 0, 40))
    whole = F.fingerprint(text)
    ls = ops.host_line_starts(text)
    for cuts in ((0, 50), (0, 1, 50), (0, 17, 18, 49, 50)):
        pieces = list(zip(cuts, cuts[1:]))
        rnd.shuffle(pieces)
        total = dict.fromkeys(F.FIELDS, 0)
        for a, b in pieces:
            part = ops.fingerprint_host(text, ls, first_read=a, nreads=b - a, index_base=a)
            assert part == F.fingerprint(text, a, b - a, read_index_base=a)
            total = F.add(total, part)
        assert total == whole
    # an index base shifts `ordered` and nothing else
    assert differing(ops.fingerprint_host(text, index_base=5), whole) == {'ordered'}


def test_permuting_records_changes_ordered_only():
    rnd = random.Random(7)
    recs = random_records(rnd, 40, 1, 30)
    a = F.fingerprint(text_of(recs))
    rnd.shuffle(recs)
    assert differing(F.fingerprint(text_of(recs)), a) == {'ordered'}
    assert differing(ops.fingerprint_host(text_of(recs)), a) == {'ordered'}


def test_line_3_enters_plus_text_only():
    rnd = random.Random(8)
    recs = [(q, s, b'+', u) for q, s, _, u in random_records(rnd, 10, 1, 30)]
    a = F.fingerprint(text_of(recs))
    assert a['plus_text'] == 0
    for p in (b'+x', b'+' + recs[3][0][1:], b'', b'-', b'++'):
        recs[3] = (recs[3][0], recs[3][1], p, recs[3][3])
        b = ops.fingerprint_host(text_of(recs))
        assert differing(b, a) == {'plus_text'} and b['plus_text'] == 1 and b == F.fingerprint(text_of(recs))


def test_a_rewritten_qname_leaves_the_pairs_alone():
    """an integer QNAME field loses its leading zeros."""
    a = F.fingerprint(b'@r:007\nACGT\n+\nIIII\n@r:8\nAC\n+\nII\n')
    b = F.fingerprint(b'@r:7\nACGT\n+\nIIII\n@r:8\nAC\n+\nII\n')
    assert differing(a, b) == {'qname', 'records', 'ordered'}
    assert differing(ops.fingerprint_host(b'@r:7\nACGT\n+\nIIII\n@r:8\nAC\n+\nII\n'), a) == {'qname', 'records', 'ordered'}


def test_trailing_nul_bytes_and_the_length_are_told_apart():
    hashes = [F.line_hash(2, b) for b in (b'A', b'A\0', b'A\0\0', b'', b'\0', b'\0' * 8, b'\0' * 9, b'A' + b'\0' * 7, b'A' + b'\0' * 8)]
    assert len(set(hashes)) == len(hashes)
    fp = [ops.fingerprint_host(text_of([(b'@q', b, b'+', b)]))['dna'] for b in (b'A', b'A\0', b'', b'\0', b'\0' * 8, b'\0' * 9)]
    assert len(set(fp)) == len(fp)
    assert F.line_hash(1, b'A') != F.line_hash(2, b'A')                         # ... and the line classes by their tag


def golden_classes():
    """name -> 'ordered' / 'records' / 'neither' for every reference-written container that has its input: the input text against the
    oracle's decode of the container.  A decoder that stops (Q9) is 'neither'."""
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLD, '*.uQ'))):
        name = os.path.basename(path)[:-3]
        fq = os.path.join(GOLD, name + '.fastq')
        if not os.path.exists(fq): continue
        a = F.fingerprint(open(fq, 'rb').read())
        cfg, members = O.read_tar(path)
        try:
            b = F.fingerprint(O.decode(cfg, members).encode('latin-1'))
        except (IndexError, KeyError, ValueError):
            out[name] = ('neither', cfg); continue
        same_size = a['reads'] == b['reads'] and a['bases'] == b['bases']
        out[name] = ('ordered' if same_size and a['ordered'] == b['ordered'] else 'records' if same_size and a['records'] == b['records'] else 'neither', cfg)
    return out


def test_the_fingerprint_separates_the_golden_containers():
    """DESIGN.md section 19's table: 25 containers give their reads back in order, 19 as a multiset -- exactly the sorted ones -- and the two
    Q9 files (a new N quality code no decoder can map back) neither."""
    import sys
    sys.path.insert(0, GOLD)
    import inflate_inputs                                           # the larger text fixtures are committed compressed
    inflate_inputs.inflate(GOLD)
    cls = golden_classes()
    by = {c: sorted(n for n, (k, _) in cls.items() if k == c) for c in ('ordered', 'records', 'neither')}
    print({c: len(v) for c, v in by.items()})
    assert len(by['ordered']) == 25 and len(by['records']) == 19
    assert by['neither'] == ['fixed_n_newcode', 'two_ntrick_bases']
    is_sorted = lambda cfg: cfg['sort'] not in ([None], None)
    assert all(is_sorted(cls[n][1]) for n in by['records'])
    assert not any(is_sorted(cls[n][1]) for n in by['ordered'])
