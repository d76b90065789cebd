"""CPU: the --bin-qual specification (uq_amd/binqual.py), its argument checks, and the host twin uq_requantise_qualities_host against
the numpy reference (tests/binqual_ref.py)."""
import random

import numpy as np
import pytest

import binqual_ref as R
from uq_amd import binqual, ops, uq
from uq_amd._lib import UqHipError
from uq_amd.uq import UqError

ILLUMINA8 = [(3, 9, 6), (10, 19, 15), (20, 24, 22), (25, 29, 27), (30, 34, 33), (35, 39, 37), (40, 93, 40)]
FOUR_LEVEL = [(3, 14, 12), (15, 30, 23), (31, 93, 37)]


def table_of(bins):
    t = list(range(256))
    for lo, hi, q in bins:
        for v in range(lo, hi + 1): t[33 + v] = 33 + q
    return t


def text_of(records):
    return b''.join(b'\n'.join(r) + b'\n' for r in records)


def line(rnd, L, alphabet=None):
    if alphabet: return bytes(rnd.choice(alphabet) for _ in range(L))
    return bytes(rnd.randrange(33, 127) for _ in range(L))


def mixed_text(seed=5):
    """Qualities of every length 0..33, 1-base reads with one-character names, a 70 000-base read between short ones."""
    rnd = random.Random(seed)
    recs = [(b'@r%d' % L, line(rnd, L, b'ACGTN'), b'+', line(rnd, L)) for L in range(34)]
    recs += [(b'@' + bytes([97 + i % 26]), line(rnd, 1, b'ACGT'), b'+', line(rnd, 1)) for i in range(60)]
    recs += [(b'@long', line(rnd, 70000, b'ACGT'), b'+', line(rnd, 70000))]
    recs += [(b'@s%d' % i, line(rnd, 5 + i, b'ACGT'), b'+', line(rnd, 5 + i)) for i in range(20)]
    return text_of(recs), len(recs)


# ------------------------------------------------------------------ the parser
@pytest.mark.parametrize('name,bins', [('illumina8', ILLUMINA8), ('4level', FOUR_LEVEL)])
def test_presets_entry_by_entry(name, bins):
    lut = binqual.parse(name)
    assert isinstance(lut, bytes) and len(lut) == 256
    assert list(lut) == table_of(bins)
    for v in (0, 1, 2): assert lut[33 + v] == 33 + v                       # the no-call quality keeps to itself
    assert all(lut[b] == b for b in list(range(33)) + [127] + list(range(128, 256)))


def test_explicit_form_round_trips():
    for name in ('illumina8', '4level'):
        assert binqual.parse(binqual.explicit(name)) == binqual.parse(name)
    spec = '0-1:0,2:2,5-7:6,93:90'
    assert binqual.explicit(spec) == spec
    assert list(binqual.parse(spec)) == table_of([(0, 1, 0), (2, 2, 2), (5, 7, 6), (93, 93, 90)])
    assert binqual.ranges(' 5-7:6 , 2:2 ') == [(5, 7, 6), (2, 2, 2)]


@pytest.mark.parametrize('spec', ['3-9:6,9-12:10', '3-9:6,5:5', '9-3:6', '3-94:6', '3-9:94', '94:1', '', '   ', 'illumina9', 'nope',
                                  '3-9', '3-9:6:7', 'a-9:6', '3-9:-6', '3-9:6,,'])
def test_refusals(spec):
    with pytest.raises(UqError):
        binqual.parse(spec)


# ------------------------------------------------------------------ argument checks
def args_of(tmp_path, *flags):
    p = tmp_path / 'x.fastq'
    p.write_bytes(b'@a\nA\n+\nI\n')
    return uq.build_parser().parse_args(['-i', str(p)] + list(flags))


def test_validate_args(tmp_path):
    with pytest.raises(UqError):
        uq.validate_args(args_of(tmp_path, '--bin-qual', 'illumina8', '--decode'))
    with pytest.raises(UqError):
        uq.validate_args(args_of(tmp_path, '--bin-qual', '9-3:1'))
    for flags in (['--peek'], ['--test'], ['--gz'], ['--verify'], ['--fingerprint'], []):
        a = uq.validate_args(args_of(tmp_path, '--bin-qual', 'illumina8', *flags))
        assert a.bin_qual == 'illumina8'
    assert uq.validate_args(args_of(tmp_path)).bin_qual is None


# ------------------------------------------------------------------ the host twin
@pytest.mark.parametrize('lut', [R.ALL_I, binqual.parse('illumina8'), binqual.parse('4level')], ids=['all-I', 'illumina8', '4level'])
def test_host_twin_against_reference(lut):
    text, n = mixed_text()
    want, changed = R.apply(text, lut)
    got, cnt = ops.requantise_qualities_host(text, lut)
    assert got.tobytes() == want and cnt == changed
    assert changed > 0


def test_host_twin_subranges_and_empty():
    text, n = mixed_text(6)
    lut = binqual.parse('illumina8')
    for first, cnt in ((0, 1), (1, 33), (34, 60), (94, 1), (93, 3), (n - 1, 1), (17, 0), (n, 0), (0, 0)):
        want, changed = R.apply(text, lut, first, cnt)
        got, c = ops.requantise_qualities_host(text, lut, first_read=first, nreads=cnt)
        assert got.tobytes() == want and c == changed, (first, cnt)
        if cnt == 0: assert want == text and c == 0
    # pieces add up to the whole
    a, c1 = ops.requantise_qualities_host(text, lut, first_read=0, nreads=50)
    b, c2 = ops.requantise_qualities_host(a, lut, first_read=50, nreads=n - 50)
    whole, c = ops.requantise_qualities_host(text, lut)
    assert b.tobytes() == whole.tobytes() and c1 + c2 == c


def test_hostile_table_touches_quality_bytes_only():
    text, n = mixed_text(7)
    got, _ = ops.requantise_qualities_host(text, R.ALL_I)
    got = got.tobytes()
    a, b = text.split(b'\n'), got.split(b'\n')
    assert len(a) == len(b) == 4 * n + 1
    for k, (x, y) in enumerate(zip(a, b)):
        if k % 4 == 3: assert y == b'I' * len(x)
        else: assert y == x


def test_table_validation():
    text, _ = mixed_text(8)
    bad = bytearray(range(256)); bad[ord('I')] = 10
    with pytest.raises(UqHipError):
        ops.requantise_qualities_host(text, bytes(bad))
    with pytest.raises(UqHipError):
        ops.requantise_qualities_host(text, b'\n' * 256)
    with pytest.raises(ValueError):
        ops.requantise_qualities_host(text, b'I' * 255)


def test_identity_and_idempotence():
    text, _ = mixed_text(9)
    got, c = ops.requantise_qualities_host(text, R.IDENTITY)
    assert got.tobytes() == text and c == 0
    lut = binqual.parse('illumina8')
    once, c1 = ops.requantise_qualities_host(text, lut)
    twice, c2 = ops.requantise_qualities_host(once, lut)
    assert c1 > 0 and c2 == 0 and twice.tobytes() == once.tobytes()
