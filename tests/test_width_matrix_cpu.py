"""The reference side of the symbol-width matrix, without a GPU: for every case of width_matrix_inputs (base width 1 .. 8 x quality
width 1 .. 8 x fixed / variable x three N-trick forms x two alphabets = 768) the three packers of the oracle -- the faithful per-base
loop, the closed big-integer form and the C restatement -- agree, and the C unpack gives the input back.  test_gpu_width_matrix.py holds
the HIP kernels to oracle_c on the same cases; this file is what makes oracle_c a reference there, and it asserts that each case
covers what it is built for (width, lengths, which kernel family its alphabet selects).

The only exclusion: the 'new' N-trick form (Q9: a quality code beyond the alphabet) is not decodable by the reference, so its 256
cases are packed but not decoded -- the rule the existing tests apply."""
import numpy as np
import pytest

import oracle_c
import uq_oracle as O
import width_matrix_inputs as W

CASES = W.all_cases()


def pack_is_lookup_free(c):
    """The packer's `fast` predicate (uq_amd/csrc/pack.hip, pack_impl), restated: bases ACGT at two bits, or at three bits up to
    eight 7-bit characters that three of their bits tell apart; qualities one contiguous run below 128 coded in order; at most one
    N-trick base, its code and character below 128."""
    b = [ord(x) for x in c['bases']]; q = [ord(x) for x in c['qualities']]
    bd = c['bits_per_base']
    two = bd == 2 and c['bases'] == 'ACGT'
    three = bd == 3 and 1 <= len(b) <= 8 and all(1 <= ch < 128 for ch in b) and \
        any(len(set((ch >> sh) & 7 for ch in b)) == len(b) for sh in range(5))
    contiguous = len(q) >= 1 and q == sorted(q) and q[-1] - q[0] + 1 == len(q) and q[-1] < 128
    ntrick = len(c['N_qual']) <= 1 and all(code < 128 and ord(ch) < 128 for ch, code in c['N_qual'].items())
    return (two or three) and contiguous and ntrick


def decode_is_lookup_free(c):
    """fast_alphabet() of uq_amd/csrc/codes.h, restated: 2- or 3-bit bases (all four at two bits), at most 7-bit qualities whose
    characters are code + the first one, no N code among the codes the alphabet leaves free, at most one among its own."""
    q = [ord(x) for x in c['qualities']]
    bd, bq = c['bits_per_base'], c['bits_per_quality']
    nq = min(len(q), 1 << bq)
    ok = bd in (2, 3) and bq <= 7 and nq >= 1 and all(q[i] == q[0] + i for i in range(nq))
    codes = list(c['N_qual'].values())
    ok = ok and not any(nq <= v < (1 << bq) for v in codes) and sum(v < nq for v in codes) <= 1
    if bd == 2: ok = ok and len(c['bases']) >= 4
    return bool(ok)


def test_matrix_size_and_the_one_exclusion():
    assert len(CASES) == len(set(CASES)) == 8 * 8 * 2 * 3 * 2 == 768
    skipped = [p for p in CASES if not W.case(*p)['decodable']]
    assert len(skipped) == 256 and all(p[3] == 'new' for p in skipped)            # exactly the Q9 third, nothing else
    assert all(W.case(*p)['decodable'] for p in CASES if p[3] != 'new')
    # the six fixed cases of a width pair take all five lengths between them
    for bd in range(1, 9):
        for bq in range(1, 9):
            assert {W.case(bd, bq, False, nt, al)['dna_max'] for nt in W.NTRICKS for al in W.ALPHABETS} == set(W.FIXED_LENGTHS)


@pytest.mark.parametrize('bd,bq,variable,ntrick,alphabet', CASES, ids=[W.case_id(*p) for p in CASES])
def test_reference_packers_agree_and_unpack_is_the_input(bd, bq, variable, ntrick, alphabet):
    c = W.case(bd, bq, variable, ntrick, alphabet)
    n = c['n']
    # ---- the case covers what it is built for
    for b, alpha in ((bd, c['bases']), (bq, c['qualities'])):
        assert len(set(alpha)) == len(alpha) == W.SYMBOLS[b] and alpha == ''.join(sorted(alpha))
        assert (len(alpha) == 2) if b == 1 else (2 ** (b - 1) < len(alpha) <= 2 ** b)
        assert '\n' not in alpha and '\r' not in alpha and '\0' not in alpha
    assert 'N' not in c['bases'] and n == W.N_READS == 120
    assert c['bits_per_base'] == bd and c['bits_per_quality'] == bq and c['variable_read_lengths'] == variable
    lv = c['dna_max'] + (1 if variable else 0)
    assert c['dna_bytes_per_row'] == (bd * lv + 7) // 8 and c['quality_bytes_per_row'] == (bq * lv + 7) // 8
    if variable:
        assert set(c['lengths']) == set(W.VARIABLE_LENGTHS) and c['dna_max'] == 67
        # a partial group alone, whole groups alone, both; rows that end on a byte and rows that end inside one (L mod 8 = 0, 1, 2, 3, 5, 7)
        L = set(c['lengths'])
        assert any(l < 8 for l in L) and any(l % 8 == 0 for l in L) and any(l > 8 and l % 8 for l in L) and {l % 8 for l in L} == {0, 1, 2, 3, 5, 7}
    else:
        assert set(c['lengths']) == {c['dna_max']} and c['dna_max'] in W.FIXED_LENGTHS
    assert c['N_qual'] == {None: {}, 'shared': {'N': len(c['qualities']) - 1}, 'new': {'N': len(c['qualities']) + 1}}[ntrick]
    assert c['carry'] == (bool(c['N_qual']) and max(c['N_qual'].values()) >= 2 ** bq)
    assert c['carry'] == (ntrick == 'new' and bq <= 3)                              # 3 >= 2, 5 >= 4, 8 >= 8; 14 < 16 and so on
    if alphabet == 'scattered':
        assert not pack_is_lookup_free(c) and not decode_is_lookup_free(c)
    elif bd in (2, 3):
        # (a run of 100 or 150 characters from '!' passes 127: from 7 bits on the packer goes through its tables, at 8 the decoder too;
        # a NEW N code is never one the lookup-free decoder knows, and one that carries has no lookup-free packer that could hold it)
        assert pack_is_lookup_free(c) == (bq <= 6)
        assert decode_is_lookup_free(c) == (bq <= 7 and (ntrick != 'new' or c['carry']))
    else:
        assert not pack_is_lookup_free(c) and not decode_is_lookup_free(c)
    text = c['fastq']
    lines = O.read_lines(text)
    assert len(lines) == 4 * n and [len(l) - 1 for l in lines[1::4]] == c['lengths'] and lines[0] == '@r:0:0\n' and lines[-4] == '@r:119:2\n'
    if ntrick is not None:
        seq = ''.join(l[:-1] for l in lines[1::4]); qs = ''.join(l[:-1] for l in lines[3::4])
        nq = {q for s, q in zip(seq, qs) if s == 'N'}
        others = {q for s, q in zip(seq, qs) if s != 'N'}
        assert len(nq) == 1 and 1 <= seq.count('N') < len(seq) // 4 + 2
        assert (nq.isdisjoint(others) and nq == {c['qualities'][-1]}) if ntrick == 'shared' else nq == {c['qualities'][0]}
    # ---- pack: C oracle == closed form (where nothing carries) == the faithful loop on a prefix
    host = np.frombuffer(text, dtype=np.uint8)
    hls = oracle_c.index_lines(host)
    args = (c['bases'], c['qualities'], c['N_qual'])
    rd, rq, bad = oracle_c.pack(host, hls, 0, n, *args, bd, bq, variable, c['dna_bytes_per_row'], c['quality_bytes_per_row'])
    assert bad is None
    if not c['carry']:
        bd_, bq_ = O.encoder_bigint(lines, *args, c['dna_bytes_per_row'], c['quality_bytes_per_row'], bd, bq, variable)
        assert np.array_equal(rd, bd_) and np.array_equal(rq, bq_)
    ed, eq = O.encoder(lines, *args, c['dna_bytes_per_row'], c['quality_bytes_per_row'], bd, bq, variable, count=20)
    assert np.array_equal(rd[:20], ed) and np.array_equal(rq[:20], eq)
    # ---- decode: the C unpack gives the input lines back (Q9 excluded, see the module docstring)
    if not c['decodable']:
        assert ntrick == 'new'
        return
    seq, qt, ln, ubad = oracle_c.unpack(rd, rq, c)
    assert ubad is None and ln.tolist() == c['lengths']
    for r in range(n):
        assert seq[r, :ln[r]].tobytes().decode('latin-1') == lines[4 * r + 1][:-1], r
        assert qt[r, :ln[r]].tobytes().decode('latin-1') == lines[4 * r + 3][:-1], r
        assert not seq[r, ln[r]:].any() and not qt[r, ln[r]:].any()
