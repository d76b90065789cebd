"""CPU: 3' adapter removal (include/uqhip.h).  The host twin uq_adapter_mark_host against the pure-Python statement of the
definition (tests/adapter_ref.py) on the golden FASTQ files and on seeded records with the adapter written into a third of them, on the
threshold's edges, on N / lower case / '\\r', on given windows, mates, slices and lines of different lengths; the report's invariants; every
library error; the spec parser; what validate_args and the sharded tool refuse; header, binding and library agree; trim, adapter, plan and
copy in a row."""
import ctypes
import os
import re

import numpy as np
import pytest

import adapter_inputs as I
import adapter_ref as R
import trim_ref as TR
from filter_inputs import record, text as join
from uq_amd import _lib, adapters, ops, uq
from uq_amd._lib import UqHipError
from uq_amd.uq import UqError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['uq_adapter_report_init', 'uq_adapter_report_init_host', 'uq_adapter_mark', 'uq_adapter_mark_host']
LIMIT = 240                                   # records of a golden file that are taken (the reference is a Python loop per position)
# what test_the_conditions_hold_on_most_of_the_golden_set requires of the 87 golden files x 10 sets: how often the fifth-cut bound and the four
# kinds are asserted, and how many sets stay without the bound although some read reaches overlap = La (too few reads do: 10; a file of reads
# shorter than overlap = 3: 4)
FIFTH_ASSERTED, FOUR_KINDS_ASSERTED, FIFTH_UNREACHED = 752, 525, 14
# (La, err, overlap): every La, err and overlap the definition's edges name, overlap = La among them
SETS = [(1, 0, 1), (12, 10, 3), (13, 10, 3), (13, 0, 13), (32, 30, 1), (33, 10, 3), (63, 30, 3), (64, 0, 1), (64, 10, 64), (33, 30, 33)]


def host(text, c, first=0, n=None, windows=None, report=None):
    """uq_adapter_mark_host with the reference's parameters -> (windows, report)."""
    letters = lambda cl: None if cl is None else ''.join('ACGT'[k] for k in cl)
    p = ops.adapter_params(letters(c['seq']), letters(c['seq2']), c['err'], c['overlap'], c['flags'])
    w, rep = ops.adapter_mark_host(text, p, None, first, n, window=None if windows is None else np.array(windows, np.uint32).reshape(-1, 2), report=report)
    return [(int(a), int(b)) for a, b in w], rep


def check(text, c, first=0, n=None, windows=None, want=None):
    if want is None: want = R.run(text, c, first, n, windows)
    got = host(text, c, first, n, windows)
    assert got[0] == want[0]
    assert got[1] == want[1]
    rep = got[1]
    assert rep['reads_cut'] == rep['full'] + rep['partial']
    received = [(0, len(r[1])) for r in TR.records(text)[first:first + len(want[0])]] if c['flags'] & R.FRESH else windows
    assert rep['bases_in'] - rep['bases_out'] == sum(b - b2 for (a, b), (a2, b2), r in zip(received, want[0], TR.records(text)[first:]) if len(r[1]) == len(r[3]))
    return want


def occurs(rep, n, La=13, overlap=3):
    """The condition of the implanted inputs: a fifth of the records cut; a full and a partial match, an untouched and an emptied read.  (With
    overlap = La the definition has no partial match; an adapter of one base is found in every read that holds its letter, so none stays
    untouched.)"""
    return rep['reads_cut'] * 5 >= n and four_kinds(rep, La, overlap)


def four_kinds(rep, La=13, overlap=3):
    return bool(rep['full'] and rep['emptied'] and (rep['partial'] or overlap == La) and (rep['reads_cut'] < rep['reads_in'] or La == 1))


def implanted(raw, La, err, overlap, **kw):
    """A text with the adapter of La bases written into every third record, and what the definition promises of it, worked out from where the
    builder wrote (not from any search): (text, adapter, records, the number of records that MUST be cut, whether all four kinds must be
    there).  A written adapter must be cut when the m = min(La, L - start) bases of it that fit hold at most (m * err) / 100 of the wrong
    places and m >= overlap (the leftmost candidate lies there or left of it).  The four kinds -- as far as La and overlap admit them,
    see `occurs` -- are promised when two adapters each were written in full, over the line's end with overlap <= m < La (where
    overlap < La) and at the start of a line, and two records with equal lines were left alone."""
    A = I.adapter(La)
    placed = []
    text = I.implant_text(raw, A, partial=overlap < La, wrong=(La * err) // 100 > 0, placed=placed, **kw)
    recs = TR.records(text)
    must = {'full': 0, 'partial': 0, 'start': 0}
    for i, kind, L, start, bad in placed:
        m = min(La, L - start)
        if m < overlap or sum(1 for j in bad if j < m) > (m * err) // 100: continue
        must['start' if start == 0 else ('full' if m == La else 'partial')] += 1
    alone = sum(1 for i, r in enumerate(recs) if len(r[1]) == len(r[3]) and i not in {p[0] for p in placed})
    kinds = must['full'] >= 2 and must['start'] >= 2 and (must['partial'] >= 2 or overlap == La) and (alone >= 2 or La == 1)
    return text, A, len(recs), sum(must.values()), kinds


# ------------------------------------------------------------------ the twin
@pytest.mark.parametrize('path', I.GOLDEN, ids=[os.path.basename(p) for p in I.GOLDEN])
def test_twin_on_the_golden_files(path):
    raw = open(path, 'rb').read()
    for La, err, overlap in SETS:
        text, A, n, must, kinds = implanted(raw, La, err, overlap, limit=LIMIT)
        want = R.run(text, R.params(A, err=err, overlap=overlap, flags=R.FRESH))
        # the conditions first, on the reference's report: per file and parameter set, wherever the builder could reach them
        assert want[1]['reads_cut'] >= must
        if must * 5 >= n: assert want[1]['reads_cut'] * 5 >= n, (La, err, overlap, want[1])
        if kinds: assert four_kinds(want[1], La, overlap), (La, err, overlap, want[1])
        check(text, R.params(A, err=err, overlap=overlap, flags=R.FRESH), want=want)


def test_the_conditions_hold_on_most_of_the_golden_set():
    """How often test_twin_on_the_golden_files asserts its two conditions, counted over every golden file and parameter set from the
    builder's placements alone: the fifth-cut bound wherever an adapter that must be found was written into a fifth of the records -- which
    leaves out parameter sets whose overlap = La no read of the file reaches and, listed and bounded, FIFTH_UNREACHED others --,
    the four kinds wherever the file holds enough reads longer than the adapter."""
    total = fifth = four = 0
    missing = []
    for path in I.GOLDEN:
        raw = open(path, 'rb').read()
        longest = max((len(r[1]) for r in TR.records(raw)[:LIMIT]), default=0)
        for La, err, overlap in SETS:
            text, A, n, must, kinds = implanted(raw, La, err, overlap, limit=LIMIT)
            total += 1; fifth += must * 5 >= n; four += kinds
            if must * 5 < n and not (overlap == La and longest < La): missing.append((os.path.basename(path), La, err, overlap, must, n))
    assert total == len(I.GOLDEN) * len(SETS) >= 700
    assert fifth >= FIFTH_ASSERTED and four >= FOUR_KINDS_ASSERTED, (total, fifth, four)
    assert len(missing) <= FIFTH_UNREACHED, missing


def test_twin_on_seeded_records():
    for La, err, overlap in SETS:
        A = I.adapter(La)
        text = I.seeded(3000, A, seed=30 + La, lo=66, hi=140, partial=overlap < La, wrong=(La * err) // 100 > 0)
        want = check(text, R.params(A, err=err, overlap=overlap, flags=R.FRESH))
        assert occurs(want[1], 3000, La, overlap), (La, err, overlap, want[1])
    # short and empty lines among them
    text = I.seeded(1500, I.ILLUMINA, lo=0, hi=40)
    want = check(text, R.params(I.ILLUMINA, flags=R.FRESH))
    assert occurs(want[1], 1500) and any(len(r[1]) == 0 for r in TR.records(text))


def test_threshold_edges():
    cases = 0
    for m in (9, 10, 19, 20):
        # full matches: an adapter of m bases; partial ones: m bases of a longer adapter at the line's end
        for A, full in ((I.adapter(m), True), (I.adapter(33), False)):
            k = (m * 10) // 100
            for name, line, mm, wrong in I.threshold_edges(A, 10, (m,)):
                text = record(name, line)
                c = R.params(A, err=10, overlap=3, flags=R.FRESH)
                want = check(text, c)
                start = 17 if full else 40 - m
                hit = want[0][0] == (0, start)
                assert hit == (len(wrong) <= k), (name, wrong, want[0])
                if hit: assert want[1]['full' if full else 'partial'] == 1
                cases += 1
    assert cases >= 24


def test_n_lower_case_and_cr_in_the_compared_stretch():
    A = I.adapter(20)
    for bad, cut_at_10 in ((b'N', False), (b'n', False), (b'\r', False), (None, True)):
        for j in (0, 7, 19):
            s = bytearray(b'N' * 10 + A + b'N' * 5)
            if bad: s[10 + j:11 + j] = bad
            for err in (0, 10):                                                # 20 * 10 / 100 = 2: one odd byte passes, at err=0 it does not
                want = check(record(b'r', bytes(s)), R.params(A, err=err, flags=R.FRESH))
                assert (want[0][0] == (0, 10)) == (cut_at_10 or err == 10), (bad, j, err)
    lower = record(b'lc', b'N' * 10 + A.lower() + b'NN')
    assert check(lower, R.params(A, err=0, flags=R.FRESH))[0] == [(0, 10)]
    crlf = b'@r\r\n' + b'NNNN' + A[:6] + b'\r\n+\r\n' + b'I' * 10 + b'\r\n'      # the '\r' is the line's last byte: a mismatch in a partial match of 7
    assert check(crlf, R.params(A, err=0, flags=R.FRESH))[0] == [(0, 11)]
    assert check(crlf, R.params(A, err=20, flags=R.FRESH))[0] == [(0, 4)]       # 7 * 20 / 100 = 1


def test_the_left_of_two_candidates_wins():
    A = I.adapter(20)
    worse = I.implant(A, A, 0, wrong=(3, 11))                                   # two mismatches: a candidate at err=10
    s = b'N' * 6 + worse + b'N' * 4 + A + b'N' * 3
    want = check(record(b'two', s), R.params(A, err=10, flags=R.FRESH))
    assert want[0] == [(0, 6)] and want[1]['full'] == 1
    assert check(record(b'two', s), R.params(A, err=0, flags=R.FRESH))[0] == [(0, 30)]


def test_given_windows():
    A = I.adapter(13)
    s = b'N' * 20 + A + b'N' * 7
    text = record(b'w', s) + record(b'x', s) + record(b'y', s) + record(b'z', s)
    c = R.params(A, err=0, overlap=3)
    wins = [(5, 18), (21, 40), (2, 25), (20, 40)]                               # beyond b; begins inside it; 5 bases of it in front of b; at a: emptied
    want = check(text, c, windows=wins)
    assert want[0] == [(5, 18), (21, 40), (2, 20), (20, 20)]
    assert (want[1]['partial'], want[1]['full'], want[1]['emptied'], want[1]['bases_in'], want[1]['bases_out']) == (1, 1, 1, 13 + 19 + 23 + 20, 13 + 19 + 18)
    # FRESH against the identity windows handed in
    text = I.seeded(400, A, lo=0, hi=90)
    ident = [(0, len(r[1])) for r in TR.records(text)]
    fresh = check(text, dict(c, flags=R.FRESH))
    assert check(text, c, windows=ident)[:2] == fresh[:2]
    # FRESH does not read the windows
    assert host(text, dict(c, flags=R.FRESH), windows=[(9, 1)] * 400) == (fresh[0], fresh[1])
    # an empty window stays empty and is no emptied read
    e = check(record(b'e', A), c, windows=[(4, 4)])
    assert e[0] == [(4, 4)] and e[1]['emptied'] == 0 and e[1]['reads_cut'] == 0


def test_mates():
    A1, A2 = I.adapter(33), I.adapter(20, seed=7)
    text = I.seeded(600, A1, lo=40, hi=100, A2=A2)
    c = R.params(A1, A2, err=10, overlap=3, flags=R.FRESH | R.PAIRED)
    want = check(text, c)
    assert want[1]['mate2'] > 20 and want[1]['reads_cut'] - want[1]['mate2'] > 20
    # an odd first_read: the slice's record 0 is a second mate
    s = check(text, c, first=1, n=301)
    assert s[0] == want[0][1:302] and s[1]['mate2'] > 10
    # without the flag every record uses seq1
    one = check(text, dict(c, flags=R.FRESH))
    assert one[1]['mate2'] == 0 and one[0] != want[0]


def test_lines_of_different_lengths_and_empty_lines():
    A = I.ILLUMINA
    text = join([record(b'a', b'NN' + A, b'I' * 14), record(b'b', b'NN' + A, b'I' * 15), record(b'c', b'', b''), record(b'd', b'', b'II'),
                 record(b'e', A, b''), record(b'f', A[:3])])
    want = check(text, R.params(A, err=0, flags=R.FRESH))
    assert want[0] == [(0, 15), (0, 2), (0, 0), (0, 0), (0, 13), (0, 0)]
    assert want[1] == dict(dict.fromkeys(R.FIELDS, 0), reads_in=6, bases_in=15 + 15 + 13 + 3, bases_out=15 + 2 + 13, reads_cut=2, full=1, partial=1,
                           emptied=1, len_mismatch=3)
    # given windows: a record whose lines differ keeps (0, Ls) whatever was handed in
    got = host(text, R.params(A, err=0), windows=[(7, 3), (0, 15), (0, 0), (5, 5), (1, 2), (0, 3)])
    assert got[0] == want[0] and got[1] == want[1]


def test_slices_and_reports_add():
    A = I.adapter(33)
    text = I.seeded(500, A, lo=0, hi=120)
    c = R.params(A, flags=R.FRESH)
    whole = check(text, c)
    rep, parts = None, {}
    for first, k in ((300, 200), (0, 101), (101, 199)):
        w, rep = host(text, c, first, k, report=rep)
        parts[first] = w
        assert w == R.run(text, c, first, k)[0]
    assert rep == whole[1] and parts[0] + parts[101] + parts[300] == whole[0]
    assert rep['reads_cut'] == rep['full'] + rep['partial']
    twice = host(text, c, report=whole[1])[1]
    assert twice == {k: 2 * v for k, v in whole[1].items()}
    assert host(b'', c) == ([], dict.fromkeys(R.FIELDS, 0))


# ------------------------------------------------------------------ the library's errors
def test_twin_refusals():
    text = record(b'r', b'ACGTACGTAC')
    P = ops.adapter_params
    ok = dict(seq='ACGTACGT', err=10, overlap=3, flags=1)
    ops.adapter_mark_host(text, P(**ok))
    for kw, words in ((dict(ok, seq=''), 'len1'), (dict(ok, len1=65), 'len1'), (dict(ok, seq2='ACG', len2=65), 'len2'), (dict(ok, flags=3), 'len2'),
                      (dict(ok, seq=[0, 1, 4, 2]), r'seq1\[2\]'), (dict(ok, seq2=[0, 1, 2, 9]), r'seq2\[3\]'), (dict(ok, overlap=0), 'overlap'),
                      (dict(ok, overlap=9), 'overlap'), (dict(ok, seq2='ACGT', flags=3, overlap=5), 'overlap'), (dict(ok, err=31), 'err_pct'),
                      (dict(ok, flags=5), 'flag'), (dict(ok, reserved=(0, 1, 0)), 'reserved'), (dict(ok, reserved=(0, 0, 7)), 'reserved')):
        with pytest.raises(UqHipError, match=words):
            ops.adapter_mark_host(text, P(**kw))
    ops.adapter_mark_host(text, P(**dict(ok, seq2='ACGT', overlap=5)))            # seq2 is not used without PAIRED: the overlap is measured on seq1
    ops.adapter_mark_host(text, P(**dict(ok, err=30, overlap=8)))
    # windows that are none: a > b, b > Ls
    for bad in ((3, 2), (0, 11)):
        with pytest.raises(UqHipError, match='window'):
            ops.adapter_mark_host(text, P(**dict(ok, flags=0)), window=[bad])
    with pytest.raises(ValueError):
        ops.adapter_mark_host(text, P(**dict(ok, flags=0)))
    # null arguments
    a = np.frombuffer(text, np.uint8)
    ls = ops.host_line_starts(text)
    w = np.zeros(2, np.uint32)
    rep = _lib.AdapterReport()
    p = P(**ok)
    good = [ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(ls.ctypes.data), 0, 1, ctypes.byref(p), ctypes.c_void_p(w.ctypes.data), ctypes.byref(rep)]
    _lib.call('uq_adapter_mark_host', *good)
    for k in (0, 1, 4, 5, 6):
        args = list(good); args[k] = None
        with pytest.raises(UqHipError, match='null'):
            _lib.call('uq_adapter_mark_host', *args)
    with pytest.raises(UqHipError, match='null'):
        _lib.call('uq_adapter_report_init_host', None)
    rep.full = 5
    _lib.call('uq_adapter_report_init_host', ctypes.byref(rep))
    assert all(getattr(rep, k) == 0 for k in R.FIELDS)
    with pytest.raises(ValueError):
        P('ACGN')


def test_an_error_leaves_windows_and_report_as_they_were():
    """A bad window at the last record: nothing of the records in front of it has been written or counted."""
    A = I.ILLUMINA
    text = join([record(b'r%d' % k, b'NNNN' + A + b'NN') for k in range(5)])
    a = np.frombuffer(text, np.uint8)
    ls = ops.host_line_starts(text)
    p = ops.adapter_params(A.decode(), None, 0, 3, 0)
    for bad in ((3, 2), (0, 20)):
        w = np.array([(0, 19)] * 4 + [bad], np.uint32)
        before = w.copy()
        rep = _lib.AdapterReport(*range(1, 10))
        with pytest.raises(UqHipError, match='record 4: the window'):
            _lib.call('uq_adapter_mark_host', ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(ls.ctypes.data), 0, 5, ctypes.byref(p),
                      ctypes.c_void_p(w.ctypes.data), ctypes.byref(rep))
        assert (w == before).all() and [getattr(rep, k) for k in R.FIELDS] == list(range(1, 10))
    ls2 = ls.copy(); ls2[17] = ls2[16]                                         # record 4's line starts out of order
    w = np.array([(0, 19)] * 5, np.uint32)
    rep = _lib.AdapterReport()
    with pytest.raises(UqHipError, match='out of order'):
        _lib.call('uq_adapter_mark_host', ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(ls2.ctypes.data), 0, 5, ctypes.byref(p),
                  ctypes.c_void_p(w.ctypes.data), ctypes.byref(rep))
    assert (w == (0, 19)).all() and rep.reads_in == 0


# ------------------------------------------------------------------ the spec
def test_spec_parser_accepts():
    P, E = adapters.parse, adapters.explicit
    assert P('seq=ACGT') == {'seq': 'ACGT', 'seq2': None, 'err': 10, 'overlap': 3}
    assert P(' seq = acgt , err = 05 ') == {'seq': 'ACGT', 'seq2': None, 'err': 5, 'overlap': 3}
    for name, letters in R.PRESETS.items():
        assert P('seq=' + name)['seq'] == letters == adapters.PRESETS[name] and P('seq=%s,seq2=%s' % (name, name.upper()))['seq2'] == letters
    assert adapters.PRESETS == R.PRESETS == {'illumina': 'AGATCGGAAGAGC', 'nextera': 'CTGTCTCTTATA', 'smallrna': 'TGGAATTCTCGG'}
    assert E('seq=illumina') == 'seq=AGATCGGAAGAGC,err=10,overlap=3'
    assert E('overlap=5,err=0,seq2=Nextera,seq=acgtacgt') == 'seq=ACGTACGT,seq2=CTGTCTCTTATA,err=0,overlap=5'
    assert E(E('seq=illumina, err=030')) == E('seq=illumina, err=030') == 'seq=AGATCGGAAGAGC,err=30,overlap=3'
    assert P('seq=' + 'ACGT' * 16 + ',overlap=64')['overlap'] == 64 and P('seq=A,overlap=1,err=0')['seq'] == 'A'
    assert adapters.KEYS == ('seq', 'seq2', 'err', 'overlap') and isinstance(adapters.HELP, str) and 'illumina' in adapters.HELP
    c = P('seq=illumina,seq2=ACGTT')
    p = ops.adapter_params(c['seq'], c['seq2'], c['err'], c['overlap'], 3)
    assert (p.len1, p.len2, p.overlap, p.err_pct, p.flags, list(p.reserved)) == (13, 5, 3, 10, 3, [0, 0, 0])
    assert list(p.seq1)[:13] == [0, 2, 0, 3, 1, 2, 2, 0, 0, 2, 0, 2, 1] and list(p.seq2)[:6] == [0, 1, 2, 3, 3, 0]


@pytest.mark.parametrize('spec,words', [
    ('', 'empty'), ('   ', 'empty'), ('seq', 'key=value'), ('seq=A=C', 'key=value'), ('seq=ACGT,,err=2', 'key=value'), ('sequence=ACGT', 'unknown key'),
    ('seq=ACGT,seq=ACGT', 'twice'), ('seq=ACGT,err=-1', 'integer'), ('seq=ACGT,err=x', 'integer'), ('seq=ACGT,err=1.5', 'integer'),
    ('seq=ACGT,err=31', 'outside'), ('seq=ACGT,overlap=0', 'outside'), ('seq=ACGT,overlap=65', 'outside'), ('seq=ACGT,overlap=5', 'shorter'),
    ('seq=illumina,seq2=ACGT,overlap=5', 'shorter'), ('err=10', 'required'), ('seq2=ACGT', 'required'), ('seq=', 'empty'), ('seq=ACGN', 'ACGT'),
    ('seq=AC GT', 'ACGT'), ('seq=trueseq', 'preset'), ('seq=' + 'A' * 65, 'at most 64'), ('seq=ACGT,err=²', 'integer'), ('seq=ACGT,overlap=٣', 'integer'),
    ('seq=ACGT,e rr=3', 'unknown key'), ('seq=ACGT,q3=20', 'unknown key'), ('seq=ÀCGT', 'ACGT'),
])
def test_spec_parser_refuses(spec, words):
    for f in (adapters.parse, adapters.explicit):
        with pytest.raises(UqError) as e:
            f(spec)
        assert str(e.value).startswith('ERROR: --adapter') and words in str(e.value), str(e.value)
        if spec.strip(): assert repr(spec) in str(e.value)


def test_report_line():
    rep = dict(dict.fromkeys(R.FIELDS, 0), reads_in=200, reads_cut=50, full=30, partial=20, bases_in=1000, bases_out=750)
    assert adapters.report_line(rep) == 'adapter: 50 of 200 reads cut (30 full, 20 partial), 750 of 1000 bases kept (75.00 %)'
    assert adapters.report_line(dict.fromkeys(R.FIELDS, 0)).endswith('0 of 0 bases kept (0.00 %)')


# ------------------------------------------------------------------ argument checks
def args_of(tmp_path, *flags):
    p = tmp_path / 'x.fastq'
    p.write_bytes(b'@a\nA\n+\nI\n')
    return uq.build_parser().parse_args(['-i', str(p)] + list(flags))


def refused(args, *words):
    with pytest.raises(UqError) as e:
        uq.validate_args(args)
    for w in words: assert w in str(e.value), (w, str(e.value))
    assert str(e.value).startswith('ERROR: ')


def test_validate_args(tmp_path):
    assert uq.validate_args(args_of(tmp_path)).adapter is None
    for flags in ([], ['--peek'], ['--test'], ['--gz'], ['--verify'], ['--fingerprint'], ['--qc'], ['--bin-qual', 'illumina8'], ['--sort', 'DNA'],
                  ['--interleaved'], ['--multi-pass'], ['--filter', 'min-len=1'], ['--trim', 'q3=20']):
        assert uq.validate_args(args_of(tmp_path, '--adapter', 'seq=illumina', *flags)).adapter == 'seq=illumina'
    assert uq.validate_args(args_of(tmp_path, '--adapter', 'seq=illumina,seq2=nextera', '--interleaved')).adapter
    refused(args_of(tmp_path, '--adapter', 'seq=illumina', '--decode'), '--adapter', '--decode')
    refused(args_of(tmp_path, '--adapter', 'seq=ACGX'), '--adapter', "'seq=ACGX'")
    refused(args_of(tmp_path, '--adapter', 'seq=illumina,seq2=nextera'), '--adapter', 'seq2', '--mate2', '--interleaved')
    assert uq.adapter_criteria('seq=nextera') == (adapters.parse('seq=nextera'), 'seq=CTGTCTCTTATA,err=10,overlap=3')


def test_the_sharded_tool_refuses_the_flag_by_name(tmp_path, capsys):
    from uq_amd import dist_encode
    p = tmp_path / 'x.fastq'
    p.write_bytes(b'@a\nA\n+\nI\n')
    assert dist_encode.main(['-i', str(p), '--adapter', 'seq=illumina']) == 1
    out = capsys.readouterr().out
    assert out.startswith('ERROR: --adapter') and 'python -m uq_amd.uq' in out


# ------------------------------------------------------------------ header, binding, library
def test_header_binding_and_library_agree():
    lib = _lib.load()
    assert _lib.MISSING == []
    header = open(os.path.join(REPO, 'include', 'uqhip.h')).read()
    for name in NEW:
        m = re.search(r'^int\s+%s\s*\(([^;]*)\);' % name, header, re.M | re.S)
        assert m, name + ' is not declared in include/uqhip.h'
        assert len([a for a in m.group(1).split(',') if a.strip()]) == len(_lib.SIGNATURES[name]), name
        assert hasattr(lib, name), name
    m = re.search(r'typedef struct uq_adapter_report \{ uint64_t ([^}]*); \} uq_adapter_report;', header)
    assert m and tuple(''.join(m.group(1).split()).split(',')) == R.FIELDS == ops.ADAPTER_REPORT_FIELDS
    assert [f for f, _ in _lib.AdapterReport._fields_] == list(R.FIELDS) and ctypes.sizeof(_lib.AdapterReport) == 72
    assert re.search(r'typedef struct uq_adapter_params \{ uint32_t len1, len2, overlap, err_pct, flags, reserved\[3\]; uint8_t seq1\[64\], seq2\[64\]; \} '
                     r'uq_adapter_params;', header)
    assert [f for f, _ in _lib.AdapterParams._fields_] == ['len1', 'len2', 'overlap', 'err_pct', 'flags', 'reserved', 'seq1', 'seq2']
    assert ctypes.sizeof(_lib.AdapterParams) == 160 and _lib.AdapterParams.seq1.offset == 32 and _lib.AdapterParams.seq2.offset == 96
    for name, value in (('UQ_ADAPTER_MAX', '64'), ('UQ_ADAPTER_FRESH', '1u'), ('UQ_ADAPTER_PAIRED', '2u')):
        assert re.search(r'#define %s\s+%s\b' % (name, value), header)
    assert (ops.ADAPTER_MAX, ops.ADAPTER_FRESH, ops.ADAPTER_PAIRED) == (64, 1, 2) == (adapters.MAX_LEN, R.FRESH, R.PAIRED)
    assert lib.uq_abi_version() == 1 == _lib.ABI_VERSION


# ------------------------------------------------------------------ trim, adapter, plan, copy
def test_trim_then_adapter_then_plan_then_copy():
    A = I.A33
    rnd_text = I.seeded(400, A, lo=0, hi=130)
    # poly-G tails behind the adapter and low qualities at the end: the trimmer uncovers what the adapter step then finds
    recs = []
    for i, (qn, s, p, u) in enumerate(TR.records(rnd_text)):
        if i % 5 == 0: s, u = s + b'G' * 12, u + b'#' * 12
        recs.append(qn + b'\n' + s + b'\n' + p + b'\n' + u + b'\n')
    text = b''.join(recs)
    steps = TR.steps(polyg=8, q3=20, head=1)
    c = R.params(A, err=10, overlap=3)
    twins, _, _, _ = TR.run(text, steps)
    want = R.run(text, c, windows=twins)
    ls = ops.host_line_starts(text)
    w, trep = ops.trim_mark_host(text, ops.trim_params(**steps), ls)
    w2, arep = ops.adapter_mark_host(text, ops.adapter_params(A.decode(), None, 10, 3, 0), ls, window=w)
    assert [(int(a), int(b)) for a, b in w2] == want[0] and arep == want[1]
    assert arep['bases_in'] == trep['bases_out']                               # what the trimmer left is what the adapter step receives
    dst, size = ops.trim_plan_host(ls, w2)
    out, lso = ops.trim_records_host(text, ls, w2, dst, index=True)
    assert [int(x) for x in dst] == want[2] and out.tobytes() == want[3] == R.after_trim(text, steps, c)
    assert lso.tolist() == ops.host_line_starts(want[3]).tolist()
    assert arep['reads_cut'] > 80 and want[3] != TR.trimmed(text, steps)
