"""CPU: the per-cycle tables `uqqc1` (include/uqhip.h).  The hand example of the definition field by field, the
sequential host twin (uq_qc_host) against the numpy statement (tests/qc_ref.py) word for word, the invariants, additivity, the argument
refusals of the ABI and of the command line, and the JSON line's round trip."""
import ctypes as C
import glob
import json
import os
import random

import numpy as np
import pytest

import qc_ref as Q
from uq_amd import _lib, ops, uq

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
HAND = b'@a\nACGN\n+\nII#5\n@b\nGg\n+\n!~\n'


def text_of(records):
    return b''.join(b'\n'.join(r) + b'\n' for r in records)


def line(rnd, L, alphabet=None):
    if alphabet: return bytes(rnd.choice(alphabet) for _ in range(L))
    return bytes(rnd.choice([c for c in range(256) if c != 10]) for _ in range(L))


def same(got, want):
    got, want = np.asarray(got, dtype=np.uint64), np.asarray(want, dtype=np.uint64)
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, 'first differing word %d: %d != %d' % (bad[0], got[bad[0]], want[bad[0]])


def check_invariants(flat):
    f = Q.fields(flat)
    assert int(f['base_by_cycle'].sum()) == f['bases']
    assert int(f['qual_by_cycle'].sum()) == f['qual_chars']
    assert int(f['length_hist'].sum()) == f['reads']
    assert f['reserved'] == [0, 0, 0]


@pytest.mark.parametrize('impl', ['ref', 'host'])
def test_the_hand_example_field_by_field(impl):
    flat = Q.qc(HAND, 3) if impl == 'ref' else ops.qc_host(HAND, 3)
    assert len(flat) == 8 + 100 * 4 + 4 + 94 + 101
    f = Q.fields(flat)
    assert (f['reads'], f['bases'], f['qual_chars'], f['qual_out_of_range'], f['len_mismatch']) == (2, 6, 6, 0, 0)
    base = np.zeros((4, 6), dtype=np.uint64)
    base[0, 0] = base[0, 2] = base[1, 1] = base[1, 2] = base[2, 2] = base[3, 4] = 1
    assert (f['base_by_cycle'] == base).all()
    qual = np.zeros((4, 94), dtype=np.uint64)
    qual[0, 40] = qual[0, 0] = qual[1, 40] = qual[1, 93] = qual[2, 2] = qual[3, 20] = 1
    assert (f['qual_by_cycle'] == qual).all()
    assert f['length_hist'].tolist() == [0, 0, 1, 1]
    assert {int(i): int(f['mean_qual_hist'][i]) for i in np.flatnonzero(f['mean_qual_hist'])} == {25: 1, 46: 1}
    assert {int(i): int(f['gc_hist'][i]) for i in np.flatnonzero(f['gc_hist'])} == {50: 1, 100: 1}
    check_invariants(flat)


GOLDEN_FASTQ = sorted(glob.glob(os.path.join(GOLD, '*.fastq')))


def test_there_are_golden_files():
    assert len(GOLDEN_FASTQ) >= 20


@pytest.mark.parametrize('path', GOLDEN_FASTQ, ids=lambda p: os.path.basename(p)[:-6])
def test_host_twin_equals_the_statement_on_the_golden_files(path):
    text = open(path, 'rb').read()
    for cycles in (1024, 4):
        want = Q.qc(text, cycles)
        same(ops.qc_host(text, cycles), want)
        check_invariants(want)


def test_host_twin_on_random_records_of_every_short_length():
    """Lines of 0..17 bytes in all three line classes, every byte value but the newline."""
    rnd = random.Random(21)
    recs = [(line(rnd, a), line(rnd, b), b'+', line(rnd, c)) for a in (0, 1, 17) for b in range(18) for c in range(18)]
    rnd.shuffle(recs)
    text = text_of(recs)
    for cycles in (1024, 17, 16, 5, 1):
        got = ops.qc_host(text, cycles)
        same(got, Q.qc(text, cycles))
        check_invariants(got)
    f = Q.fields(ops.qc_host(text, 1024))
    assert f['len_mismatch'] == 3 * 18 * 17 and f['reads'] == len(recs)


def test_qualities_out_of_range_are_clamped_and_counted():
    quals = b' \t\x7f\x80\xff!~'
    text = text_of([(b'@r', b'ACGTACG', b'+', quals)])
    got = ops.qc_host(text, 1024)
    same(got, Q.qc(text, 1024))
    f = Q.fields(got)
    assert f['qual_out_of_range'] == 5 and f['qual_chars'] == 7
    assert [int(np.flatnonzero(f['qual_by_cycle'][p])[0]) for p in range(7)] == [0, 0, 93, 93, 93, 0, 93]
    assert int(f['mean_qual_hist'][(4 * 93) // 7]) == 1


def test_crlf_lower_case_iupac_and_unequal_lengths():
    rnd = random.Random(22)
    recs = []
    for i in range(200):
        s = line(rnd, rnd.randint(0, 40), b'ACGTNacgtnRYKMSWBDHVUryu.-*')
        u = line(rnd, len(s) if i % 3 else rnd.randint(0, 40), bytes(range(33, 127)))
        recs.append((b'@c%d' % i, s, b'+', u))
    text = text_of(recs)
    crlf = text.replace(b'\n', b'\r\n')
    for t in (text, crlf):
        got = ops.qc_host(t, 32)
        same(got, Q.qc(t, 32))
        check_invariants(got)
    f, g = Q.fields(ops.qc_host(text, 32)), Q.fields(ops.qc_host(crlf, 32))
    assert g['bases'] == f['bases'] + 200 and g['qual_out_of_range'] == 200          # the '\r' is a byte of its line: class 5, Phred 0, out of range
    assert int(g['base_by_cycle'][:, 5].sum()) == int(f['base_by_cycle'][:, 5].sum()) + 200
    assert int(f['base_by_cycle'][:, 0].sum()) == sum(r[1].count(b'A') + r[1].count(b'a') for r in recs)
    assert f['len_mismatch'] == sum(len(r[1]) != len(r[3]) for r in recs) > 0


def test_pieces_add_up_to_the_whole():
    rnd = random.Random(23)
    recs = [(b'@p%d' % i, line(rnd, rnd.randint(0, 80), b'ACGTN'), b'+', line(rnd, rnd.randint(0, 80), bytes(range(33, 127)))) for i in range(300)]
    text = text_of(recs)
    whole = ops.qc_host(text, 64)
    for k in (0, 1, 150, 299, 300):
        same(ops.qc_host(text, 64, first_read=0, nreads=k) + ops.qc_host(text, 64, first_read=k, nreads=300 - k), whole)
    same(ops.qc_host(text, 64, first_read=100, nreads=50), Q.qc(text, 64, 100, 50))
    # the twin ADDS into the array it is given
    a = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8))
    ls = ops.host_line_starts(a)
    acc = whole.copy()
    ops.call('uq_qc_host', C.c_void_p(a.ctypes.data), C.c_void_p(ls.ctypes.data), 0, 300, 64, C.c_void_p(acc.ctypes.data))
    same(acc, 2 * whole)


def test_words():
    lib = _lib.load()
    for cycles in (1, 2, 3, 4, 150, 301, 1023, 1024):
        assert lib.uq_qc_words(cycles) == 8 + 100 * (cycles + 1) + (cycles + 1) + 94 + 101 == Q.words(cycles) == ops.qc_words(cycles)
    for cycles in (0, 1025, 2 ** 31, 2 ** 32 - 1):
        assert lib.uq_qc_words(cycles) == 0
        with pytest.raises(ValueError): ops.qc_words(cycles)
    assert ops.QC_MAX_CYCLES == 1024 and ops.QC_NBASE == Q.NBASE and ops.QC_NQUAL == Q.NQUAL


def test_argument_refusals():
    lib = _lib.load()
    a = np.frombuffer(HAND, dtype=np.uint8).copy()
    ls = ops.host_line_starts(a)
    out = np.zeros(ops.qc_words(4), dtype=np.uint64)
    pa, pl, po = C.c_void_p(a.ctypes.data), C.c_void_p(ls.ctypes.data), C.c_void_p(out.ctypes.data)
    for args, word in (((pa, None, 0, 2, 4, po), 'null'), ((pa, pl, 0, 2, 4, None), 'null'), ((None, pl, 0, 2, 4, po), 'null'),
                       ((pa, pl, 0, 2, 0, po), 'ncycles'), ((pa, pl, 0, 2, 1025, po), 'ncycles')):
        assert lib.uq_qc_host(*args) != 0
        assert word in lib.uq_last_error().decode()
    assert not out.any()
    # the device entry points refuse the same before they touch a device (a null context among them)
    assert lib.uq_qc_init(None, po, 4) != 0 and 'null' in lib.uq_last_error().decode()
    assert lib.uq_qc_accumulate(None, pa, pl, 0, 2, 4, po) != 0 and 'null' in lib.uq_last_error().decode()
    with pytest.raises(ValueError): ops.qc_host(HAND, 4, first_read=1, nreads=2)
    with pytest.raises(ValueError): ops.qc_host(b'@a\nA\n+\n', 4)
    with pytest.raises(_lib.UqHipError): ops.call('uq_qc_host', pa, pl, 0, 2, 0, po)
    same(ops.qc_host(b'', 4), np.zeros(ops.qc_words(4), dtype=np.uint64))


@pytest.mark.parametrize('flags', [['--gz'], ['--peek'], ['--test'], ['-o', 'x.uQ'], ['--verify'], ['--fingerprint'], ['--decode', '--bgzf']],
                         ids=lambda f: f[-1].strip('-') if f[0] != '-o' else 'o')
def test_cli_refuses_what_does_not_go_with_qc(capsys, tmp_path, flags):
    inp = tmp_path / 'in.fastq'
    inp.write_bytes(HAND)
    rc = uq.main(['-i', str(inp), '--qc'] + flags)
    cap = capsys.readouterr()
    assert rc == 1 and cap.out.startswith('ERROR: ') and '--qc' in cap.out and 'Traceback' not in cap.out + cap.err
    assert sorted(os.listdir(str(tmp_path))) == ['in.fastq']


def test_cli_refuses_qc_cycles_alone_and_out_of_range(capsys, tmp_path):
    inp = tmp_path / 'in.fastq'
    inp.write_bytes(HAND)
    for argv in (['--qc-cycles', '50'], ['--qc', '--qc-cycles', '0'], ['--qc', '--qc-cycles', '1025']):
        rc = uq.main(['-i', str(inp)] + argv)
        cap = capsys.readouterr()
        assert rc == 1 and cap.out.startswith('ERROR: --qc-cycles'), cap.out
    assert sorted(os.listdir(str(tmp_path))) == ['in.fastq']


def test_sharded_tool_refuses_qc(capsys, tmp_path):
    from uq_amd import dist_encode
    inp = tmp_path / 'in.fastq'
    inp.write_bytes(HAND)
    assert dist_encode.main(['-i', str(inp), '--qc']) == 1
    assert capsys.readouterr().out.startswith('ERROR: --qc')


def test_json_round_trip():
    rnd = random.Random(24)
    recs = [(b'@j%d' % i, line(rnd, rnd.randint(0, 30), b'ACGTNx'), b'+', line(rnd, rnd.randint(0, 30), b'#5?I')) for i in range(100)]
    texts = [HAND, text_of(recs), b'', text_of([(b'@e', b'', b'+', b'')])]
    for text in texts:
        for cycles in (1024, 30, 8, 1):
            flat = Q.qc(text, cycles)
            said = ops.qc_json(flat)
            assert '\n' not in said
            same(ops.qc_from_json(said), flat)
            d = json.loads(said)
            assert d['format'] == 'uqqc1' and d['cycles'] == cycles
            f = Q.fields(flat)
            for k in Q.SCALARS: assert d[k] == f[k]
            assert d['beyond']['base'] == f['base_by_cycle'][cycles].tolist() and d['beyond']['length'] == int(f['length_hist'][cycles])
            assert len(d['base_by_cycle']) <= cycles and all(len(r) == 6 for r in d['base_by_cycle'])
            if d['base_by_cycle']: assert any(d['base_by_cycle'][-1])
    d = json.loads(ops.qc_json(Q.qc(HAND, 3)))
    assert d['base_by_cycle'] == [[1, 0, 1, 0, 0, 0], [0, 1, 1, 0, 0, 0], [0, 0, 1, 0, 0, 0]] and d['beyond']['base'] == [0, 0, 0, 0, 1, 0]
    assert len(d['qual_by_cycle'][0]) == 94 and d['length_hist'] == [0, 0, 1] and d['beyond']['length'] == 1
    d = json.loads(ops.qc_json(Q.qc(text_of(recs), 1024)))
    assert len(d['qual_by_cycle'][0]) == ord('I') - 33 + 1 and len(d['base_by_cycle']) == 30
