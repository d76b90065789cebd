"""CPU: paired-end input (include/uqhip.h).  The host twins uq_interleave_records_host and uq_mate_check_host against
the pure-Python statement of the definitions (tests/pairs_ref.py) on the hand-made inputs of tests/pairs_inputs.py; what validate_args
accepts and refuses; header, binding and library agree on the new symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

import pairs_inputs as I
import pairs_ref as R
from uq_amd import _lib, ops, uq
from uq_amd._lib import UqHipError
from uq_amd.uq import UqError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 16384
NEW = ['uq_interleave_records', 'uq_interleave_records_host', 'uq_mate_report_init', 'uq_mate_check', 'uq_mate_check_host']


# ------------------------------------------------------------------ the interleave twin
def interleave_inputs():
    yield 'one pair', I.one_pair()
    yield 'tiny', I.tiny_pairs()
    yield 'unequal', I.unequal_pairs()
    yield 'many in a tile', I.many_pairs_in_a_tile()
    for d in (-17, -1, 0, 1, 17):
        for which in (1, 2, 3):
            yield 'edge %d %d' % (d, which), I.edge_pairs(TILE, d, which)[:2]
    for where in ('first', 'middle', 'last'):
        yield 'long ' + where, I.long_record_pairs(where)


@pytest.mark.parametrize('name,texts', list(interleave_inputs()), ids=[n for n, _ in interleave_inputs()])
def test_interleave_twin_against_reference(name, texts):
    a, b = texts
    want = R.interleave(a, b)
    assert len(want) == len(a) + len(b)
    assert ops.interleave_records_host(a, b).tobytes() == want


def test_interleave_twin_subranges_and_refusals():
    a, b = I.unequal_pairs()
    n = len(R.records(a))
    for first, cnt in ((0, 1), (0, n), (5, 17), (n - 1, 1), (3, 0), (n, 0)):
        got = ops.interleave_records_host(a, b, first_pair=first, npairs=cnt)
        assert got.tobytes() == R.interleave(a, b, first, cnt), (first, cnt)
    with pytest.raises(ValueError):
        ops.interleave_records_host(a, b, first_pair=1, npairs=n)
    # a capacity one byte short is an error and nothing is written
    A, B = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    la, lb = ops.host_line_starts(A), ops.host_line_starts(B)
    out = np.full(len(a) + len(b), 0xA5, np.uint8)
    args = [ctypes.c_void_p(A.ctypes.data), ctypes.c_void_p(la.ctypes.data), ctypes.c_void_p(B.ctypes.data), ctypes.c_void_p(lb.ctypes.data), 0, n,
            ctypes.c_void_p(out.ctypes.data)]
    with pytest.raises(UqHipError):
        _lib.call('uq_interleave_records_host', *args, len(a) + len(b) - 1)
    assert (out == 0xA5).all()
    _lib.call('uq_interleave_records_host', *args, len(a) + len(b))
    assert out.tobytes() == R.interleave(a, b)


# ------------------------------------------------------------------ the mate rule
def test_reference_rule_by_hand():
    assert R.mate_id(b'@a b\tc') == b'@a' and R.mate_id(b'@a\tb c') == b'@a' and R.mate_id(b'@abc') == b'@abc' and R.mate_id(b'') == b''
    for x, y, ok, slash in I.RULE_CASES:
        assert R.mates(x, y) == (ok, slash), (x, y)


@pytest.mark.parametrize('k', range(len(I.RULE_CASES)))
def test_mate_twin_rule_cases(k):
    x, y, ok, slash = I.RULE_CASES[k]
    a, b = I.name_pair(x, y)
    want = {'pairs': 1, 'mismatches': 0 if ok else 1, 'first_mismatch': None if ok else 0, 'slash_pairs': int(slash)}
    assert ops.mate_check_host(a, b) == want
    # the same pair as one interleaved buffer
    both = R.interleave(a, b)
    assert ops.mate_check_host(both, both, first_a=0, step_a=2, first_b=1, step_b=2, npairs=1) == want


def test_mate_twin_positions_base_and_pieces():
    for n, bad, first in ((100, {0}, 0), (100, {99}, 99), (100, {3, 77}, 3), (100, set(), None)):
        a, b = I.mismatch_texts(n, bad)
        got = ops.mate_check_host(a, b)
        assert got == {'pairs': n, 'mismatches': len(bad), 'first_mismatch': first, 'slash_pairs': 0}
        assert got == R.check_texts(a, b)
        both = R.interleave(a, b)
        assert ops.mate_check_host(both, both, 0, 2, 1, 2, n) == got == R.check_texts(both, both, 0, 2, 1, 2)
    a, b = I.mismatch_texts(100, {3, 77})
    assert ops.mate_check_host(a, b, pair_index_base=1000)['first_mismatch'] == 1003
    # two calls over halves sum to the whole; the second half alone finds 77
    la, lb = ops.host_line_starts(a), ops.host_line_starts(b)
    r = ops.mate_check_host(a, b, first_a=50, first_b=50, npairs=50, pair_index_base=50, ls_a=la, ls_b=lb)
    assert r == {'pairs': 50, 'mismatches': 1, 'first_mismatch': 77, 'slash_pairs': 0}
    r = ops.mate_check_host(a, b, npairs=50, ls_a=la, ls_b=lb, report=r)
    assert r == ops.mate_check_host(a, b)


def test_mate_twin_random_pairs():
    a, b = I.random_pairs()
    want = R.check_texts(a, b)
    assert 20 <= want['mismatches'] <= 90 and want['slash_pairs'] > 300
    assert ops.mate_check_host(a, b) == want
    both = R.interleave(a, b)
    assert ops.interleave_records_host(a, b).tobytes() == both
    assert ops.mate_check_host(both, both, 0, 2, 1, 2) == want


# ------------------------------------------------------------------ argument checks
def args_of(tmp_path, *flags, mate2=None):
    p = tmp_path / 'x.fastq'
    p.write_bytes(b'@a\nA\n+\nI\n')
    q = tmp_path / 'y.fastq'
    q.write_bytes(b'@a\nC\n+\nI\n')
    argv = ['-i', str(p)] + list(flags)
    if mate2: argv += ['--mate2', str(q) if mate2 is True else mate2]
    return uq.build_parser().parse_args(argv)


def refused(args, *words):
    with pytest.raises(UqError) as e:
        uq.validate_args(args)
    for w in words: assert w in str(e.value), (w, str(e.value))
    assert str(e.value).startswith('ERROR: ')


def test_validate_args(tmp_path):
    for flags in ([], ['--peek'], ['--test'], ['--gz'], ['--verify'], ['--fingerprint'], ['--qc'], ['--bin-qual', 'illumina8'], ['--sort', 'None'],
                  ['--raw', 'DNA', 'QUAL', 'QNAME']):
        a = uq.validate_args(args_of(tmp_path, *flags, mate2=True))
        assert a.mate2.endswith('y.fastq') and not a.interleaved
        a = uq.validate_args(args_of(tmp_path, '--interleaved', *flags))
        assert a.interleaved and a.mate2 is None
    a = uq.validate_args(args_of(tmp_path))
    assert a.mate2 is None and a.interleaved is False and a.split_mates is None
    refused(args_of(tmp_path, '--interleaved', mate2=True), '--mate2', '--interleaved')
    for sort in ('DNA', 'QUAL', 'QNAME', 'dna'):
        refused(args_of(tmp_path, '--sort', sort, mate2=True), '--sort ' + sort, '--mate2', 'mates')
        refused(args_of(tmp_path, '--sort', sort, '--interleaved'), '--sort ' + sort, '--interleaved', 'mates')
    refused(args_of(tmp_path, '--decode', mate2=True), '--mate2', '--decode')
    refused(args_of(tmp_path, '--decode', '--interleaved'), '--interleaved', '--decode')
    refused(args_of(tmp_path, mate2=str(tmp_path / 'nope.fastq')), '--mate2', 'not a file')
    # --split-mates: with --decode only, two files, not with the flags that write no text
    a = uq.validate_args(args_of(tmp_path, '--decode', '--split-mates', 'o1', 'o2'))
    assert a.split_mates == ['o1', 'o2']
    uq.validate_args(args_of(tmp_path, '--decode', '--bgzf', '--bgzf-level', '2', '--split-mates', 'o1', 'o2'))
    refused(args_of(tmp_path, '--split-mates', 'o1', 'o2'), '--split-mates', '--decode')
    refused(args_of(tmp_path, '--decode', '--split-mates', 'o1', 'o1'), '--split-mates', 'different')
    refused(args_of(tmp_path, '--decode', '--fingerprint', '--split-mates', 'o1', 'o2'), '--split-mates')
    with pytest.raises(SystemExit):
        args_of(tmp_path, '--decode', '--split-mates', 'o1')


def test_the_sharded_tool_refuses_the_flags_by_name(tmp_path, capsys):
    from uq_amd import dist_encode
    p = tmp_path / 'x.fastq'
    p.write_bytes(b'@a\nA\n+\nI\n')
    for argv, flag in ((['-i', str(p), '--mate2', str(p)], '--mate2'), (['-i', str(p), '--interleaved'], '--interleaved'),
                       (['-i', str(p), '--decode', '--split-mates', 'a', 'b'], '--split-mates')):
        capsys.readouterr()
        assert dist_encode.main(argv) == 1
        out = capsys.readouterr().out
        assert out.startswith('ERROR: ' + flag) and 'python -m uq_amd.uq' in out


# ------------------------------------------------------------------ header, binding, library
def test_header_binding_and_library_agree():
    lib = _lib.load()
    assert _lib.MISSING == []
    header = open(os.path.join(REPO, 'include', 'uqhip.h')).read()
    for name in NEW:
        m = re.search(r'^int\s+%s\s*\(([^;]*)\);' % name, header, re.M | re.S)
        assert m, name + ' is not declared in include/uqhip.h'
        nargs = len([a for a in m.group(1).split(',') if a.strip()])
        assert nargs == len(_lib.SIGNATURES[name]), name
        assert hasattr(lib, name), name
    assert re.search(r'typedef struct uq_mate_report \{ uint64_t pairs, mismatches, first_mismatch, slash_pairs; \} uq_mate_report;', header)
    assert [f for f, _ in _lib.MateReport._fields_] == ['pairs', 'mismatches', 'first_mismatch', 'slash_pairs'] and ctypes.sizeof(_lib.MateReport) == 32
    assert ops.MATE_REPORT_FIELDS == ('pairs', 'mismatches', 'first_mismatch', 'slash_pairs')
    assert lib.uq_abi_version() == 1 == _lib.ABI_VERSION
    src = open(os.path.join(REPO, 'uq_amd', 'csrc', 'pairs.hip')).read()
    assert re.search(r'PR_TILE = PR_THREADS \* PR_UNROLL \* 16;', src)
    assert int(re.search(r'PR_THREADS = (\d+);', src).group(1)) * int(re.search(r'PR_UNROLL = (\d+);', src).group(1)) * 16 == TILE
