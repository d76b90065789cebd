"""CPU: read filtering (include/uqhip.h).  The host twins uq_filter_mark_host, uq_filter_plan_host and
uq_compact_records_host against the pure-Python statement of the definition (tests/filter_ref.py) on the golden FASTQ files and the hand-made
inputs of tests/filter_inputs.py; the spec parser; what validate_args and the sharded tool refuse; header, binding and library agree."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import filter_inputs as I
import filter_ref as R
from uq_amd import _lib, ops, recfilter, uq
from uq_amd._lib import UqHipError
from uq_amd.uq import UqError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 16384
NEW = ['uq_filter_report_init', 'uq_filter_report_init_host', 'uq_filter_mark', 'uq_filter_mark_host', 'uq_filter_plan', 'uq_filter_plan_host',
       'uq_compact_records', 'uq_compact_records_host']
GOLDEN = sorted(glob.glob(os.path.join(REPO, 'tests', 'golden', '*.fastq')))
SPECS = [
    {},                                                                  # all off
    {'min_len': 50}, {'max_len': 99}, {'min_len': 100, 'max_len': 100}, {'max_n': 0}, {'max_n': 2}, {'min_mean_q': 30}, {'min_mean_q': 93},
    {'sample_threshold': 1 << 63, 'flags': 1}, {'sample_threshold': (1 << 64) // 10, 'seed': 7, 'flags': 1},
    {'sample_threshold': 5, 'seed': 9},                                  # the flag clear: threshold and seed mean nothing
    {'min_len': 30, 'max_len': 120, 'max_n': 1, 'min_mean_q': 25, 'sample_threshold': 3 << 62, 'seed': 1, 'flags': 1},      # all on
]


def host_run(text, c, unit=1, first=0, n=None, index_base=0):
    """The three twins in a row -> what filter_ref.run returns."""
    ls = ops.host_line_starts(text)
    v, rep = ops.filter_mark_host(text, ops.filter_params(unit=unit, **c), ls, first, n, index_base)
    src, dst, kept, size, rep = ops.filter_plan_host(ls, v, unit, first, report=rep)
    out = ops.compact_records_host(text, src, dst, kept)
    assert size == (int(dst[kept]) if kept else 0) == len(out)
    return [int(x) for x in v], [int(x) for x in src], [int(x) for x in dst], out.tobytes(), rep


def check(text, c, unit=1):
    c = R.criteria(**c)
    want = R.run(text, c, unit)
    got = host_run(text, c, unit)
    assert got[0] == want[0]
    assert got[1:3] == want[1:3]
    assert got[3] == want[3]
    assert got[4] == want[4]
    rep = got[4]
    dropped = sum(1 for w in range(len(want[0]) // unit) if any(want[0][w * unit:(w + 1) * unit])) * unit
    assert rep['reads_in'] == rep['reads_out'] + dropped and rep['bytes_out'] == want[2][-1]
    return want


@pytest.mark.parametrize('path', GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_twins_on_the_golden_files(path):
    text = open(path, 'rb').read()
    nrec = len(R.records(text))
    for c in SPECS:
        check(text, c)
        if nrec % 2 == 0: check(text, c, unit=2)


@pytest.mark.parametrize('name,text', list(I.hand_inputs()), ids=[n for n, _ in I.hand_inputs()])
def test_twins_on_the_hand_inputs(name, text):
    for c in SPECS + [{'min_len': 10}, {'max_len': 10}, {'max_n': 3}, {'min_mean_q': 20}, {'min_mean_q': 1}, {'min_len': 1}]:
        check(text, c)


def test_threshold_edges_by_hand():
    v = R.verdicts(I.edges_len(), R.criteria(min_len=10))
    assert v == [1, 0, 0, 0, 0, 1]
    assert R.verdicts(I.edges_len(), R.criteria(max_len=10)) == [0, 0, 2, 2, 0, 0]
    assert R.verdicts(I.edges_n(), R.criteria(max_n=3)) == [0, 0, 4, 4, 0, 0, 4, 0]
    assert R.verdicts(I.edges_q(), R.criteria(min_mean_q=20)) == [8, 0, 0] * 5
    # bytes outside 33 .. 126 clamp: sums 0, 93 + 93 + 93 + 93, 5 * 93, 8 + 0
    lo, hi, mix, at = R.records(I.odd_quality_bytes())
    assert [sum(R.q(b) for b in r[3]) for r in (lo, hi, mix, at)] == [0, 4 * 93, 5 * 93, 8]
    assert R.verdicts(I.odd_quality_bytes(), R.criteria(min_mean_q=1)) == [8, 0, 0, 8]
    # an empty quality line passes every mean; CRLF counts the '\r' as a base and a quality; lower-case n is N
    v = R.verdicts(I.odd_shapes(), R.criteria(min_mean_q=93))
    assert v[0] == 0 and v[2] == 0 and v[1] == 8
    assert R.records(I.odd_shapes())[5][1] == b'ACNT\r'
    for name, text in I.hand_inputs():
        for c in ({'min_len': 10}, {'max_len': 10}, {'max_n': 3}, {'min_mean_q': 20}):
            c = R.criteria(**c)
            assert [int(x) for x in ops.filter_mark_host(text, ops.filter_params(**c))[0]] == R.verdicts(text, c), (name, c)


def test_sample_bit():
    text = I.four_byte_units(10000)
    for f_num, f_den in ((1, 1000), (1, 2), (999, 1000)):
        thr = (f_num << 64) // f_den
        for seed in (0, 12345):
            c = R.criteria(sample_threshold=thr, seed=seed, flags=1)
            want = [16 if R.mix(seed + R.K * (w + 1)) >= thr else 0 for w in range(10000)]
            assert R.verdicts(text, c) == want
            got = ops.filter_mark_host(text, ops.filter_params(**c))[0]
            assert [int(x) for x in got] == want
            kept = want.count(0)
            assert abs(kept - 10000 * f_num / f_den) < 4 * (10000 * f_num * (f_den - f_num)) ** 0.5 / f_den + 1
    for thr in (1, (1 << 64) - 1):
        c = R.criteria(sample_threshold=thr, flags=1)
        got = [int(x) for x in ops.filter_mark_host(text, ops.filter_params(**c))[0]]
        assert got == R.verdicts(text, c)
    assert set(R.verdicts(text, R.criteria(sample_threshold=1, flags=1))) == {16}            # (no mix value of these indexes is 0)
    assert 16 not in R.verdicts(text, R.criteria(sample_threshold=1, seed=3, flags=0))
    # the mates of a unit agree, whatever the base
    c = R.criteria(sample_threshold=1 << 63, seed=5, flags=1)
    for base in (0, 2, 1000):
        v = [int(x) for x in ops.filter_mark_host(text, ops.filter_params(unit=2, **c), index_base=base)[0]]
        assert v == R.verdicts(text, c, unit=2, index_base=base)
        assert all(v[2 * i] == v[2 * i + 1] for i in range(5000)) and 1000 < v.count(16) < 9000


def test_index_base_and_pieces():
    text = I.short_records()
    c = R.criteria(min_len=8, max_n=1, min_mean_q=19, sample_threshold=1 << 63, seed=2, flags=1)
    whole_v, whole_rep = ops.filter_mark_host(text, ops.filter_params(**c))
    assert [int(x) for x in whole_v] == R.verdicts(text, c)
    ls = ops.host_line_starts(text)
    rep, parts = None, []
    for first, n in ((200, 100), (0, 57), (57, 143)):
        v, rep = ops.filter_mark_host(text, ops.filter_params(**c), ls, first, n, index_base=first, report=rep)
        assert [int(x) for x in v] == R.verdicts(text, c, first=first, n=n, index_base=first)
        parts.append((first, v))
    assert rep == whole_rep
    assert np.concatenate([v for _, v in sorted(parts, key=lambda p: p[0])]).tobytes() == whole_v.tobytes()
    # a slice as a shard sees it: other global indexes, other sample
    v, _ = ops.filter_mark_host(text, ops.filter_params(**c), ls, 10, 50, index_base=5000)
    assert [int(x) for x in v] == R.verdicts(text, c, first=10, n=50, index_base=5000)
    # the plan of a slice
    want = R.run(text, c, first=40, n=100, index_base=40)
    assert host_run(text, c, first=40, n=100, index_base=40) == want


def test_plan_counters_and_mates():
    text = I.pairs_text()
    c = R.criteria(max_n=2, min_len=12)
    want = check(text, c, unit=2)
    v, rep = want[0], want[4]
    assert rep['fail_mate'] > 5 and rep['fail_mate'] == sum(1 for i in range(len(v)) if v[i] == 0 and v[i ^ 1] != 0)
    assert rep['reads_out'] % 2 == 0 and 0 < rep['reads_out'] < rep['reads_in'] == 120
    assert check(text, c, unit=1)[4]['fail_mate'] == 0
    # nothing kept, everything kept, no records
    none = host_run(text, R.criteria(min_len=1000))
    assert none[1] == [] and none[2] == [0] and none[3] == b'' and none[4]['reads_out'] == 0
    assert host_run(text, R.criteria())[3] == text
    empty = host_run(b'', R.criteria())
    assert empty[0] == [] and empty[2] == [0] and empty[4] == dict.fromkeys(R.FIELDS, 0)
    # reports add
    ls = ops.host_line_starts(text)
    v1, rep1 = ops.filter_mark_host(text, ops.filter_params(unit=2, **c), ls, 0, 60)
    *_, rep1 = ops.filter_plan_host(ls, v1, 2, 0, report=rep1)
    v2, rep2 = ops.filter_mark_host(text, ops.filter_params(unit=2, **c), ls, 60, 60, index_base=60, report=rep1)
    *_, rep2 = ops.filter_plan_host(ls, v2, 2, 60, report=rep2)
    assert rep2 == rep


def test_twin_refusals():
    text = I.pairs_text()
    ls = ops.host_line_starts(text)
    for kw, words in (({'min_len': 5, 'max_len': 4}, 'min_len'), ({'min_mean_q': 94}, 'min_mean_q')):
        with pytest.raises(UqHipError, match=words):
            ops.filter_mark_host(text, ops.filter_params(**kw))
    with pytest.raises(UqHipError, match='unit'):
        ops.filter_mark_host(text, ops.filter_params(unit=3))
    with pytest.raises(UqHipError, match='unit'):
        ops.filter_mark_host(text, ops.filter_params(unit=0))
    with pytest.raises(UqHipError, match='pairs'):
        ops.filter_mark_host(text, ops.filter_params(unit=2), ls, 0, 3)
    with pytest.raises(UqHipError, match='pairs'):
        ops.filter_mark_host(text, ops.filter_params(unit=2), ls, 0, 4, index_base=1)
    with pytest.raises(UqHipError, match='pairs'):
        ops.filter_plan_host(ls, np.zeros(3, np.uint8), 2)
    with pytest.raises(UqHipError, match='unit'):
        ops.filter_plan_host(ls, np.zeros(4, np.uint8), 3)
    # a capacity one byte short is an error and nothing is written
    v, _ = ops.filter_mark_host(text, ops.filter_params(max_n=2))
    src, dst, kept, size, _ = ops.filter_plan_host(ls, v)
    a = np.frombuffer(text, np.uint8)
    out = np.full(size, 0xA5, np.uint8)
    args = [ctypes.c_void_p(a.ctypes.data), len(text), ctypes.c_void_p(src.ctypes.data), ctypes.c_void_p(dst.ctypes.data), kept, ctypes.c_void_p(out.ctypes.data)]
    with pytest.raises(UqHipError, match='out_capacity'):
        _lib.call('uq_compact_records_host', *args, size - 1)
    assert (out == 0xA5).all()
    _lib.call('uq_compact_records_host', *args, size)
    assert out.tobytes() == R.filtered(text, R.criteria(max_n=2))


# ------------------------------------------------------------------ the spec
def test_spec_parser_accepts():
    P, E = recfilter.parse, recfilter.explicit
    off = {'min_len': 0, 'max_len': R.U32, 'max_n': R.U32, 'min_mean_q': 0, 'sample_threshold': 0, 'seed': 0, 'flags': 0}
    assert P('min-len=36') == dict(off, min_len=36)
    assert P('max-len=0') == dict(off, max_len=0)
    assert P(' min-len=036 , max-n = 2 ') == dict(off, min_len=36, max_n=2) and E(' min-len=036 , max-n = 2 ') == 'min-len=36,max-n=2'
    assert P('min-mean-q=93,max-len=4294967295') == dict(off, min_mean_q=93)
    assert P('sample=0.1') == dict(off, sample_threshold=(1 << 64) // 10, flags=1)
    assert P('sample=0.5,seed=18446744073709551615') == dict(off, sample_threshold=1 << 63, seed=(1 << 64) - 1, flags=1)
    assert P('sample=1') == off and P('sample=1.000,seed=3') == dict(off, seed=3)
    assert P('sample=0.001')['sample_threshold'] == (1 << 64) // 1000
    assert P('sample=0.00000000000000000001')['sample_threshold'] == (1 << 64) // 10 ** 20 == 0
    assert E('seed=4,sample=0.25,min-mean-q=20,max-n=1,max-len=9,min-len=1') == 'min-len=1,max-len=9,max-n=1,min-mean-q=20,sample=0.25,seed=4'
    assert E(E('seed=4,sample=0.25')) == E('seed=4,sample=0.25')
    # one form for one meaning: the sample's decimal loses its leading and trailing zeros
    assert E('sample=0.10') == E('sample=.1') == E('sample=00.100') == 'sample=0.1' and P('sample=0.10') == P('sample=.1')
    assert E('sample=1.000,seed=03') == 'sample=1,seed=3' and E('sample = 0.5') == 'sample=0.5'
    # the criteria are exactly what the library takes
    p = ops.filter_params(unit=2, **P('min-len=3,sample=0.75,seed=2'))
    assert (p.min_len, p.max_len, p.max_n, p.min_mean_q, p.sample_threshold, p.seed, p.unit, p.flags) == (3, R.U32, R.U32, 0, 3 << 62, 2, 2, 1)
    assert ctypes.sizeof(_lib.FilterParams) == 40


@pytest.mark.parametrize('spec,words', [
    ('', 'empty'), ('   ', 'empty'), ('min-len', 'key=value'), ('min-len=1=2', 'key=value'), ('min-len=1,,max-n=2', 'key=value'),
    ('minlen=3', 'unknown key'), ('min_len=3', 'unknown key'), ('min-len=3,min-len=3', 'twice'), ('min-len=-1', 'integer'), ('min-len=x', 'integer'),
    ('min-len=1.5', 'integer'), ('min-len=4294967296', 'outside'), ('max-n=4294967296', 'outside'), ('min-mean-q=94', 'outside'),
    ('min-len=10,max-len=9', 'larger'), ('sample=0', 'outside'), ('sample=1.01', 'outside'), ('sample=-0.5', 'fraction'), ('sample=half', 'fraction'),
    ('sample=1/2', 'fraction'), ('sample=', 'fraction'), ('seed=3', 'sample'), ('sample=0.5,seed=-1', 'integer'),
    ('sample=0.5,seed=18446744073709551616', '64 bits'),
    ('min-len=3 6', 'integer'), ('min-len=\u00b2', 'integer'), ('max-n=\u0663', 'integer'), ('sample=0.5,seed=\u00b2', 'integer'), ('sample=1e-1', 'fraction'),
    ('sample=0. 5', 'fraction'), ('sample=\u0660.5', 'fraction'), ('sample=0.5.1', 'fraction'), ('min - len=3', 'unknown key'),
])
def test_spec_parser_refuses(spec, words):
    for f in (recfilter.parse, recfilter.explicit):
        with pytest.raises(UqError) as e:
            f(spec)
        assert str(e.value).startswith('ERROR: --filter') and words in str(e.value), str(e.value)
        if spec.strip(): assert repr(spec) in str(e.value)


def test_report_line():
    rep = dict(dict.fromkeys(R.FIELDS, 0), reads_in=200, reads_out=50, fail_min_len=100, fail_mate=7)
    line = recfilter.report_line(rep)
    assert line.startswith('filter: kept 50 of 200 reads (25.00 %), by criterion: ') and 'min_len 100' in line and 'mate 7' in line


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
    assert uq.validate_args(args_of(tmp_path)).filter is None
    for flags in ([], ['--peek'], ['--test'], ['--gz'], ['--verify'], ['--fingerprint'], ['--qc'], ['--bin-qual', 'illumina8'], ['--sort', 'DNA'],
                  ['--interleaved'], ['--multi-pass'], ['--pad'], ['--notricks']):
        a = uq.validate_args(args_of(tmp_path, '--filter', 'min-len=30,sample=0.5', *flags))
        assert a.filter == 'min-len=30,sample=0.5'
    refused(args_of(tmp_path, '--filter', 'min-len=30', '--decode'), '--filter', '--decode')
    refused(args_of(tmp_path, '--filter', 'min-len=x'), '--filter', "'min-len=x'")
    refused(args_of(tmp_path, '--filter', 'min-len=3,max-len=2'), '--filter', 'larger')
    assert uq.filter_criteria('max-n=0') == (recfilter.parse('max-n=0'), 'max-n=0')


def test_the_sharded_tool_refuses_the_flag_by_name(tmp_path, capsys):
    from uq_amd import dist_encode
    p = tmp_path / 'x.fastq'
    p.write_bytes(b'@a\nA\n+\nI\n')
    assert dist_encode.main(['-i', str(p), '--filter', 'min-len=1']) == 1
    out = capsys.readouterr().out
    assert out.startswith('ERROR: --filter') and 'python -m uq_amd.uq' in out


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
    m = re.search(r'typedef struct uq_filter_report \{ uint64_t ([^}]*); \} uq_filter_report;', header)
    assert m and tuple(''.join(m.group(1).split()).split(',')) == R.FIELDS == ops.FILTER_REPORT_FIELDS
    assert [f for f, _ in _lib.FilterReport._fields_] == list(R.FIELDS) and ctypes.sizeof(_lib.FilterReport) == 96
    assert re.search(r'typedef struct uq_filter_params \{ uint32_t min_len, max_len, max_n, min_mean_q; uint64_t sample_threshold, seed; uint32_t unit, flags; \} uq_filter_params;', header)
    assert [f for f, _ in _lib.FilterParams._fields_] == ['min_len', 'max_len', 'max_n', 'min_mean_q', 'sample_threshold', 'seed', 'unit', 'flags']
    assert re.search(r'#define UQ_FILTER_SAMPLE 1u', header) and ops.FILTER_SAMPLE == 1 == R.SAMPLE
    assert lib.uq_abi_version() == 1 == _lib.ABI_VERSION
    src = open(os.path.join(REPO, 'uq_amd', 'csrc', 'filter.hip')).read()
    assert re.search(r'CP_TILE = CP_THREADS \* CP_UNROLL \* 16;', src)
    assert int(re.search(r'CP_THREADS = (\d+);', src).group(1)) * int(re.search(r'CP_UNROLL = (\d+);', src).group(1)) * 16 == TILE
    assert re.search(r'CP_NP = CP_TILE / 4 \+ 3;', src)
