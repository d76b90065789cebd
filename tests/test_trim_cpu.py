"""CPU: read trimming (include/uqhip.h).  The two forms of the quality step in tests/trim_ref.py against each other; the host
twins uq_trim_mark_host, uq_trim_plan_host and uq_trim_records_host against that pure-Python statement of the definition on the golden FASTQ
files and the hand-made inputs of tests/trim_inputs.py; the two report invariants; the index of the trimmed text; the spec parser; what
validate_args and the sharded tool refuse; header, binding and library agree."""
import ctypes
import glob
import os
import random
import re

import numpy as np
import pytest

import filter_inputs as FI
import trim_inputs as I
import trim_ref as R
from uq_amd import _lib, ops, rectrim, uq
from uq_amd._lib import UqHipError
from uq_amd.uq import UqError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 16384
NEW = ['uq_trim_report_init', 'uq_trim_report_init_host', 'uq_trim_mark', 'uq_trim_mark_host', 'uq_trim_plan', 'uq_trim_plan_host',
       'uq_trim_records', 'uq_trim_records_host']
GOLDEN = sorted(glob.glob(os.path.join(REPO, 'tests', 'golden', '*.fastq')))
ALL_ON = dict(head=2, tail=1, crop=150, polyg=8, q5=18, q3=20, flags=1)
SPECS = [
    {},                                                                  # all off: the identity
    {'head': 5}, {'tail': 7}, {'head': 3, 'tail': 2, 'crop': 20}, {'crop': 1}, {'head': 1000}, {'tail': 1000}, {'polyg': 10}, {'polyg': 1},
    {'q3': 20}, {'q5': 20}, {'q3': 20, 'q5': 15}, {'q3': 93, 'q5': 93}, {'q3': 1, 'q5': 1}, {'flags': 1}, ALL_ON,
]


def host_run(text, c, first=0, n=None):
    """The three twins in a row -> what trim_ref.run returns, and the index the copy wrote."""
    ls = ops.host_line_starts(text)
    w, rep = ops.trim_mark_host(text, ops.trim_params(**c), ls, first, n)
    dst, size = ops.trim_plan_host(ls, w, first)
    out, lso = ops.trim_records_host(text, ls, w, dst, first, index=True)
    assert size == int(dst[-1]) == len(out)
    return [(int(a), int(b)) for a, b in w], [int(x) for x in dst], out.tobytes(), rep, lso


def check(text, c, first=0, n=None):
    c = R.steps(**c)
    want = R.run(text, c, first, n)
    got = host_run(text, c, first, n)
    assert got[0] == want[0]
    assert got[1] == want[1]
    assert got[2] == want[2]
    assert got[3] == want[3]
    rep = got[3]
    # the two invariants
    assert rep['bases_in'] - rep['bases_out'] == rep['cut_fixed'] + rep['cut_polyg'] + rep['cut_q5'] + rep['cut_q3'] + rep['cut_n']
    assert rep['bytes_in'] - rep['bytes_out'] == 2 * (rep['bases_in'] - rep['bases_out'])
    # the index of the trimmed text
    assert got[4].tolist() == ops.host_line_starts(want[2]).tolist()
    return want


# ------------------------------------------------------------------ the definition's two forms
def test_the_sequential_and_the_closed_form_agree():
    rnd = random.Random(28)
    lines = []
    for t in (1, 20, 93):
        for L in (0, 1, 2, 7, 8, 9, 150): lines.append((bytes([33 + t]) * L, t))                    # every sum is 0: nothing is cut (the strict >)
    lines.append((b'#####IIIIIIIIII' + b'#' * 200, 20))                                              # 5': negative after 5 + 5, far positive later
    lines.append((b'#' * 200 + b'IIIIIIIIII#####', 20))
    for k in range(3000):
        L, t = rnd.randrange(0, 120), rnd.randrange(1, 94)
        kind = k % 3
        if kind == 0: u = bytes(rnd.randrange(0, 256) for _ in range(L))
        elif kind == 1: u = bytes(33 + max(0, min(93, t + rnd.choice((-1, 0, 0, 1)))) for _ in range(L))
        else: u = bytes(33 + max(0, min(93, t + rnd.randrange(-8, 7))) for _ in range(L))
        lines.append((u, t))
    cut3 = cut5 = 0
    for u, t in lines:
        for a, b in ((0, len(u)), (min(3, len(u)), max(len(u) - 2, min(3, len(u))))):
            for t3, t5 in ((t, t), (t, 0), (0, t), (max(t - 1, 1), min(t + 1, 93))):
                s = R.quality_sequential(u, a, b, t3, t5)
                assert s == R.quality_closed(u, a, b, t3, t5), (u, a, b, t3, t5)
                cut3 += b - s[1]; cut5 += s[0] - a
    assert cut3 > 1000 and cut5 > 1000
    for L in (1, 8, 150):                                                                           # all equal to T: sums of 0 cut nothing
        assert R.quality_sequential(bytes([53]) * L, 0, L, 20, 20) == (0, L)
    assert R.quality_sequential(b'#####IIIIIIIIII' + b'#' * 200, 0, 215, 0, 20) == (5, 215)         # the stop holds
    assert R.quality_sequential(b'#' * 200 + b'IIIIIIIIII#####', 0, 215, 20, 0) == (0, 210)


def test_windows_by_hand():
    c = R.steps
    assert R.window(c(head=2, tail=3), b'ACGTACGTAC', b'I' * 10)[:2] == (2, 7)
    assert R.window(c(head=20), b'ACGT', b'IIII')[:2] == (4, 4)
    assert R.window(c(head=3, tail=20), b'ACGTAC', b'IIIIII')[:2] == (3, 3)
    assert R.window(c(head=1, crop=1), b'ACGT', b'IIII')[:2] == (1, 2)
    assert R.window(c(polyg=3), b'ACGGG', b'IIIII')[:2] == (0, 2) and R.window(c(polyg=4), b'ACGGG', b'IIIII')[:2] == (0, 5)
    assert R.window(c(polyg=2), b'gGgG', b'IIII')[:2] == (0, 0)
    assert R.window(c(tail=1, polyg=2), b'ACGGA', b'IIIII')[:2] == (0, 2)                             # poly-G sees the window the fixed step left
    assert R.window(c(flags=1), b'nNACNGTNn', b'I' * 9)[:2] == (2, 7) and R.window(c(flags=1), b'NNNN', b'IIII')[:2] == (4, 4)      # (the first loop takes all)
    assert R.window(c(q3=20), b'ACGTAC', b'IIII##')[:2] == (0, 4) and R.window(c(q5=20), b'ACGTAC', b'##IIII')[:2] == (2, 6)
    assert R.window(c(q3=20, q5=20), b'ACGT', b'####')[:2] == (0, 0)                                  # both ends cut everything: a'' = min(a', b')
    a, b, cut = R.window(c(q3=20, q5=20), b'ACGT', b'####')
    assert cut['q3'] == 4 and cut['q5'] == 0
    assert R.window(c(head=1, q3=20), b'ACGT', b'III')[2] is None                                     # Ls != Lu: unchanged
    # bytes outside 33 .. 126 clamp to 0 and 93
    assert R.window(c(q3=1), b'ACGT', bytes([200, 255, 0, 32]))[:2] == (0, 2)
    # CRLF: the '\r' is the last base and the last quality
    assert R.records(b'@r\r\nACGT\r\n+\r\nIIII\r\n')[0][1] == b'ACGT\r'
    assert R.run(b'@r\r\nACGT\r\n+\r\nIIII\r\n', c(tail=1))[2] == b'@r\r\nACGT\n+\r\nIIII\n'


# ------------------------------------------------------------------ the twins
@pytest.mark.parametrize('path', GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_twins_on_the_golden_files(path):
    text = open(path, 'rb').read()
    for c in SPECS:
        check(text, c)
    assert R.trimmed(text, R.steps()) == text


@pytest.mark.parametrize('name,text', list(I.hand_inputs()), ids=[n for n, _ in I.hand_inputs()])
def test_twins_on_the_hand_inputs(name, text):
    for c in SPECS + [{'polyg': 9}, {'polyg': 11}, {'q3': 20, 'flags': 1}, {'head': 8, 'q5': 20}]:
        check(text, c)


def test_the_shaped_inputs_cut_what_they_say():
    text = I.quality_cuts()
    wins = R.run(text, R.steps(q3=I.T, q5=I.T))[0]
    recs = R.records(text)
    seen = set()
    for (qn, s, p, u), (a, b) in zip(recs, wins):
        kind, L, c = qn[1:2], int(qn[2:].split(b'_')[0]), int(qn.split(b'_')[1])
        assert len(s) == L
        if c == L: assert a == b
        elif kind == b'e': assert (a, b) == (0, L - c)
        else: assert (a, b) == (c, L)
        seen.add((L, c))
    assert all((L, c) in seen for L in (17, 63, 64, 65, 255, 256, 257) for c in range(18))
    # poly-G: G - 1 stays, G goes
    w = dict(zip([r[0] for r in R.records(I.polyg_runs())], R.run(I.polyg_runs(), R.steps(polyg=10))[0]))
    assert w[b'@g9_60'] == (0, 69) and w[b'@g10_60'] == (0, 60) and w[b'@g130_3'] == (0, 3) and w[b'@allg'] == (0, 0) and w[b'@lower'] == (0, 20)
    assert w[b'@broken'] == (0, 38) and w[b'@broken_lc'] == (0, 36) and w[b'@allg_lc'] == (0, 9)
    # the 70 000-base read: 1700 and 3000 bases deep
    text, at = I.deep_text('middle')
    assert R.run(text, R.steps(q3=I.T, q5=I.T))[0][at] == (1700, 67000)
    check(text, dict(q3=I.T, q5=I.T))
    check(I.long_reads_among_short(), ALL_ON)


def test_slices_and_reports_add():
    text = I.quality_shapes()
    c = R.steps(**ALL_ON)
    whole = check(text, c)
    ls = ops.host_line_starts(text)
    n = len(whole[0])
    rep, parts = None, {}
    for first, k in ((80, n - 80), (0, 31), (31, 49)):
        w, rep = ops.trim_mark_host(text, ops.trim_params(**c), ls, first, k, report=rep)
        parts[first] = [(int(a), int(b)) for a, b in w]
        assert parts[first] == R.run(text, c, first, k)[0]
    assert rep == whole[3] and parts[0] + parts[31] + parts[80] == whole[0]
    check(text, c, first=17, n=40)
    assert host_run(b'', R.steps(head=1))[:4] == ([], [0], b'', dict.fromkeys(R.FIELDS, 0))


def test_twin_refusals():
    text = I.n_ends()
    ls = ops.host_line_starts(text)
    for kw, words in (({'q5': 94}, 'q5'), ({'q3': 94}, 'q3'), ({'crop': 0}, 'crop')):
        with pytest.raises(UqHipError, match=words):
            ops.trim_mark_host(text, ops.trim_params(**kw))
    w, _ = ops.trim_mark_host(text, ops.trim_params(flags=1))
    dst, size = ops.trim_plan_host(ls, w)
    # a window that is not one: a > b, b > Ls, and another one than (0, Ls) where the lines differ
    for bad in ((3, 2), (0, 1000)):
        w2 = w.copy(); w2[5] = bad
        with pytest.raises(UqHipError, match='window'):
            ops.trim_plan_host(ls, w2)
        with pytest.raises(UqHipError, match='window'):
            ops.trim_records_host(text, ls, w2, dst)
    odd = FI.odd_shapes()
    ls_o = ops.host_line_starts(odd)
    w_o, rep_o = ops.trim_mark_host(odd, ops.trim_params(head=1))
    assert rep_o['len_mismatch'] == 4 and (w_o[3] == (0, 2)).all()
    w_o[3] = (1, 2)
    with pytest.raises(UqHipError, match='unchanged'):
        ops.trim_plan_host(ls_o, w_o)
    # a plan that does not belong to the windows
    w3 = w.copy(); w3[0] = (0, 0)
    with pytest.raises(UqHipError, match='plan'):
        ops.trim_records_host(text, ls, w3, dst)
    # a capacity one byte short is an error and nothing is written
    a = np.frombuffer(text, np.uint8)
    out = np.full(size, 0xA5, np.uint8)
    args = [ctypes.c_void_p(a.ctypes.data), len(text), ctypes.c_void_p(ls.ctypes.data), 0, len(w), ctypes.c_void_p(w.ctypes.data),
            ctypes.c_void_p(dst.ctypes.data), ctypes.c_void_p(out.ctypes.data)]
    with pytest.raises(UqHipError, match='out_capacity'):
        _lib.call('uq_trim_records_host', *args, size - 1, None)
    assert (out == 0xA5).all()
    _lib.call('uq_trim_records_host', *args, size, None)
    assert out.tobytes() == R.trimmed(text, R.steps(flags=1))


# ------------------------------------------------------------------ the spec
def test_spec_parser_accepts():
    P, E = rectrim.parse, rectrim.explicit
    off = dict(R.OFF)
    assert P('head=5') == dict(off, head=5) and P('tail=0,q3=20') == dict(off, q3=20)
    assert P(' q3 = 020 , head=1 ') == dict(off, q3=20, head=1) and E(' q3 = 020 , head=1 ') == 'head=1,q3=20'
    assert P('crop=4294967294,polyg=4294967295,head=4294967295') == dict(off, crop=R.U32 - 1, polyg=R.U32, head=R.U32)
    assert P('trim-n=1') == dict(off, flags=1) and P('trim-n=0,q5=93') == dict(off, q5=93)
    assert E('trim-n=1,q3=20,q5=18,polyg=10,crop=100,tail=2,head=1') == 'head=1,tail=2,crop=100,polyg=10,q5=18,q3=20,trim-n=1'
    assert E(E('q3=20,head=01')) == E('q3=20,head=01') == 'head=1,q3=20'
    assert E('head=0,q3=2') == 'head=0,q3=2'
    p = ops.trim_params(**P('head=3,crop=9,trim-n=1'))
    assert (p.head, p.tail, p.crop, p.polyg, p.q5, p.q3, p.flags, p.reserved) == (3, 0, 9, 0, 0, 0, 1, 0)
    assert ctypes.sizeof(_lib.TrimParams) == 32 and rectrim.KEYS == ('head', 'tail', 'crop', 'polyg', 'q5', 'q3', 'trim-n')


@pytest.mark.parametrize('spec,words', [
    ('', 'empty'), ('   ', 'empty'), ('head', 'key=value'), ('head=1=2', 'key=value'), ('head=1,,q3=2', 'key=value'), ('hed=3', 'unknown key'),
    ('trim_n=1', 'unknown key'), ('head=3,head=3', 'twice'), ('head=-1', 'integer'), ('q3=x', 'integer'), ('q3=1.5', 'integer'),
    ('head=4294967296', 'outside'), ('tail=4294967296', 'outside'), ('crop=0', 'outside'), ('crop=4294967295', 'outside'), ('polyg=0', 'outside'),
    ('q5=0', 'outside'), ('q3=0', 'outside'), ('q5=94', 'outside'), ('q3=94', 'outside'), ('trim-n=2', 'outside'), ('head=0', 'no step'),
    ('head=0,tail=0,trim-n=0', 'no step'), ('q3=2 0', 'integer'), ('q3=²', 'integer'), ('head=٣', 'integer'), ('q 3=20', 'unknown key'),
    ('min-len=3', 'unknown key'),
])
def test_spec_parser_refuses(spec, words):
    for f in (rectrim.parse, rectrim.explicit):
        with pytest.raises(UqError) as e:
            f(spec)
        assert str(e.value).startswith('ERROR: --trim') and words in str(e.value), str(e.value)
        if spec.strip(): assert repr(spec) in str(e.value)


def test_report_line():
    rep = dict(dict.fromkeys(R.FIELDS, 0), reads_in=200, reads_trimmed=50, bases_in=1000, bases_out=750, cut_q3=200, cut_n=50)
    line = rectrim.report_line(rep)
    assert line.startswith('trim: 50 of 200 reads cut, 750 of 1000 bases kept (75.00 %), by step: ') and 'q3 200' in line and 'n 50' in line


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
    assert uq.validate_args(args_of(tmp_path)).trim is None
    for flags in ([], ['--peek'], ['--test'], ['--gz'], ['--verify'], ['--fingerprint'], ['--qc'], ['--bin-qual', 'illumina8'], ['--sort', 'DNA'],
                  ['--interleaved'], ['--multi-pass'], ['--pad'], ['--notricks'], ['--filter', 'min-len=1']):
        a = uq.validate_args(args_of(tmp_path, '--trim', 'q3=20,trim-n=1', *flags))
        assert a.trim == 'q3=20,trim-n=1'
    refused(args_of(tmp_path, '--trim', 'q3=20', '--decode'), '--trim', '--decode')
    refused(args_of(tmp_path, '--trim', 'q3=x'), '--trim', "'q3=x'")
    refused(args_of(tmp_path, '--trim', 'head=0'), '--trim', "'head=0'", 'no step')
    assert uq.trim_steps('q3=20') == (rectrim.parse('q3=20'), 'q3=20')


def test_the_sharded_tool_refuses_the_flag_by_name(tmp_path, capsys):
    from uq_amd import dist_encode
    p = tmp_path / 'x.fastq'
    p.write_bytes(b'@a\nA\n+\nI\n')
    assert dist_encode.main(['-i', str(p), '--trim', 'q3=20']) == 1
    out = capsys.readouterr().out
    assert out.startswith('ERROR: --trim') and 'python -m uq_amd.uq' in out


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
    m = re.search(r'typedef struct uq_trim_report \{ uint64_t ([^}]*); \} uq_trim_report;', header)
    assert m and tuple(''.join(m.group(1).split()).split(',')) == R.FIELDS == ops.TRIM_REPORT_FIELDS
    assert [f for f, _ in _lib.TrimReport._fields_] == list(R.FIELDS) and ctypes.sizeof(_lib.TrimReport) == 104
    assert re.search(r'typedef struct uq_trim_params \{ uint32_t head, tail, crop, polyg, q5, q3, flags, reserved; \} uq_trim_params;', header)
    assert [f for f, _ in _lib.TrimParams._fields_] == ['head', 'tail', 'crop', 'polyg', 'q5', 'q3', 'flags', 'reserved']
    assert re.search(r'#define UQ_TRIM_N 1u', header) and ops.TRIM_N == 1 == R.TRIM_N == rectrim.FLAG_N
    assert ops.TRIM_OFF == R.OFF == rectrim.OFF
    assert lib.uq_abi_version() == 1 == _lib.ABI_VERSION
    src = open(os.path.join(REPO, 'uq_amd', 'csrc', 'trim.hip')).read()
    assert re.search(r'TC_TILE = TC_THREADS \* TC_UNROLL \* 16;', src)
    assert int(re.search(r'TC_THREADS = (\d+);', src).group(1)) * int(re.search(r'TC_UNROLL = (\d+);', src).group(1)) * 16 == TILE
    assert re.search(r'TC_NP = TC_TILE / 4 \+ 3;', src)
