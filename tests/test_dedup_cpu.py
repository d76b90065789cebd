"""CPU: duplicate removal (include/uqhip.h).  The host twins uq_dedup_keys_host and uq_dedup_mark_host against the two
pure-Python statements of the definition (tests/dedup_ref.py) on the golden FASTQ files (their first 2 000 records) and the hand-made inputs
of tests/dedup_inputs.py; the driver loop; the spec parser; what validate_args and the sharded tool refuse; header, binding and library agree;
the session step on host tensors."""
import ctypes
import glob
import itertools
import os
import re

import numpy as np
import pytest
import torch

import dedup_inputs as I
import dedup_ref as R
import fake_decode_ops as F
from uq_amd import _lib, ops, recdedup, uq
from uq_amd._lib import UqHipError
from uq_amd.uq import UqError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['uq_dedup_report_init', 'uq_dedup_report_init_host', 'uq_dedup_keys', 'uq_dedup_keys_host', 'uq_dedup_mark', 'uq_dedup_mark_host']
GOLDEN = sorted(glob.glob(os.path.join(REPO, 'tests', 'golden', '*.fastq')))
HEAD = 2000                                                       # records of a golden file the matrix below runs on
PREFIXES = (0, 1, 8, 9, 1000)


def twins(text, unit=1, prefix=0, best=False, seed=0, hash_bits=64, first=0, n=None, index_base=0, report=None):
    """keys, numpy order, mark -> (key rows, verdicts, report)."""
    ls = ops.host_line_starts(text)
    p = ops.dedup_params(unit=unit, prefix=prefix, hash_bits=hash_bits, flags=ops.DEDUP_BEST if best else 0, seed=seed)
    keys, rep = ops.dedup_keys_host(text, p, ls, first, n, index_base, report)
    v, rep = ops.dedup_mark_host(text, p, keys, ops.dedup_order_host(keys), ls, first, n, index_base, rep)
    return [bytes(k) for k in keys], [int(x) for x in v], rep


def check(text, unit, prefix, best, seed, hash_bits):
    """The twins against the rule; where nothing collided, the rule against the plain meaning."""
    want = R.rule(text, unit, prefix, best, seed, hash_bits)
    got = twins(text, unit, prefix, best, seed, hash_bits)
    assert got[0] == want[0]
    assert got[1] == want[1]
    assert got[2] == want[2]
    rep = want[2]
    assert rep['classes'] + rep['dup_units'] == rep['units_in'] and rep['dup_reads'] == unit * rep['dup_units'] == sum(want[1])
    if hash_bits == 64:
        assert rep['collisions'] == 0                            # the condition on the inputs: an exact case is never a retried one
    if rep['collisions'] == 0:
        assert want[1] == R.plain(text, unit, prefix, best)
    return rep


def matrix(text):
    nrec = len(R.records(text))
    for unit, prefix, best, seed, bits in itertools.product((1, 2), PREFIXES, (False, True), (0, 1), (64, 3)):
        if nrec % unit == 0: check(text, unit, prefix, best, seed, bits)


def head_of(path):
    lines = open(path, 'rb').read().split(b'\n')
    return b'\n'.join(lines[:4 * HEAD]) + (b'\n' if len(lines) > 4 * HEAD else b'')


@pytest.mark.parametrize('path', GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_twins_on_the_golden_files(path):
    matrix(head_of(path))


@pytest.mark.parametrize('name,text', list(I.hand_inputs()), ids=[n for n, _ in I.hand_inputs()])
def test_twins_on_the_hand_inputs(name, text):
    matrix(text)


def test_forced_collisions_are_counted():
    for text in (I.counted(129), I.edge_lengths(), I.spread(3000)):
        for bits in (1, 2, 3, 4):
            rep = check(text, 1, 0, False, 0, bits)
            assert rep['collisions'] > 0
    # with collisions no non-duplicate is dropped: every verdict 1 of the rule is one of the plain meaning's class members
    text = I.spread(3000)
    _, v, rep = R.rule(text, hash_bits=4)
    us = R.units(text)
    kept = {c for w, (c, _, _) in enumerate(us) if v[w] == 0}
    assert rep['collisions'] > 0 and all(us[w][0] in kept for w in range(len(us)))


def test_larger_inputs():
    for text, unit in ((I.spread(6000), 1), (I.spread(6000), 2), (I.long_run(), 1), (I.huge_line(1), 1), (I.huge_line(2), 1), (I.one_class(1000), 1)):
        for best in (False, True):
            rep = check(text, unit, 0, best, 0, 64)
            check(text, unit, 9, best, 1, 64)
    assert check(I.huge_line(2), 1, 0, False, 0, 64)['dup_bases'] == 70000
    assert check(I.one_class(1000), 1, 0, False, 0, 64)['dup_units'] == 999


def test_by_hand():
    # near misses: length, last byte and case all tell texts apart; N equals N
    text = I.near_misses()
    seqs = [r[1] for r in R.records(text)]
    _, v, rep = twins(text)
    assert v == [1 if s in seqs[:i] else 0 for i, s in enumerate(seqs)]
    assert rep['classes'] == len(set(seqs))
    # a prefix folds texts that differ behind it
    assert twins(text, prefix=3)[1] == [1 if s[:3] in [x[:3] for x in seqs[:i]] else 0 for i, s in enumerate(seqs)]
    # pairs: only whole equal pairs are duplicates; swapped mates are another pair
    text = I.pairs()
    _, v, rep = twins(text, unit=2)
    assert v == [0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 1] and rep['dup_reads'] == 10 and rep['units_in'] == 12
    # the best of a class: the highest clamped sum, ties to the lower index
    text = I.score_ties()
    quals = [r[3] for r in R.records(text)]
    sums = [R.score([u]) for u in quals[:10]]
    assert sums[6] == sums[7] == 930 and sums[8] == sums[9] == 0
    _, v, _ = twins(text, best=True)
    assert v == [1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 1]
    assert twins(text)[1] == [0] + [1] * 9 + [0, 1]
    # the key row's layout
    keys, _, _ = twins(text, best=True, index_base=7)
    assert keys[1][8:12] == (0xFFFFFFFF - 400).to_bytes(4, 'big') and keys[1][12:] == (8).to_bytes(4, 'big')
    assert keys[0][:8] == keys[1][:8] == R.unit_hash((b'ACGTACGTAC',), 0).to_bytes(8, 'big')
    assert twins(text)[0][1][8:12] == bytes(4)


def test_score_clamp():
    text = I.score_clamp()
    quals = [r[3] for r in R.records(text)]
    assert [sum(u.translate(R.QTAB)) for u in quals] == [(1 << 32) - 2, (1 << 32) - 1, (1 << 32) + 3 * 93 - 2]
    keys, v, rep = twins(text, best=True)
    assert [k[8:12] for k in keys] == [b'\0\0\0\1', b'\0\0\0\0', b'\0\0\0\0']
    assert v == [1, 0, 1] == R.plain(text, best=True) and rep['classes'] == 1
    assert (keys, v, rep) == R.rule(text, best=True)


def test_pieces_and_reports_add():
    text = I.spread(3000)
    ls = ops.host_line_starts(text)
    for unit, best in ((1, False), (2, True)):
        whole = twins(text, unit=unit, best=best)
        # first_read > 0: a slice is judged by itself, with its own unit numbers from the base on
        for first, n, base in ((1000, 500, 1000), (10, 64, 0), (2998, 2, 40)):
            assert twins(text, unit=unit, best=best, first=first, n=n, index_base=base) == R.rule(text, unit, 0, best, first=first, n=n, index_base=base)
        # two calls add into one report
        _, _, rep1 = twins(text, unit=unit, best=best, first=0, n=1000)
        _, _, rep2 = twins(text, unit=unit, best=best, first=1000, n=2000, index_base=1000, report=rep1)
        a, b = R.rule(text, unit, 0, best, first=0, n=1000)[2], R.rule(text, unit, 0, best, first=1000, n=2000)[2]
        assert rep2 == {k: a[k] + b[k] for k in R.FIELDS}
        assert whole[2]['reads_in'] == rep2['reads_in'] and whole[2]['bases_in'] == rep2['bases_in']
    # mark writes every verdict, whatever the array held (the binding hands it 0xEE bytes)
    assert set(twins(text)[1]) == {0, 1}
    empty = twins(b'')
    assert empty[0] == [] and empty[1] == [] and empty[2] == dict.fromkeys(R.FIELDS, 0)


# ------------------------------------------------------------------ the driver loop
def test_driver_loop_retries_with_the_next_seed():
    seen = []

    def run(collide):
        def run_seed(seed):
            seen.append(seed)
            return 'v%d' % seed, dict(dict.fromkeys(R.FIELDS, 0), collisions=1 if seed < collide else 0)
        return run_seed
    assert ops.dedup_verdicts(run(0))[1:] == (dict.fromkeys(R.FIELDS, 0), 0) and seen == [0]
    del seen[:]
    v, rep, seed = ops.dedup_verdicts(run(1))
    assert (v, seed, rep['collisions']) == ('v1', 1, 0) and seen == [0, 1]
    del seen[:]
    assert ops.dedup_verdicts(run(7))[2] == 7
    del seen[:]
    with pytest.raises(UqError) as e:
        ops.dedup_verdicts(run(8))
    assert str(e.value) == 'ERROR: --dedup: 8 hash seeds in a row collided' and seen == list(range(8))


class HostCtx(F.FakeCtx):
    @staticmethod
    def sync():
        pass

    @staticmethod
    def empty(n):
        return torch.empty(n, dtype=torch.uint8)


class HostDedupOps(F.FakeLoadOps):
    """The host twins behind the names Session.dedup_records calls, on CPU tensors.  `collide`: seeds below it run with 2 hash bits."""
    DEDUP_BEST = ops.DEDUP_BEST
    dedup_verdicts = staticmethod(ops.dedup_verdicts)
    collide = 0

    def __init__(self):
        self.seeds = []

    def dedup_params(self, unit=1, prefix=0, hash_bits=64, flags=0, seed=0):
        self.seeds.append(seed)
        return ops.dedup_params(unit, prefix, 2 if seed < self.collide else hash_bits, flags, seed)

    @staticmethod
    def dedup_report_new(ctx):
        return dict.fromkeys(R.FIELDS, 0)

    @staticmethod
    def dedup_keys(ctx, rep, buf, ls, first, n, params):
        keys, got = ops.dedup_keys_host(buf.numpy(), params, ls.numpy().view(np.uint64), first, n, report=rep)
        rep.update(got)
        return torch.from_numpy(keys.reshape(-1))

    @staticmethod
    def argsort_rows(ctx, keys, rows, cols):
        assert cols == 16 and keys.numel() == 16 * rows
        return torch.from_numpy(ops.dedup_order_host(keys.numpy()).view(np.int32))

    @staticmethod
    def dedup_mark(ctx, rep, buf, ls, first, n, params, keys, perm):
        v, got = ops.dedup_mark_host(buf.numpy(), params, keys.numpy(), perm.numpy().view(np.uint32), ls.numpy().view(np.uint64), first, n, report=rep)
        rep.update(got)
        return torch.from_numpy(v)

    @staticmethod
    def dedup_report_fetch(ctx, rep):
        return dict(rep)

    @staticmethod
    def filter_report_new(ctx):
        return None

    @staticmethod
    def filter_plan(ctx, rep, ls, first, n, unit, verdict):
        src, dst, kept, size, _ = ops.filter_plan_host(ls.numpy().view(np.uint64), verdict.numpy(), unit, first)
        return src, dst, kept, size

    @staticmethod
    def compact_records(ctx, buf, src, dst, kept, out_bytes=None):
        return torch.from_numpy(ops.compact_records_host(buf.numpy(), src, dst, kept))

    @staticmethod
    def mate_report_new(ctx):
        return None

    @staticmethod
    def mate_check(ctx, rep, *a):
        pass

    @staticmethod
    def mate_report_fetch(ctx, rep):
        return {'pairs': 0, 'mismatches': 0, 'first_mismatch': None, 'slash_pairs': 0}


def session(tmp_path, flags, collide=0):
    p = tmp_path / 'x.fastq'
    p.write_bytes(b'@a\nA\n+\nI\n')
    s = uq.Session(uq.validate_args(uq.build_parser().parse_args(['-i', str(p), '--quiet', '--multi-pass'] + list(flags))), ctx=HostCtx())
    s.ops = HostDedupOps()
    s.ops.collide = collide
    return s


def test_session_step_and_config_value(tmp_path):
    text = I.spread(2000)
    s = session(tmp_path, ['--dedup', 'keep=best, prefix=040'])
    s.load_device(torch.frombuffer(bytearray(text), dtype=torch.uint8))
    want = R.deduped(text, prefix=40, best=True)
    assert s.d_buf.numpy().tobytes() == want and s.total == len(R.records(want)) and s.path is None
    rep = R.rule(text, prefix=40, best=True)[2]
    assert s.deduping == {'spec': 'keep=best, prefix=040', 'criteria': 'by=seq,prefix=40,keep=best', 'unit': 1, 'seed': 0, 'report': rep}
    assert s.ops.seeds == [0]
    # a seed that collides is left behind, and the seed that held is recorded
    s = session(tmp_path, ['--dedup', 'by=seq'], collide=2)
    s.load_device(torch.frombuffer(bytearray(text), dtype=torch.uint8))
    assert s.ops.seeds == [0, 1, 2] and s.deduping['seed'] == 2 and s.deduping['report'] == R.rule(text, seed=2)[2]
    assert s.d_buf.numpy().tobytes() == R.deduped(text)
    # every seed collides: the refusal, and the text stays
    s = session(tmp_path, ['--dedup', 'by=seq'], collide=99)
    with pytest.raises(UqError, match='8 hash seeds in a row collided'):
        s.load_device(torch.frombuffer(bytearray(text), dtype=torch.uint8))
    assert s.ops.seeds == list(range(8)) and s.deduping is None
    # pairs are units of two
    text = I.pairs()
    s = session(tmp_path, ['--dedup', 'by=seq', '--interleaved'])
    s.load_device(torch.frombuffer(bytearray(text), dtype=torch.uint8))
    assert s.d_buf.numpy().tobytes() == R.deduped(text, unit=2) and s.deduping['unit'] == 2 and s.deduping['report']['dup_reads'] == 10


# ------------------------------------------------------------------ the spec
def test_spec_parser_accepts():
    P, E = recdedup.parse, recdedup.explicit
    assert P('by=seq') == {'prefix': 0, 'flags': 0} and E('by=seq') == 'by=seq,prefix=0,keep=first'
    assert P('prefix=50') == {'prefix': 50, 'flags': 0} and P('keep=best') == {'prefix': 0, 'flags': 1} and P('keep=first') == P('by=seq')
    assert P(' keep = best , prefix=007 ,by=seq') == {'prefix': 7, 'flags': 1} and E(' keep = best , prefix=007 ,by=seq') == 'by=seq,prefix=7,keep=best'
    assert P('prefix=4294967295')['prefix'] == 0xFFFFFFFF and P('prefix=0') == P('by=seq')
    assert E(E('keep=best')) == E('keep=best')
    assert recdedup.items('prefix=3,by=seq') == [('prefix', '3'), ('by', 'seq')]
    c = P('prefix=12,keep=best')
    p = ops.dedup_params(unit=2, seed=5, **c)
    assert (p.unit, p.prefix, p.hash_bits, p.flags, p.seed) == (2, 12, 64, 1, 5)
    assert uq.dedup_criteria('keep=best') == (P('keep=best'), 'by=seq,prefix=0,keep=best')


@pytest.mark.parametrize('spec,words', [
    ('', 'empty'), ('   ', 'empty'), ('by', 'key=value'), ('prefix=1=2', 'key=value'), ('by=seq,,keep=best', 'key=value'), ('seq', 'key=value'),
    ('prefx=3', 'unknown key'), ('by=seq,by=seq', 'twice'), ('prefix=1,prefix=1', 'twice'), ('by=qual', 'only value'), ('by=', 'only value'),
    ('by=SEQ', 'only value'), ('prefix=-1', 'integer'), ('prefix=x', 'integer'), ('prefix=1.5', 'integer'), ('prefix=', 'integer'),
    ('prefix=4294967296', 'outside'), ('prefix=²', 'integer'), ('prefix=٣', 'integer'), ('prefix=3 6', 'integer'),
    ('keep=last', 'neither'), ('keep=', 'neither'), ('keep=Best', 'neither'), ('ke ep=best', 'unknown key'), ('seed=1', 'unknown key'),
])
def test_spec_parser_refuses(spec, words):
    for f in (recdedup.parse, recdedup.explicit):
        with pytest.raises(UqError) as e:
            f(spec)
        assert str(e.value).startswith('ERROR: --dedup') and words in str(e.value), str(e.value)
        if spec.strip(): assert repr(spec) in str(e.value)


def test_report_line():
    rep = dict(dict.fromkeys(R.FIELDS, 0), reads_in=200, units_in=200, dup_reads=50, dup_units=50, classes=150)
    assert recdedup.report_line(rep) == 'dedup: kept 150 of 200 reads (25.00 % duplicates), 150 distinct sequences'
    assert recdedup.report_line(dict.fromkeys(R.FIELDS, 0)) == 'dedup: kept 0 of 0 reads (0.00 % duplicates), 0 distinct sequences'


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
    assert uq.validate_args(args_of(tmp_path)).dedup is None
    for flags in ([], ['--peek'], ['--test'], ['--gz'], ['--verify'], ['--fingerprint'], ['--qc'], ['--bin-qual', 'illumina8'], ['--sort', 'DNA'],
                  ['--interleaved'], ['--multi-pass'], ['--pad'], ['--notricks'], ['--filter', 'min-len=1'], ['--trim', 'head=1'],
                  ['--test', '--device-compressor']):
        assert uq.validate_args(args_of(tmp_path, '--dedup', 'keep=best,prefix=30', *flags)).dedup == 'keep=best,prefix=30'
    refused(args_of(tmp_path, '--dedup', 'by=seq', '--decode'), '--dedup', '--decode')
    refused(args_of(tmp_path, '--dedup', 'prefix=x'), '--dedup', "'prefix=x'")
    refused(args_of(tmp_path, '--dedup', ''), '--dedup', 'empty')
    refused(args_of(tmp_path, '--dedup', 'keep=worst'), '--dedup', "'keep=worst'")


def test_the_sharded_tool_refuses_the_flag_by_name(tmp_path, capsys):
    from uq_amd import dist_encode
    p = tmp_path / 'x.fastq'
    p.write_bytes(b'@a\nA\n+\nI\n')
    assert dist_encode.main(['-i', str(p), '--dedup', 'by=seq']) == 1
    out = capsys.readouterr().out
    assert out.startswith('ERROR: --dedup is for the single-GPU tool (python -m uq_amd.uq): the sharded encoder does not ')


def test_twin_refusals():
    text = I.pairs()
    ls = ops.host_line_starts(text)
    P = ops.dedup_params
    for host in (lambda p, *a: ops.dedup_keys_host(text, p, ls, *a),
                 lambda p, *a: ops.dedup_mark_host(text, p, np.zeros((24, 16), np.uint8), np.arange(24, dtype=np.uint32), ls, *a)):
        for p in (P(unit=0), P(unit=3)):
            with pytest.raises(UqHipError, match='unit is'): host(p)
        for a in ((0, 3), (1, 2), (0, 2, 1)):                    # an odd nreads, first_read, unit_index_base
            with pytest.raises(UqHipError, match='whole pairs'): host(P(unit=2), *a)
        for bits in (0, 65):
            with pytest.raises(UqHipError, match='hash_bits'): host(P(hash_bits=bits))
        with pytest.raises(UqHipError, match='flag'): host(P(flags=2))
        with pytest.raises(UqHipError, match='2\\^32 units'): host(P(), 0, 24, (1 << 32) - 23)
        with pytest.raises(UqHipError, match='2\\^32 units'): host(P(unit=2), 0, 24, (1 << 33) - 22)
        host(P(), 0, 24, (1 << 32) - 24); host(P(unit=2), 0, 24, (1 << 33) - 24)
    with pytest.raises(UqHipError, match='beyond the 24 units'):
        ops.dedup_mark_host(text, P(), np.zeros((24, 16), np.uint8), np.full(24, 24, np.uint32), ls)
    # the device entry points check their arguments before they touch the device: no context, no GPU needed
    rep8, keys16 = ctypes.c_void_p(0x1008), ctypes.c_void_p(0x1010)
    ctx, buf, lsp = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1000), ctypes.c_void_p(ls.ctypes.data)

    def dev_keys(p, first=0, n=24, base=0, keys=keys16, rep=rep8):
        _lib.call('uq_dedup_keys', ctx, buf, lsp, first, n, base, ctypes.byref(p), keys, rep)

    def dev_mark(p, first=0, n=24, base=0, keys=keys16, perm=ctypes.c_void_p(0x1004), rep=rep8):
        _lib.call('uq_dedup_mark', ctx, buf, lsp, first, n, base, ctypes.byref(p), keys, perm, buf, rep)
    for dev in (dev_keys, dev_mark):
        with pytest.raises(UqHipError, match='unit is'): dev(P(unit=3))
        with pytest.raises(UqHipError, match='whole pairs'): dev(P(unit=2), 0, 3)
        with pytest.raises(UqHipError, match='whole pairs'): dev(P(unit=2), 1, 2)
        with pytest.raises(UqHipError, match='whole pairs'): dev(P(unit=2), 0, 2, 1)
        with pytest.raises(UqHipError, match='hash_bits'): dev(P(hash_bits=0))
        with pytest.raises(UqHipError, match='hash_bits'): dev(P(hash_bits=65))
        with pytest.raises(UqHipError, match='2\\^32 units'): dev(P(), 0, 24, (1 << 32) - 23)
        with pytest.raises(UqHipError, match='d_keys must be 16-byte aligned'): dev(P(), keys=ctypes.c_void_p(0x1008))
        with pytest.raises(UqHipError, match='d_report must be 8-byte aligned'): dev(P(), rep=ctypes.c_void_p(0x1004))
        with pytest.raises(UqHipError, match='null argument'): dev(P(), rep=ctypes.c_void_p(0))
    with pytest.raises(UqHipError, match='d_perm must be 4-byte aligned'): dev_mark(P(), perm=ctypes.c_void_p(0x1002))


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
    m = re.search(r'typedef struct uq_dedup_report \{ uint64_t ([^}]*); \} uq_dedup_report;', header)
    assert m and tuple(''.join(m.group(1).split()).split(',')) == R.FIELDS == ops.DEDUP_REPORT_FIELDS
    assert [f for f, _ in _lib.DedupReport._fields_] == list(R.FIELDS) and ctypes.sizeof(_lib.DedupReport) == 64
    assert re.search(r'typedef struct uq_dedup_params \{ uint32_t unit, prefix, hash_bits, flags; uint64_t seed; \} uq_dedup_params;', header)
    assert [f for f, _ in _lib.DedupParams._fields_] == ['unit', 'prefix', 'hash_bits', 'flags', 'seed'] and ctypes.sizeof(_lib.DedupParams) == 24
    assert re.search(r'#define UQ_DEDUP_BEST 1u', header) and ops.DEDUP_BEST == 1 == R.BEST == recdedup.FLAG_BEST
    assert lib.uq_abi_version() == 1 == _lib.ABI_VERSION
    src = open(os.path.join(REPO, 'uq_amd', 'csrc', 'dedup.hip')).read()
    assert int(re.search(r'DK_RMAX = (\d+);', src).group(1)) == I.TILE_RECORDS
    assert int(re.search(r'DK_NV = (\d+);', src).group(1)) * 256 * 16 == I.STAGE and re.search(r'DK_CAP = DK_NV \* 256 \* 16;', src)
