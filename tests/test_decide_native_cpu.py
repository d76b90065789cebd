"""CPU: the host decisions that moved into the library (csrc/decide.hip: uq_decide_from_stats, uq_make_pack_params,
uq_same_pack_params) against their Python twins (analysis.decide_from_pairs_py, ops.make_pack_params_py, ops.same_pack_params_py):
the decisions as exact dicts, the pack parameters byte for byte -- on the statistics of every FASTQ fixture under tests/golden and on
seeded random histograms built to reach every branch (1- to 8-bit alphabets on both sides, no / one / two / three N-trick candidates,
the Q9 new-code case, --notricks, --pad, fixed and variable lengths, single symbols, more non-zero counters than the compact list)."""
import glob
import os

import numpy as np
import pytest

import oracle_c
from uq_amd import analysis, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, '*.fastq')))
N_RANDOM = 5400
SIZES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 200)        # alphabet sizes on both sides of every rung of the width ladder
LENGTHS = ((100, 100), (150, 150), (7, 7), (1, 1), (36, 301), (149, 150), (5, 6), (0, 3), (2 ** 31 - 8, 2 ** 31 - 8))


def _compact_hs(keys, cnts, len_min, len_max):
    """A HostStats as ops.stats_fetch builds it from a uq_stats_compact."""
    raw = np.zeros(1, dtype=ops.STATS_COMPACT_DTYPE)
    raw[0]['n'] = len(keys); raw[0]['len_min'] = len_min; raw[0]['len_max'] = len_max
    raw[0]['bad_plus'] = raw[0]['bad_len'] = np.iinfo(np.uint64).max
    raw[0]['key'][:len(keys)] = keys; raw[0]['count'][:len(keys)] = cnts
    return ops.HostStats(raw[0])


def _params(d, max_record_bytes=640, avg=0, make=None):
    make = make or ops.make_pack_params
    return make(d['bases'], d['qualities'], d['N_qual'], d['bits_per_base'], d['bits_per_quality'], d['variable_read_lengths'],
                d['dna_bytes_per_row'], d['quality_bytes_per_row'], d['dna_max'], max_record_bytes, avg_record_bytes=avg)


def _check(counts, len_min, len_max, first_seen, notricks, pad, order=None):
    """Every form of the native decisions == the twin (as a dict, key order of N_qual included); the pack parameters byte for byte."""
    flat = np.asarray(counts, dtype=np.uint64).reshape(65536)
    keys = np.flatnonzero(flat)
    if order is not None: keys = keys[order.permutation(keys.size)]
    kw = dict(notricks=notricks, pad=pad, first_seen=first_seen)
    want = analysis.decide_from_pairs_py(keys, flat[keys].astype(np.int64), len_min, len_max, **kw)
    got = [analysis.decide_from_counts(flat.reshape(256, 256), len_min, len_max, **kw),
           analysis.decide_from_pairs(keys, flat[keys], len_min, len_max, **kw)]
    if keys.size <= ops.STATS_COMPACT_CAP:
        hs = _compact_hs(keys, flat[keys], len_min, len_max)
        assert hs.compact is not None and np.array_equal(hs.nz_keys, keys)
        got.append(analysis.decide_from_stats(hs, **kw))
    for d in got:
        assert d == want
        assert list(d['N_qual'].items()) == list(want['N_qual'].items())
        assert [type(d[k]) for k in sorted(d)] == [type(want[k]) for k in sorted(want)]
    if max([len(want['qualities'])] + [v for v in want['N_qual'].values()]) < 32768:
        a, b = _params(want), _params(want, make=ops.make_pack_params_py)
        assert bytes(a) == bytes(b)
        assert ops.same_pack_params(a, b) and ops.same_pack_params_py(a, b)
    return want


@pytest.mark.parametrize('path', FIXTURES, ids=[os.path.basename(p) for p in FIXTURES])
def test_fixture_statistics(path):
    assert len(FIXTURES) >= 40
    buf = np.fromfile(path, dtype=np.uint8)
    ls = oracle_c.index_lines(buf)
    n = (len(ls) - 1) // 4
    assert n > 0
    st = oracle_c.stats(buf, ls, 0, n)
    for notricks in (False, True):
        for pad in (False, True):
            for fs in (None, st['first_seen'], lambda: st['first_seen']):
                _check(st['counts'], st['len_min'], st['len_max'], fs, notricks, pad)


def _random_case(rng, i):
    """Histogram i: `nreg` bases with two or more qualities each, `ncand` bases with exactly one (the N-trick candidates: with a quality of
    their own, or one they share -- the Q9 new code), over `nqual` quality symbols."""
    nreg = SIZES[i % len(SIZES)]
    nqual = SIZES[(i // len(SIZES)) % len(SIZES)]
    ncand = (i // 7) % 4 if nqual > 1 else 0
    dense = i % 29 == 0                                       # more than 2048 non-zero counters: the dense form
    if dense: nreg, nqual = max(nreg, 64), max(nqual, 40)
    syms = rng.permutation(256)
    bases, cands = syms[:nreg], syms[200:200 + ncand]         # (nreg <= 200: disjoint)
    quals = rng.permutation(256)[:nqual]
    counts = np.zeros((256, 256), dtype=np.uint64)
    big = i % 11 == 0                                         # counts beyond 2^32
    for b in bases:
        k = nqual if (dense or nqual == 1) else int(rng.integers(2, min(nqual, 6) + 1))
        for q in (quals if k == nqual else rng.choice(quals, size=k, replace=False)):
            counts[b, q] = int(rng.integers(1, 1 << 40)) if big else int(rng.integers(1, 1000))
    q9 = False
    for j, b in enumerate(cands):
        used = np.flatnonzero(counts.sum(axis=0))
        free = np.setdiff1d(quals, used)
        if free.size and (i + j) % 2 == 0: q = int(free[0])   # a quality of its own: the N-trick proper (an existing code)
        else: q = int(rng.choice(used)); q9 = True            # shared with other bases: a new code
        counts[b, q] = int(rng.integers(1, 50))
    lmin, lmax = LENGTHS[(i // 3) % len(LENGTHS)]
    fs_kind = i % 3
    fs = None
    if fs_kind: fs = rng.permutation(256).astype(np.uint64 if fs_kind == 1 else np.int64) - (0 if fs_kind == 1 else 128)
    return counts, lmin, lmax, fs, bool((i // 5) % 2), bool((i // 13) % 2), dict(nreg=nreg, nqual=nqual, ncand=ncand, dense=dense, q9=q9)


def test_random_histograms_reach_every_branch():
    rng = np.random.default_rng(20261019)
    seen = dict(bpb=set(), bpq=set(), ntrick=set(), q9=set(), flags=set(), variable=set(), lmod4=set(), single=set(), dense=set(), remaining_one=0)
    for i in range(N_RANDOM):
        counts, lmin, lmax, fs, notricks, pad, meta = _random_case(rng, i)
        if i % 17 == 0 and fs is not None: fs = (lambda a: (lambda: a))(fs)
        d = _check(counts, lmin, lmax, fs, notricks, pad, order=rng)
        seen['bpb'].add(d['bits_per_base']); seen['bpq'].add(d['bits_per_quality'])
        seen['ntrick'].add(len(d['N_qual'])); seen['flags'].add((notricks, pad)); seen['variable'].add(d['variable_read_lengths'])
        if d['N_qual']: seen['q9'].add(max(d['N_qual'].values()) >= len(d['qualities']))
        if d['N_qual'] and max(d['N_qual'].values()) == 2 ** d['bits_per_quality'] and not pad: seen['q9'].add('code = 2^b')
        seen['lmod4'].add(lmax % 4); seen['dense'].add(int(np.count_nonzero(counts)) > ops.STATS_COMPACT_CAP)
        seen['single'].add((len(d['bases']) == 1, len(d['qualities']) == 1))
        if meta['ncand'] and not notricks and len(d['N_qual']) < meta['ncand'] + (meta['nqual'] == 1) * meta['nreg']: seen['remaining_one'] += 1
    assert seen['bpb'] == set(range(2, 9)) and seen['bpq'] == set(range(2, 9))
    assert {0, 1, 2, 3} <= seen['ntrick']
    assert seen['q9'] == {False, True, 'code = 2^b'}
    assert seen['flags'] == {(a, b) for a in (False, True) for b in (False, True)}
    assert seen['variable'] == {False, True} and seen['lmod4'] == {0, 1, 2, 3}
    assert {(True, False), (False, True), (True, True), (False, False)} <= seen['single']
    assert seen['dense'] == {False, True}


def test_single_candidate_alone_is_kept_and_empty_table_is_refused():
    counts = np.zeros((256, 256), dtype=np.uint64)
    counts[ord('N'), ord('#')] = 7                            # the only base qualifies for the N-trick: it stays in the alphabet (uq.py:482)
    d = _check(counts, 4, 4, None, False, False)
    assert d['bases'] == 'N' and d['N_qual'] == {}
    counts[ord('A'), ord('#')] = 1                            # two candidates for one place: the first goes (a shared quality: a new code), the second stays
    d = _check(counts, 4, 4, None, False, False)
    assert d['bases'] == 'N' and d['N_qual'] == {'A': 2}
    fs = np.zeros(256, dtype=np.uint64); fs[ord('A')] = 5
    d = _check(counts, 4, 4, fs, False, False)
    assert d['bases'] == 'A' and d['N_qual'] == {'N': 2}
    for f in (analysis.decide_from_counts, analysis.decide_from_counts_py):
        with pytest.raises(ValueError):
            f(np.zeros((256, 256), dtype=np.uint64), 0, 0)


def test_same_pack_params_tells_every_field_apart():
    counts = np.zeros((256, 256), dtype=np.uint64)
    for b in 'ACGT':
        for q in '#5I': counts[ord(b), ord(q)] = 9
    counts[ord('N'), ord('!')] = 2
    d = analysis.decide_from_counts(counts, 10, 12)
    a = _params(d)
    assert ops.same_pack_params(a, _params(d, max_record_bytes=99, avg=77))          # the tile-sizing hints do not count
    for field in ('bits_per_base', 'bits_per_quality', 'variable', 'dna_bytes_per_row', 'quality_bytes_per_row', 'dna_max'):
        b = _params(d); setattr(b, field, getattr(b, field) + 1)
        assert not ops.same_pack_params(a, b) and not ops.same_pack_params_py(a, b), field
    for table in ('dna_code', 'qual_code', 'n_qual'):
        for at in (0, 255):
            b = _params(d); getattr(b, table)[at] += 1
            assert not ops.same_pack_params(a, b) and not ops.same_pack_params_py(a, b), (table, at)
