"""CPU: the texts of the record-count refusals (whole_records and the three places of a session that use it), the argument checks the five
host twins of uq_amd.ops share, and one UqError class however uq_amd.uq is started."""
import runpy
import sys

import numpy as np
import pytest
import torch

import fake_decode_ops as F
from uq_amd import container, errors, ops, uq

NOT_BY_4 = 'ERROR: The FASTQ file provided contains255rows, which is not divisible by 4!'
RECORD = b'@r:1\nACGT\n+\nIIII\n'


def _text(nlines):
    return torch.frombuffer(bytearray((RECORD * 64)[:-1] if nlines == 255 else RECORD * (nlines // 4)), dtype=torch.uint8) if nlines \
        else torch.empty(0, dtype=torch.uint8)


def _session(tmp_path, flags=()):
    p = tmp_path / 'x.fastq'
    p.write_bytes(RECORD)
    s = uq.Session(uq.validate_args(uq.build_parser().parse_args(['-i', str(p), '--quiet'] + list(flags))), ctx=F.FakeCtx())
    s.ops = F.FakeLoadOps()
    return s


# ------------------------------------------------------------------ whole records
def test_whole_records_texts():
    assert uq.whole_records(256) == 64 and uq.whole_records(256, 'R1 (a.fastq)') == 64 and uq.whole_records(4) == 1
    for what, text in ((None, NOT_BY_4), ('R1 (a.fastq)', 'ERROR: R1 (a.fastq) contains 255 rows, which is not divisible by 4!')):
        with pytest.raises(uq.UqError) as e:
            uq.whole_records(255, what)
        assert str(e.value) == text
        with pytest.raises(uq.UqError) as e:
            uq.whole_records(0, what)
        assert str(e.value) == 'ERROR: empty input'


@pytest.mark.parametrize('index_only', [False, True])
def test_load_device_record_count(tmp_path, index_only):
    for nlines, text in ((0, 'ERROR: empty input'), (255, NOT_BY_4)):
        s = _session(tmp_path, ['--multi-pass'])
        s.index_only = index_only
        with pytest.raises(uq.UqError) as e:
            s.load_device(_text(nlines))
        assert str(e.value) == text
    s = _session(tmp_path, ['--multi-pass'])
    s.index_only = index_only
    s.load_device(_text(256))
    assert s.total == 64 and s.load_path == ('index only' if index_only else 'multi-pass')
    assert s.path is None and s.host.tobytes() == RECORD * 64             # load() never ran: the host copy comes from d_buf
    assert s.d_ls.numel() == 257


def test_indexed_record_count(tmp_path):
    s = _session(tmp_path)
    for nlines, text in ((0, 'ERROR: empty input'), (255, 'ERROR: R2 (b.fastq) contains 255 rows, which is not divisible by 4!')):
        with pytest.raises(uq.UqError) as e:
            s.indexed(_text(nlines), 'R2 (b.fastq)')
        assert str(e.value) == text
    n, ls = s.indexed(_text(256), 'R2 (b.fastq)')
    assert n == 64 and ls.numel() == 257


# ------------------------------------------------------------------ the host twins' arguments
FIVE_LINES = RECORD + b'@r:2\n'
LUT = bytes(range(256))


@pytest.mark.parametrize('who,twin', [('fingerprint', ops.fingerprint_host), ('qc', ops.qc_host),
                                      ('requantise', lambda data, **kw: ops.requantise_qualities_host(data, LUT, **kw))])
def test_host_twin_refusals(who, twin):
    with pytest.raises(ValueError) as e:
        twin(FIVE_LINES)
    assert str(e.value) == '%s: 5 lines are not whole FASTQ records' % who
    for kw in (dict(first_read=3), dict(first_read=-1, nreads=1), dict(first_read=1, nreads=2), dict(nreads=-1)):
        with pytest.raises(ValueError) as e:
            twin(RECORD * 2, **kw)
        assert str(e.value) == '%s: records beyond the index' % who
    twin(RECORD * 2, first_read=2)                                         # no records: nothing to refuse
    twin(np.frombuffer(FIVE_LINES, np.uint8), first_read=0, nreads=1)       # a count of the caller's: the fifth line is nobody's


def test_pair_twin_refusals():
    for a, b in ((FIVE_LINES, FIVE_LINES), (RECORD * 2, RECORD)):
        with pytest.raises(ValueError) as e:
            ops.interleave_records_host(a, b)
        assert str(e.value) == 'interleave: the two texts are not the same number of whole FASTQ records'
    for kw in (dict(first_pair=3), dict(first_pair=-1, npairs=1), dict(first_pair=1, npairs=2)):
        with pytest.raises(ValueError) as e:
            ops.interleave_records_host(RECORD * 2, RECORD * 2, **kw)
        assert str(e.value) == 'interleave: records beyond the index'
    with pytest.raises(ValueError) as e:
        ops.interleave_records_host(RECORD * 2, RECORD, npairs=2)
    assert str(e.value) == 'interleave: records beyond the index'
    assert ops.interleave_records_host(RECORD * 2, RECORD * 2, first_pair=2).size == 0
    # the mate check takes the pairs its strides reach: a fifth line is nobody's, a first record beyond the index is a negative count
    assert ops.mate_check_host(FIVE_LINES, FIVE_LINES) == {'pairs': 1, 'mismatches': 0, 'first_mismatch': None, 'slash_pairs': 0}
    with pytest.raises(ValueError) as e:
        ops.mate_check_host(RECORD * 2, RECORD * 2, first_a=3)
    assert str(e.value) == 'mate check: negative argument'
    for kw in (dict(first_a=2, npairs=1), dict(first_b=1, npairs=2), dict(step_a=2, npairs=2)):
        with pytest.raises(ValueError) as e:
            ops.mate_check_host(RECORD * 2, RECORD * 2, **kw)
        assert str(e.value) == 'mate check: records beyond the index'


# ------------------------------------------------------------------ one UqError class
def test_script_reports_a_bad_bin_qual_spec_in_one_line(tmp_path, capsys, monkeypatch):
    p = tmp_path / 'x.fastq'
    p.write_bytes(RECORD)
    monkeypatch.setattr(sys, 'argv', ['uq', '-i', str(p), '--bin-qual', 'bogus'])
    with pytest.raises(SystemExit) as e:
        runpy.run_module('uq_amd.uq', run_name='__main__')                 # (validation fails before a Session exists: no GPU)
    assert e.value.code == 1
    out = capsys.readouterr().out
    assert out.startswith("ERROR: --bin-qual: unknown preset 'bogus'") and out.count('\n') == 1


def test_one_error_class_however_the_module_is_started():
    script = runpy.run_module('uq_amd.uq', run_name='uq_amd_uq_as_a_script')      # what `python -m uq_amd.uq` executes, main() not called
    assert script['UqError'] is errors.UqError is uq.UqError and uq.error is errors.error
    with pytest.raises(script['UqError'], match='not a tar'):                 # what main() catches is what the container reader raises
        container._error(container.NOT_A_TAR)
