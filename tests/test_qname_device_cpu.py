"""CPU check of the HOST half of the device QNAME path (uq_amd/qname_device.py): the closed form that
replaces the reference's sequential loop (uq.py:394-444) and the checkpointed typing rules (uq.py:586-676),
fed by numpy stand-ins for the kernels (tests/fake_qname_ops.py), against the oracle.  The same cases run
on the real kernels in tests/test_gpu_qname.py."""
import numpy as np
import pytest
import torch

import fake_qname_ops as F
import oracle_c
import test_gpu_qname as T
from uq_amd import qname_device


@pytest.fixture()
def fake(monkeypatch):
    def index(ctx, fq):
        host = np.frombuffer(fq, dtype=np.uint8).copy()
        ls = oracle_c.index_lines(host)
        return torch.from_numpy(host), torch.from_numpy(ls.view(np.int64).copy()), (len(ls) - 1) // 4
    monkeypatch.setattr(T, 'INDEX', index)
    monkeypatch.setattr(T, 'FUSED', False)
    monkeypatch.setattr(qname_device, 'ops', F)
    return F.FakeCtx()


@pytest.mark.parametrize('case', ['test_synthetic_illumina_names', 'test_golden_fastq', 'test_mapping_columns_and_suffix',
                                  'test_long_integer_fields', 'test_demotion_checkpoints', 'test_refusals_and_declines',
                                  'test_random_grammars_differential', 'test_mutated_names_differential'])
def test_host_logic_with_numpy_kernels(fake, case):
    getattr(T, case)(fake)


def _restated_tokens(f):
    import qname_raw_inputs as R
    host = R.fastq(f[4])
    ls = oracle_c.index_lines(host)
    return F.qname_tokenise(F.FakeCtx(), torch.from_numpy(host), torch.from_numpy(ls.view(np.int64).copy()), len(f[4]), f[1], f[2], f[3])


def test_tokeniser_inputs_clean_and_flagged():
    """The classification tests/test_gpu_helpers_exact.py relies on, pinned without a GPU: the restatement raises no flag on the clean
    files (there every output is compared with the kernel's) and exactly its one flag on each flagged file (there only the flags are)."""
    import qname_raw_inputs as R
    clean, flagged = R.clean_files(), R.flagged_files()
    assert [f[0] for f in clean] == ['two_columns', 'no_prefix_no_suffix', 'thirty_one_separators']
    for f in clean:
        vals, strs, r = _restated_tokens(f)
        assert r.flags == 0, f[0]
        assert len(vals) == len(strs) == len(f[3]) + 1
    # what the clean files are there for is really in them
    vals, strs, r = _restated_tokens(clean[0])
    assert r.any_long[0] == 7 and r.any_long[1] == 7 and r.first_nonint[0] == 0 and r.first_nonint[1] == len(R.FIELDS)
    assert r.vmin[0] == -(10 ** 18 - 1) and r.vmax[0] == 10 ** 18 - 1
    assert len(clean[2][3]) == 31 and max(len(nm) for nm in clean[0][4]) == 200
    assert {f[0]: f[5] for f in flagged} == {'nineteen_digits': 4, 'nineteen_digits_signed': 4, 'blank_in_field': 2, 'tab_in_field': 2,
                                             'separator_missing': 1, 'separator_extra': 1, 'separators_out_of_order': 1,
                                             'shorter_than_prefix_and_suffix': 8}
    for f in flagged:
        assert _restated_tokens(f)[2].flags == f[5], f[0]
    # the last name of one clean file and of two layout files is staged in LDS and its last 16-byte chunk would cross the end of the buffer: stage_line's byte loop
    assert R.byte_tail_lines(clean[1][4]) == [len(clean[1][4]) - 1] and clean[1][2] == 0       # (no suffix: the bytes copied alone are a field's)
    layouts = dict(R.layout_files())
    for label in ('lengths', 'long_lines_last'):
        assert R.byte_tail_lines(layouts[label]) == [len(layouts[label]) - 1], label
