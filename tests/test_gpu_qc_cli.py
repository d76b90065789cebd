"""GPU: `--qc` through the command line's main(argv): the one line it prints is qc_json of the numpy statement (tests/qc_ref.py) of the text
it was pointed at -- plain and gzip input, the text a container decodes to, the text --bin-qual makes of the input -- and nothing is written."""
import gzip
import json
import os

import pytest

import binqual_ref as R
import qc_ref as Q
from uq_amd import binqual, ops, uq

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def golden(name):
    raw = open(os.path.join(GOLD, name), 'rb').read()
    return gzip.decompress(raw) if name.endswith('.gz') else raw


def run(capsys, argv):
    capsys.readouterr()
    rc = uq.main(argv)
    cap = capsys.readouterr()
    assert 'Traceback' not in cap.out + cap.err
    return rc, cap.out


@pytest.mark.parametrize('name', ['cfg1_10k_100bp.fastq', 'bench_var_36_301.fastq.gz'])
def test_qc_of_the_input(ctx, capsys, tmp_path, name):
    text = golden(name)
    inp = tmp_path / name
    inp.write_bytes(open(os.path.join(GOLD, name), 'rb').read())
    rc, out = run(capsys, ['-i', str(inp), '--qc'])
    assert rc == 0, out
    assert out == ops.qc_json(Q.qc(text, 1024)) + '\n'
    assert sorted(os.listdir(str(tmp_path))) == [name]
    d = json.loads(out)
    assert d['reads'] == text.count(b'\n') // 4 and d['cycles'] == 1024 and d['beyond'] == {'base': [0] * 6, 'qual': [0] * len(d['beyond']['qual']), 'length': 0}


def test_qc_of_the_decoded_text(ctx, capsys, tmp_path):
    want = ops.qc_json(Q.qc(golden('cfg1_10k_100bp.refdecode.fastq'), 1024))
    rc, out = run(capsys, ['-i', os.path.join(GOLD, 'cfg1_10k_100bp.uQ'), '--decode', '--qc'])
    assert rc == 0 and out == want + '\n'
    rc, plain = run(capsys, ['-i', os.path.join(GOLD, 'cfg1_10k_100bp.fastq'), '--qc'])
    assert rc == 0 and plain == out                                              # the container gives the per-cycle profile of its source back


def test_qc_of_the_binned_text(ctx, capsys, tmp_path):
    text = golden('cfg1_10k_100bp.fastq')
    binned, changed = R.apply(text, binqual.parse('illumina8'))
    assert changed > 0
    rc, out = run(capsys, ['-i', os.path.join(GOLD, 'cfg1_10k_100bp.fastq'), '--qc', '--bin-qual', 'illumina8', '--quiet'])
    assert rc == 0, out
    line = [l for l in out.split('\n') if l.startswith('{')]
    assert line == [ops.qc_json(Q.qc(binned, 1024))]
    assert line[0] != ops.qc_json(Q.qc(text, 1024))
    assert not os.path.exists(os.path.join(GOLD, 'cfg1_10k_100bp.fastq.uQ'))


def test_qc_cycles_puts_the_rest_under_beyond(ctx, capsys):
    text = golden('cfg1_10k_100bp.fastq')
    rc, out = run(capsys, ['-i', os.path.join(GOLD, 'cfg1_10k_100bp.fastq'), '--qc', '--qc-cycles', '50'])
    assert rc == 0 and out == ops.qc_json(Q.qc(text, 50)) + '\n'
    d, full = json.loads(out), Q.fields(Q.qc(text, 1024))
    assert d['cycles'] == 50 and len(d['base_by_cycle']) == 50 and len(d['qual_by_cycle']) == 50
    assert d['beyond']['base'] == full['base_by_cycle'][50:100].sum(axis=0).tolist()
    assert sum(d['beyond']['qual']) == 50 * d['reads'] and d['beyond']['length'] == d['reads'] and d['length_hist'] == []
    assert d['base_by_cycle'] == full['base_by_cycle'][:50].tolist()
