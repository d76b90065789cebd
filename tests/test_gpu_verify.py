"""GPU: `--verify` and `--fingerprint` through the command line's main(argv), on files of at most a few thousand reads."""
import glob
import gzip
import io
import json
import os
import random

import numpy as np
import pytest

import fingerprint_ref as F
import uq_oracle as O
from uq_amd import synth, uq

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
READS = synth.fastq(20261019, 1500, (36, 151), n_rate=1)


def run(capsys, argv):
    capsys.readouterr()
    rc = uq.main(argv)
    cap = capsys.readouterr()
    assert 'Traceback' not in cap.out + cap.err
    return rc, cap.out


def encode_verify(capsys, tmp_path, fq, flags, name='in.fastq'):
    inp = tmp_path / name
    inp.write_bytes(fq)
    out = tmp_path / ('out.uQ.gz' if '--gz' in flags else 'out.uQ')
    rc, text = run(capsys, ['-i', str(inp), '-o', str(out), '--quiet', '--verify'] + flags)
    return rc, text, str(out)


def decoded(ctx, path):
    args = uq.build_parser().parse_args(['-i', path, '--decode', '--quiet'])
    uq.validate_args(args)
    buf = io.BytesIO()
    uq.Session(args, ctx=ctx).decode(out=buf)
    return buf.getvalue()


@pytest.mark.parametrize('case', ['raw', 'default', 'gz', 'gzip-input'])
def test_verify_passes_in_order(ctx, capsys, tmp_path, case):
    flags = {'raw': ['--raw', 'DNA', 'QUAL', 'QNAME'], 'default': [], 'gz': ['--gz'], 'gzip-input': []}[case]
    fq, name = (gzip.compress(READS), 'in.fastq.gz') if case == 'gzip-input' else (READS, 'in.fastq')
    rc, text, out = encode_verify(capsys, tmp_path, fq, flags, name)
    want = F.fingerprint(READS)
    assert rc == 0, text
    lines = text.strip().split('\n')
    assert len(lines) == 1 and lines[0].startswith('Verified: ') and 'in the same order' in lines[0] and 'multiset' not in lines[0]
    assert '%016x' % want['records'] in lines[0] and 'third lines' not in lines[0]
    assert os.path.getsize(out) > 0


@pytest.mark.parametrize('sort', ['DNA', 'QUAL', 'QNAME'])
def test_verify_passes_as_a_multiset_when_sorted(ctx, capsys, tmp_path, sort):
    rc, text, out = encode_verify(capsys, tmp_path, READS, ['--sort', sort])
    assert rc == 0, text
    assert 'as a multiset' in text and '--sort ' + sort in text and 'in the same order' not in text
    assert '%016x' % F.fingerprint(READS)['records'] in text
    # the sort did move reads: the decoded text is not the input
    got = F.fingerprint(decoded(ctx, out))
    assert got['records'] == F.fingerprint(READS)['records'] and got['ordered'] != F.fingerprint(READS)['ordered']


def test_verify_counts_the_line_3_comments_the_format_drops(ctx, capsys, tmp_path):
    lines = READS.split(b'\n')
    for i in range(2, 4 * 100, 4): lines[i] = b'+' + lines[i - 2][1:]
    rc, text, _ = encode_verify(capsys, tmp_path, b'\n'.join(lines), [])
    assert rc == 0 and 'in the same order' in text and 'of 100 third lines is not kept' in text


def test_leading_zeros_fail_with_the_qname_diagnosis(ctx, capsys, tmp_path):
    """`:007:` is stored as the number 7.  The sequence and quality lines are verified, the QNAME lines are named as the cause,
    the status is 1 and the container is still there and decodes."""
    rnd = random.Random(5)
    recs = [(b'@run:%03d:%d' % ((i * 7) % 1000, i), bytes(rnd.choice(b'ACGT') for _ in range(40)), b'+', bytes(rnd.randrange(35, 70) for _ in range(40)))
            for i in range(1200)]
    fq = b''.join(b'\n'.join(r) + b'\n' for r in recs)
    assert b':007:' in fq
    rc, text, out = encode_verify(capsys, tmp_path, fq, [])
    assert rc == 1
    assert text.startswith('VERIFY FAILED') and 'sequence and quality lines are verified' in text and 'QNAME lines are not reproduced' in text
    assert 'Q12' in text and 'leading zeros' in text and 'reordered' not in text and 'stays where it was written' in text
    back = decoded(ctx, out)
    assert back != fq and back.split(b'\n')[1::4] == fq.split(b'\n')[1::4] and back.split(b'\n')[3::4] == fq.split(b'\n')[3::4]
    assert b'@run:7:1\n' in back


def test_a_container_no_decoder_reads_fails_without_a_traceback(ctx, capsys, tmp_path):
    """the N-trick gives N a quality code of its own, which no decoder maps back."""
    fq = open(os.path.join(GOLD, 'fixed_n_newcode.fastq'), 'rb').read()
    rc, text, out = encode_verify(capsys, tmp_path, fq, [])
    assert rc == 1 and text.startswith('VERIFY FAILED') and os.path.getsize(out) > 0
    # and with --notricks the same reads verify
    rc, text, _ = encode_verify(capsys, tmp_path, fq, ['--notricks'])
    assert rc == 0 and 'in the same order' in text


def test_host_built_qname_text_verifies(ctx, capsys, tmp_path):
    """40 numeric QNAME columns: more than the device text kernel writes, the decoded text is built on the host and uploaded."""
    names = [b'@' + b':'.join(b'%d' % (i * 7 + k) for k in range(40)) for i in range(400)]
    fq = b''.join(n + b'\nACGTACGTAC\n+\nIIIIHHHHII\n' for n in names)
    rc, text, out = encode_verify(capsys, tmp_path, fq, [])
    args = uq.build_parser().parse_args(['-i', out, '--decode', '--quiet'])
    s = uq.Session(uq.validate_args(args), ctx=ctx)
    assert not uq.Session.device_text_possible(s.open_container()[1])
    assert rc == 0 and 'in the same order' in text
    assert ctx.to_numpy(s.decode_to_device()).tobytes() == fq == decoded(ctx, out)


def test_verify_is_refused_where_nothing_is_written(capsys, tmp_path):
    inp = tmp_path / 'in.fastq'
    inp.write_bytes(READS)
    for extra in (['--peek'], ['--test'], ['--decode'], ['--fingerprint']):
        rc, text = run(capsys, ['-i', str(inp), '--verify'] + extra)
        assert rc == 1 and text.startswith('ERROR: ') and not os.path.exists(str(inp) + '.uQ')
    rc, text = run(capsys, ['-i', str(inp), '--decode', '--fingerprint', '--bgzf'])
    assert rc == 1 and text.startswith('ERROR: ')


@pytest.mark.parametrize('flags', [['--sort', 'QUAL', '--raw', 'DNA'], ['--raw', 'QNAME', '--pattern', '1.2', '2.1']], ids=['sorted', 'unsorted'])
def test_fingerprint_of_the_input_and_of_the_decoded_container(ctx, capsys, tmp_path, flags):
    inp, out = tmp_path / 'in.fastq', tmp_path / 'out.uQ'
    inp.write_bytes(READS)
    rc, text = run(capsys, ['-i', str(inp), '--fingerprint'])
    assert rc == 0 and not os.path.exists(str(inp) + '.uQ')
    a = json.loads(text)
    want = F.fingerprint(READS)
    assert list(a) == ['uqfp'] + list(F.FIELDS) and a['uqfp'] == 1
    assert a == dict({'uqfp': 1}, **{k: (v if k in F.FIELDS[:3] else '%016x' % v) for k, v in want.items()})
    assert uq.main(['-i', str(inp), '-o', str(out), '--quiet'] + flags) == 0
    rc, text = run(capsys, ['-i', str(out), '--decode', '--fingerprint'])
    b = json.loads(text)
    assert rc == 0 and text.count('\n') == 1                              # one line, no FASTQ text
    assert b['records'] == a['records'] and b['reads'] == a['reads'] and b['bases'] == a['bases']
    assert (b['ordered'] == a['ordered']) == ('--sort' not in flags)
    gz = tmp_path / 'in.fastq.gz'
    gz.write_bytes(gzip.compress(READS))
    assert json.loads(run(capsys, ['-i', str(gz), '--fingerprint'])[1]) == a


GOLDEN = sorted(os.path.basename(f)[:-3] for f in glob.glob(os.path.join(GOLD, '*.uQ')))
DECODABLE = [n for n in GOLDEN if n not in ('fixed_n_newcode', 'two_ntrick_bases')]


@pytest.mark.parametrize('name', DECODABLE[::4])
def test_decode_writes_the_same_bytes_either_way(ctx, name):
    """`--decode` writes what it wrote before decode was split up, and the text tensor the fingerprint reads is those bytes: both against
    the oracle's decode of the reference-written container."""
    path = os.path.join(GOLD, name + '.uQ')
    want = O.decode(*O.read_tar(path)).encode('latin-1')
    assert decoded(ctx, path) == want
    args = uq.build_parser().parse_args(['-i', path, '--decode', '--quiet'])
    assert ctx.to_numpy(uq.Session(uq.validate_args(args), ctx=ctx).decode_to_device()).tobytes() == want
