"""GPU: `--bin-qual` through the command line's main(argv) and through the sharded encoder: the container it writes is, member for
member, the container of a plain encode of the text binned on the host (tests/binqual_ref.py) -- config.json gains `quality_binning` and
nothing else."""
import glob
import gzip
import io
import json
import os
import random
import tarfile

import pytest

import binqual_ref as R
from uq_amd import bgzf_host, binqual, uq

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ILLUMINA8 = binqual.parse('illumina8')
RANGES = '3-9:6,10-19:15,20-24:22,25-29:27,30-34:33,35-39:37,40-93:40'


def golden(name):
    plain = os.path.join(GOLD, name + '.fastq')
    if os.path.exists(plain): return open(plain, 'rb').read()
    return gzip.decompress(open(plain + '.gz', 'rb').read())


_REF = {}


def binned(name):
    """(input text, the text binned on the host, bytes changed), once per input."""
    if name not in _REF:
        fq = golden(name)
        _REF[name] = (fq,) + R.apply(fq, ILLUMINA8)
    return _REF[name]


def run(capsys, argv):
    capsys.readouterr()
    rc = uq.main(argv)
    cap = capsys.readouterr()
    assert 'Traceback' not in cap.out + cap.err
    return rc, cap.out


def members_of(path):
    """name -> bytes of every member of a container, plain or --gz (BGZF is a chain of gzip members)."""
    raw = open(path, 'rb').read()
    if raw[:2] == b'\x1f\x8b': raw = gzip.decompress(raw)
    with tarfile.open(fileobj=io.BytesIO(raw)) as t:
        return {m.name: t.extractfile(m).read() for m in t.getmembers()}


def decoded(ctx, path):
    args = uq.build_parser().parse_args(['-i', path, '--decode', '--quiet'])
    uq.validate_args(args)
    buf = io.BytesIO()
    uq.Session(args, ctx=ctx).decode(out=buf)
    return buf.getvalue()


def same_container(a, b, spec, changed):
    """a: written with --bin-qual; b: a plain encode of the binned text."""
    assert sorted(a) == sorted(b)
    for k in a:
        if k != 'config.json': assert a[k] == b[k], k
    ca, cb = json.loads(a['config.json']), json.loads(b['config.json'])
    assert 'quality_binning' not in cb
    assert ca.pop('quality_binning') == {'spec': spec, 'ranges': RANGES, 'changed': changed}
    assert ca == cb
    assert json.dumps(ca, indent=4, sort_keys=True).encode() == b['config.json']


CASES = [('bench_150bp_raw', []), ('bench_var_36_301', []), ('qn_illumina_comment', []),
         ('bench_150bp_raw', ['--sort', 'QUAL']), ('bench_var_36_301', ['--gz']), ('qn_illumina_comment', ['--multi-pass']),
         ('bench_150bp_raw', ['--exact-qname'])]


@pytest.mark.parametrize('name,flags', CASES, ids=lambda v: v if isinstance(v, str) else ('plain' if not v else v[0].strip('-') + ''.join(v[1:])))
def test_container_equals_a_plain_encode_of_the_binned_text(ctx, capsys, tmp_path, name, flags):
    fq, want, changed = binned(name)
    assert changed > 0
    ext = '.uQ.gz' if '--gz' in flags else '.uQ'
    (tmp_path / 'in.fastq').write_bytes(fq)
    (tmp_path / 'binned.fastq').write_bytes(want)
    a, b = str(tmp_path / ('a' + ext)), str(tmp_path / ('b' + ext))
    rc, text = run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', a, '--bin-qual', 'illumina8'] + flags)
    assert rc == 0, text
    total = sum(len(q) for q in fq.split(b'\n')[3::4])
    assert 'Binned qualities (illumina8): %d of %d quality characters changed' % (changed, total) in text
    rc, text = run(capsys, ['-i', str(tmp_path / 'binned.fastq'), '-o', b, '--quiet'] + flags)
    assert rc == 0, text
    same_container(members_of(a), members_of(b), 'illumina8', changed)
    if '--sort' not in flags:
        assert decoded(ctx, a) == want


def test_quiet_and_peek(ctx, capsys, tmp_path):
    fq, want, changed = binned('qn_illumina_comment')
    (tmp_path / 'in.fastq').write_bytes(fq)
    rc, text = run(capsys, ['-i', str(tmp_path / 'in.fastq'), '--bin-qual', 'illumina8', '--peek'])
    assert rc == 0 and 'Binned qualities (illumina8): %d of ' % changed in text and not os.path.exists(str(tmp_path / 'in.fastq.uQ'))
    shown = json.loads(text[text.index('The config.json would look like:') + len('The config.json would look like:'):])
    levels = sorted({chr(c) for q in want.split(b'\n')[3::4] for c in q})   # the eight bins and what the file holds of Q0-Q2
    assert 8 <= len(levels) <= 11 and len({chr(c) for q in fq.split(b'\n')[3::4] for c in q}) > 32
    assert shown['quality_binning']['changed'] == changed and shown['qualities'] == ''.join(levels)
    assert shown['bits_per_quality'] == (3 if len(levels) == 8 else 4)
    assert sorted(shown['qual_distribution']) == levels
    rc, text = run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', str(tmp_path / 'q.uQ'), '--bin-qual', 'illumina8', '--quiet'])
    assert rc == 0 and text == ''


def test_explicit_spec_and_decode_refusal(ctx, capsys, tmp_path):
    fq = golden('qn_illumina_comment')
    spec = '0-19:10,20-93:30'
    want, changed = R.apply(fq, binqual.parse(spec))
    (tmp_path / 'in.fastq').write_bytes(fq)
    out = str(tmp_path / 'o.uQ')
    rc, text = run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', out, '--bin-qual', spec, '--quiet'])
    assert rc == 0
    cfg = json.loads(members_of(out)['config.json'])
    assert cfg['quality_binning'] == {'spec': spec, 'ranges': spec, 'changed': changed} and cfg['qualities'] == '+?' and cfg['bits_per_quality'] == 2
    assert decoded(ctx, out) == want
    rc, text = run(capsys, ['-i', out, '--decode', '--bin-qual', 'illumina8'])
    assert rc == 1 and text.startswith('ERROR: ')
    rc, text = run(capsys, ['-i', str(tmp_path / 'in.fastq'), '--bin-qual', '9-3:1'])
    assert rc == 1 and text.startswith('ERROR: ') and not os.path.exists(str(tmp_path / 'in.fastq.uQ'))


def test_bgzf_input_gives_the_same_container(ctx, capsys, tmp_path):
    fq, want, changed = binned('bench_var_36_301')
    (tmp_path / 'in.fastq').write_bytes(fq)
    (tmp_path / 'in.fastq.gz').write_bytes(bgzf_host.compress(fq))
    a, b = str(tmp_path / 'a.uQ'), str(tmp_path / 'b.uQ')
    assert run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', a, '--bin-qual', 'illumina8', '--quiet'])[0] == 0
    assert run(capsys, ['-i', str(tmp_path / 'in.fastq.gz'), '-o', b, '--bin-qual', 'illumina8', '--quiet'])[0] == 0
    ma, mb = members_of(a), members_of(b)
    assert ma == mb and json.loads(ma['config.json'])['quality_binning']['changed'] == changed
    assert decoded(ctx, b) == want


def n_trick_file():
    rnd = random.Random(31)
    recs = []
    for i in range(400):
        s = bytes(rnd.choice(b'ACGTN' if rnd.random() < 0.15 else b'ACGT') for _ in range(50))
        q = bytes(35 if c == 78 else 33 + rnd.randint(3, 41) for c in s)          # every N carries '#' (Q2), every other base Q3..Q41
        recs.append((b'@n:%d:%d' % (i % 9, i), s, b'+', q))
    return b''.join(b'\n'.join(r) + b'\n' for r in recs)


def test_the_n_trick_survives_the_presets(ctx, capsys, tmp_path):
    """Ns that all carry '#' keep a quality of their own under illumina8 (Q0-Q2 are left alone): bits_per_base stays 2, N_qual holds N
    under the code of an EXISTING quality, and the container verifies.
    With the explicit spec 2-9:6 the no-call quality is merged into a bin other bases use.  What that costs in THIS encoder is not the
    trick as such -- a base with one quality stays a candidate whether it shares that quality or not (analysis.py, uq.py:479-494), so
    bits_per_base stays 2 and N_qual stays non-empty -- but its clean form: N gets a NEW quality code beyond the alphabet,
    which no decoder maps back, and --verify fails.  (Measured on this file: illumina8 N_qual {'N': 0} of 8 qualities; 2-9:6 N_qual
    {'N': 34} of 33 qualities.)  That is what makes this test not vacuous."""
    fq = n_trick_file()
    (tmp_path / 'in.fastq').write_bytes(fq)
    out = str(tmp_path / 'o.uQ')
    rc, text = run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', out, '--bin-qual', 'illumina8', '--quiet', '--verify'])
    assert rc == 0 and text.startswith('Verified: '), text
    cfg = json.loads(members_of(out)['config.json'])
    assert cfg['bits_per_base'] == 2 and cfg['bases'] == 'ACGT' and cfg['N_qual'] == {'N': cfg['qualities'].index('#')}
    assert decoded(ctx, out) == R.apply(fq, ILLUMINA8)[0]
    rc, text = run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', out, '--bin-qual', '2-9:6', '--quiet', '--verify'])
    cfg = json.loads(members_of(out)['config.json'])
    assert '#' not in cfg['qualities'] and cfg['N_qual']['N'] >= len(cfg['qualities'])      # the Q9 form: a code no quality has
    assert rc == 1 and text.startswith('VERIFY FAILED'), text


def test_verify_and_fingerprint(ctx, capsys, tmp_path):
    fq, want, changed = binned('bench_150bp_raw')
    inp, out = str(tmp_path / 'in.fastq'), str(tmp_path / 'o.uQ')
    (tmp_path / 'in.fastq').write_bytes(fq)
    rc, text = run(capsys, ['-i', inp, '-o', out, '--bin-qual', 'illumina8', '--quiet', '--verify'])
    assert rc == 0, text
    lines = text.strip().split('\n')
    assert len(lines) == 1 and lines[0].startswith('Verified: ') and 'in the same order' in lines[0]
    assert lines[0].endswith('; qualities binned by --bin-qual illumina8, %d characters changed' % changed)
    rc, text = run(capsys, ['-i', inp, '--fingerprint', '--bin-qual', 'illumina8'])
    assert rc == 0 and text.count('\n') == 1 and not os.path.exists(inp + '.uQ')
    a = json.loads(text)
    b = json.loads(run(capsys, ['-i', out, '--decode', '--fingerprint'])[1])
    assert a == b
    import fingerprint_ref as F
    assert a == json.loads(__import__('uq_amd.ops', fromlist=['x']).fingerprint_json(F.fingerprint(want)))
    plain = json.loads(run(capsys, ['-i', inp, '--fingerprint'])[1])
    assert {k for k in plain if plain[k] != a[k]} == {'qual', 'pairs', 'records', 'ordered'}


def test_no_flag_no_change(ctx, capsys, tmp_path):
    fq = golden('qn_illumina_comment')
    (tmp_path / 'in.fastq').write_bytes(fq)
    out = str(tmp_path / 'o.uQ')
    assert run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', out, '--quiet'])[0] == 0
    assert 'quality_binning' not in json.loads(members_of(out)['config.json'])
    assert decoded(ctx, out) == fq


@pytest.mark.parametrize('world,flags', [(2, []), (3, ['--sort', 'QUAL', '--raw', 'DNA'])], ids=['2-ranks', '3-ranks-sorted'])
def test_sharded_encoder_writes_the_same_bytes(capsys, tmp_path, world, flags):
    """dist_encode over ranks that share the one card, over gloo (fresh child processes, as tests/test_gpu_dist.py starts them): every rank
    bins its shard at the head of its load, `changed` is summed."""
    from test_gpu_dist import _run_sharded
    fq, want, changed = binned('bench_var_36_301')
    inp = tmp_path / 'in.fastq'
    inp.write_bytes(fq)
    one, many = str(tmp_path / 'one.uQ'), str(tmp_path / 'many.uQ')
    assert run(capsys, ['-i', str(inp), '-o', one, '--bin-qual', 'illumina8', '--quiet'] + flags)[0] == 0
    _run_sharded(world, inp, many, ['--bin-qual', 'illumina8'] + flags)
    a, b = members_of(one), members_of(many)
    assert a == b
    assert json.loads(b['config.json'])['quality_binning'] == {'spec': 'illumina8', 'ranges': RANGES, 'changed': changed}
