"""GPU: `--filter` through the command line's main(argv): the container it writes is, member for member, the container of a plain encode of
the text filtered in Python (tests/filter_ref.py) -- config.json gains `filter` and nothing else; `--decode` gives the filtered text back;
pairs stay pairs; the flags that read the text in HBM (--verify, --fingerprint, --qc, --test, --bin-qual) see the filtered text; every
refusal with its message."""
import gzip
import io
import json
import os
import random
import tarfile

import pytest

import filter_ref as R
from uq_amd import bgzf_host, ops, recfilter, uq

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SPEC = 'min-len=100,max-n=1,min-mean-q=19,sample=0.8,seed=3'
EXPLICIT = 'min-len=100,max-n=1,min-mean-q=19,sample=0.8,seed=3'


def golden(name):
    plain = os.path.join(GOLD, name + '.fastq')
    if os.path.exists(plain): return open(plain, 'rb').read()
    return gzip.decompress(open(plain + '.gz', 'rb').read())


_REF = {}


def reference(name, spec=SPEC, unit=1):
    """(input text, the text filtered in Python, its report), once per input and spec."""
    key = (name, spec, unit)
    if key not in _REF:
        fq = golden(name)
        v, src, dst, out, rep = R.run(fq, recfilter.parse(spec), unit)
        _REF[key] = (fq, out, rep)
    return _REF[key]


def run(capsys, argv):
    capsys.readouterr()
    rc = uq.main(argv)
    cap = capsys.readouterr()
    assert 'Traceback' not in cap.out + cap.err
    return rc, cap.out


def members_of(path):
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


def same_container(a, b, want_filter, extra=()):
    """a: written with --filter; b: a plain encode of the filtered text."""
    assert sorted(a) == sorted(b)
    for k in a:
        if k != 'config.json': assert a[k] == b[k], k
    ca, cb = json.loads(a['config.json']), json.loads(b['config.json'])
    assert 'filter' not in cb
    assert ca.pop('filter') == want_filter
    assert ca == cb
    assert json.dumps(ca, indent=4, sort_keys=True).encode() == b['config.json']


def filter_value(rep, spec=SPEC, explicit=EXPLICIT, unit=1):
    return {'spec': spec, 'criteria': explicit, 'unit': unit, 'report': rep}


CASES = [('bench_var_36_301', 'plain', []), ('bench_var_36_301', 'bgzf', []), ('bench_var_36_301', 'gzip', []), ('bench_var_36_301', 'gzip', ['--host-inflate']),
         ('bench_var_36_301', 'plain', ['--multi-pass']), ('bench_150bp_raw', 'plain', ['--gz']), ('qn_illumina_comment', 'plain', ['--sort', 'QUAL'])]


@pytest.mark.parametrize('name,kind,flags', CASES, ids=['%s-%s%s' % (n, k, ''.join(f)) for n, k, f in CASES])
def test_container_equals_a_plain_encode_of_the_filtered_text(ctx, capsys, tmp_path, name, kind, flags):
    spec = SPEC if name != 'qn_illumina_comment' else 'min-mean-q=20,sample=0.9'          # (short reads of mean quality 14 .. 25)
    fq, want, rep = reference(name, spec)
    assert 0 < rep['reads_out'] < rep['reads_in'] and len(want) == rep['bytes_out']
    ext = '.uQ.gz' if '--gz' in flags else '.uQ'
    inp = tmp_path / ('in.fastq' if kind == 'plain' else 'in.fastq.gz')
    inp.write_bytes(fq if kind == 'plain' else (bgzf_host.compress(fq) if kind == 'bgzf' else gzip.compress(fq)))
    (tmp_path / 'filtered.fastq').write_bytes(want)
    a, b = str(tmp_path / ('a' + ext)), str(tmp_path / ('b' + ext))
    rc, text = run(capsys, ['-i', str(inp), '-o', a, '--filter', spec] + flags)
    assert rc == 0, text
    assert recfilter.report_line(rep) in text
    assert 'filter: kept %d of %d reads (' % (rep['reads_out'], rep['reads_in']) in text
    rc, text = run(capsys, ['-i', str(tmp_path / 'filtered.fastq'), '-o', b, '--quiet'] + [f for f in flags if f != '--host-inflate'])
    assert rc == 0, text
    same_container(members_of(a), members_of(b), filter_value(rep, spec, recfilter.explicit(spec)))
    if '--sort' not in flags:
        assert decoded(ctx, a) == want
        rc, text = run(capsys, ['-i', a, '--decode'])
        assert rc == 0 and text.encode() == want


def test_quiet_peek_and_an_untidy_spec(ctx, capsys, tmp_path):
    fq = golden('bench_var_36_301')
    spec = ' max-n=0 , min-len=0100 '
    c = recfilter.parse(spec)
    want, rep = R.run(fq, c)[3:]
    (tmp_path / 'in.fastq').write_bytes(fq)
    inp = str(tmp_path / 'in.fastq')
    rc, text = run(capsys, ['-i', inp, '--filter', spec, '--peek'])
    assert rc == 0 and recfilter.report_line(rep) in text and not os.path.exists(inp + '.uQ')
    shown = json.loads(text[text.index('The config.json would look like:') + len('The config.json would look like:'):])
    assert shown['filter'] == filter_value(rep, spec, 'min-len=100,max-n=0') and shown['reads'] == rep['reads_out']
    assert 'N' not in shown['base_distribution']
    rc, text = run(capsys, ['-i', inp, '-o', str(tmp_path / 'q.uQ'), '--filter', spec, '--quiet'])
    assert rc == 0 and text == ''
    assert decoded(ctx, str(tmp_path / 'q.uQ')) == want


# ------------------------------------------------------------------ pairs
def mates(n=300, seed=41):
    rnd = random.Random(seed)
    out = []
    for m in (1, 2):
        recs = []
        for i in range(n):
            L = rnd.randint(36, 151)
            seq = bytes(rnd.choice(b'ACGT') if rnd.random() > 0.01 else 78 for _ in range(L))
            recs.append(b'\n'.join((b'@A00:7:HX:%d:%d:%d %d:N:0:ACGT' % (1 + i % 4, 1000 + i // 7, 2000 + 3 * i, m), seq, b'+',
                                    bytes(35 if c == 78 else rnd.randint(36, 73) for c in seq))) + b'\n')
        out.append(b''.join(recs))
    return out


def interleave(a, b):
    ra, rb = a.split(b'\n')[:-1], b.split(b'\n')[:-1]
    return b''.join(b'\n'.join(ra[4 * i:4 * i + 4]) + b'\n' + b'\n'.join(rb[4 * i:4 * i + 4]) + b'\n' for i in range(len(ra) // 4))


def test_pairs_keep_both_mates_or_neither(ctx, capsys, tmp_path):
    r1, r2 = mates()
    both = interleave(r1, r2)
    spec = 'max-n=0,min-len=50,sample=0.9,seed=5'
    v, src, dst, want, rep = R.run(both, recfilter.parse(spec), 2)
    assert rep['fail_mate'] > 20 and 0 < rep['reads_out'] < 600 and rep['reads_out'] % 2 == 0
    for name, data in (('r1.fastq', r1), ('r2.fastq', r2), ('both.fastq', both), ('filtered.fastq', want)): (tmp_path / name).write_bytes(data)
    p = lambda name: str(tmp_path / name)
    a, b, k = p('a.uQ'), p('b.uQ'), p('k.uQ')
    rc, text = run(capsys, ['-i', p('r1.fastq'), '--mate2', p('r2.fastq'), '-o', a, '--filter', spec])
    assert rc == 0 and recfilter.report_line(rep) in text, text
    assert run(capsys, ['-i', p('both.fastq'), '--interleaved', '-o', b, '--filter', spec, '--quiet'])[0] == 0
    assert run(capsys, ['-i', p('filtered.fastq'), '--interleaved', '-o', k, '--quiet'])[0] == 0
    ma, mb, mk = members_of(a), members_of(b), members_of(k)
    assert ma == mb
    same_container(ma, mk, filter_value(rep, spec, 'min-len=50,max-n=0,sample=0.9,seed=5', 2))
    assert json.loads(ma['config.json'])['paired'] == {'layout': 'interleaved', 'pairs': rep['reads_out'] // 2, 'slash_pairs': 0}
    assert decoded(ctx, a) == want
    o1, o2 = p('o1.fastq'), p('o2.fastq')
    rc, text = run(capsys, ['-i', a, '--decode', '--split-mates', o1, o2])
    assert rc == 0, text
    recs = R.records(want)
    assert open(o1, 'rb').read() == b''.join(b'\n'.join(r) + b'\n' for r in recs[0::2])
    assert open(o2, 'rb').read() == b''.join(b'\n'.join(r) + b'\n' for r in recs[1::2])
    # mates that do not match are still refused on the input as given, with the message of a paired encode without --filter
    bad = r2.replace(b'@A00:7:HX:2:1000:2003 2', b'@A00:7:HX:2:1000:2004 2', 1)
    (tmp_path / 'bad.fastq').write_bytes(bad)
    (tmp_path / 'badboth.fastq').write_bytes(interleave(r1, bad))
    plain = run(capsys, ['-i', p('r1.fastq'), '--mate2', p('bad.fastq'), '-o', p('x.uQ'), '--quiet'])
    assert plain[0] == 1 and plain[1].startswith('ERROR: pair 1: ')
    assert run(capsys, ['-i', p('r1.fastq'), '--mate2', p('bad.fastq'), '-o', p('x.uQ'), '--quiet', '--filter', spec]) == plain
    assert run(capsys, ['-i', p('badboth.fastq'), '--interleaved', '-o', p('x.uQ'), '--quiet', '--filter', spec]) == plain
    (tmp_path / 'odd.fastq').write_bytes(both + b'\n'.join(R.records(r1)[0]) + b'\n')
    rc, text = run(capsys, ['-i', p('odd.fastq'), '--interleaved', '-o', p('x.uQ'), '--quiet', '--filter', spec])
    assert rc == 1 and text.startswith('ERROR: --interleaved: the input holds 601 reads, an odd number') and not os.path.exists(p('x.uQ'))


# ------------------------------------------------------------------ with the other flags
def test_verify_fingerprint_and_qc_see_the_filtered_text(ctx, capsys, tmp_path):
    fq, want, rep = reference('bench_150bp_raw')
    inp, out = str(tmp_path / 'in.fastq'), str(tmp_path / 'o.uQ')
    (tmp_path / 'in.fastq').write_bytes(fq)
    rc, text = run(capsys, ['-i', inp, '-o', out, '--filter', SPEC, '--quiet', '--verify'])
    assert rc == 0, text
    lines = text.strip().split('\n')
    assert len(lines) == 1 and lines[0].startswith('Verified: ') and 'in the same order' in lines[0]
    assert '%s decodes to the same %d reads' % (out, rep['reads_out']) in lines[0]
    assert lines[0].endswith('; gives back the %d reads --filter kept of %d' % (rep['reads_out'], rep['reads_in']))
    rc, text = run(capsys, ['-i', inp, '--fingerprint', '--filter', SPEC])
    assert rc == 0 and text.count('\n') == 1 and not os.path.exists(inp + '.uQ')
    a = json.loads(text)
    assert a == json.loads(run(capsys, ['-i', out, '--decode', '--fingerprint'])[1])
    import fingerprint_ref as F
    assert a == json.loads(ops.fingerprint_json(F.fingerprint(want)))
    rc, text = run(capsys, ['-i', inp, '--qc', '--filter', SPEC])
    assert rc == 0 and text.count('\n') == 1
    assert json.loads(text) == json.loads(ops.qc_json(ops.qc_host(want)))
    assert json.loads(text) == json.loads(run(capsys, ['-i', out, '--decode', '--qc'])[1])


def test_bin_qual_judges_the_qualities_as_given(ctx, capsys, tmp_path):
    """The filter runs first: min-mean-q sees the qualities of the file, the binning the reads that are left."""
    import binqual_ref
    from uq_amd import binqual
    fq = golden('bench_var_36_301')
    spec = 'min-mean-q=20'
    want, rep = R.run(fq, recfilter.parse(spec))[3:]
    assert 0 < rep['fail_mean_q'] < rep['reads_in']
    binned, changed = binqual_ref.apply(want, binqual.parse('4level'))
    (tmp_path / 'in.fastq').write_bytes(fq)
    out = str(tmp_path / 'o.uQ')
    rc, text = run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', out, '--filter', spec, '--bin-qual', '4level', '--quiet', '--verify'])
    assert rc == 0 and text.startswith('Verified: '), text
    assert '; gives back the %d reads --filter kept of %d; qualities binned by --bin-qual 4level, %d characters changed' % (
        rep['reads_out'], rep['reads_in'], changed) in text
    cfg = json.loads(members_of(out)['config.json'])
    assert cfg['filter']['report'] == rep and cfg['quality_binning']['changed'] == changed
    assert decoded(ctx, out) == binned


def test_test_with_the_device_compressor(ctx, capsys, tmp_path):
    fq, want, rep = reference('bench_var_36_301')
    (tmp_path / 'in.fastq').write_bytes(fq)
    (tmp_path / 'filtered.fastq').write_bytes(want)
    a, b = str(tmp_path / 'a.uQ'), str(tmp_path / 'b.uQ')
    flags = ['--test', '--device-compressor', '--quiet']
    assert run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', a, '--filter', SPEC] + flags)[0] == 0
    assert run(capsys, ['-i', str(tmp_path / 'filtered.fastq'), '-o', b] + flags)[0] == 0
    same_container(members_of(a), members_of(b), filter_value(rep))


@pytest.mark.parametrize('kind', ['plain', 'gzip', 'interleaved'])
def test_the_unfiltered_text_is_freed_before_the_load_step(ctx, tmp_path, kind):
    """When the step after the filter starts (the queued census and pack), the session holds the kept tenth of the text, not the 6.8 MB it
    read: the loaders keep no name of the unfiltered buffer."""
    from uq_amd import synth
    fq = synth.fastq(20261020, 20000, 150)
    inp = tmp_path / ('in.fastq.gz' if kind == 'gzip' else 'in.fastq')
    inp.write_bytes(gzip.compress(fq, 1) if kind == 'gzip' else fq)
    flags = ['--interleaved'] if kind == 'interleaved' else []       # (synth-v1 gives every read its own name: as "pairs" they are refused, so the mate check is left out below)
    args = uq.validate_args(uq.build_parser().parse_args(['-i', str(inp), '-o', str(tmp_path / 'o.uQ'), '--quiet', '--filter', 'sample=0.1'] + flags))
    s = uq.Session(args, ctx=ctx)
    if kind == 'interleaved': s.require_mates = lambda *a: None
    t = ctx.torch
    seen = []
    queued = s._load_queued

    def spy(census):
        t.cuda.synchronize()
        seen.append(t.cuda.memory_allocated() - base)
        return queued(census)
    s._load_queued = spy
    t.cuda.synchronize()
    base = t.cuda.memory_allocated()
    s.load_input()
    assert len(seen) == 1 and s.filtering['report']['reads_in'] == 20000
    assert s.d_buf.numel() == s.filtering['report']['bytes_out'] < len(fq) // 8
    assert seen[0] < len(fq) // 2, 'the unfiltered text (%d bytes) is still allocated when the load step starts: %d bytes' % (len(fq), seen[0])


def test_no_flag_no_change(ctx, capsys, tmp_path):
    fq = golden('qn_illumina_comment')
    (tmp_path / 'in.fastq').write_bytes(fq)
    out = str(tmp_path / 'o.uQ')
    assert run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', out, '--quiet'])[0] == 0
    assert 'filter' not in json.loads(members_of(out)['config.json'])
    assert decoded(ctx, out) == fq


# ------------------------------------------------------------------ refusals
def test_refusals(ctx, capsys, tmp_path):
    fq = golden('qn_illumina_comment')
    inp, out = str(tmp_path / 'in.fastq'), str(tmp_path / 'o.uQ')
    (tmp_path / 'in.fastq').write_bytes(fq)
    n = len(R.records(fq))
    assert run(capsys, ['-i', inp, '-o', out, '--quiet'])[0] == 0
    rc, text = run(capsys, ['-i', out, '--decode', '--filter', 'min-len=1'])
    assert rc == 1 and text.startswith('ERROR: --filter') and '--decode' in text
    os.remove(out)
    for spec, words in (('min-len=x', "'min-len=x'"), ('minlen=3', 'unknown key'), ('min-len=9,max-len=3', 'larger'), ('sample=0', 'outside'),
                        ('seed=1', 'sample'), ('min-len=1,min-len=2', 'twice')):
        rc, text = run(capsys, ['-i', inp, '-o', out, '--filter', spec])
        assert rc == 1 and text.startswith('ERROR: --filter') and words in text and repr(spec) in text, text
        assert not os.path.exists(out)
    for flags in ([], ['--fingerprint'], ['--qc'], ['--peek']):
        rc, text = run(capsys, ['-i', inp, '--filter', 'min-len=100000'] + (flags if flags and flags != ['--peek'] else flags + ['-o', out]))
        assert rc == 1 and text.strip().split('\n')[-1] == 'ERROR: --filter min-len=100000 keeps none of the %d reads' % n, text
        assert not os.path.exists(out) and not os.path.exists(inp + '.uQ')
    from uq_amd import dist_encode
    capsys.readouterr()
    assert dist_encode.main(['-i', inp, '-o', out, '--filter', 'min-len=1']) == 1
    assert capsys.readouterr().out.startswith('ERROR: --filter') and not os.path.exists(out)
