"""GPU: `--adapter` through the command line's main(argv): the container it writes is, member for member, the container of a plain encode of the
text cut in Python (tests/adapter_ref.py, behind tests/trim_ref.py where --trim is given) -- config.json gains `adapter` and nothing else;
`--decode` gives the cut text back; each mate is matched against its own adapter; the flags that read the text in HBM (--verify,
--fingerprint, --qc, --test) see the cut text; every refusal with its message; --trim alone does what it did."""
import gzip
import io
import json
import os
import tarfile

import pytest

import adapter_inputs as I
import adapter_ref as R
import filter_ref
import trim_ref as TR
from uq_amd import adapters, bgzf_host, ops, recfilter, rectrim, uq

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
A33 = I.A33.decode()
SPEC = 'seq=' + A33
READS = 800                           # records of the golden input that are taken (the reference is a Python loop per position)


def golden(name):
    plain = os.path.join(GOLD, name + '.fastq')
    if os.path.exists(plain): return open(plain, 'rb').read()
    return gzip.decompress(open(plain + '.gz', 'rb').read())


def ref_params(spec, flags=0):
    c = adapters.parse(spec)
    return R.params(c['seq'], c['seq2'], c['err'], c['overlap'], flags)


_REF = {}


def reference(name='bench_var_36_301', dimers=False):
    """(input with the adapter written into a third of its reads, the text cut in Python, its report), once per input."""
    key = (name, dimers)
    if key not in _REF:
        fq = I.implant_text(golden(name), I.A33, limit=READS, dimers=dimers)
        wins, rep, dst, out = R.run(fq, ref_params(SPEC, R.FRESH))
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


def same_container(a, b, want):
    """a: written with --adapter (and the flags whose keys `want` holds); b: a plain encode of the text they leave."""
    assert sorted(a) == sorted(b)
    for k in a:
        if k != 'config.json': assert a[k] == b[k], k
    ca, cb = json.loads(a['config.json']), json.loads(b['config.json'])
    for key, value in want.items():
        assert key not in cb
        assert ca.pop(key) == value
    assert ca == cb
    assert json.dumps(ca, indent=4, sort_keys=True).encode() == b['config.json']


def adapter_value(rep, spec=SPEC):
    return {'spec': spec, 'criteria': adapters.explicit(spec), 'report': rep}


CASES = [('plain', []), ('bgzf', []), ('gzip', []), ('gzip', ['--host-inflate']), ('plain', ['--gz']), ('plain', ['--multi-pass'])]


@pytest.mark.parametrize('kind,flags', CASES, ids=['%s%s' % (k, ''.join(f)) for k, f in CASES])
def test_container_equals_a_plain_encode_of_the_cut_text(ctx, capsys, tmp_path, kind, flags):
    fq, want, rep = reference()
    assert rep['reads_cut'] * 5 >= rep['reads_in'] and rep['full'] > 100 and rep['partial'] > 50 and rep['emptied'] == 0 and len(want) < len(fq)
    ext = '.uQ.gz' if '--gz' in flags else '.uQ'
    inp = tmp_path / ('in.fastq' if kind == 'plain' else 'in.fastq.gz')
    inp.write_bytes(fq if kind == 'plain' else (bgzf_host.compress(fq) if kind == 'bgzf' else gzip.compress(fq)))
    (tmp_path / 'cut.fastq').write_bytes(want)
    a, b = str(tmp_path / ('a' + ext)), str(tmp_path / ('b' + ext))
    rc, text = run(capsys, ['-i', str(inp), '-o', a, '--adapter', SPEC] + flags)
    assert rc == 0, text
    assert adapters.report_line(rep) in text and 'trim: ' not in text
    assert 'adapter: %d of %d reads cut (%d full, %d partial), %d of %d bases kept (' % (
        rep['reads_cut'], rep['reads_in'], rep['full'], rep['partial'], rep['bases_out'], rep['bases_in']) in text
    rc, text = run(capsys, ['-i', str(tmp_path / 'cut.fastq'), '-o', b, '--quiet'] + [f for f in flags if f != '--host-inflate'])
    assert rc == 0, text
    same_container(members_of(a), members_of(b), {'adapter': adapter_value(rep)})
    assert decoded(ctx, a) == want
    rc, text = run(capsys, ['-i', a, '--decode'])
    assert rc == 0 and text.encode() == want


def test_trim_then_adapter_then_filter(ctx, capsys, tmp_path):
    """polyg= uncovers an adapter in front of a poly-G tail; the adapter step narrows the trimmer's windows; the filter judges what is left."""
    base = I.implant_text(golden('bench_var_36_301'), I.ILLUMINA, limit=READS)
    recs = []
    for i, (qn, s, p, u) in enumerate(TR.records(base)):
        if i % 6 == 0: s, u = s + b'G' * 10, u + b'F' * 10
        recs.append(qn + b'\n' + s + b'\n' + p + b'\n' + u + b'\n')
    fq = b''.join(recs)
    tspec, aspec, fspec = 'polyg=8,q3=20', 'seq=illumina', 'min-len=20'
    twins, _, _, trep = TR.run(fq, rectrim.parse(tspec))
    wins, arep, dst, cut = R.run(fq, ref_params(aspec), windows=twins)
    want, frep = filter_ref.run(cut, recfilter.parse(fspec))[3:]
    assert arep['emptied'] > 50 and arep['reads_cut'] > 200 and trep['cut_polyg'] > 1000 and 0 < frep['reads_out'] < frep['reads_in']
    assert arep['bases_in'] == trep['bases_out'] and cut == R.after_trim(fq, rectrim.parse(tspec), ref_params(aspec))
    assert wins != R.run(fq, ref_params(aspec, R.FRESH))[0] and wins != twins                           # (neither step alone gives these windows)
    (tmp_path / 'in.fastq').write_bytes(fq)
    (tmp_path / 'left.fastq').write_bytes(want)
    inp, a, b = str(tmp_path / 'in.fastq'), str(tmp_path / 'a.uQ'), str(tmp_path / 'b.uQ')
    rc, text = run(capsys, ['-i', inp, '-o', a, '--trim', tspec, '--adapter', aspec, '--filter', fspec])
    assert rc == 0 and rectrim.report_line(trep) in text and adapters.report_line(arep) in text and recfilter.report_line(frep) in text, text
    assert text.index('trim: ') < text.index('adapter: ') < text.index('filter: ')
    assert run(capsys, ['-i', str(tmp_path / 'left.fastq'), '-o', b, '--quiet'])[0] == 0
    same_container(members_of(a), members_of(b), {'trim': {'spec': tspec, 'criteria': tspec, 'report': trep},
                                                  'adapter': {'spec': aspec, 'criteria': 'seq=AGATCGGAAGAGC,err=10,overlap=3', 'report': arep},
                                                  'filter': {'spec': fspec, 'criteria': fspec, 'unit': 1, 'report': frep}})
    assert decoded(ctx, a) == want
    # --verify: the adapter clause behind the trim clause
    rc, text = run(capsys, ['-i', inp, '-o', a, '--trim', tspec, '--adapter', aspec, '--filter', fspec, '--quiet', '--verify'])
    assert rc == 0 and text.startswith('Verified: '), text
    t_clause = '; gives back the reads as --trim %s cut them, %d of %d bases' % (tspec, trep['bases_out'], trep['bases_in'])
    a_clause = '; gives back the reads as --adapter seq=AGATCGGAAGAGC,err=10,overlap=3 cut them, %d of %d bases' % (arep['bases_out'], arep['bases_in'])
    assert t_clause + a_clause in text
    # --peek shows the same config and writes nothing
    rc, text = run(capsys, ['-i', inp, '--trim', tspec, '--adapter', aspec, '--filter', fspec, '--peek'])
    assert rc == 0 and not os.path.exists(inp + '.uQ')
    shown = json.loads(text[text.index('The config.json would look like:') + len('The config.json would look like:'):])
    assert shown['adapter']['report'] == arep and shown['trim']['report'] == trep and shown['reads'] == frep['reads_out']


# ------------------------------------------------------------------ pairs
def test_each_mate_has_its_own_adapter(ctx, capsys, tmp_path):
    from trim_inputs import interleave, mates
    A2 = I.adapter(20, seed=7)
    # (the mates' N carry a quality of their own, which the format's N trick relies on: an adapter written over an N would leave that quality on
    # another base, SURVEY.md Q9 -- so the N are taken out first: this test is about adapters)
    r1, r2 = (b''.join(qn + b'\n' + s.replace(b'N', b'A') + b'\n' + p + b'\n' + u.replace(b'#', b'$') + b'\n' for qn, s, p, u in TR.records(m)) for m in mates())
    r1, r2 = I.implant_text(r1, I.A33, dimers=False), I.implant_text(r2, A2, every=2, seed=9, dimers=False)
    both = interleave(r1, r2)
    p = lambda name: str(tmp_path / name)
    for spec in (SPEC + ',seq2=' + A2.decode(), SPEC):
        c = ref_params(spec, R.FRESH | R.PAIRED)
        if c['seq2'] is None: c['seq2'] = c['seq']
        wins, rep, dst, want = R.run(both, c)
        assert rep['emptied'] == 0 and rep['reads_in'] == 600 and rep['reads_cut'] - rep['mate2'] > 60
        assert (rep['mate2'] > 100) == ('seq2' in spec)
        one = lambda t, s: R.run(t, R.params(s, err=10, overlap=3, flags=R.FRESH))[3]
        halves = (one(r1, I.A33), one(r2, A2 if 'seq2' in spec else I.A33))
        assert want == interleave(*halves)
        for name, data in (('r1.fastq', r1), ('r2.fastq', r2), ('both.fastq', both), ('cut.fastq', want)): (tmp_path / name).write_bytes(data)
        a, b, k = p('a.uQ'), p('b.uQ'), p('k.uQ')
        rc, text = run(capsys, ['-i', p('r1.fastq'), '--mate2', p('r2.fastq'), '-o', a, '--adapter', spec])
        assert rc == 0 and adapters.report_line(rep) in text, text
        assert run(capsys, ['-i', p('both.fastq'), '--interleaved', '-o', b, '--adapter', spec, '--quiet'])[0] == 0
        assert run(capsys, ['-i', p('cut.fastq'), '--interleaved', '-o', k, '--quiet'])[0] == 0
        ma, mb, mk = members_of(a), members_of(b), members_of(k)
        assert ma == mb
        same_container(ma, mk, {'adapter': adapter_value(rep, spec)})
        assert json.loads(ma['config.json'])['paired'] == {'layout': 'interleaved', 'pairs': 300, 'slash_pairs': 0}
        assert decoded(ctx, a) == want
        o1, o2 = p('o1.fastq'), p('o2.fastq')
        rc, text = run(capsys, ['-i', a, '--decode', '--split-mates', o1, o2])
        assert rc == 0, text
        assert (open(o1, 'rb').read(), open(o2, 'rb').read()) == halves


# ------------------------------------------------------------------ with the other flags
def test_verify_fingerprint_and_qc_see_the_cut_text(ctx, capsys, tmp_path):
    fq, want, rep = reference()
    inp, out = str(tmp_path / 'in.fastq'), str(tmp_path / 'o.uQ')
    (tmp_path / 'in.fastq').write_bytes(fq)
    rc, text = run(capsys, ['-i', inp, '-o', out, '--adapter', SPEC, '--quiet', '--verify'])
    assert rc == 0, text
    lines = text.strip().split('\n')
    assert len(lines) == 1 and lines[0].startswith('Verified: ') and 'in the same order' in lines[0] and '--trim' not in lines[0]
    assert '%s decodes to the same %d reads' % (out, rep['reads_in']) in lines[0]
    assert lines[0].endswith('; gives back the reads as --adapter %s cut them, %d of %d bases' % (adapters.explicit(SPEC), rep['bases_out'], rep['bases_in']))
    rc, text = run(capsys, ['-i', inp, '--fingerprint', '--adapter', SPEC])
    assert rc == 0 and text.count('\n') == 1 and not os.path.exists(inp + '.uQ')
    a = json.loads(text)
    assert a == json.loads(run(capsys, ['-i', out, '--decode', '--fingerprint'])[1])
    import fingerprint_ref as F
    assert a == json.loads(ops.fingerprint_json(F.fingerprint(want)))
    assert a['bases'] == rep['bases_out'] and a['reads'] == rep['reads_in']
    rc, text = run(capsys, ['-i', inp, '--qc', '--adapter', SPEC])
    assert rc == 0 and text.count('\n') == 1
    assert json.loads(text) == json.loads(ops.qc_json(ops.qc_host(want)))


def test_test_with_the_device_compressor(ctx, capsys, tmp_path):
    fq, want, rep = reference()
    (tmp_path / 'in.fastq').write_bytes(fq)
    (tmp_path / 'cut.fastq').write_bytes(want)
    a, b = str(tmp_path / 'a.uQ'), str(tmp_path / 'b.uQ')
    flags = ['--test', '--device-compressor', '--quiet']
    assert run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', a, '--adapter', SPEC] + flags)[0] == 0
    assert run(capsys, ['-i', str(tmp_path / 'cut.fastq'), '-o', b] + flags)[0] == 0
    same_container(members_of(a), members_of(b), {'adapter': adapter_value(rep)})


def test_trim_alone_does_what_it_did(ctx, capsys, tmp_path):
    """--trim without --adapter: the container of the plain encode of the text trimmed in Python, the `trim` key alone, the trimmer's line and
    no word of adapters."""
    fq = golden('qn_illumina_comment')
    spec = 'head=2,tail=3,crop=120,polyg=5,q5=6,q3=8,trim-n=1'
    wins, dst, want, rep = TR.run(fq, rectrim.parse(spec))
    (tmp_path / 'in.fastq').write_bytes(fq)
    (tmp_path / 'trimmed.fastq').write_bytes(want)
    a, b = str(tmp_path / 'a.uQ'), str(tmp_path / 'b.uQ')
    rc, text = run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', a, '--trim', spec])
    assert rc == 0 and text.count(rectrim.report_line(rep)) == 1 and 'adapter' not in text
    rc, plain = run(capsys, ['-i', str(tmp_path / 'trimmed.fastq'), '-o', b])
    assert rc == 0
    same_container(members_of(a), members_of(b), {'trim': {'spec': spec, 'criteria': rectrim.explicit(spec), 'report': rep}})
    rc, text = run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', a, '--trim', spec, '--quiet', '--verify'])
    assert rc == 0 and text.strip().endswith('; gives back the reads as --trim %s cut them, %d of %d bases' % (spec, rep['bases_out'], rep['bases_in']))
    # and no flag: no key
    assert run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', a, '--quiet'])[0] == 0
    cfg = json.loads(members_of(a)['config.json'])
    assert 'adapter' not in cfg and 'trim' not in cfg and decoded(ctx, a) == fq


# ------------------------------------------------------------------ refusals
def test_refusals(ctx, capsys, tmp_path):
    fq, want, rep = reference(dimers=True)
    inp, out = str(tmp_path / 'in.fastq'), str(tmp_path / 'o.uQ')
    (tmp_path / 'in.fastq').write_bytes(fq)
    small = str(tmp_path / 'small.fastq')
    (tmp_path / 'small.fastq').write_bytes(golden('qn_illumina_comment'))
    assert run(capsys, ['-i', small, '-o', out, '--quiet'])[0] == 0
    rc, text = run(capsys, ['-i', out, '--decode', '--adapter', SPEC])
    assert rc == 1 and text.startswith('ERROR: --adapter') and '--decode' in text
    os.remove(out)
    for spec, words in (('seq=ACGX', "'seq=ACGX'"), ('sequence=ACGT', 'unknown key'), ('seq=ACGT,err=31', 'outside'), ('seq=ACGT,overlap=5', 'shorter'),
                        ('err=3', 'required'), ('seq=ACGT,seq=ACGT', 'twice'), ('', 'empty')):
        rc, text = run(capsys, ['-i', small, '-o', out, '--adapter', spec])
        assert rc == 1 and text.startswith('ERROR: --adapter') and words in text and (not spec or repr(spec) in text), text
        assert not os.path.exists(out)
    rc, text = run(capsys, ['-i', small, '-o', out, '--adapter', SPEC + ',seq2=nextera'])
    assert rc == 1 and text.startswith('ERROR: --adapter') and 'seq2' in text and '--mate2' in text and '--interleaved' in text and not os.path.exists(out)
    # reads left without bases: refused before anything is written, unless --filter drops them
    assert rep['emptied'] > 50
    message = 'ERROR: --adapter %s leaves %d reads without bases; add --filter min-len=1 (or higher)' % (SPEC, rep['emptied'])
    for flags in ([], ['--fingerprint'], ['--qc'], ['--peek'], ['--filter', 'max-n=5'], ['--filter', 'min-len=0']):
        with_out = [] if flags in (['--fingerprint'], ['--qc']) else ['-o', out]
        rc, text = run(capsys, ['-i', inp, '--adapter', SPEC] + flags + with_out)
        assert rc == 1 and text.strip().split('\n')[-1] == message, text
        assert not os.path.exists(out) and not os.path.exists(inp + '.uQ')
    rc, text = run(capsys, ['-i', inp, '-o', out, '--adapter', SPEC, '--filter', 'min-len=1', '--quiet'])
    assert rc == 0 and os.path.exists(out)
    assert decoded(ctx, out) == filter_ref.filtered(want, filter_ref.criteria(min_len=1))
    os.remove(out)
    # both steps empty reads: the trimmer's message comes first
    hard = 'q5=30,q3=30'
    temptied = TR.run(fq, rectrim.parse(hard))[3]['emptied']
    assert temptied > 100
    rc, text = run(capsys, ['-i', inp, '-o', out, '--trim', hard, '--adapter', SPEC])
    assert rc == 1 and text.strip().split('\n')[-1] == 'ERROR: --trim %s leaves %d reads without bases; add --filter min-len=1 (or higher)' % (hard, temptied)
    assert not os.path.exists(out)
    from uq_amd import dist_encode
    capsys.readouterr()
    assert dist_encode.main(['-i', inp, '-o', out, '--adapter', SPEC]) == 1
    assert capsys.readouterr().out.startswith('ERROR: --adapter') and not os.path.exists(out)
