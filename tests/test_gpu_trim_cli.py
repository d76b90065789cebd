"""GPU: `--trim` through the command line's main(argv): the container it writes is, member for member, the container of a plain encode of the
text trimmed in Python (tests/trim_ref.py) -- config.json gains `trim` and nothing else; `--decode` gives the trimmed text back; `--filter`
judges the reads as trimmed; each mate of a pair is trimmed on its own; the flags that read the text in HBM (--verify, --fingerprint, --qc,
--test, --bin-qual) see the trimmed text; every refusal with its message."""
import gzip
import io
import json
import os
import tarfile

import pytest

import filter_ref
import trim_ref as R
from uq_amd import bgzf_host, ops, recfilter, rectrim, uq

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SPEC = 'head=2,tail=3,crop=120,polyg=5,q5=6,q3=8,trim-n=1'         # leaves bases in every read of the golden inputs
HARD = 'q5=30,q3=30'                                                # empties many


def golden(name):
    plain = os.path.join(GOLD, name + '.fastq')
    if os.path.exists(plain): return open(plain, 'rb').read()
    return gzip.decompress(open(plain + '.gz', 'rb').read())


_REF = {}


def reference(name, spec=SPEC):
    """(input text, the text trimmed in Python, its report), once per input and spec."""
    key = (name, spec)
    if key not in _REF:
        fq = golden(name)
        wins, dst, out, rep = R.run(fq, rectrim.parse(spec))
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


def same_container(a, b, want, drop=()):
    """a: written with --trim (and the flags whose keys `want` holds); b: a plain encode of the text they leave."""
    assert sorted(a) == sorted(b)
    for k in a:
        if k != 'config.json': assert a[k] == b[k], k
    ca, cb = json.loads(a['config.json']), json.loads(b['config.json'])
    for key, value in want.items():
        assert key not in cb
        assert ca.pop(key) == value
    assert ca == cb
    assert json.dumps(ca, indent=4, sort_keys=True).encode() == b['config.json']


def trim_value(rep, spec=SPEC):
    return {'spec': spec, 'criteria': rectrim.explicit(spec), 'report': rep}


CASES = [('bench_var_36_301', 'plain', []), ('bench_var_36_301', 'bgzf', []), ('bench_var_36_301', 'gzip', []), ('bench_var_36_301', 'gzip', ['--host-inflate']),
         ('bench_var_36_301', 'plain', ['--multi-pass']), ('bench_150bp_raw', 'plain', ['--gz']), ('qn_illumina_comment', 'plain', ['--sort', 'QUAL'])]


@pytest.mark.parametrize('name,kind,flags', CASES, ids=['%s-%s%s' % (n, k, ''.join(f)) for n, k, f in CASES])
def test_container_equals_a_plain_encode_of_the_trimmed_text(ctx, capsys, tmp_path, name, kind, flags):
    fq, want, rep = reference(name)
    assert rep['reads_trimmed'] == rep['reads_in'] and rep['emptied'] == 0 and len(want) == rep['bytes_out'] < len(fq)
    assert rep['cut_q3'] > 0 and rep['cut_q5'] > 0 and rep['cut_fixed'] > 0
    ext = '.uQ.gz' if '--gz' in flags else '.uQ'
    inp = tmp_path / ('in.fastq' if kind == 'plain' else 'in.fastq.gz')
    inp.write_bytes(fq if kind == 'plain' else (bgzf_host.compress(fq) if kind == 'bgzf' else gzip.compress(fq)))
    (tmp_path / 'trimmed.fastq').write_bytes(want)
    a, b = str(tmp_path / ('a' + ext)), str(tmp_path / ('b' + ext))
    rc, text = run(capsys, ['-i', str(inp), '-o', a, '--trim', SPEC] + flags)
    assert rc == 0, text
    assert rectrim.report_line(rep) in text
    assert 'trim: %d of %d reads cut, %d of %d bases kept (' % (rep['reads_trimmed'], rep['reads_in'], rep['bases_out'], rep['bases_in']) in text
    rc, text = run(capsys, ['-i', str(tmp_path / 'trimmed.fastq'), '-o', b, '--quiet'] + [f for f in flags if f != '--host-inflate'])
    assert rc == 0, text
    same_container(members_of(a), members_of(b), {'trim': trim_value(rep)})
    if '--sort' not in flags:
        assert decoded(ctx, a) == want
        rc, text = run(capsys, ['-i', a, '--decode'])
        assert rc == 0 and text.encode() == want


def test_the_filter_judges_the_reads_as_trimmed(ctx, capsys, tmp_path):
    fq = golden('bench_var_36_301')
    tspec, fspec = ' q3 = 25 ', 'min-len=30,min-mean-q=20'
    trimmed, trep = R.run(fq, rectrim.parse(tspec))[2:]
    want, frep = filter_ref.run(trimmed, recfilter.parse(fspec))[3:]
    assert trep['emptied'] > 50 and 0 < frep['reads_out'] < frep['reads_in'] == trep['reads_in'] and frep['bytes_in'] == trep['bytes_out']
    assert frep['reads_out'] != filter_ref.run(fq, recfilter.parse(fspec))[4]['reads_out']          # (the other order keeps other reads)
    (tmp_path / 'in.fastq').write_bytes(fq)
    (tmp_path / 'left.fastq').write_bytes(want)
    inp, a, b = str(tmp_path / 'in.fastq'), str(tmp_path / 'a.uQ'), str(tmp_path / 'b.uQ')
    rc, text = run(capsys, ['-i', inp, '-o', a, '--trim', tspec, '--filter', fspec])
    assert rc == 0 and rectrim.report_line(trep) in text and recfilter.report_line(frep) in text, text
    assert text.index('trim: ') < text.index('filter: ')
    assert run(capsys, ['-i', str(tmp_path / 'left.fastq'), '-o', b, '--quiet'])[0] == 0
    same_container(members_of(a), members_of(b), {'trim': {'spec': tspec, 'criteria': 'q3=25', 'report': trep},
                                                  'filter': {'spec': fspec, 'criteria': fspec, 'unit': 1, 'report': frep}})
    assert decoded(ctx, a) == want
    # --peek shows the same config and writes nothing; --quiet says nothing
    rc, text = run(capsys, ['-i', inp, '--trim', tspec, '--filter', fspec, '--peek'])
    assert rc == 0 and not os.path.exists(inp + '.uQ')
    shown = json.loads(text[text.index('The config.json would look like:') + len('The config.json would look like:'):])
    assert shown['trim']['report'] == trep and shown['reads'] == frep['reads_out']
    rc, text = run(capsys, ['-i', inp, '-o', str(tmp_path / 'q.uQ'), '--trim', SPEC, '--quiet'])
    assert rc == 0 and text == ''


# ------------------------------------------------------------------ pairs
def test_each_mate_is_trimmed_on_its_own(ctx, capsys, tmp_path):
    from trim_inputs import interleave, mates
    r1, r2 = mates()
    both = interleave(r1, r2)
    spec = 'tail=5,q3=15,trim-n=1'
    want, rep = R.run(both, rectrim.parse(spec))[2:]
    assert rep['emptied'] == 0 and rep['cut_q3'] > 100 and rep['reads_in'] == 600
    assert want == interleave(R.trimmed(r1, rectrim.parse(spec)), R.trimmed(r2, rectrim.parse(spec)))
    for name, data in (('r1.fastq', r1), ('r2.fastq', r2), ('both.fastq', both), ('trimmed.fastq', want)): (tmp_path / name).write_bytes(data)
    p = lambda name: str(tmp_path / name)
    a, b, k = p('a.uQ'), p('b.uQ'), p('k.uQ')
    rc, text = run(capsys, ['-i', p('r1.fastq'), '--mate2', p('r2.fastq'), '-o', a, '--trim', spec])
    assert rc == 0 and rectrim.report_line(rep) in text, text
    assert run(capsys, ['-i', p('both.fastq'), '--interleaved', '-o', b, '--trim', spec, '--quiet'])[0] == 0
    assert run(capsys, ['-i', p('trimmed.fastq'), '--interleaved', '-o', k, '--quiet'])[0] == 0
    ma, mb, mk = members_of(a), members_of(b), members_of(k)
    assert ma == mb
    same_container(ma, mk, {'trim': trim_value(rep, spec)})
    assert json.loads(ma['config.json'])['paired'] == {'layout': 'interleaved', 'pairs': 300, 'slash_pairs': 0}
    assert decoded(ctx, a) == want
    o1, o2 = p('o1.fastq'), p('o2.fastq')
    rc, text = run(capsys, ['-i', a, '--decode', '--split-mates', o1, o2])
    assert rc == 0, text
    assert open(o1, 'rb').read() == R.trimmed(r1, rectrim.parse(spec)) and open(o2, 'rb').read() == R.trimmed(r2, rectrim.parse(spec))
    # trim, then filter whole pairs: the order check -> interleave -> trim -> filter
    tspec, fspec = 'q3=20', 'min-len=40'
    trimmed = R.trimmed(both, rectrim.parse(tspec))
    left, frep = filter_ref.run(trimmed, recfilter.parse(fspec), 2)[3:]
    assert 0 < frep['reads_out'] < 600 and frep['fail_mate'] > 0
    for flags in (['-i', p('r1.fastq'), '--mate2', p('r2.fastq')], ['-i', p('both.fastq'), '--interleaved']):
        assert run(capsys, flags + ['-o', p('f.uQ'), '--trim', tspec, '--filter', fspec, '--quiet'])[0] == 0
        assert decoded(ctx, p('f.uQ')) == left
    # mates that do not match are still refused on the input as given
    bad = r2.replace(b'@A00:7:HX:2:1000:2003 2', b'@A00:7:HX:2:1000:2004 2', 1)
    (tmp_path / 'bad.fastq').write_bytes(bad)
    plain = run(capsys, ['-i', p('r1.fastq'), '--mate2', p('bad.fastq'), '-o', p('x.uQ'), '--quiet'])
    assert plain[0] == 1 and plain[1].startswith('ERROR: pair 1: ')
    assert run(capsys, ['-i', p('r1.fastq'), '--mate2', p('bad.fastq'), '-o', p('x.uQ'), '--quiet', '--trim', spec]) == plain


# ------------------------------------------------------------------ with the other flags
def test_verify_fingerprint_and_qc_see_the_trimmed_text(ctx, capsys, tmp_path):
    fq, want, rep = reference('bench_150bp_raw')
    inp, out = str(tmp_path / 'in.fastq'), str(tmp_path / 'o.uQ')
    (tmp_path / 'in.fastq').write_bytes(fq)
    rc, text = run(capsys, ['-i', inp, '-o', out, '--trim', SPEC, '--quiet', '--verify'])
    assert rc == 0, text
    lines = text.strip().split('\n')
    assert len(lines) == 1 and lines[0].startswith('Verified: ') and 'in the same order' in lines[0]
    assert '%s decodes to the same %d reads' % (out, rep['reads_in']) in lines[0]
    assert lines[0].endswith('; gives back the reads as --trim %s cut them, %d of %d bases' % (SPEC, rep['bases_out'], rep['bases_in']))
    rc, text = run(capsys, ['-i', inp, '--fingerprint', '--trim', SPEC])
    assert rc == 0 and text.count('\n') == 1 and not os.path.exists(inp + '.uQ')
    a = json.loads(text)
    assert a == json.loads(run(capsys, ['-i', out, '--decode', '--fingerprint'])[1])
    import fingerprint_ref as F
    assert a == json.loads(ops.fingerprint_json(F.fingerprint(want)))
    assert a['bases'] == rep['bases_out'] and a['reads'] == rep['reads_in']
    rc, text = run(capsys, ['-i', inp, '--qc', '--trim', SPEC])
    assert rc == 0 and text.count('\n') == 1
    assert json.loads(text) == json.loads(ops.qc_json(ops.qc_host(want)))
    assert json.loads(text) == json.loads(run(capsys, ['-i', out, '--decode', '--qc'])[1])
    # trim, then filter, then the tables
    rc, text = run(capsys, ['-i', inp, '--qc', '--trim', HARD, '--filter', 'min-len=1'])
    assert rc == 0 and json.loads(text) == json.loads(ops.qc_json(ops.qc_host(filter_ref.filtered(R.trimmed(fq, rectrim.parse(HARD)), filter_ref.criteria(min_len=1)))))


def test_bin_qual_bins_what_the_trim_left(ctx, capsys, tmp_path):
    """The trim runs first, on the qualities as given; the binning sees the reads that are left."""
    import binqual_ref
    from uq_amd import binqual
    fq, want, rep = reference('bench_var_36_301')
    binned, changed = binqual_ref.apply(want, binqual.parse('4level'))
    (tmp_path / 'in.fastq').write_bytes(fq)
    out = str(tmp_path / 'o.uQ')
    rc, text = run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', out, '--trim', SPEC, '--bin-qual', '4level', '--quiet', '--verify'])
    assert rc == 0 and text.startswith('Verified: '), text
    assert '; gives back the reads as --trim %s cut them, %d of %d bases; qualities binned by --bin-qual 4level, %d characters changed' % (
        SPEC, rep['bases_out'], rep['bases_in'], changed) in text
    cfg = json.loads(members_of(out)['config.json'])
    assert cfg['trim']['report'] == rep and cfg['quality_binning']['changed'] == changed
    assert decoded(ctx, out) == binned


def test_test_with_the_device_compressor(ctx, capsys, tmp_path):
    fq, want, rep = reference('bench_var_36_301')
    (tmp_path / 'in.fastq').write_bytes(fq)
    (tmp_path / 'trimmed.fastq').write_bytes(want)
    a, b = str(tmp_path / 'a.uQ'), str(tmp_path / 'b.uQ')
    flags = ['--test', '--device-compressor', '--quiet']
    assert run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', a, '--trim', SPEC] + flags)[0] == 0
    assert run(capsys, ['-i', str(tmp_path / 'trimmed.fastq'), '-o', b] + flags)[0] == 0
    same_container(members_of(a), members_of(b), {'trim': trim_value(rep)})


@pytest.mark.parametrize('kind', ['plain', 'gzip', 'filter'])
def test_the_untrimmed_text_is_freed_before_the_next_step(ctx, tmp_path, kind):
    """When the step after the trim starts (the filter, or the queued census and pack), the session holds the trimmed text and its index, not
    the 6.8 MB it read: the loaders keep no name of the untrimmed buffer."""
    from uq_amd import synth
    fq = synth.fastq(20261020, 20000, 150)
    inp = tmp_path / ('in.fastq.gz' if kind == 'gzip' else 'in.fastq')
    inp.write_bytes(gzip.compress(fq, 1) if kind == 'gzip' else fq)
    flags = ['--filter', 'min-len=1'] if kind == 'filter' else []
    args = uq.validate_args(uq.build_parser().parse_args(['-i', str(inp), '-o', str(tmp_path / 'o.uQ'), '--quiet', '--trim', 'crop=10'] + flags))
    s = uq.Session(args, ctx=ctx)
    t = ctx.torch
    seen = []
    name = 'filter_records' if kind == 'filter' else '_load_queued'
    inner = getattr(s, name)

    def spy(census):
        t.cuda.synchronize()
        seen.append(t.cuda.memory_allocated() - base)
        return inner(census)
    setattr(s, name, spy)
    t.cuda.synchronize()
    base = t.cuda.memory_allocated()
    s.load_input()
    assert len(seen) == 1 and s.trimming['report']['reads_in'] == 20000 and s.trimming['report']['bases_out'] == 200000
    assert s.d_buf.numel() == s.trimming['report']['bytes_out'] < len(fq) // 4
    assert seen[0] < len(fq) // 2, 'the untrimmed text (%d bytes) is still allocated when the next step starts: %d bytes' % (len(fq), seen[0])


def test_no_flag_no_change(ctx, capsys, tmp_path):
    fq = golden('qn_illumina_comment')
    (tmp_path / 'in.fastq').write_bytes(fq)
    out = str(tmp_path / 'o.uQ')
    assert run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', out, '--quiet'])[0] == 0
    assert 'trim' not in json.loads(members_of(out)['config.json'])
    assert decoded(ctx, out) == fq


# ------------------------------------------------------------------ refusals
def test_refusals(ctx, capsys, tmp_path):
    fq = golden('qn_illumina_comment')
    inp, out = str(tmp_path / 'in.fastq'), str(tmp_path / 'o.uQ')
    (tmp_path / 'in.fastq').write_bytes(fq)
    assert run(capsys, ['-i', inp, '-o', out, '--quiet'])[0] == 0
    rc, text = run(capsys, ['-i', out, '--decode', '--trim', 'q3=20'])
    assert rc == 1 and text.startswith('ERROR: --trim') and '--decode' in text
    os.remove(out)
    for spec, words in (('q3=x', "'q3=x'"), ('q33=3', 'unknown key'), ('q3=94', 'outside'), ('crop=0', 'outside'), ('head=0', 'no step'),
                        ('q3=1,q3=2', 'twice')):
        rc, text = run(capsys, ['-i', inp, '-o', out, '--trim', spec])
        assert rc == 1 and text.startswith('ERROR: --trim') and words in text and repr(spec) in text, text
        assert not os.path.exists(out)
    # reads left without bases: refused before anything is written, unless --filter drops them
    emptied = R.run(fq, rectrim.parse(HARD))[3]['emptied']
    assert emptied > 100
    message = 'ERROR: --trim %s leaves %d reads without bases; add --filter min-len=1 (or higher)' % (HARD, emptied)
    for flags in ([], ['--fingerprint'], ['--qc'], ['--peek'], ['--filter', 'max-n=5'], ['--filter', 'min-len=0']):
        with_out = [] if flags in (['--fingerprint'], ['--qc']) else ['-o', out]
        rc, text = run(capsys, ['-i', inp, '--trim', HARD] + flags + with_out)
        assert rc == 1 and text.strip().split('\n')[-1] == message, text
        assert not os.path.exists(out) and not os.path.exists(inp + '.uQ')
    rc, text = run(capsys, ['-i', inp, '-o', out, '--trim', HARD, '--filter', 'min-len=1', '--quiet'])
    assert rc == 0 and os.path.exists(out)
    assert decoded(ctx, out) == filter_ref.filtered(R.trimmed(fq, rectrim.parse(HARD)), filter_ref.criteria(min_len=1))
    os.remove(out)
    from uq_amd import dist_encode
    capsys.readouterr()
    assert dist_encode.main(['-i', inp, '-o', out, '--trim', 'q3=20']) == 1
    assert capsys.readouterr().out.startswith('ERROR: --trim') and not os.path.exists(out)
