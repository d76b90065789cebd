"""GPU: `--dedup` through the command line's main(argv): the container it writes is, member for member, the container of a plain encode of
the text deduplicated in Python (tests/dedup_ref.py) -- config.json gains `dedup` and nothing else; `--decode` gives the deduplicated text
back; pairs stay pairs; the flags that read the text in HBM (--verify, --fingerprint, --qc, --test, --sort, --bin-qual) see the deduplicated
text; the chain --trim, --adapter, --filter, --dedup, --bin-qual against the same chain in Python; every refusal with its message.

The golden inputs get their duplicates here: every seventh record takes the sequence and quality lines of an earlier record and keeps its own
name.  Each input is shown to have no hash collision at seed 0 under the Python reference before anything is compared."""
import gzip
import io
import json
import os
import random
import tarfile

import pytest

import dedup_ref as R
from uq_amd import bgzf_host, ops, recdedup, uq

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SPEC = 'by=seq'
READS = 1000                          # records of a golden input that are taken (the reference hashes in Python integers)


def golden(name):
    plain = os.path.join(GOLD, name + '.fastq')
    if os.path.exists(plain): return open(plain, 'rb').read()
    return gzip.decompress(open(plain + '.gz', 'rb').read())


def with_duplicates(text, unit=1, every=7, seed=17, better=False, limit=READS):
    """Every `every`-th unit repeats the sequence and quality lines of an earlier unit under its own names; better: the copy's qualities are
    raised to the line's highest, so that keep=best prefers the later read."""
    rnd = random.Random(seed)
    recs = R.records(text)[:limit - limit % unit]
    for w in range(1, len(recs) // unit):
        if w % every: continue
        src = rnd.randrange(w)
        for m in range(unit):
            qn, _, plus, _ = recs[w * unit + m]
            _, s, _, u = recs[src * unit + m]
            if better and u: u = bytes([max(u)]) * len(u)
            recs[w * unit + m] = [qn, s, plus, u]
    return b''.join(b'\n'.join(r) + b'\n' for r in recs)


_REF = {}


def reference(name, spec=SPEC, unit=1, better=False):
    """(input text, the text deduplicated in Python, its report), once per input and spec; no collision at seed 0."""
    key = (name, spec, unit, better)
    if key not in _REF:
        fq = with_duplicates(golden(name), unit, better=better)
        c = recdedup.parse(spec)
        best = bool(c['flags'] & R.BEST)
        _, v, rep = R.rule(fq, unit, c['prefix'], best)
        assert rep['collisions'] == 0 and v == R.plain(fq, unit, c['prefix'], best)
        _REF[key] = (fq, R.kept_text(fq, v, unit), rep)
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
    """a: written with --dedup (and the flags whose keys `want` holds); b: a plain encode of the text they leave."""
    assert sorted(a) == sorted(b)
    for k in a:
        if k != 'config.json': assert a[k] == b[k], k
    ca, cb = json.loads(a['config.json']), json.loads(b['config.json'])
    for key, value in want.items():
        assert key not in cb
        assert ca.pop(key) == value
    assert ca == cb
    assert json.dumps(ca, indent=4, sort_keys=True).encode() == b['config.json']


def dedup_value(rep, spec=SPEC, unit=1):
    return {'spec': spec, 'criteria': recdedup.explicit(spec), 'unit': unit, 'seed': 0, 'report': rep}


CASES = [('bench_var_36_301', 'plain', [], SPEC), ('bench_var_36_301', 'bgzf', [], SPEC), ('bench_var_36_301', 'gzip', [], 'keep=best'),
         ('bench_var_36_301', 'gzip', ['--host-inflate'], SPEC), ('bench_var_36_301', 'plain', ['--multi-pass'], 'prefix=50,keep=best'),
         ('bench_150bp_raw', 'plain', ['--gz'], SPEC)]


@pytest.mark.parametrize('name,kind,flags,spec', CASES, ids=['%s-%s%s-%s' % (n, k, ''.join(f), s) for n, k, f, s in CASES])
def test_container_equals_a_plain_encode_of_the_deduplicated_text(ctx, capsys, tmp_path, name, kind, flags, spec):
    fq, want, rep = reference(name, spec, better='best' in spec)
    assert rep['dup_reads'] > 100 and rep['reads_in'] - rep['dup_reads'] == len(R.records(want)) and rep['classes'] == rep['units_in'] - rep['dup_units']
    if 'best' in spec: assert want != reference(name, spec.replace('best', 'first'), better=True)[1]
    ext = '.uQ.gz' if '--gz' in flags else '.uQ'
    inp = tmp_path / ('in.fastq' if kind == 'plain' else 'in.fastq.gz')
    inp.write_bytes(fq if kind == 'plain' else (bgzf_host.compress(fq) if kind == 'bgzf' else gzip.compress(fq)))
    (tmp_path / 'left.fastq').write_bytes(want)
    a, b = str(tmp_path / ('a' + ext)), str(tmp_path / ('b' + ext))
    rc, text = run(capsys, ['-i', str(inp), '-o', a, '--dedup', spec] + flags)
    assert rc == 0, text
    assert recdedup.report_line(rep) in text
    assert 'dedup: kept %d of %d reads (%.2f %% duplicates), %d distinct sequences' % (
        rep['reads_in'] - rep['dup_reads'], rep['reads_in'], 100.0 * rep['dup_reads'] / rep['reads_in'], rep['classes']) in text
    rc, text = run(capsys, ['-i', str(tmp_path / 'left.fastq'), '-o', b, '--quiet'] + [f for f in flags if f != '--host-inflate'])
    assert rc == 0, text
    same_container(members_of(a), members_of(b), {'dedup': dedup_value(rep, spec)})
    assert decoded(ctx, a) == want
    rc, text = run(capsys, ['-i', a, '--decode'])
    assert rc == 0 and text.encode() == want


def test_quiet_and_peek(ctx, capsys, tmp_path):
    fq, want, rep = reference('bench_var_36_301')
    (tmp_path / 'in.fastq').write_bytes(fq)
    inp = str(tmp_path / 'in.fastq')
    rc, text = run(capsys, ['-i', inp, '--dedup', ' keep = first ', '--peek'])
    assert rc == 0 and recdedup.report_line(rep) in text and not os.path.exists(inp + '.uQ')
    shown = json.loads(text[text.index('The config.json would look like:') + len('The config.json would look like:'):])
    assert shown['dedup'] == dedup_value(rep, ' keep = first ') and shown['reads'] == rep['reads_in'] - rep['dup_reads']
    rc, text = run(capsys, ['-i', inp, '-o', str(tmp_path / 'q.uQ'), '--dedup', SPEC, '--quiet'])
    assert rc == 0 and text == ''
    assert decoded(ctx, str(tmp_path / 'q.uQ')) == want


# ------------------------------------------------------------------ pairs
def mates(n=400, seed=43):
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


def test_pairs_are_dropped_whole(ctx, capsys, tmp_path):
    r1, r2 = mates()
    recs = R.records(with_duplicates(interleave(r1, r2), unit=2, every=5))
    for w in range(3, 400, 10):                                  # ... and pairs where only the first mate repeats an earlier one: not duplicates
        recs[2 * w][1], recs[2 * w][3] = recs[0][1], recs[0][3]
    both = b''.join(b'\n'.join(r) + b'\n' for r in recs)
    r1, r2 = (b''.join(b'\n'.join(r) + b'\n' for r in recs[m::2]) for m in (0, 1))
    _, v, rep = R.rule(both, 2)
    want = R.kept_text(both, v, 2)
    assert rep['collisions'] == 0 and v == R.plain(both, 2) and 60 < rep['dup_units'] < 90 and rep['dup_reads'] == 2 * rep['dup_units']
    assert R.rule(both, 1)[2]['dup_units'] > rep['dup_reads'] + 30
    for name, data in (('r1.fastq', r1), ('r2.fastq', r2), ('both.fastq', both), ('left.fastq', want)): (tmp_path / name).write_bytes(data)
    p = lambda name: str(tmp_path / name)
    a, b, k = p('a.uQ'), p('b.uQ'), p('k.uQ')
    rc, text = run(capsys, ['-i', p('r1.fastq'), '--mate2', p('r2.fastq'), '-o', a, '--dedup', SPEC])
    assert rc == 0 and recdedup.report_line(rep) in text, text
    assert run(capsys, ['-i', p('both.fastq'), '--interleaved', '-o', b, '--dedup', SPEC, '--quiet'])[0] == 0
    assert run(capsys, ['-i', p('left.fastq'), '--interleaved', '-o', k, '--quiet'])[0] == 0
    ma, mb, mk = members_of(a), members_of(b), members_of(k)
    assert ma == mb
    same_container(ma, mk, {'dedup': dedup_value(rep, unit=2)})
    assert json.loads(ma['config.json'])['paired'] == {'layout': 'interleaved', 'pairs': (rep['reads_in'] - rep['dup_reads']) // 2, 'slash_pairs': 0}
    assert decoded(ctx, a) == want
    o1, o2 = p('o1.fastq'), p('o2.fastq')
    rc, text = run(capsys, ['-i', a, '--decode', '--split-mates', o1, o2])
    assert rc == 0, text
    left = R.records(want)
    assert open(o1, 'rb').read() == b''.join(b'\n'.join(r) + b'\n' for r in left[0::2])
    assert open(o2, 'rb').read() == b''.join(b'\n'.join(r) + b'\n' for r in left[1::2])
    # mates that do not match are refused on the input as given, with the message of a paired encode without --dedup
    bad = r2.replace(b'@A00:7:HX:2:1000:2003 2', b'@A00:7:HX:2:1000:2004 2', 1)
    (tmp_path / 'bad.fastq').write_bytes(bad)
    (tmp_path / 'badboth.fastq').write_bytes(interleave(r1, bad))
    plain = run(capsys, ['-i', p('r1.fastq'), '--mate2', p('bad.fastq'), '-o', p('x.uQ'), '--quiet'])
    assert plain[0] == 1 and plain[1].startswith('ERROR: pair 1: ')
    assert run(capsys, ['-i', p('r1.fastq'), '--mate2', p('bad.fastq'), '-o', p('x.uQ'), '--quiet', '--dedup', SPEC]) == plain
    assert run(capsys, ['-i', p('badboth.fastq'), '--interleaved', '-o', p('x.uQ'), '--quiet', '--dedup', SPEC]) == plain
    (tmp_path / 'odd.fastq').write_bytes(both + b'\n'.join(recs[0]) + b'\n')
    rc, text = run(capsys, ['-i', p('odd.fastq'), '--interleaved', '-o', p('x.uQ'), '--quiet', '--dedup', SPEC])
    assert rc == 1 and text.startswith('ERROR: --interleaved: the input holds 801 reads, an odd number') and not os.path.exists(p('x.uQ'))


# ------------------------------------------------------------------ the chain
def test_trim_adapter_filter_dedup_bin_qual(ctx, capsys, tmp_path):
    """Duplicates are judged on the reads as trimmed, cut and filtered; the binning sees what is left."""
    import adapter_inputs as AI
    import adapter_ref as AR
    import binqual_ref
    import filter_ref
    import trim_ref as TR
    from uq_amd import adapters, binqual, recfilter, rectrim
    fq = AI.implant_text(with_duplicates(golden('bench_var_36_301'), limit=1200), AI.ILLUMINA, limit=1200)
    recs = TR.records(fq)
    for i in range(0, len(recs), 11):                            # reads that differ only in what --trim head=3 removes: duplicates once trimmed
        qn, s, p, u = recs[i]
        s0 = recs[(i + 5) % len(recs)][1]
        if len(s0) > 3: recs[i] = (qn, b'TTT'[:3] + s0[3:], p, (u * 9)[:len(s0)])
    fq = b''.join(b'\n'.join(r) + b'\n' for r in recs)
    tspec, aspec, fspec, dspec, bspec = 'head=3,q3=15', 'seq=illumina', 'min-len=30', 'keep=best', '4level'
    ac = adapters.parse(aspec)
    twins, _, _, trep = TR.run(fq, rectrim.parse(tspec))
    wins, arep, dst, cut = AR.run(fq, AR.params(ac['seq'], ac['seq2'], ac['err'], ac['overlap'], 0), windows=twins)
    left, frep = filter_ref.run(cut, recfilter.parse(fspec))[3:]
    _, v, drep = R.rule(left, best=True)
    assert drep['collisions'] == 0 and v == R.plain(left, best=True)
    kept = R.kept_text(left, v)
    want, changed = binqual_ref.apply(kept, binqual.parse(bspec))
    assert drep['dup_reads'] > 60 and drep['dup_reads'] > 30 + R.rule(fq, best=True)[2]['dup_reads'] and 0 < frep['reads_out'] < frep['reads_in']
    (tmp_path / 'in.fastq').write_bytes(fq)
    (tmp_path / 'left.fastq').write_bytes(want)
    inp, a, b = str(tmp_path / 'in.fastq'), str(tmp_path / 'a.uQ'), str(tmp_path / 'b.uQ')
    chain = ['--trim', tspec, '--adapter', aspec, '--filter', fspec, '--dedup', dspec, '--bin-qual', bspec]
    rc, text = run(capsys, ['-i', inp, '-o', a] + chain)
    assert rc == 0 and recfilter.report_line(frep) in text and recdedup.report_line(drep) in text, text
    assert text.index('trim: ') < text.index('adapter: ') < text.index('filter: ') < text.index('dedup: ')
    assert run(capsys, ['-i', str(tmp_path / 'left.fastq'), '-o', b, '--quiet'])[0] == 0
    ca = json.loads(members_of(a)['config.json'])
    assert ca['dedup'] == dedup_value(drep, dspec) and ca['filter']['report'] == frep and ca['trim']['report'] == trep and ca['adapter']['report'] == arep
    assert ca['quality_binning']['changed'] == changed
    ma, mb = members_of(a), members_of(b)
    assert sorted(ma) == sorted(mb) and all(ma[k] == mb[k] for k in ma if k != 'config.json')
    assert decoded(ctx, a) == want
    rc, text = run(capsys, ['-i', inp, '-o', a, '--quiet', '--verify'] + chain)
    assert rc == 0 and text.startswith('Verified: '), text
    assert '; gives back the %d reads --filter kept of %d; gives back the %d reads --dedup kept of %d; qualities binned by --bin-qual 4level' % (
        frep['reads_out'], frep['reads_in'], drep['reads_in'] - drep['dup_reads'], drep['reads_in']) in text


# ------------------------------------------------------------------ with the other flags
def test_verify_fingerprint_and_qc_see_the_deduplicated_text(ctx, capsys, tmp_path):
    fq, want, rep = reference('bench_150bp_raw')
    inp, out = str(tmp_path / 'in.fastq'), str(tmp_path / 'o.uQ')
    (tmp_path / 'in.fastq').write_bytes(fq)
    rc, text = run(capsys, ['-i', inp, '-o', out, '--dedup', SPEC, '--quiet', '--verify'])
    assert rc == 0, text
    lines = text.strip().split('\n')
    assert len(lines) == 1 and lines[0].startswith('Verified: ') and 'in the same order' in lines[0]
    kept = rep['reads_in'] - rep['dup_reads']
    assert '%s decodes to the same %d reads' % (out, kept) in lines[0]
    assert lines[0].endswith('; gives back the %d reads --dedup kept of %d' % (kept, rep['reads_in']))
    rc, text = run(capsys, ['-i', inp, '--fingerprint', '--dedup', SPEC])
    assert rc == 0 and text.count('\n') == 1 and not os.path.exists(inp + '.uQ')
    a = json.loads(text)
    assert a == json.loads(run(capsys, ['-i', out, '--decode', '--fingerprint'])[1])
    import fingerprint_ref as F
    assert a == json.loads(ops.fingerprint_json(F.fingerprint(want)))
    rc, text = run(capsys, ['-i', inp, '--qc', '--dedup', SPEC])
    assert rc == 0 and text.count('\n') == 1
    assert json.loads(text) == json.loads(ops.qc_json(ops.qc_host(want)))
    assert json.loads(text) == json.loads(run(capsys, ['-i', out, '--decode', '--qc'])[1])


def test_sort_dna(ctx, capsys, tmp_path):
    fq, want, rep = reference('bench_150bp_raw')
    (tmp_path / 'in.fastq').write_bytes(fq)
    (tmp_path / 'left.fastq').write_bytes(want)
    a, b = str(tmp_path / 'a.uQ'), str(tmp_path / 'b.uQ')
    rc, text = run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', a, '--dedup', SPEC, '--sort', 'DNA', '--quiet', '--verify'])
    assert rc == 0 and text.startswith('Verified: ') and 'as a multiset' in text, text
    assert run(capsys, ['-i', str(tmp_path / 'left.fastq'), '-o', b, '--sort', 'DNA', '--quiet'])[0] == 0
    same_container(members_of(a), members_of(b), {'dedup': dedup_value(rep)})
    got = R.records(decoded(ctx, a))
    assert sorted(got) == sorted(R.records(want)) and len({r[1] for r in got}) == len(got) == rep['classes']


def test_test_with_the_device_compressor(ctx, capsys, tmp_path):
    fq, want, rep = reference('bench_var_36_301')
    (tmp_path / 'in.fastq').write_bytes(fq)
    (tmp_path / 'left.fastq').write_bytes(want)
    a, b = str(tmp_path / 'a.uQ'), str(tmp_path / 'b.uQ')
    flags = ['--test', '--device-compressor', '--quiet']
    assert run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', a, '--dedup', SPEC] + flags)[0] == 0
    assert run(capsys, ['-i', str(tmp_path / 'left.fastq'), '-o', b] + flags)[0] == 0
    same_container(members_of(a), members_of(b), {'dedup': dedup_value(rep)})


def test_no_flag_no_change(ctx, capsys, tmp_path):
    fq = with_duplicates(golden('qn_illumina_comment'))
    (tmp_path / 'in.fastq').write_bytes(fq)
    out = str(tmp_path / 'o.uQ')
    assert run(capsys, ['-i', str(tmp_path / 'in.fastq'), '-o', out, '--quiet'])[0] == 0
    assert 'dedup' not in json.loads(members_of(out)['config.json'])
    assert decoded(ctx, out) == fq


# ------------------------------------------------------------------ refusals
def test_refusals(ctx, capsys, tmp_path):
    fq = golden('qn_illumina_comment')
    inp, out = str(tmp_path / 'in.fastq'), str(tmp_path / 'o.uQ')
    (tmp_path / 'in.fastq').write_bytes(fq)
    assert run(capsys, ['-i', inp, '-o', out, '--quiet'])[0] == 0
    rc, text = run(capsys, ['-i', out, '--decode', '--dedup', SPEC])
    assert rc == 1 and text.startswith('ERROR: --dedup') and '--decode' in text
    os.remove(out)
    for spec, words in (('prefix=x', "'prefix=x'"), ('prefx=3', 'unknown key'), ('by=name', 'only value'), ('keep=last', 'neither'),
                        ('by=seq,by=seq', 'twice'), ('prefix=4294967296', 'outside'), ('by', 'key=value')):
        rc, text = run(capsys, ['-i', inp, '-o', out, '--dedup', spec])
        assert rc == 1 and text.startswith('ERROR: --dedup') and words in text and repr(spec) in text, text
        assert not os.path.exists(out)
    rc, text = run(capsys, ['-i', inp, '-o', out, '--dedup', ''])
    assert rc == 1 and text.startswith('ERROR: --dedup: the specification is empty') and not os.path.exists(out)
    from uq_amd import dist_encode
    capsys.readouterr()
    assert dist_encode.main(['-i', inp, '-o', out, '--dedup', SPEC]) == 1
    assert capsys.readouterr().out.startswith('ERROR: --dedup is for the single-GPU tool') and not os.path.exists(out)
