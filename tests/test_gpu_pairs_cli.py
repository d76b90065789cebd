"""GPU: paired-end input through the command line's main(argv).  The container `-i R1 --mate2 R2` (or `--interleaved`) writes is, member for
member, the plain encode of the text interleaved in Python (tests/pairs_ref.py) -- config.json gains `paired` and nothing else; `--decode`
prints the interleaved text, `--decode --split-mates` gives R1 and R2 back byte for byte; the refusals, each with its message, exit
status 1 and no output file."""
import gzip
import io
import json
import os
import random
import tarfile

import pytest

import binqual_ref
import pairs_ref as R
from uq_amd import bgzf_host, binqual, uq

pytestmark = pytest.mark.gpu

N = 300


def mates(n=N, seed=41, name=lambda i, m: b'@A00:7:HX:%d:%d:%d %d:N:0:ACGT' % (1 + i % 4, 1000 + i // 7, 2000 + 3 * i, m), lengths=(36, 151)):
    rnd = random.Random(seed)
    out = []
    for m in (1, 2):
        recs = []
        for i in range(n):
            L = rnd.randint(*lengths)
            recs.append(b'\n'.join((name(i, m), bytes(rnd.choice(b'ACGT') for _ in range(L)), b'+', bytes(rnd.randint(35, 73) for _ in range(L)))) + b'\n')
        out.append(b''.join(recs))
    return out


R1, R2 = mates()
BOTH = R.interleave(R1, R2)
PAIRED = {'layout': 'interleaved', 'pairs': N, 'slash_pairs': 0}


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


def same_container(a, b, paired):
    """a: a paired encode; b: the plain encode of the interleaved text."""
    assert sorted(a) == sorted(b)
    for k in a:
        if k != 'config.json': assert a[k] == b[k], k
    ca, cb = json.loads(a['config.json']), json.loads(b['config.json'])
    assert 'paired' not in cb
    assert ca.pop('paired') == paired
    assert ca == cb
    assert json.dumps(ca, indent=4, sort_keys=True).encode() == b['config.json']


def write(tmp_path, **files):
    paths = {}
    for k, v in files.items():
        p = tmp_path / k.replace('_', '.')
        p.write_bytes(v)
        paths[k] = str(p)
    return paths


@pytest.fixture(scope='module')
def plain_container(ctx, tmp_path_factory):
    """The plain encode of the interleaved text, once: (members with default flags, members with every table raw)."""
    d = tmp_path_factory.mktemp('plain')
    (d / 'both.fastq').write_bytes(BOTH)
    assert uq.main(['-i', str(d / 'both.fastq'), '-o', str(d / 'k.uQ'), '--quiet']) == 0
    assert uq.main(['-i', str(d / 'both.fastq'), '-o', str(d / 'r.uQ'), '--quiet', '--raw', 'DNA', 'QUAL', 'QNAME']) == 0
    return members_of(str(d / 'k.uQ')), members_of(str(d / 'r.uQ'))


@pytest.mark.parametrize('flags', [[], ['--raw', 'DNA', 'QUAL', 'QNAME']], ids=['keyed', 'raw'])
def test_two_files_give_the_plain_encode_of_the_interleaved_text(ctx, capsys, tmp_path, plain_container, flags):
    p = write(tmp_path, r1_fastq=R1, r2_fastq=R2)
    rc, text = run(capsys, ['-i', p['r1_fastq'], '--mate2', p['r2_fastq'], '--quiet'] + flags)
    assert rc == 0, text
    out = p['r1_fastq'] + '.uQ'                                      # the default name: the -i name + .uQ
    same_container(members_of(out), plain_container[1 if flags else 0], PAIRED)
    assert decoded(ctx, out) == BOTH
    rc, text = run(capsys, ['-i', out, '--decode'])
    assert rc == 0 and text.encode() == BOTH


def test_bgzf_r1_and_gzip_r2(ctx, capsys, tmp_path, plain_container):
    p = write(tmp_path, r1_fastq_gz=bgzf_host.compress(R1), r2_fastq_gz=gzip.compress(R2))
    out = str(tmp_path / 'o.uQ')
    rc, text = run(capsys, ['-i', p['r1_fastq_gz'], '--mate2', p['r2_fastq_gz'], '-o', out, '--quiet'])
    assert rc == 0, text
    same_container(members_of(out), plain_container[0], PAIRED)
    rc, text = run(capsys, ['-i', p['r1_fastq_gz'], '--mate2', p['r2_fastq_gz'], '-o', out, '--quiet', '--host-inflate'])
    assert rc == 0, text
    same_container(members_of(out), plain_container[0], PAIRED)


def test_interleaved_gives_the_same_container(ctx, capsys, tmp_path, plain_container):
    p = write(tmp_path, both_fastq=BOTH, r1_fastq=R1, r2_fastq=R2)
    a, b = str(tmp_path / 'a.uQ'), str(tmp_path / 'b.uQ')
    assert run(capsys, ['-i', p['both_fastq'], '--interleaved', '-o', a, '--quiet'])[0] == 0
    assert run(capsys, ['-i', p['r1_fastq'], '--mate2', p['r2_fastq'], '-o', b, '--quiet'])[0] == 0
    assert members_of(a) == members_of(b)
    same_container(members_of(a), plain_container[0], PAIRED)
    rc, text = run(capsys, ['-i', p['both_fastq'], '--interleaved', '--peek'])
    assert rc == 0 and json.loads(text[text.index('The config.json would look like:') + len('The config.json would look like:'):])['paired'] == PAIRED


def slash_mates():
    return mates(120, 43, name=lambda i, m: b'@run9.%d/%d' % (i + 1, m), lengths=(20, 60))


def test_slash_names_are_counted(ctx, capsys, tmp_path):
    a, b = slash_mates()
    p = write(tmp_path, r1_fastq=a, r2_fastq=b)
    out = str(tmp_path / 'o.uQ')
    assert run(capsys, ['-i', p['r1_fastq'], '--mate2', p['r2_fastq'], '-o', out, '--quiet'])[0] == 0
    assert json.loads(members_of(out)['config.json'])['paired'] == {'layout': 'interleaved', 'pairs': 120, 'slash_pairs': 120}
    assert decoded(ctx, out) == R.interleave(a, b)


def split(capsys, tmp_path, container, *flags):
    o1, o2 = str(tmp_path / 'out1'), str(tmp_path / 'out2')
    for o in (o1, o2):
        if os.path.exists(o): os.remove(o)
    rc, text = run(capsys, ['-i', container, '--decode', '--split-mates', o1, o2] + list(flags))
    assert rc == 0 and text == '', text
    return open(o1, 'rb').read(), open(o2, 'rb').read()


@pytest.mark.parametrize('flags', [[], ['--raw', 'DNA', 'QUAL', 'QNAME'], ['--raw', 'QUAL'], ['--gz']], ids=['keyed', 'raw', 'raw-qual', 'gz'])
def test_split_mates_gives_both_files_back(ctx, capsys, tmp_path, flags):
    p = write(tmp_path, r1_fastq=R1, r2_fastq=R2)
    out = str(tmp_path / ('o.uQ.gz' if '--gz' in flags else 'o.uQ'))
    assert run(capsys, ['-i', p['r1_fastq'], '--mate2', p['r2_fastq'], '-o', out, '--quiet'] + flags)[0] == 0
    names = set(members_of(out))
    assert ('DNA.raw' in names) == ('DNA' in flags) and ('QUAL.raw' in names) == ('QUAL' in flags) and ('QUAL.key' in names) == ('QUAL' not in flags)
    assert split(capsys, tmp_path, out) == (R1, R2)
    if '--gz' in flags: return
    assert split(capsys, tmp_path, out, '--two-pass-decode') == (R1, R2)
    z1, z2 = split(capsys, tmp_path, out, '--bgzf')
    assert z1[:4] == b'\x1f\x8b\x08\x04' and (gzip.decompress(z1), gzip.decompress(z2)) == (R1, R2)
    if not flags:
        z1, z2 = split(capsys, tmp_path, out, '--bgzf', '--bgzf-level', '2')
        assert (gzip.decompress(z1), gzip.decompress(z2)) == (R1, R2)


def test_split_mates_where_the_host_writes_the_names(ctx, capsys, tmp_path):
    """A 20-digit field next to a field with an offset (golden qn_u8_offset_negative): device_text_possible is False."""
    a, b = mates(200, 44, name=lambda i, m: b'@s:%d:%d' % (-25 + 50000 * i * i + 7 * i, (1 + i % 2) * 10 ** 19 + 12345 * i), lengths=(24, 24))
    p = write(tmp_path, r1_fastq=a, r2_fastq=b)
    out = str(tmp_path / 'o.uQ')
    assert run(capsys, ['-i', p['r1_fastq'], '--mate2', p['r2_fastq'], '-o', out, '--quiet', '--raw', 'DNA', 'QUAL', 'QNAME'])[0] == 0
    cfg = json.loads(members_of(out)['config.json'])
    assert cfg['paired']['pairs'] == 200 and not uq.Session.device_text_possible(cfg)
    assert decoded(ctx, out) == R.interleave(a, b)
    assert split(capsys, tmp_path, out) == (a, b)
    z1, z2 = split(capsys, tmp_path, out, '--bgzf')
    assert (gzip.decompress(z1), gzip.decompress(z2)) == (a, b)


def test_verify_fingerprint_qc_and_gz_see_the_interleaved_text(ctx, capsys, tmp_path, plain_container):
    p = write(tmp_path, r1_fastq=R1, r2_fastq=R2, both_fastq=BOTH)
    out = str(tmp_path / 'o.uQ.gz')
    rc, text = run(capsys, ['-i', p['r1_fastq'], '--mate2', p['r2_fastq'], '-o', out, '--quiet', '--verify', '--gz'])
    assert rc == 0, text
    lines = text.strip().split('\n')
    assert len(lines) == 1 and lines[0].startswith('Verified: ') and 'in the same order' in lines[0] and '%d pairs' % N in lines[0]
    same_container(members_of(out), plain_container[0], PAIRED)
    for flag in ('--fingerprint', '--qc'):
        rc, a = run(capsys, ['-i', p['r1_fastq'], '--mate2', p['r2_fastq'], flag])
        rc2, b = run(capsys, ['-i', p['both_fastq'], flag])
        rc3, c = run(capsys, ['-i', p['both_fastq'], '--interleaved', flag])
        assert rc == rc2 == rc3 == 0 and a == b == c and a.count('\n') == 1
    assert not os.path.exists(p['r1_fastq'] + '.uQ')
    rc, text = run(capsys, ['-i', p['r1_fastq'], '--mate2', p['r2_fastq'], '--test', '-o', str(tmp_path / 't.uQ'), '--quiet'])
    assert rc == 0 and decoded(ctx, str(tmp_path / 't.uQ')) == BOTH


def test_bin_qual_with_mate2(ctx, capsys, tmp_path):
    binned, changed = binqual_ref.apply(BOTH, binqual.parse('illumina8'))
    assert changed > 0
    p = write(tmp_path, r1_fastq=R1, r2_fastq=R2, binned_fastq=binned)
    a, b = str(tmp_path / 'a.uQ'), str(tmp_path / 'b.uQ')
    assert run(capsys, ['-i', p['r1_fastq'], '--mate2', p['r2_fastq'], '-o', a, '--quiet', '--bin-qual', 'illumina8'])[0] == 0
    assert run(capsys, ['-i', p['binned_fastq'], '-o', b, '--quiet'])[0] == 0
    ma, mb = members_of(a), members_of(b)
    ca = json.loads(ma['config.json'])
    assert ca.pop('quality_binning')['changed'] == changed
    ma['config.json'] = json.dumps(ca, indent=4, sort_keys=True).encode()
    same_container(ma, mb, PAIRED)
    assert decoded(ctx, a) == binned


# ------------------------------------------------------------------ refusals
def refused(capsys, tmp_path, argv, *words):
    before = sorted(os.listdir(str(tmp_path)))
    rc, text = run(capsys, argv)
    assert rc == 1 and text.startswith('ERROR: '), text
    for w in words: assert w in text, (w, text)
    assert sorted(os.listdir(str(tmp_path))) == before
    return text


def test_refusals(ctx, capsys, tmp_path, plain_container):
    recs = R.records(R2)
    k = 117
    renamed = b''.join(recs[:k]) + b'@somebody:else 2:N:0:ACGT' + recs[k][recs[k].index(b'\n'):] + b''.join(recs[k + 1:])
    renamed2 = b''.join(b'@x%d\n' % i + r[r.index(b'\n') + 1:] if i in (k, 200, 250) else r for i, r in enumerate(recs))
    p = write(tmp_path, r1_fastq=R1, r2_fastq=R2, renamed_fastq=renamed, renamed2_fastq=renamed2, short_fastq=b''.join(recs[:-1]),
              odd_fastq=b''.join(R.records(BOTH)[:-1]), bad_fastq=R.interleave(R1, renamed), both_fastq=BOTH)
    name1 = R.qname(R.records(R1)[k]).decode()
    text = refused(capsys, tmp_path, ['-i', p['r1_fastq'], '--mate2', p['renamed_fastq'], '--quiet'])
    assert text == 'ERROR: pair %d: %s and @somebody:else 2:N:0:ACGT are not mates (1 of %d pairs differ)\n' % (k, name1, N)
    text = refused(capsys, tmp_path, ['-i', p['r1_fastq'], '--mate2', p['renamed2_fastq'], '--quiet', '--gz'])
    assert text == 'ERROR: pair %d: %s and @x%d are not mates (3 of %d pairs differ)\n' % (k, name1, k, N)
    text = refused(capsys, tmp_path, ['-i', p['bad_fastq'], '--interleaved', '--quiet'])
    assert text == 'ERROR: pair %d: %s and @somebody:else 2:N:0:ACGT are not mates (1 of %d pairs differ)\n' % (k, name1, N)
    text = refused(capsys, tmp_path, ['-i', p['r1_fastq'], '--mate2', p['short_fastq'], '--quiet'])
    assert text == 'ERROR: R1 holds %d reads, R2 holds %d\n' % (N, N - 1)
    refused(capsys, tmp_path, ['-i', p['odd_fastq'], '--interleaved', '--quiet'], '--interleaved', '%d reads' % (2 * N - 1), 'odd')
    refused(capsys, tmp_path, ['-i', p['r1_fastq'], '--mate2', p['r2_fastq'], '--sort', 'DNA'], '--sort DNA', '--mate2')
    refused(capsys, tmp_path, ['-i', p['both_fastq'], '--interleaved', '--sort', 'DNA'], '--sort DNA', '--interleaved')
    refused(capsys, tmp_path, ['-i', p['r1_fastq'], '--mate2', p['r2_fastq'], '--interleaved'], '--mate2', '--interleaved')
    # --split-mates on a container without the key
    assert run(capsys, ['-i', p['both_fastq'], '-o', str(tmp_path / 'plain.uQ'), '--quiet'])[0] == 0
    refused(capsys, tmp_path, ['-i', str(tmp_path / 'plain.uQ'), '--decode', '--split-mates', str(tmp_path / 'o1'), str(tmp_path / 'o2')],
            '--split-mates', 'paired', '--interleaved')
    refused(capsys, tmp_path, ['-i', p['r1_fastq'], '--mate2', p['r2_fastq'], '--decode'], '--mate2', '--decode')


def test_slash_mates_the_wrong_way_round(ctx, capsys, tmp_path):
    a, b = slash_mates()
    p = write(tmp_path, r1_fastq=a, r2_fastq=b)
    text = refused(capsys, tmp_path, ['-i', p['r2_fastq'], '--mate2', p['r1_fastq'], '--quiet'])
    assert text == 'ERROR: pair 0: @run9.1/2 and @run9.1/1 are not mates (120 of 120 pairs differ)\n'


def test_the_sharded_tool_refuses_the_three_flags(capsys, tmp_path):
    from uq_amd import dist_encode
    p = write(tmp_path, r1_fastq=R1, r2_fastq=R2, both_fastq=BOTH)
    for argv, flag in ((['-i', p['r1_fastq'], '--mate2', p['r2_fastq']], '--mate2'), (['-i', p['both_fastq'], '--interleaved'], '--interleaved'),
                       (['-i', p['both_fastq'], '--decode', '--split-mates', str(tmp_path / 'a'), str(tmp_path / 'b')], '--split-mates')):
        before = sorted(os.listdir(str(tmp_path)))
        capsys.readouterr()
        assert dist_encode.main(argv) == 1
        out = capsys.readouterr().out
        assert out.startswith('ERROR: ' + flag) and 'python -m uq_amd.uq' in out
        assert sorted(os.listdir(str(tmp_path))) == before
