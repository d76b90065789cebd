#!/usr/bin/env python3
"""Times uq_requantise_qualities on the two benchmark geometries, generated on the device -- 10 M x 150 bp (BASELINE
configs[1]) and 36-301 bp with Ns (configs[4]), the inputs of tools/bench_fingerprint.py -- beside the kernel it must not be slower than:
uq_fingerprint_accumulate on the same input, which reads the whole stream where this one reads and writes the quality lines only.  The two
alternate in one process (device events, min and median of the rounds); the kernel is checked against the host twin on a prefix first.  The
table is `illumina8`; after the first round the qualities are binned already, which changes no byte that is moved (every quality byte is
read, looked up and written whatever its value).  Bytes touched = the quality bytes twice + 16 B of line starts per read.
Then the size effect on --size-reads reads x 150 bp of synth-v1, all tables raw: bits_per_quality, QUAL row bytes, .uQ and .uQ.gz bytes
with the flag off and with illumina8.

Every GPU step is a child process of its own under its own time limit; the first failure stops the run; at most 16 threads.
    python tools/bench_requant.py [reads] [--rounds R] [--size-reads N] [--no-size]     one JSON line per measurement"""
import json, os, statistics, subprocess, sys, tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
COPY_CEILING = 5.3e12                               # bytes / s: what a plain copy kernel reaches (tools/membench.hip)
STEP_LIMIT_S = {'kernel:150': 240, 'kernel:var': 240, 'size': 420}


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


pos = [a for i, a in enumerate(sys.argv[1:], 1) if a.isdigit() and not sys.argv[i - 1].startswith('--')]
n = int(pos[0]) if pos else 10_000_000
rounds, size_reads = opt('--rounds', 7), opt('--size-reads', 2_000_000)


def kernel_bench(label, spec):
    import numpy as np, torch
    from uq_amd import binqual, ops
    from uq_amd.device import Context
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ctx = Context(0)
    lut = binqual.parse('illumina8')

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    d_buf = ops.synth_fastq(ctx, spec, 0, n)
    nl = ops.count_lines(ctx, d_buf); ls = ops.index_lines(ctx, d_buf, nl)
    # the answer first: a prefix (a copy of it: the kernel works in place) against the sequential host twin
    k = min(n, 20000)
    end = int(ctx.to_numpy(ls[4 * k:4 * k + 1], np.uint64)[0])
    d_head = d_buf[:end].clone()
    head = ctx.to_numpy(d_head)
    d_c = ops.changed_new(ctx)
    ops.requantise_qualities(ctx, d_head, ls, 0, k, lut, d_c)
    want, c = ops.requantise_qualities_host(head, lut)
    assert np.array_equal(ctx.to_numpy(d_head), want) and int(ctx.to_numpy(d_c).view(np.uint64)[0]) == c, 'device binning != host twin'
    del d_head
    before = ops.fingerprint(ctx, d_buf, ls, n)
    d_changed, d_fp = ops.changed_new(ctx), ops.fingerprint_new(ctx)
    def rq(): ops.requantise_qualities(ctx, d_buf, ls, 0, n, lut, d_changed)
    def fp(): ops.fingerprint_accumulate(ctx, d_fp, d_buf, ls, 0, n)
    fp(); torch.cuda.synchronize()                  # (warm; the first requantise is a measured round: it is the one that changes bytes)
    t_rq, t_fp = [], []
    for _ in range(rounds):
        t_rq.append(timed(rq)); t_fp.append(timed(fp))
    after = ops.fingerprint(ctx, d_buf, ls, n)
    assert all(after[f] == before[f] for f in ('reads', 'bases', 'qname', 'dna')) and after['qual'] != before['qual'], 'binning touched another line'
    changed = int(ctx.to_numpy(d_changed).view(np.uint64)[0])
    qbytes = before['bases']                         # quality characters = bases
    touched = 2 * qbytes + 16 * n
    med_rq, med_fp = statistics.median(t_rq), statistics.median(t_fp)
    print(json.dumps({'bench': 'requant_kernel', 'input': label, 'reads': n, 'bytes': d_buf.numel(), 'quality_bytes': qbytes, 'bytes_touched': touched,
                      'rounds': rounds, 'requant_ms_min': round(min(t_rq), 3), 'requant_ms_median': round(med_rq, 3),
                      'fingerprint_ms_min': round(min(t_fp), 3), 'fingerprint_ms_median': round(med_fp, 3),
                      'requant_TBps': round(touched / (med_rq * 1e-3) / 1e12, 3), 'fraction_of_copy_ceiling_5.3TBps': round(touched / (med_rq * 1e-3) / COPY_CEILING, 3),
                      'no_slower_than_fingerprint': med_rq <= med_fp, 'changed': changed}), flush=True)
    ctx.close()


def size_bench():
    import numpy as np, torch
    from uq_amd import ops, synth, uq
    from uq_amd.device import Context
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ctx = Context(0)
    tmp = tempfile.mkdtemp(prefix='bench_rq_')
    path = os.path.join(tmp, 'reads.fastq')
    ctx.to_numpy(ops.synth_fastq(ctx, synth.Spec(20261005, 150), 0, size_reads)).tofile(path)
    ctx.close(); torch.cuda.empty_cache()
    try:
        for spec in (None, 'illumina8'):
            row = {'bench': 'requant_size', 'reads': size_reads, 'input_bytes': os.path.getsize(path), 'bin_qual': spec}
            for gz in (False, True):
                out = path + ('.uQ.gz' if gz else '.uQ')
                argv = ['-i', path, '-o', out, '--quiet', '--raw', 'DNA', 'QUAL', 'QNAME'] + (['--gz'] if gz else []) + (['--bin-qual', spec] if spec else [])
                assert uq.main(argv) == 0
                row['uQ_gz_bytes' if gz else 'uQ_bytes'] = os.path.getsize(out)
                if not gz:
                    import tarfile
                    with tarfile.open(out) as t:
                        cfg = json.loads(t.extractfile('config.json').read().decode())
                        qual = t.getmember('QUAL.raw').size
                    row['bits_per_quality'] = cfg['bits_per_quality']
                    row['qual_row_bytes'] = -(-cfg['bits_per_quality'] * (cfg['dna_max'] + (1 if cfg['variable_read_lengths'] else 0)) // 8)
                    row['QUAL_raw_member_bytes'] = qual
                    if spec: row['changed'] = cfg['quality_binning']['changed']
                os.remove(out)
            print(json.dumps(row), flush=True)
    finally:
        for f in os.listdir(tmp): os.remove(os.path.join(tmp, f))
        os.rmdir(tmp)


if '--step' in sys.argv:
    from uq_amd import synth
    step = sys.argv[sys.argv.index('--step') + 1]
    if step == 'kernel:150': kernel_bench('10M x 150 bp' if n == 10_000_000 else '%d x 150 bp' % n, synth.Spec(20261005, 150))
    elif step == 'kernel:var': kernel_bench('36-301 bp, Ns', synth.Spec(20261003 + 5, (36, 301), n_rate=1))
    elif step == 'size': size_bench()
    else: sys.exit('unknown step ' + step)
    sys.exit(0)

steps = ['kernel:150', 'kernel:var'] + ([] if '--no-size' in sys.argv else ['size'])
for step in steps:
    env = dict(os.environ)
    for k in ('OMP_NUM_THREADS', 'MKL_NUM_THREADS'):
        env[k] = str(min(16, int(env.get(k, '16') or 16)))
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step] + sys.argv[1:], cwd=REPO, env=env, timeout=STEP_LIMIT_S[step])
    except subprocess.TimeoutExpired:
        sys.exit('bench_requant: step %s passed its limit of %d s: stopped' % (step, STEP_LIMIT_S[step]))
    if r.returncode != 0:
        sys.exit('bench_requant: step %s failed (exit status %d): stopped' % (step, r.returncode))
