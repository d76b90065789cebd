#!/usr/bin/env python3
"""Times uq_fingerprint_accumulate on the two benchmark geometries, generated on the device -- 10 M x 150 bp (BASELINE
configs[1]) and 36-301 bp with Ns (configs[4]) -- beside the launch it must not be slower than: uq_pack_stats_qname on the same input, which
reads the same stream and writes the packed rows as well.  The two alternate in one process (device events, min and median of the rounds); the
fingerprint is checked against the host twin on a prefix first.  Then the CLI's work_s (UQ_TIMING) for a plain encode and for the same
encode with --verify, on a file of --cli-reads reads.
    python tools/bench_fingerprint.py [reads] [--cli-reads N] [--rounds R] [--no-cli]     one JSON line per measurement"""
import json, os, statistics, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from uq_amd import analysis, ops, synth
from uq_amd.device import Context

def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default

pos = [a for i, a in enumerate(sys.argv[1:], 1) if a.isdigit() and not sys.argv[i - 1].startswith('--')]
n = int(pos[0]) if pos else 10_000_000
rounds, cli_reads = opt('--rounds', 7), opt('--cli-reads', 2_000_000)
ctx = Context(0)
HBM_PEAK = 8.0e12                                   # bytes / s (spec); the algorithmic bytes are the input's

def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1), out

def kernel_bench(label, spec):
    d_buf = ops.synth_fastq(ctx, spec, 0, n)
    nl = ops.count_lines(ctx, d_buf); ls = ops.index_lines(ctx, d_buf, nl)
    # the answer first: a prefix against the sequential host twin, and the whole against the sum of two halves
    k = min(n, 20000)
    end = int(ctx.to_numpy(ls[4 * k:4 * k + 1], np.uint64)[0])
    head = ctx.to_numpy(d_buf[:end])
    d = ops.fingerprint_new(ctx); ops.fingerprint_accumulate(ctx, d, d_buf, ls, 0, k)
    assert ops.fingerprint_fetch(ctx, d) == ops.fingerprint_host(head), 'device fingerprint != host twin'
    whole = ops.fingerprint(ctx, d_buf, ls, n)
    d = ops.fingerprint_new(ctx)
    ops.fingerprint_accumulate(ctx, d, d_buf, ls, n // 2, n - n // 2, n // 2); ops.fingerprint_accumulate(ctx, d, d_buf, ls, 0, n // 2)
    assert ops.fingerprint_fetch(ctx, d) == whole, 'halves do not add up'
    # the launch to beat: pack + statistics + QNAME phase with the file's own decisions (the guess is made once, outside the timing)
    st = ops.stats_new(ctx); ops.stats_accumulate(ctx, st, d_buf, ls, 0, n); hs = ops.stats_fetch(ctx, st)
    dd = analysis.decide_from_counts(hs.counts, hs.len_min, hs.len_max)
    p = ops.make_pack_params(dd['bases'], dd['qualities'], dd['N_qual'], dd['bits_per_base'], dd['bits_per_quality'], dd['variable_read_lengths'],
                             dd['dna_bytes_per_row'], dd['quality_bytes_per_row'], dd['dna_max'], hs.max_record_bytes, avg_record_bytes=d_buf.numel() // n)
    fq = ops.FusedQname(ctx, n); ops.qname_guess(ctx, d_buf, ls, n, fq)
    d_fp = ops.fingerprint_new(ctx)
    def fp(): ops.fingerprint_accumulate(ctx, d_fp, d_buf, ls, 0, n)
    def pack(): return ops.pack_stats(ctx, d_buf, ls, 0, n, p, fq=fq)
    assert pack() is not None, 'no fused pack kernel for this geometry'
    fp(); torch.cuda.synchronize()
    t_fp, t_pk = [], []
    for _ in range(rounds):
        t_fp.append(timed(fp)[0]); t_pk.append(timed(pack)[0])
    nbytes = d_buf.numel()
    r = {'bench': 'fingerprint_kernel', 'input': label, 'reads': n, 'bytes': nbytes, 'rounds': rounds,
         'fingerprint_ms_min': round(min(t_fp), 3), 'fingerprint_ms_median': round(statistics.median(t_fp), 3),
         'pack_stats_qname_ms_min': round(min(t_pk), 3), 'pack_stats_qname_ms_median': round(statistics.median(t_pk), 3),
         'fingerprint_GBps': round(nbytes / 1e6 / min(t_fp), 1), 'fraction_of_8TBps': round(nbytes / (min(t_fp) * 1e-3) / HBM_PEAK, 3),
         'no_slower_than_pack_stats_qname': min(t_fp) <= min(t_pk) and statistics.median(t_fp) <= statistics.median(t_pk), 'records': '%016x' % whole['records']}
    print(json.dumps(r), flush=True)

kernel_bench('10M x 150 bp' if n == 10_000_000 else '%d x 150 bp' % n, synth.Spec(20261005, 150))
kernel_bench('36-301 bp, Ns', synth.Spec(20261003 + 5, (36, 301), n_rate=1))

if '--no-cli' not in sys.argv:
    # the CLI in processes of their own (this one lets go of the GPU's memory first)
    d_buf = ops.synth_fastq(ctx, synth.Spec(20261005, 150), 0, cli_reads)
    tmp = tempfile.mkdtemp(prefix='bench_fp_')
    path = os.path.join(tmp, 'reads.fastq')
    ctx.to_numpy(d_buf).tofile(path)
    del d_buf; torch.cuda.empty_cache()
    def cli(extra):
        best, last = None, ''
        for _ in range(3):
            r = subprocess.run([sys.executable, '-m', 'uq_amd.uq', '-i', path, '-o', path + '.uQ', '--quiet'] + extra, capture_output=True, text=True,
                               env=dict(os.environ, UQ_TIMING='1'), cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
            assert r.returncode == 0, r.stdout + r.stderr
            w = [json.loads(l)['work_s'] for l in r.stderr.split('\n') if l.startswith('{"uq_timing"')][-1]
            best, last = (w if best is None or w < best else best), r.stdout.strip()
        return best, last
    plain, _ = cli([])
    ver, line = cli(['--verify'])
    print(json.dumps({'bench': 'cli_verify', 'reads': cli_reads, 'bytes': os.path.getsize(path), 'encode_work_s': plain, 'encode_verify_work_s': ver,
                      'verify_overhead_s': round(ver - plain, 3), 'said': line}), flush=True)
    for f in os.listdir(tmp): os.remove(os.path.join(tmp, f))
    os.rmdir(tmp)
