#!/usr/bin/env python3
"""Times the paired-end kernels on the two benchmark geometries, generated on the device -- 10 M pairs of 150 bp
(BASELINE configs[1]) and of 36-301 bp with Ns (configs[4]), the inputs of tools/bench_requant.py, each mate in a buffer of its own:
uq_interleave_records, uq_mate_check, a plain device-to-device copy of the same output bytes, and uq_requantise_qualities on the
interleaved text, all in one process, alternating (device events; best and median of the rounds).  The answer first: the output's
fingerprint sums are the two sources' added, and uq_mate_check on it reports no mismatch.
Bytes touched: interleave = the output twice (once read, once written) + 64 B of index sectors per pair; copy = the output twice;
requantise = the quality bytes twice + 16 B of line starts per read.  The rates to compare are bytes touched per millisecond.

Every GPU step is a child process of its own under its own time limit; the first failure stops the run; at most 16 threads.
    python tools/bench_interleave.py [pairs] [--rounds R] [--out FILE]     one JSON line per shape (appended to FILE when given)"""
import json, os, statistics, subprocess, sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
COPY_CEILING = 5.3e12                               # bytes / s: what a plain copy kernel reaches (tools/membench.hip)
STEP_LIMIT_S = {'150': 300, 'var': 300}


def opt(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


pos = [a for i, a in enumerate(sys.argv[1:], 1) if a.isdigit() and not sys.argv[i - 1].startswith('--')]
n = int(pos[0]) if pos else 10_000_000
rounds, out_file = opt('--rounds', 5), opt('--out', None, str)


def bench(label, spec):
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

    def indexed(buf):
        nl = ops.count_lines(ctx, buf)
        assert nl == 4 * n
        return ops.index_lines(ctx, buf, nl)

    d_a = ops.synth_fastq(ctx, spec, 0, n); ls_a = indexed(d_a)
    d_b = ops.synth_fastq(ctx, spec, 0, n); ls_b = indexed(d_b)      # the same reads: equal names, so every pair is a pair of mates
    size = d_a.numel() + d_b.numel()
    d_out, d_copy = ctx.empty(size), ctx.empty(size)
    d_rep, d_changed = ops.mate_report_new(ctx), ops.changed_new(ctx)
    def il(): ops.interleave_records(ctx, d_a, ls_a, d_b, ls_b, 0, n, out=d_out)
    def mc(): ops.mate_check(ctx, d_rep, d_a, ls_a, 0, 1, d_b, ls_b, 0, 1, n)
    def cp(): d_copy.copy_(d_out)
    # the answer first
    il(); ctx.sync()
    nl = ops.count_lines(ctx, d_out)
    assert nl == 8 * n, 'the interleaved text holds %d lines, not %d' % (nl, 8 * n)
    ls_o = ops.index_lines(ctx, d_out, nl)
    fa, fo = ops.fingerprint(ctx, d_a, ls_a, n), ops.fingerprint(ctx, d_out, ls_o, 2 * n)
    assert all(fo[k] == (2 * fa[k]) % (1 << 64) for k in ('reads', 'bases', 'qname', 'dna', 'qual', 'records')), 'interleaved text != its two sources'
    d_chk = ops.mate_report_new(ctx)
    ops.mate_check(ctx, d_chk, d_out, ls_o, 0, 2, d_out, ls_o, 1, 2, n)
    assert ops.mate_report_fetch(ctx, d_chk) == {'pairs': n, 'mismatches': 0, 'first_mismatch': None, 'slash_pairs': 0}, 'the output does not alternate mates'
    def rq(): ops.requantise_qualities(ctx, d_out, ls_o, 0, 2 * n, lut, d_changed)
    cp(); mc(); rq(); torch.cuda.synchronize()                       # warm (the binning changes no byte that is moved afterwards)
    t = {'il': [], 'mc': [], 'cp': [], 'rq': []}
    for _ in range(rounds):
        t['il'].append(timed(il)); t['cp'].append(timed(cp)); t['mc'].append(timed(mc)); t['rq'].append(timed(rq))
    rep = ops.mate_report_fetch(ctx, d_rep)
    assert rep['mismatches'] == 0 and rep['pairs'] == (rounds + 1) * n
    best = {k: min(v) for k, v in t.items()}
    il_bytes, cp_bytes, rq_bytes = 2 * size + 64 * n, 2 * size, 2 * fo['bases'] + 16 * 2 * n
    il_rate, cp_rate, rq_rate = il_bytes / best['il'], cp_bytes / best['cp'], rq_bytes / best['rq']     # bytes touched per ms
    row = {'bench': 'interleave', 'input': label, 'pairs': n, 'output_bytes': size, 'rounds': rounds,
           'interleave_ms_min': round(best['il'], 3), 'interleave_ms_median': round(statistics.median(t['il']), 3),
           'mate_check_ms_min': round(best['mc'], 3), 'mate_check_ms_median': round(statistics.median(t['mc']), 3),
           'copy_ms_min': round(best['cp'], 3), 'copy_ms_median': round(statistics.median(t['cp']), 3),
           'requant_ms_min': round(best['rq'], 3), 'requant_ms_median': round(statistics.median(t['rq']), 3),
           'interleave_bytes_touched': il_bytes, 'requant_bytes_touched': rq_bytes,
           'interleave_TBps': round(il_rate * 1e3 / 1e12, 3), 'copy_TBps': round(cp_rate * 1e3 / 1e12, 3), 'requant_TBps': round(rq_rate * 1e3 / 1e12, 3),
           'interleave_fraction_of_copy': round(best['cp'] / best['il'], 3),
           'interleave_fraction_of_copy_ceiling_5.3TBps': round(il_rate * 1e3 / COPY_CEILING, 3),
           'interleave_rate_over_requant_rate': round(il_rate / rq_rate, 3), 'at_least_0.9_of_requant_rate': il_rate >= 0.9 * rq_rate}
    line = json.dumps(row)
    print(line, flush=True)
    if out_file:
        with open(out_file, 'a') as f: f.write(line + '\n')
    ctx.close()


if '--step' in sys.argv:
    from uq_amd import synth
    step = sys.argv[sys.argv.index('--step') + 1]
    if step == '150': bench('10M pairs x 150 bp' if n == 10_000_000 else '%d pairs x 150 bp' % n, synth.Spec(20261005, 150))
    elif step == 'var': bench('%s pairs x 36-301 bp, Ns' % ('10M' if n == 10_000_000 else n), synth.Spec(20261003 + 5, (36, 301), n_rate=1))
    else: sys.exit('unknown step ' + step)
    sys.exit(0)

for step in ('150', 'var'):
    env = dict(os.environ)
    for k in ('OMP_NUM_THREADS', 'MKL_NUM_THREADS'):
        env[k] = str(min(16, int(env.get(k, '16') or 16)))
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step] + sys.argv[1:], cwd=REPO, env=env, timeout=STEP_LIMIT_S[step])
    except subprocess.TimeoutExpired:
        sys.exit('bench_interleave: step %s passed its limit of %d s: stopped' % (step, STEP_LIMIT_S[step]))
    if r.returncode != 0:
        sys.exit('bench_interleave: step %s failed (exit status %d): stopped' % (step, r.returncode))
