#!/usr/bin/env python3
"""Times the read filter's kernels on the two benchmark geometries, generated on the device -- 10 M reads of 150 bp
(BASELINE configs[1]) and of 36-301 bp with Ns (configs[4]): uq_filter_mark beside uq_fingerprint_accumulate and uq_stats_accumulate on the
same buffers; uq_filter_plan (its launches counted from the source); uq_compact_records at keep-all, sample=0.5 and sample=0.1 beside a plain
device-to-device copy of the same output bytes and uq_interleave_records producing the same number of output bytes -- all in one process,
alternating (device events; one warm-up launch each; best and median of the rounds).  The answer first: keep-all gives the source back, and
the sampled outputs hold the reads the report says.
Bytes touched: compaction = the output twice (once read, once written) + 16 B of plan entries per kept unit; copy = the output twice;
interleave = the output twice + 64 B of index sectors per pair.  The rates to compare are bytes touched per millisecond.

Every GPU step is a child process of its own under its own time limit; the first failure stops the run; at most 16 threads.
    python tools/bench_filter.py [reads] [--rounds R] [--out FILE]     one JSON line per shape (appended to FILE when given)"""
import json, os, statistics, subprocess, sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
STEP_LIMIT_S = {'150': 300, 'var': 300}


def opt(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


pos = [a for i, a in enumerate(sys.argv[1:], 1) if a.isdigit() and not sys.argv[i - 1].startswith('--')]
n = int(pos[0]) if pos else 10_000_000
rounds, out_file = opt('--rounds', 5), opt('--out', None, str)


def bench(label, spec):
    import torch
    from uq_amd import ops, recfilter
    from uq_amd.device import Context
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ctx = Context(0)

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    d_buf = ops.synth_fastq(ctx, spec, 0, n)
    nl = ops.count_lines(ctx, d_buf)
    assert nl == 4 * n
    ls = ops.index_lines(ctx, d_buf, nl)
    size = d_buf.numel()
    fp_src = ops.fingerprint(ctx, d_buf, ls, n)
    d_rep, d_fp, d_st = ops.filter_report_new(ctx), ops.fingerprint_new(ctx), ops.stats_new(ctx)
    verdict = ctx.empty(n)
    typical = ops.filter_params(**recfilter.parse('min-len=50,max-n=2,min-mean-q=20,sample=0.5'))
    def mk(): ops.filter_mark(ctx, d_rep, d_buf, ls, 0, n, typical, verdict=verdict)
    def mk_lds():                                                   # the same with the quality clamp as a 256-byte LDS table (read by the library at every call)
        os.environ['UQ_FILTER_CLAMP'] = 'lds'
        try: mk()
        finally: del os.environ['UQ_FILTER_CLAMP']
    def fp(): ops.fingerprint_accumulate(ctx, d_fp, d_buf, ls, 0, n)
    def st(): ops.stats_accumulate(ctx, d_st, d_buf, ls, 0, n)
    mk(); ctx.sync(); v_swar = verdict.clone()
    mk_lds(); ctx.sync()
    assert torch.equal(verdict, v_swar), 'the two clamps give different verdicts'
    fp(); st(); torch.cuda.synchronize()                             # warm
    t = {'mark': [], 'mark_lds_table': [], 'fingerprint': [], 'stats': []}
    for _ in range(rounds):
        t['mark'].append(timed(mk)); t['mark_lds_table'].append(timed(mk_lds)); t['fingerprint'].append(timed(fp)); t['stats'].append(timed(st))
    row = {'bench': 'filter', 'input': label, 'reads': n, 'source_bytes': size, 'rounds': rounds}
    for k, v in t.items():
        row[k + '_ms_min'] = round(min(v), 3); row[k + '_ms_median'] = round(statistics.median(v), 3); row[k + '_ms_max'] = round(max(v), 3)
    row['mark_TBps'] = round(size / min(t['mark']) * 1e3 / 1e12, 3)
    row['mark_no_slower_than_fingerprint_beyond_its_spread'] = min(t['mark']) <= min(t['fingerprint']) + (max(t['fingerprint']) - min(t['fingerprint']))

    # the plan and the compaction at three keep rates
    src_text = open(os.path.join(REPO, 'uq_amd', 'csrc', 'filter.hip')).read()
    d_copy = None
    for name, spec_text in (('keep_all', 'min-len=0'), ('sample_0.5', 'sample=0.5'), ('sample_0.1', 'sample=0.1')):
        prm = ops.filter_params(**recfilter.parse(spec_text))
        rep = ops.filter_report_new(ctx)
        v = ops.filter_mark(ctx, rep, d_buf, ls, 0, n, prm)
        src, dst, kept, out_bytes = ops.filter_plan(ctx, rep, ls, 0, n, 1, v)
        def pl(): ops.filter_plan(ctx, rep, ls, 0, n, 1, v)
        pl(); tp = [timed(pl) for _ in range(rounds)]                # (host time of the closing read-back included: the call synchronises)
        d_out = ctx.empty(out_bytes)
        d_copy = ctx.empty(out_bytes)
        def cr(): ops.compact_records(ctx, d_buf, src, dst, kept, out=d_out)
        def cp(): d_copy.copy_(d_out)
        cr(); ctx.sync()
        # the answer first
        if name == 'keep_all':
            assert kept == n and out_bytes == size and torch.equal(d_out, d_buf), 'keep-all does not give the source back'
        else:
            assert ops.count_lines(ctx, d_out) == 4 * kept
            fo = ops.fingerprint(ctx, d_out, ops.index_lines(ctx, d_out, 4 * kept), kept)
            r = ops.filter_report_fetch(ctx, rep)
            assert fo['reads'] == kept == r['reads_out'] // (rounds + 2) and fo['bases'] == r['bases_out'] // (rounds + 2), 'the sampled output is not what the report says'
        # an interleave that writes the same number of bytes: the first pairs of the source with itself
        half = ctx.to_numpy(ls[0:4 * n + 1:4]).view('uint64')
        import numpy as np
        npairs = int(np.searchsorted(half, out_bytes // 2, side='right')) - 1
        il_bytes_out = 2 * int(half[npairs])
        d_il = ctx.empty(il_bytes_out)
        def il(): ops.interleave_records(ctx, d_buf, ls, d_buf, ls, 0, npairs, out=d_il)
        cp(); il(); torch.cuda.synchronize()
        tc = {'compact': [], 'copy': [], 'interleave': []}
        for _ in range(rounds):
            tc['compact'].append(timed(cr)); tc['copy'].append(timed(cp)); tc['interleave'].append(timed(il))
        touched = {'compact': 2 * out_bytes + 16 * kept, 'copy': 2 * out_bytes, 'interleave': 2 * il_bytes_out + 64 * npairs}
        sub = {'kept_reads': kept, 'output_bytes': out_bytes, 'plan_ms_min': round(min(tp), 3), 'plan_ms_median': round(statistics.median(tp), 3),
               'interleave_output_bytes': il_bytes_out}
        for k, vv in tc.items():
            sub[k + '_ms_min'] = round(min(vv), 3); sub[k + '_ms_median'] = round(statistics.median(vv), 3)
            sub[k + '_bytes_touched'] = touched[k]; sub[k + '_TBps'] = round(touched[k] / min(vv) * 1e3 / 1e12, 3)
        sub['compact_fraction_of_copy'] = round(min(tc['copy']) / min(tc['compact']), 3)
        sub['compact_rate_over_interleave_rate'] = round((touched['compact'] / min(tc['compact'])) / (touched['interleave'] / min(tc['interleave'])), 3)
        row[name] = sub
        del d_out, d_copy, d_il, src, dst, v
    # the plan's launches: its own two kernels, the two scans (reduce + partials + tiles each at this size), one read-back
    scan_text = open(os.path.join(REPO, 'uq_amd', 'csrc', 'scan.hip')).read()
    import re
    tile = int(re.search(r'SCAN_THREADS = (\d+);', scan_text).group(1)) * int(re.search(r'SCAN_ITEMS = (\d+);', scan_text).group(1))
    assert re.search(r'SCAN_TILE = SCAN_THREADS \* SCAN_ITEMS;', scan_text)
    m, levels = n, []
    while m > tile: m = (m + tile - 1) // tile; levels.append(m)
    scan_launches = 1 + 2 * len(levels)
    row['plan_launches'] = 2 + 2 * scan_launches + 1
    assert 'filter_units_kernel<<<' in src_text and 'filter_scatter_kernel<<<' in src_text and src_text.count('uq_scan_exclusive_u64(ctx') == 2
    line = json.dumps(row)
    print(line, flush=True)
    if out_file:
        with open(out_file, 'a') as f: f.write(line + '\n')
    ctx.close()


if '--step' in sys.argv:
    from uq_amd import synth
    step = sys.argv[sys.argv.index('--step') + 1]
    if step == '150': bench('10M x 150 bp' if n == 10_000_000 else '%d x 150 bp' % n, synth.Spec(20261005, 150))
    elif step == 'var': bench('%s x 36-301 bp, Ns' % ('10M' if n == 10_000_000 else n), synth.Spec(20261003 + 5, (36, 301), n_rate=1))
    else: sys.exit('unknown step ' + step)
    sys.exit(0)

for step in ('150', 'var'):
    env = dict(os.environ)
    for k in ('OMP_NUM_THREADS', 'MKL_NUM_THREADS'):
        env[k] = str(min(16, int(env.get(k, '16') or 16)))
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step] + sys.argv[1:], cwd=REPO, env=env, timeout=STEP_LIMIT_S[step])
    except subprocess.TimeoutExpired:
        sys.exit('bench_filter: step %s passed its limit of %d s: stopped' % (step, STEP_LIMIT_S[step]))
    if r.returncode != 0:
        sys.exit('bench_filter: step %s failed (exit status %d): stopped' % (step, r.returncode))
