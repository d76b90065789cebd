#!/usr/bin/env python3
"""Times the read trimmer's kernels on the two benchmark geometries, generated on the device -- 10 M reads of 150 bp
(BASELINE configs[1]) and of 36-301 bp with Ns (configs[4]): uq_trim_mark with q3 alone and with every step on, beside uq_filter_mark,
uq_stats_accumulate and uq_fingerprint_accumulate on the same buffers; uq_trim_plan (its launches counted from the source); uq_trim_records at
the identity trim, at q3=20 and at tail=50, with and without the index of the trimmed text, beside uq_compact_records keep-all, a plain
device-to-device copy of the same output bytes and uq_interleave_records producing the same number of output bytes -- all in one process,
alternating (device events; one warm-up launch each; best and median of the rounds).  The answer first: the identity trim gives the source
back, and the trimmed outputs hold the reads and bases the report says.
Bytes touched: trim copy = source bytes of the pieces read (about the output) + the output + 40 B of index and 8 B of window and 8 B of plan
per record, counted as twice the output + 56 B per record; compaction = the output twice + 16 B per unit; copy = the output twice;
interleave = the output twice + 64 B of index sectors per pair.  The rates to compare are bytes touched per millisecond.

Every GPU step is a child process of its own under its own time limit; the first failure stops the run; at most 16 threads.
    python tools/bench_trim.py [reads] [--rounds R] [--out FILE]     one JSON line per shape (appended to FILE when given)"""
import json, os, re, statistics, subprocess, sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
STEP_LIMIT_S = {'150': 300, 'var': 300}


def opt(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


pos = [a for i, a in enumerate(sys.argv[1:], 1) if a.isdigit() and not sys.argv[i - 1].startswith('--')]
n = int(pos[0]) if pos else 10_000_000
rounds, out_file = opt('--rounds', 5), opt('--out', None, str)


def bench(label, spec):
    import numpy as np
    import torch
    from uq_amd import ops, recfilter, rectrim
    from uq_amd.device import Context
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ctx = Context(0)

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def stats_of(row, key, v):
        row[key + '_ms_min'] = round(min(v), 3); row[key + '_ms_median'] = round(statistics.median(v), 3); row[key + '_ms_max'] = round(max(v), 3)

    d_buf = ops.synth_fastq(ctx, spec, 0, n)
    nl = ops.count_lines(ctx, d_buf)
    assert nl == 4 * n
    ls = ops.index_lines(ctx, d_buf, nl)
    size = d_buf.numel()
    fp_src = ops.fingerprint(ctx, d_buf, ls, n)
    d_rep, d_frep, d_fp, d_st = ops.trim_report_new(ctx), ops.filter_report_new(ctx), ops.fingerprint_new(ctx), ops.stats_new(ctx)
    window = torch.empty(2 * n, dtype=torch.int32, device=ctx.device)
    verdict = ctx.empty(n)
    q3_only = ops.trim_params(**rectrim.parse('q3=20'))
    all_on = ops.trim_params(**rectrim.parse('head=1,tail=1,crop=250,polyg=10,q5=15,q3=20,trim-n=1'))
    typical = ops.filter_params(**recfilter.parse('min-len=50,max-n=2,min-mean-q=20,sample=0.5'))
    def mk_q3(): ops.trim_mark(ctx, d_rep, d_buf, ls, 0, n, q3_only, window=window)
    def mk_all(): ops.trim_mark(ctx, d_rep, d_buf, ls, 0, n, all_on, window=window)
    def fm(): ops.filter_mark(ctx, d_frep, d_buf, ls, 0, n, typical, verdict=verdict)
    def fp(): ops.fingerprint_accumulate(ctx, d_fp, d_buf, ls, 0, n)
    def st(): ops.stats_accumulate(ctx, d_st, d_buf, ls, 0, n)
    cands = {'mark_q3': mk_q3, 'mark_all': mk_all, 'filter_mark': fm, 'fingerprint': fp, 'stats': st}
    for f in cands.values(): f()
    torch.cuda.synchronize()                                         # warm
    t = {k: [] for k in cands}
    for _ in range(rounds):
        for k, f in cands.items(): t[k].append(timed(f))
    row = {'bench': 'trim', 'input': label, 'reads': n, 'source_bytes': size, 'rounds': rounds}
    for k, v in t.items(): stats_of(row, k, v)
    row['mark_q3_TBps'] = round(size / min(t['mark_q3']) * 1e3 / 1e12, 3)
    for k in ('mark_q3', 'mark_all'):
        row[k + '_no_slower_than_fingerprint_beyond_its_spread'] = min(t[k]) <= min(t['fingerprint']) + (max(t['fingerprint']) - min(t['fingerprint']))

    # keep-all compaction: what the identity trim is measured against
    frep = ops.filter_report_new(ctx)
    v = ops.filter_mark(ctx, frep, d_buf, ls, 0, n, ops.filter_params())
    src, cdst, kept, cbytes = ops.filter_plan(ctx, frep, ls, 0, n, 1, v)
    assert kept == n and cbytes == size
    half = ctx.to_numpy(ls[0:4 * n + 1:4]).view('uint64')

    for name, spec_text in (('identity', None), ('q3_20', 'q3=20'), ('tail_50', 'tail=50')):
        prm = ops.trim_params(**(rectrim.parse(spec_text) if spec_text else {}))
        rep = ops.trim_report_new(ctx)
        w = ops.trim_mark(ctx, rep, d_buf, ls, 0, n, prm)
        dst, out_bytes = ops.trim_plan(ctx, ls, 0, n, w)
        def pl(): ops.trim_plan(ctx, ls, 0, n, w, dst=dst)
        pl(); tp = [timed(pl) for _ in range(rounds)]                # (host time of the closing read-back included: the call synchronises)
        d_out, d_copy, lso = ctx.empty(out_bytes), ctx.empty(out_bytes), torch.empty(4 * n + 1, dtype=torch.int64, device=ctx.device)
        def tr(): ops.trim_records(ctx, d_buf, ls, 0, n, w, dst, out=d_out)
        def tri(): ops.trim_records(ctx, d_buf, ls, 0, n, w, dst, out=d_out, index=True, line_start_out=lso)
        def cp(): d_copy.copy_(d_out)
        tri(); ctx.sync()
        r = ops.trim_report_fetch(ctx, rep)
        # the answer first
        if name == 'identity':
            assert out_bytes == size and torch.equal(d_out, d_buf) and torch.equal(lso, ls), 'the identity trim does not give the source back'
        else:
            assert ops.count_lines(ctx, d_out) == 4 * n and torch.equal(lso, ops.index_lines(ctx, d_out, 4 * n))
            fo = ops.fingerprint(ctx, d_out, lso, n)
            assert fo['reads'] == n and fo['qname'] == fp_src['qname'] and fo['bases'] == r['bases_out'], 'the trimmed output is not what the report says'
        cands = {'trim': tr, 'trim_with_index': tri, 'copy': cp}
        touched = {'trim': 2 * out_bytes + 56 * n, 'trim_with_index': 2 * out_bytes + 56 * n + 32 * n, 'copy': 2 * out_bytes}
        d_cout = d_il = None
        if name == 'identity':
            d_cout = ctx.empty(size)
            cands['compact_keep_all'] = lambda: ops.compact_records(ctx, d_buf, src, cdst, kept, out=d_cout)
            touched['compact_keep_all'] = 2 * size + 16 * n
        npairs = int(np.searchsorted(half, out_bytes // 2, side='right')) - 1       # an interleave that writes the same number of bytes
        il_bytes_out = 2 * int(half[npairs])
        d_il = ctx.empty(il_bytes_out)
        cands['interleave'] = lambda: ops.interleave_records(ctx, d_buf, ls, d_buf, ls, 0, npairs, out=d_il)
        touched['interleave'] = 2 * il_bytes_out + 64 * npairs
        for f in cands.values(): f()
        torch.cuda.synchronize()
        tc = {k: [] for k in cands}
        for _ in range(rounds):
            for k, f in cands.items(): tc[k].append(timed(f))
        sub = {'spec': spec_text, 'output_bytes': out_bytes, 'bases_out': r['bases_out'], 'reads_trimmed': r['reads_trimmed'], 'emptied': r['emptied'],
               'interleave_output_bytes': il_bytes_out}
        stats_of(sub, 'plan', tp)
        for k, vv in tc.items():
            stats_of(sub, k, vv)
            sub[k + '_bytes_touched'] = touched[k]; sub[k + '_TBps'] = round(touched[k] / min(vv) * 1e3 / 1e12, 3)
        sub['trim_fraction_of_copy'] = round(min(tc['copy']) / min(tc['trim']), 3)
        sub['trim_rate_over_interleave_rate'] = round((touched['trim'] / min(tc['trim'])) / (touched['interleave'] / min(tc['interleave'])), 3)
        if name == 'identity':
            c = tc['compact_keep_all']
            sub['trim_over_compact_keep_all'] = round(min(tc['trim']) / min(c), 3)
            sub['identity_within_the_spread_of_compact_keep_all'] = min(tc['trim']) <= max(c)
        row[name] = sub
        del d_out, d_copy, d_il, d_cout, lso, dst, w
    # the plan's launches: its own kernel, one scan (reduce + partials + tiles at this size), one read-back
    scan_text = open(os.path.join(REPO, 'uq_amd', 'csrc', 'scan.hip')).read()
    src_text = open(os.path.join(REPO, 'uq_amd', 'csrc', 'trim.hip')).read()
    tile = int(re.search(r'SCAN_THREADS = (\d+);', scan_text).group(1)) * int(re.search(r'SCAN_ITEMS = (\d+);', scan_text).group(1))
    assert re.search(r'SCAN_TILE = SCAN_THREADS \* SCAN_ITEMS;', scan_text)
    m, levels = n, []
    while m > tile: m = (m + tile - 1) // tile; levels.append(m)
    row['plan_launches'] = 1 + (1 + 2 * len(levels)) + 1
    assert 'trim_len_kernel<<<' in src_text and src_text.count('uq_scan_exclusive_u64(ctx') == 1
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
        sys.exit('bench_trim: step %s passed its limit of %d s: stopped' % (step, STEP_LIMIT_S[step]))
    if r.returncode != 0:
        sys.exit('bench_trim: step %s failed (exit status %d): stopped' % (step, r.returncode))
