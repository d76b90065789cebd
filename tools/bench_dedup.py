#!/usr/bin/env python3
"""Times the duplicate remover's kernels on the two benchmark geometries, generated on the device -- 10 M reads of
150 bp and of 36-301 bp with Ns, each with the generator's duplicate rule (every tenth read takes its bases from a pool of templates) and, for
uq_dedup_mark, once more without it: uq_dedup_keys (keep=first and keep=best), the 16-byte row sort, uq_dedup_mark, uq_filter_plan +
uq_compact_records on the verdicts, and uq_fingerprint_accumulate and uq_filter_mark on the same buffers -- all in one process, alternating
(device events; one warm-up launch each; best and median of the rounds).  The answer first: no collision at seed 0, the device verdicts of the
first 200 000 reads equal the host twin's, and the compacted text holds the reads the report says.

Every GPU step is a child process of its own under its own time limit; the first failure stops the run; at most 16 threads.
    python tools/bench_dedup.py [reads] [--rounds R] [--out FILE]     one JSON line per shape (appended to FILE when given)"""
import json, os, statistics, subprocess, sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
STEP_LIMIT_S = {'150': 300, 'var': 300}
TEMPLATES = 100_000


def opt(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


pos = [a for i, a in enumerate(sys.argv[1:], 1) if a.isdigit() and not sys.argv[i - 1].startswith('--')]
n = int(pos[0]) if pos else 10_000_000
rounds, out_file = opt('--rounds', 5), opt('--out', None, str)


def bench(label, spec, spec_unique):
    import numpy as np
    import torch
    from uq_amd import ops, recfilter
    from uq_amd.device import Context
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ctx = Context(0)

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def stats(row, t):
        for k, v in t.items():
            row[k + '_ms_min'] = round(min(v), 3); row[k + '_ms_median'] = round(statistics.median(v), 3); row[k + '_ms_max'] = round(max(v), 3)

    def text(s):
        d = ops.synth_fastq(ctx, s, 0, n)
        nl = ops.count_lines(ctx, d)
        assert nl == 4 * n
        return d, ops.index_lines(ctx, d, nl)

    d_buf, ls = text(spec)
    size = d_buf.numel()
    first, best = ops.dedup_params(), ops.dedup_params(flags=ops.DEDUP_BEST)
    d_rep, d_fp, d_frep = ops.dedup_report_new(ctx), ops.fingerprint_new(ctx), ops.filter_report_new(ctx)
    keys, keys_b, verdict, fverdict = ctx.empty(16 * n), ctx.empty(16 * n), ctx.empty(n), ctx.empty(n)
    typical = ops.filter_params(**recfilter.parse('min-len=50,max-n=2,min-mean-q=20,sample=0.5'))
    def kf(): ops.dedup_keys(ctx, d_rep, d_buf, ls, 0, n, first, keys=keys)
    def kb(): ops.dedup_keys(ctx, d_rep, d_buf, ls, 0, n, best, keys=keys_b)
    def fp(): ops.fingerprint_accumulate(ctx, d_fp, d_buf, ls, 0, n)
    def fm(): ops.filter_mark(ctx, d_frep, d_buf, ls, 0, n, typical, verdict=fverdict)
    kf(); kb(); fp(); fm(); torch.cuda.synchronize()                 # warm
    perm = ops.argsort_rows(ctx, keys, n, 16)
    def so(): ops.argsort_rows(ctx, keys, n, 16)
    def mk(): ops.dedup_mark(ctx, d_rep, d_buf, ls, 0, n, first, keys, perm, verdict=verdict)
    # the answer first
    rep = ops.dedup_report_new(ctx)
    ops.dedup_keys(ctx, rep, d_buf, ls, 0, n, first, keys=keys)
    ops.dedup_mark(ctx, rep, d_buf, ls, 0, n, first, keys, perm, verdict=verdict)
    r = ops.dedup_report_fetch(ctx, rep)
    assert r['collisions'] == 0 and r['reads_in'] == n and r['classes'] + r['dup_units'] == n, r
    head = min(n, 200_000)
    end = int(ctx.to_numpy(ls[4 * head:4 * head + 1]).view(np.uint64)[0])
    h_text, h_ls = ctx.to_numpy(d_buf[:end]), ctx.to_numpy(ls[:4 * head + 1]).view(np.uint64)
    h_keys, _ = ops.dedup_keys_host(h_text, first, h_ls)
    assert h_keys.tobytes() == ctx.to_numpy(keys[:16 * head]).tobytes(), 'the device keys are not the host twin\'s'
    src, dst, kept, out_bytes = ops.filter_plan(ctx, ops.filter_report_new(ctx), ls, 0, n, 1, verdict)
    d_out = ctx.empty(out_bytes)
    ops.compact_records(ctx, d_buf, src, dst, kept, out=d_out)
    assert kept == r['classes'] and ops.count_lines(ctx, d_out) == 4 * kept
    fo = ops.fingerprint(ctx, d_out, ops.index_lines(ctx, d_out, 4 * kept), kept)
    assert fo['reads'] == kept and fo['bases'] == r['bases_in'] - r['dup_bases'], 'the deduplicated text is not what the report says'
    # ... and deduplicating it again finds nothing
    rep2 = ops.dedup_report_new(ctx)
    ls2 = ops.index_lines(ctx, d_out, 4 * kept)
    k2 = ops.dedup_keys(ctx, rep2, d_out, ls2, 0, kept, first)
    ops.dedup_mark(ctx, rep2, d_out, ls2, 0, kept, first, k2, ops.argsort_rows(ctx, k2, kept, 16))
    assert ops.dedup_report_fetch(ctx, rep2)['dup_units'] == 0
    del k2, ls2, fo
    frep = ops.filter_report_new(ctx)
    def pc():
        s, d, k, b = ops.filter_plan(ctx, frep, ls, 0, n, 1, verdict)
        ops.compact_records(ctx, d_buf, s, d, k, out=d_out)
    so(); mk(); pc(); torch.cuda.synchronize()
    t = {'keys_first': [], 'keys_best': [], 'fingerprint': [], 'filter_mark': [], 'sort16': [], 'mark': [], 'plan_compact': []}
    for _ in range(rounds):
        t['keys_first'].append(timed(kf)); t['fingerprint'].append(timed(fp)); t['keys_best'].append(timed(kb)); t['filter_mark'].append(timed(fm))
        t['sort16'].append(timed(so)); t['mark'].append(timed(mk)); t['plan_compact'].append(timed(pc))
    row = {'bench': 'dedup', 'input': label, 'reads': n, 'source_bytes': size, 'rounds': rounds, 'duplicate_reads': r['dup_reads'],
           'classes': r['classes'], 'duplicate_fraction': round(r['dup_reads'] / n, 4), 'output_bytes': out_bytes}
    stats(row, t)
    row['keys_first_TBps'] = round(size / min(t['keys_first']) * 1e3 / 1e12, 3)
    spread = max(t['fingerprint']) - min(t['fingerprint'])
    row['keys_first_no_slower_than_fingerprint_beyond_its_spread'] = min(t['keys_first']) <= min(t['fingerprint']) + spread
    row['keys_best_over_filter_mark_plus_keys_first'] = round(min(t['keys_best']) / (min(t['filter_mark']) + min(t['keys_first'])), 3)
    row['mark_fraction_of_keys_first'] = round(min(t['mark']) / min(t['keys_first']), 3)
    del d_out, src, dst, perm
    # the same text without the duplicate rule: the marks must not cost more
    d_u, ls_u = text(spec_unique)
    rep_u = ops.dedup_report_new(ctx)
    ops.dedup_keys(ctx, rep_u, d_u, ls_u, 0, n, first, keys=keys)
    perm_u = ops.argsort_rows(ctx, keys, n, 16)
    def mu(): ops.dedup_mark(ctx, rep_u, d_u, ls_u, 0, n, first, keys, perm_u, verdict=verdict)
    mu(); torch.cuda.synchronize()
    ru = ops.dedup_report_fetch(ctx, rep_u)
    assert ru['collisions'] == 0
    tu = {'mark_unique': [timed(mu) for _ in range(rounds)]}
    stats(row, tu)
    row['unique_text_duplicate_reads'] = ru['dup_reads']
    row['mark_does_not_grow_without_duplicates'] = min(tu['mark_unique']) <= min(t['mark']) + (max(t['mark']) - min(t['mark']))
    line = json.dumps(row)
    print(line, flush=True)
    if out_file:
        with open(out_file, 'a') as f: f.write(line + '\n')
    ctx.close()


if '--step' in sys.argv:
    from uq_amd import synth
    step = sys.argv[sys.argv.index('--step') + 1]
    many = '10M' if n == 10_000_000 else str(n)
    if step == '150':
        bench('%s x 150 bp, every tenth read from %d templates' % (many, TEMPLATES), synth.Spec(20261005, 150, dup='dna', dup_templates=TEMPLATES),
              synth.Spec(20261005, 150))
    elif step == 'var':
        bench('%s x 36-301 bp, Ns, every tenth read from %d templates' % (many, TEMPLATES),
              synth.Spec(20261003 + 5, (36, 301), n_rate=1, dup='dna', dup_templates=TEMPLATES), synth.Spec(20261003 + 5, (36, 301), n_rate=1))
    else: sys.exit('unknown step ' + step)
    sys.exit(0)

for step in ('150', 'var'):
    env = dict(os.environ)
    for k in ('OMP_NUM_THREADS', 'MKL_NUM_THREADS'):
        env[k] = str(min(16, int(env.get(k, '16') or 16)))
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step] + sys.argv[1:], cwd=REPO, env=env, timeout=STEP_LIMIT_S[step])
    except subprocess.TimeoutExpired:
        sys.exit('bench_dedup: step %s passed its limit of %d s: stopped' % (step, STEP_LIMIT_S[step]))
    if r.returncode != 0:
        sys.exit('bench_dedup: step %s failed (exit status %d): stopped' % (step, r.returncode))
