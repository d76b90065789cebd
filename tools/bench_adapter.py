#!/usr/bin/env python3
"""Times the adapter step's kernel on the two benchmark geometries, generated on the device -- 10 M reads of 150 bp
(BASELINE configs[1]) and of 36-301 bp with Ns (configs[4]): uq_adapter_mark with seq=illumina (13 bases) and with the 33 bases of the TruSeq
read-1 adapter, on
  1 the reads as synthesised: almost no read holds a candidate, so every position of every read is scanned (the worst case, and the common one);
  2 (150 bp) the same reads with the 33-base adapter written into 30 % of them at a uniform position and random bases behind it,
beside uq_trim_mark q3=20 and uq_fingerprint_accumulate on the same buffers, and uq_trim_records at the windows the adapter step leaves -- all
in one process, alternating (device events; one warm-up launch each; best and median of the rounds).  The answer first: the windows and the
report of the first 20 000 records equal the host twin's.  Input 2 is written on the device with torch (which reads get the adapter, where,
and the bases behind it come from torch's device generator under a fixed seed): `reads_with_adapter` and the counts of that column repeat
only under the same torch build.

Every GPU step is a child process of its own under its own time limit; the first failure stops the run; at most 16 threads.
    python tools/bench_adapter.py [reads] [--rounds R] [--out FILE]     one JSON line per shape (appended to FILE when given)"""
import json, os, statistics, subprocess, sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
STEP_LIMIT_S = {'150': 300, 'var': 300}
A33 = 'AGATCGGAAGAGCACACGTCTGAACTCCAGTCA'


def opt(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


pos = [a for i, a in enumerate(sys.argv[1:], 1) if a.isdigit() and not sys.argv[i - 1].startswith('--')]
n = int(pos[0]) if pos else 10_000_000
rounds, out_file = opt('--rounds', 5), opt('--out', None, str)


def implant(torch, d_buf, ls, n, L, share=0.3, seed=15):
    """A copy of the text with the 33-base adapter written into `share` of its reads (all of L bases) at a uniform position, random bases behind."""
    out = d_buf.clone()
    g = torch.Generator(device=d_buf.device); g.manual_seed(seed)
    starts = ls[1:4 * n:4]
    chosen = torch.nonzero(torch.rand(n, generator=g, device=d_buf.device) < share).flatten()
    adapter = torch.tensor(list(A33.encode()), dtype=torch.uint8, device=d_buf.device)
    letters = torch.tensor(list(b'ACGT'), dtype=torch.uint8, device=d_buf.device)
    col = torch.arange(L, device=d_buf.device)
    for lo in range(0, chosen.numel(), 500_000):
        sel = chosen[lo:lo + 500_000]
        p = torch.randint(0, L, (sel.numel(), 1), generator=g, device=d_buf.device)
        idx = starts[sel].unsqueeze(1) + col
        rnd = letters[torch.randint(0, 4, idx.shape, generator=g, device=d_buf.device)]
        rel = (col - p).clamp(0, len(A33) - 1)
        new = torch.where(col < p, out[idx], torch.where(col < p + len(A33), adapter[rel], rnd))
        out[idx] = new
    return out, int(chosen.numel())


def bench(label, spec, fixed_len):
    import numpy as np
    import torch
    from uq_amd import ops, rectrim
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
    inputs = {'as_synthesised': d_buf}
    row = {'bench': 'adapter', 'input': label, 'reads': n, 'source_bytes': size, 'rounds': rounds}
    if fixed_len:
        inputs['adapter_in_30_percent'], row['reads_with_adapter'] = implant(torch, d_buf, ls, n, fixed_len)
    p13 = ops.adapter_params('AGATCGGAAGAGC', None, 10, 3, ops.ADAPTER_FRESH)
    p33 = ops.adapter_params(A33, None, 10, 3, ops.ADAPTER_FRESH)
    q3 = ops.trim_params(**rectrim.parse('q3=20'))
    d_arep, d_trep, d_fp = ops.adapter_report_new(ctx), ops.trim_report_new(ctx), ops.fingerprint_new(ctx)
    window = torch.empty(2 * n, dtype=torch.int32, device=ctx.device)
    head = min(n, 20000)
    for name, buf in inputs.items():
        # the answer first
        for prm in (p13, p33):
            rep = ops.adapter_report_new(ctx)
            w = ops.adapter_mark(ctx, rep, buf, ls, 0, head, prm)
            end = int(ls[4 * head])
            hw, hrep = ops.adapter_mark_host(ctx.to_numpy(buf[:end]).tobytes(), prm)
            assert ctx.to_numpy(w).tobytes() == hw.tobytes() and ops.adapter_report_fetch(ctx, rep) == hrep, 'the device does not give the host twin\'s windows'
        def m13(): ops.adapter_mark(ctx, d_arep, buf, ls, 0, n, p13, window=window)
        def m33(): ops.adapter_mark(ctx, d_arep, buf, ls, 0, n, p33, window=window)
        def tq(): ops.trim_mark(ctx, d_trep, buf, ls, 0, n, q3, window=window)
        def fp(): ops.fingerprint_accumulate(ctx, d_fp, buf, ls, 0, n)
        cands = {'adapter_13': m13, 'adapter_33': m33, 'trim_mark_q3': tq, 'fingerprint': fp}
        for f in cands.values(): f()
        torch.cuda.synchronize()                                     # warm
        t = {k: [] for k in cands}
        for _ in range(rounds):
            for k, f in cands.items(): t[k].append(timed(f))
        sub = {}
        for k, v in t.items(): stats_of(sub, k, v)
        for k in ('adapter_13', 'adapter_33'):
            sub[k + '_over_trim_mark_q3'] = round(min(t[k]) / min(t['trim_mark_q3']), 3)
        # the copy at the windows the 33-base search leaves
        rep = ops.adapter_report_new(ctx)
        w = ops.adapter_mark(ctx, rep, buf, ls, 0, n, p33)
        r = ops.adapter_report_fetch(ctx, rep)
        for k in ('adapter_13', 'adapter_33'): sub[k + '_Gpositions_per_s'] = round(r['bases_in'] / min(t[k]) / 1e6, 1)      # (an upper bound of the positions: a cut read is left early)
        dst, out_bytes = ops.trim_plan(ctx, ls, 0, n, w)
        d_out = ctx.empty(out_bytes)
        def tr(): ops.trim_records(ctx, buf, ls, 0, n, w, dst, out=d_out)
        tr(); torch.cuda.synchronize()
        stats_of(sub, 'trim_records', [timed(tr) for _ in range(rounds)])
        sub.update({'reads_cut': r['reads_cut'], 'full': r['full'], 'partial': r['partial'], 'emptied': r['emptied'], 'bases_in': r['bases_in'],
                    'bases_out': r['bases_out'], 'output_bytes': out_bytes})
        row[name] = sub
        del d_out, dst, w
    line = json.dumps(row)
    print(line, flush=True)
    if out_file:
        with open(out_file, 'a') as f: f.write(line + '\n')
    ctx.close()


if '--step' in sys.argv:
    from uq_amd import synth
    step = sys.argv[sys.argv.index('--step') + 1]
    if step == '150': bench('10M x 150 bp' if n == 10_000_000 else '%d x 150 bp' % n, synth.Spec(20261005, 150), 150)
    elif step == 'var': bench('%s x 36-301 bp, Ns' % ('10M' if n == 10_000_000 else n), synth.Spec(20261003 + 5, (36, 301), n_rate=1), 0)
    else: sys.exit('unknown step ' + step)
    sys.exit(0)

for step in ('150', 'var'):
    env = dict(os.environ)
    for k in ('OMP_NUM_THREADS', 'MKL_NUM_THREADS'):
        env[k] = str(min(16, int(env.get(k, '16') or 16)))
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step] + sys.argv[1:], cwd=REPO, env=env, timeout=STEP_LIMIT_S[step])
    except subprocess.TimeoutExpired:
        sys.exit('bench_adapter: step %s passed its limit of %d s: stopped' % (step, STEP_LIMIT_S[step]))
    if r.returncode != 0:
        sys.exit('bench_adapter: step %s failed (exit status %d): stopped' % (step, r.returncode))
