#!/usr/bin/env python3
"""Times uq_qc_accumulate on the two benchmark geometries, generated on the device -- 10 M x 150 bp (BASELINE configs[1])
and 36-301 bp with Ns (configs[4]) -- beside the two passes that read the same bytes: uq_stats_accumulate (one LDS atomic per (base, quality)
pair; the yardstick) and uq_fingerprint_accumulate.  The three alternate in one process on the same buffers; each launch is timed with the
context's timer (device events on the context's stream), after a warm-up launch of each; min and median of the rounds.  The tables are
checked first: a prefix against the sequential host twin, the whole against the sum of two halves, and the invariants.
    python tools/bench_qc.py [reads] [--rounds R] [--cycles C] [--out FILE]
One JSON line per geometry, printed and appended to FILE (default: profiles/rNN_bench_qc.jsonl under the next free round prefix)."""
import ctypes as C, glob, json, os, re, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from uq_amd import ops, synth
from uq_amd._lib import call
from uq_amd.device import Context

def opt(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default

pos = [a for i, a in enumerate(sys.argv[1:], 1) if a.isdigit() and not sys.argv[i - 1].startswith('--')]
n = int(pos[0]) if pos else 10_000_000
rounds, cycles = opt('--rounds', 9), opt('--cycles', ops.QC_MAX_CYCLES)
HBM_PEAK = 8.0e12                                   # bytes / s (spec); the algorithmic bytes are the input's

def next_round_file():
    used = [int(m.group(1)) for m in (re.match(r'r(\d+)_', os.path.basename(p)) for p in glob.glob(os.path.join(ROOT, 'profiles', 'r*_*'))) if m]
    return os.path.join(ROOT, 'profiles', 'r%02d_bench_qc.jsonl' % (max(used, default=0) + 1))

out_path = opt('--out', None, str) or next_round_file()
ctx = Context(0)

def timed(fn):
    ms = C.c_float()
    call('uq_timer_start', ctx.h); fn(); call('uq_timer_stop', ctx.h, C.byref(ms))
    return ms.value

def geometry(label, spec):
    d_buf = ops.synth_fastq(ctx, spec, 0, n)
    nl = ops.count_lines(ctx, d_buf); ls = ops.index_lines(ctx, d_buf, nl)
    assert nl == 4 * n
    # the answer first
    k = min(n, 20000)
    end = int(ctx.to_numpy(ls[4 * k:4 * k + 1], np.uint64)[0])
    d = ops.qc_new(ctx, cycles); ops.qc_accumulate(ctx, d, d_buf, ls, 0, k, cycles)
    assert (ops.qc_fetch(ctx, d) == ops.qc_host(ctx.to_numpy(d_buf[:end]), cycles)).all(), 'device tables != host twin'
    whole = ops.qc(ctx, d_buf, ls, n, cycles)
    d = ops.qc_new(ctx, cycles)
    ops.qc_accumulate(ctx, d, d_buf, ls, n // 2, n - n // 2, cycles); ops.qc_accumulate(ctx, d, d_buf, ls, 0, n // 2, cycles)
    assert (ops.qc_fetch(ctx, d) == whole).all(), 'halves do not add up'
    f = ops.qc_fields(whole)
    assert f['reads'] == n and int(f['base_by_cycle'].sum()) == f['bases'] and int(f['qual_by_cycle'].sum()) == f['qual_chars'] and int(f['length_hist'].sum()) == n
    d_qc, d_st, d_fp = ops.qc_new(ctx, cycles), ops.stats_new(ctx), ops.fingerprint_new(ctx)
    runs = {'qc': lambda: ops.qc_accumulate(ctx, d_qc, d_buf, ls, 0, n, cycles),
            'stats': lambda: ops.stats_accumulate(ctx, d_st, d_buf, ls, 0, n),
            'fingerprint': lambda: ops.fingerprint_accumulate(ctx, d_fp, d_buf, ls, 0, n)}
    for fn in runs.values(): fn()                  # warm: code objects loaded, the buffers' pages touched
    ctx.sync()
    t = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items(): t[k].append(timed(fn))
    nbytes = d_buf.numel()
    r = {'bench': 'qc_kernel', 'input': label, 'reads': n, 'bytes': nbytes, 'cycles': cycles, 'rounds': rounds}
    for k in runs:
        r[k + '_ms_min'] = round(min(t[k]), 3); r[k + '_ms_median'] = round(statistics.median(t[k]), 3)
    med = {k: statistics.median(t[k]) for k in runs}
    r.update({'qc_GBps': round(nbytes / 1e6 / med['qc'], 1), 'qc_fraction_of_8TBps': round(nbytes / (med['qc'] * 1e-3) / HBM_PEAK, 3),
              'qc_over_stats': round(med['qc'] / med['stats'], 3), 'qc_over_fingerprint': round(med['qc'] / med['fingerprint'], 3),
              'bases': f['bases'], 'mean_read_length': round(f['bases'] / n, 2)})
    line = json.dumps(r)
    print(line, flush=True)
    with open(out_path, 'a') as fh: fh.write(line + '\n')

geometry('10M x 150 bp' if n == 10_000_000 else '%d x 150 bp' % n, synth.Spec(20261005, 150))
geometry('36-301 bp, Ns', synth.Spec(20261003 + 5, (36, 301), n_rate=1))
