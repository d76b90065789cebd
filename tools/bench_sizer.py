#!/usr/bin/env python3
"""The --test sizer: uq_deflate_size against uq_bgzf_compress on the candidates of bench.py's workload, the CLI's `--test` with the device
sizer against a host compressor, and (on the CPU) whether the sizer ranks the layouts as stock compressors do.

    python tools/bench_sizer.py kernel   [--reads 10000000] [--reps 5] [--compress-lib PATH] [--level {1,2}]
    python tools/bench_sizer.py cli      [--reads 1000000] [--dir /dev/shm] [--host-compressor "gzip -1"]
    python tools/bench_sizer.py grid     [--reads 10000000] [--dir /dev/shm]
    python tools/bench_sizer.py ordering [--reads 100000] [--level {1,2}] (no GPU)

kernel    bench.py's reads (synth-v1, seed 20261005, 150 bp) packed on the device; for the DNA and the QUAL table and each of the eight
          layouts: uq_pattern into one buffer, then uq_deflate_size (header + payload) and uq_bgzf_compress (payload) over --reps warm
          repetitions each, alternating, timed by events: GB/s of candidate bytes, the sizer's rate over the compressor's, and the two
          sizes (equal but for the header's few bytes).  --compress-lib: a second child process times uq_bgzf_compress alone from that
          build of the library (an earlier commit's kernel) on the same bytes.
cli       `python -m uq_amd.uq --test --sort None --raw DNA QUAL QNAME` (one mix, 16 table candidates) with --device-compressor and with
          --compressor CMD: work_s of each (UQ_TIMING), and the parameters each run found best.
grid      the full 32-mix grid with --device-compressor: work_s.
ordering  synthetic reads of both geometries (150 bp fixed, 36-301 bp): S of the 16 candidates of the no-sort all-raw mix next to
          len(zlib.compress(B, 6)) and len(lzma.compress(B)) of the same bytes, and the three orderings.  Host code only.
--level: the compressor level of every step (`--bgzf-level`).  Every GPU step runs in a child process under its own time limit, and the tool stops at the first failure.  One JSON line per step.
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

SEED = 20261003 + 2          # bench.py's workload


def _tables(ctx, reads, length):
    """The packed DNA and QUAL tables of the synthetic reads, as the CLI builds them: name -> (device tensor, rows, cols)."""
    from uq_amd import ops, synth, uq
    d = ops.synth_fastq(ctx, synth.Spec(SEED, length), 0, reads)
    args = uq.build_parser().parse_args(['-i', os.devnull, '--quiet'])
    s = uq.Session(args, ctx=ctx)
    s.load_device(d)
    s.analyse()
    s.pack()
    return {k: s.tables[k] for k in ('DNA', 'QUAL')}


def kernel_child(a):
    import torch
    from uq_amd import ops, uq
    from uq_amd.device import Context
    ctx = Context(0)
    rows_out = []
    for name, (t, rows, cols) in _tables(ctx, a.reads, a.length).items():
        payload = ctx.empty(rows * cols)
        for pat in uq.PATTERNS:
            ops.pattern(ctx, t, rows, cols, pat, out=payload)
            header = uq.pattern_header(rows, cols, pat)
            row = {'table': name, 'rows': rows, 'cols': cols, 'pattern': pat, 'bytes': rows * cols}
            times = {'size': [], 'compress': []}
            for rep in range(a.reps + 1):                                   # the first repetition warms up
                for what in (('compress',) if a.compress_only else ('size', 'compress')):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    if what == 'size':
                        q = ops.DeflateSizes(ctx, 1, level=a.level)
                        e0.record(); q.add(header, payload); e1.record()
                        row['S'] = q.fetch()[0]
                    else:
                        e0.record(); out = ops.bgzf_compress(ctx, payload, eof=False, level=a.level); e1.record()
                        row['compressed_bytes'] = out.numel()
                        del out
                    torch.cuda.synchronize()
                    if rep: times[what].append(e0.elapsed_time(e1) / 1e3)
            for what, ts in times.items():
                if ts:
                    row[what + '_s'] = round(min(ts), 5)
                    row[what + '_GBps'] = round(rows * cols / min(ts) / 1e9, 2)
            if times['size']: row['size_over_compress'] = round(min(times['compress']) / min(times['size']), 3)
            rows_out.append(row)
    print(json.dumps({'kernel': rows_out, 'lib': os.environ.get('UQ_LIB_PATH') or 'this build', 'reads': a.reads, 'level': a.level}), flush=True)


def _child(argv, limit, env=None):
    r = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit('step failed with status %d: %s' % (r.returncode, ' '.join(argv)))
    return r


def kernel(a):
    me = [os.path.abspath(__file__), 'kernel', '--child', '--reads', str(a.reads), '--reps', str(a.reps), '--length', str(a.length), '--level', str(a.level)]
    print(_child(me, a.limit).stdout.strip())
    if a.compress_lib:
        print(_child(me + ['--compress-only'], a.limit, {'UQ_LIB_PATH': os.path.abspath(a.compress_lib)}).stdout.strip())


def _write_reads(a):
    path = os.path.join(a.dir, 'bench_sizer_%d.fastq' % a.reads)
    code = ('import sys; sys.path.insert(0, %r)\nfrom uq_amd import ops, synth\nfrom uq_amd.device import Context\nctx = Context(0)\n'
            'd = ops.synth_fastq(ctx, synth.Spec(%d, %d), 0, %d)\nopen(%r, "wb").write(d.cpu().numpy().tobytes())\n'
            % (HERE, SEED, a.length, a.reads, path))
    _child(['-c', code], a.limit)
    return path


def _uq(a, path, flags, limit):
    t0 = time.perf_counter()
    r = _child(['-m', 'uq_amd.uq', '-i', path, '-o', path + '.uQ', '--test'] + flags + (['--bgzf-level', str(a.level)] if '--device-compressor' in flags and a.level != 1 else []), limit, {'UQ_TIMING': '1', 'PYTHONPATH': HERE})
    timing = [json.loads(l) for l in r.stderr.split('\n') if l.startswith('{"uq_timing"')]
    best = [l.strip() for l in r.stdout.split('\n') if l.strip().startswith('--')]
    return {'flags': flags, 'work_s': timing[-1]['work_s'], 'wall_s': round(time.perf_counter() - t0, 2), 'best': best[-1] if best else None}


def cli(a):
    path = _write_reads(a)
    try:
        one_mix = ['--sort', 'None', '--raw', 'DNA', 'QUAL', 'QNAME']
        out = {'reads': a.reads, 'device': _uq(a, path, ['--device-compressor'] + one_mix, a.limit)}
        print(json.dumps({'cli': out}), flush=True)
        out['host'] = _uq(a, path, ['--compressor', a.host_compressor] + one_mix, a.limit)
        print(json.dumps({'cli': out}), flush=True)
    finally:
        for p in (path, path + '.uQ'):
            if os.path.exists(p): os.remove(p)


def grid(a):
    path = _write_reads(a)
    try:
        print(json.dumps({'grid': dict(_uq(a, path, ['--device-compressor'], a.limit), reads=a.reads)}), flush=True)
    finally:
        for p in (path, path + '.uQ'):
            if os.path.exists(p): os.remove(p)


def ordering(a):
    """Host code only: the rows come from the C oracle's packer (what the tests compare the pack kernel with), the layouts from numpy."""
    import lzma
    import zlib
    import numpy as np
    sys.path.insert(0, os.path.join(HERE, 'oracle'))
    sys.path.insert(0, os.path.join(HERE, 'tests'))
    import oracle_c
    from uq_amd import analysis, ops, synth, uq
    for label, length in (('150bp', 150), ('36-301bp', (36, 301))):
        host = synth.fastq_array(synth.Spec(SEED, length), a.reads)
        ls = oracle_c.index_lines(host)
        st = oracle_c.stats(host, ls, 0, a.reads)
        d = analysis.decide_from_counts(st['counts'], st['len_min'], st['len_max'])
        dna, qual, _ = oracle_c.pack(host, ls, 0, a.reads, d['bases'], d['qualities'], d['N_qual'], d['bits_per_base'], d['bits_per_quality'],
                                     d['variable_read_lengths'], d['dna_bytes_per_row'], d['quality_bytes_per_row'])
        rows_out = []
        for name, T in (('DNA', dna), ('QUAL', qual)):
            for pat in uq.PATTERNS:
                r = np.rot90(T, int(pat[0]))
                B = uq.pattern_header(T.shape[0], T.shape[1], pat) + (np.ascontiguousarray(r) if pat.endswith('.1') else np.asfortranarray(r)).tobytes(order='A')
                rows_out.append({'table': name, 'pattern': pat, 'bytes': len(B), 'S': ops.deflate_size_host(B, level=a.level), 'zlib6': len(zlib.compress(B, 6)),
                                 'lzma': len(lzma.compress(B))})
        order = {name: {k: [r['pattern'] for r in sorted((r for r in rows_out if r['table'] == name), key=lambda r: (r[k], r['pattern']))]
                        for k in ('S', 'zlib6', 'lzma')} for name in ('DNA', 'QUAL')}
        print(json.dumps({'ordering': label, 'reads': a.reads, 'level': a.level, 'candidates': rows_out, 'order': order}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('step', choices=['kernel', 'cli', 'grid', 'ordering'])
    ap.add_argument('--reads', type=int)
    ap.add_argument('--length', type=int, default=150)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--dir', default='/dev/shm')
    ap.add_argument('--limit', type=int, default=900, help='seconds a child step may take')
    ap.add_argument('--host-compressor', default='gzip -1')
    ap.add_argument('--compress-lib', help='kernel: also time uq_bgzf_compress from this build of libuqhip.so')
    ap.add_argument('--level', type=int, choices=[1, 2], default=1, help='the compressor level (--bgzf-level)')
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--compress-only', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reads is None: a.reads = {'kernel': 10000000, 'cli': 1000000, 'grid': 10000000, 'ordering': 100000}[a.step]
    if a.step == 'kernel' and a.child: return kernel_child(a)
    {'kernel': kernel, 'cli': cli, 'grid': grid, 'ordering': ordering}[a.step](a)


if __name__ == '__main__':
    main()
