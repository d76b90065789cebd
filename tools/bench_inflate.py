#!/usr/bin/env python3
"""gzip input: the device inflate of BGZF members against the host zlib path, on bench.py's workload.

    python tools/bench_inflate.py [--reads 10000000] [--dir /dev/shm] [--reps 10] [--rocprof]

bench.py's reads (synth-v1, seed 20261005, 150 bp) are written as plain FASTQ and as BGZF at levels 1 and 6 (a 16-thread pool, bgzip's
65 280-byte members), plus the level-6 members without their BSIZE field (the same deflate data as a plain multi-member gzip, which
takes the host zlib path).  Then, each GPU step in a child process under its own time limit, stopping at the first failure:
  kernel   the compressed file read into HBM (timed), the member scan (timed), uq_inflate_members over --reps warm repetitions timed
           by events, the output compared with the plain file on the device;
  cli      `python -m uq_amd.uq` with UQ_TIMING=1 on every file: work_s (interpreter and device set-up excluded);
  rocprof  (--rocprof) the kernel step once more under `rocprofv3 --kernel-trace --stats`: the kernel's own time.
One JSON line.  Synthetic reads compress unlike real ones (random bases and qualities): the ratios here are not a real file's.
"""
import argparse
import glob
import json
import os
import shutil
import struct
import subprocess
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

SEED = 20261003 + 2          # bench.py's workload
CHUNK = 65280


def bgzf_member(chunk, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8)
    d = c.compress(chunk) + c.flush()
    return (b'\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00' + struct.pack('<H', 18 + len(d) + 8 - 1) + d +
            struct.pack('<II', zlib.crc32(chunk), len(chunk)))


def make(args):
    """Child step: the workload's files (generated on the device, compressed on 16 host threads)."""
    import numpy as np
    from uq_amd import ops, synth
    from uq_amd.device import Context
    ctx = Context(0)
    d = ops.synth_fastq(ctx, synth.Spec(SEED, args.length), 0, args.reads)
    data = d.cpu().numpy().tobytes()
    del d
    files = {'plain': os.path.join(args.dir, 'reads.fastq')}
    with open(files['plain'], 'wb') as f: f.write(data)
    mv = memoryview(data)
    out = {'fastq_bytes': len(data)}
    with ThreadPoolExecutor(16) as pool:
        for level in (1, 6):
            t0 = time.perf_counter()
            members = list(pool.map(lambda i: bgzf_member(mv[i:i + CHUNK], level), range(0, len(data), CHUNK)))
            dt = time.perf_counter() - t0
            name = 'bgzf%d' % level
            files[name] = os.path.join(args.dir, 'reads.l%d.fastq.gz' % level)
            with open(files[name], 'wb') as f:
                for m in members: f.write(m)
                f.write(bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000'))
            out[name + '_bytes'] = os.path.getsize(files[name])
            out[name + '_ratio'] = round(len(data) / out[name + '_bytes'], 3)
            out[name + '_compress_s_16_threads'] = round(dt, 2)
            if level == 6:
                files['gzip6'] = os.path.join(args.dir, 'reads.l6.nobsize.fastq.gz')
                with open(files['gzip6'], 'wb') as f:
                    for m in members: f.write(b'\x1f\x8b\x08\x00' + m[4:10] + m[18:])       # FEXTRA and the BC subfield dropped
    print(json.dumps({'make': out, 'files': files}))


def kernel(args):
    """Child step: read -> scan -> inflate (events over warm repetitions) -> compare with the plain file."""
    import numpy as np
    import torch
    from uq_amd import ops
    from uq_amd.device import Context
    from uq_amd.hostio import Staging
    ctx = Context(0)
    io = Staging(ctx)
    path = args.kernel
    io.file_to_device(path)                                              # pinned buffers allocated, page cache warm
    ctx.sync()
    t0 = time.perf_counter()
    d_comp = io.file_to_device(path)
    ctx.sync()
    t_read = time.perf_counter() - t0
    t0 = time.perf_counter()
    kind, members, total, _ = ops.gzip_scan(np.memmap(path, dtype=np.uint8, mode='r'))
    t_scan = time.perf_counter() - t0
    assert kind == ops.GZIP_BGZF
    d_members = ctx.to_device(members.view(np.uint8))
    out, bad = ops.inflate_members(ctx, d_comp, members, total, d_members)
    assert bad is None
    st = torch.zeros(len(members), dtype=torch.int32, device=ctx.device)
    from uq_amd._lib import call
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2):
        call('uq_inflate_members', ctx.h, ops._p(d_comp), d_comp.numel(), ops._p(d_members), len(members), ops._p(out), out.numel(), ops._p(st))
    e0.record()
    for _ in range(args.reps):
        call('uq_inflate_members', ctx.h, ops._p(d_comp), d_comp.numel(), ops._p(d_members), len(members), ops._p(out), out.numel(), ops._p(st))
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / args.reps
    ok = int(torch.count_nonzero(st)) == 0
    if args.plain:
        ok = ok and torch.equal(out, io.file_to_device(args.plain))
    print(json.dumps({'kernel': {'file': os.path.basename(path), 'comp_bytes': d_comp.numel(), 'members': len(members), 'out_bytes': total,
                                 'read_to_hbm_s': round(t_read, 4), 'scan_s': round(t_scan, 4), 'inflate_ms_events': round(ms, 3),
                                 'inflate_out_GBps': round(total / ms / 1e6, 1), 'reps': args.reps, 'output_equals_plain': bool(ok)}}))


def child(cmd, limit, env=None):
    r = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=HERE)
    if r.returncode != 0:
        print(json.dumps({'failed': ' '.join(cmd[-4:]), 'rc': r.returncode, 'stderr': r.stderr[-2000:]}))
        sys.exit(1)
    return r


def last_json(text, key):
    for line in reversed(text.strip().split('\n')):
        if line.startswith('{') and key in line:
            return json.loads(line)
    raise RuntimeError('no %s line in %r' % (key, text[-500:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=10_000_000)
    ap.add_argument('--length', type=int, default=150)
    ap.add_argument('--dir', default='/dev/shm')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rocprof', action='store_true')
    ap.add_argument('--make', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--kernel', help=argparse.SUPPRESS)
    ap.add_argument('--plain', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.make: return make(args)
    if args.kernel: return kernel(args)

    work = os.path.join(args.dir, 'uq_bench_inflate_%d' % os.getpid())
    os.makedirs(work)
    me = [sys.executable, os.path.abspath(__file__), '--reads', str(args.reads), '--length', str(args.length), '--dir', work]
    res = {'bench': 'inflate', 'workload': '%d x %d bp synth-v1 (seed %d), BGZF members of %d bytes; synthetic reads compress unlike real ones'
           % (args.reads, args.length, SEED, CHUNK)}
    try:
        m = last_json(child(me + ['--make'], 900).stdout, '"make"')
        files = m['files']
        res.update(m['make'])
        for name in ('bgzf1', 'bgzf6'):
            k = last_json(child(me + ['--kernel', files[name], '--plain', files['plain'], '--reps', str(args.reps)], 600).stdout, '"kernel"')
            res[name + '_kernel'] = k['kernel']
        env = dict(os.environ, UQ_TIMING='1')
        for name in ('plain', 'bgzf1', 'bgzf6', 'gzip6'):
            t0 = time.perf_counter()
            r = child([sys.executable, '-m', 'uq_amd.uq', '-i', files[name], '-o', os.path.join(work, 'out.uQ'), '--quiet'], 900, env)
            res[name + '_cli'] = {'work_s': last_json(r.stderr, 'uq_timing')['work_s'], 'wall_s': round(time.perf_counter() - t0, 2)}
        res['gpu_vs_host_zlib_bgzf6_work'] = round(res['gzip6_cli']['work_s'] / res['bgzf6_cli']['work_s'], 2)
        if args.rocprof:
            prof = os.path.join(work, 'prof')
            child(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', prof, '-o', 'inflate', '--'] + me +
                  ['--kernel', files['bgzf6'], '--reps', str(args.reps)], 600)
            for f in glob.glob(os.path.join(prof, '**', '*kernel_stats.csv'), recursive=True):
                import csv
                for row in csv.DictReader(open(f)):
                    if 'inflate_members_kernel' in row.get('Name', ''):
                        res['bgzf6_rocprof'] = {'calls': int(row['Calls']), 'avg_ms': round(float(row['AverageNs']) / 1e6, 3),
                                                'min_ms': round(float(row.get('MinNs', 0)) / 1e6, 3)}
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
