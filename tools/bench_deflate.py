#!/usr/bin/env python3
"""BGZF output: the device deflate (uq_bgzf_compress) against zlib on the host, on bench.py's workload.

    python tools/bench_deflate.py [--reads 10000000] [--dir /dev/shm] [--reps 10] [--rocprof] [--level {1,2}]

bench.py's reads (synth-v1, seed 20261005, 150 bp) are written as plain FASTQ and encoded to a .uQ container.  Then, each GPU step in a
child process under its own time limit, stopping at the first failure:
  ratio    (host) the compression ratio of zlib levels 1 and 6 on the same 65 280-byte blocks, 16 threads;
  kernel   the plain decode output in HBM, uq_bgzf_compress over --reps warm repetitions timed by events, the ratio, and the output inflated
           by uq_inflate_members on the device and compared with the plain decode;
  cli      `python -m uq_amd.uq --decode` with UQ_TIMING=1: work_s of the plain decode, of `--decode --bgzf`, and of `--decode` piped into a
           16-thread zlib level-1 BGZF writer (the host baseline; its wall time too);
  rocprof  (--rocprof) the kernel step once more under `rocprofv3 --kernel-trace --stats`: the kernel's own time.
--level: the compressor level of the kernel and CLI steps (`--bgzf-level`); the host baseline's zlib level is --host-level (1; DESIGN.md
section 18 compares level 2 with zlib level 6).  One JSON line.  Synthetic reads compress unlike real ones (random bases and qualities): the ratios here are not a real file's.
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
EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')


def bgzf_member(chunk, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8)
    d = c.compress(chunk) + c.flush()
    return (b'\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00' + struct.pack('<H', 18 + len(d) + 8 - 1) + d +
            struct.pack('<II', zlib.crc32(chunk), len(chunk)))


def make(args):
    """Child step: the plain FASTQ (generated on the device) and its .uQ container (the CLI)."""
    from uq_amd import ops, synth
    from uq_amd.device import Context
    ctx = Context(0)
    d = ops.synth_fastq(ctx, synth.Spec(SEED, args.length), 0, args.reads)
    plain = os.path.join(args.dir, 'reads.fastq')
    with open(plain, 'wb') as f: f.write(d.cpu().numpy().tobytes())
    print(json.dumps({'make': {'fastq_bytes': os.path.getsize(plain)}, 'plain': plain}))


def ratios(path):
    """zlib levels 1 and 6 on the 65 280-byte blocks of the file, 16 threads."""
    data = open(path, 'rb').read()
    mv = memoryview(data)
    out = {}
    with ThreadPoolExecutor(16) as pool:
        for level in (1, 6):
            t0 = time.perf_counter()
            size = sum(pool.map(lambda i: len(bgzf_member(mv[i:i + CHUNK], level)), range(0, len(data), CHUNK))) + len(EOF)
            out['zlib%d_ratio' % level] = round(len(data) / size, 4)
            out['zlib%d_s_16_threads' % level] = round(time.perf_counter() - t0, 2)
    return out


def kernel(args):
    """Child step: the plain decode in HBM -> uq_bgzf_compress (events over warm repetitions) -> uq_inflate_members = the plain decode."""
    import numpy as np
    import torch
    from uq_amd import ops
    from uq_amd.device import Context
    from uq_amd.hostio import Staging
    ctx = Context(0)
    d_text = Staging(ctx).file_to_device(args.kernel)
    blob = ops.bgzf_compress(ctx, d_text, level=args.level)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ops.bgzf_compress(ctx, d_text, level=args.level)
    e0.record()
    for _ in range(args.reps):
        ops.bgzf_compress(ctx, d_text, level=args.level)
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / args.reps
    kind, members, total, _ = ops.gzip_scan(blob.cpu().numpy())
    out, bad = ops.inflate_members(ctx, blob, members, total)
    ok = kind == ops.GZIP_BGZF and bad is None and torch.equal(out, d_text)
    print(json.dumps({'kernel': {'in_bytes': d_text.numel(), 'out_bytes': blob.numel(), 'ratio': round(d_text.numel() / blob.numel(), 4),
                                 'members': len(members), 'compress_ms_events': round(ms, 3), 'compress_in_GBps': round(d_text.numel() / ms / 1e6, 2),
                                 'reps': args.reps, 'level': args.level, 'device_inflate_equals_plain_decode': bool(ok)}}))


def writer(args):
    """Host baseline: stdin -> BGZF at zlib level --host-level on 16 threads -> file."""
    with open(args.bgzf_writer, 'wb') as f, ThreadPoolExecutor(16) as pool:
        inp = sys.stdin.buffer
        while True:
            buf = inp.read(CHUNK * 256)
            if not buf: break
            mv = memoryview(buf)
            for m in pool.map(lambda i: bgzf_member(mv[i:i + CHUNK], args.host_level), range(0, len(buf), CHUNK)):
                f.write(m)
        f.write(EOF)


def child(cmd, limit, env=None, shell=False):
    full = 'timeout -k 10 %d %s' % (limit, cmd) if shell else ['timeout', '-k', '10', str(limit)] + cmd
    r = subprocess.run(full, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=HERE, shell=shell)
    if r.returncode != 0:
        print(json.dumps({'failed': full if shell else ' '.join(cmd[-4:]), 'rc': r.returncode, 'stderr': r.stderr[-2000:]}))
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
    ap.add_argument('--level', type=int, choices=[1, 2], default=1)
    ap.add_argument('--host-level', type=int, default=1)
    ap.add_argument('--make', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--kernel', help=argparse.SUPPRESS)
    ap.add_argument('--bgzf-writer', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.make: return make(args)
    if args.kernel: return kernel(args)
    if args.bgzf_writer: return writer(args)

    work = os.path.join(args.dir, 'uq_bench_deflate_%d' % os.getpid())
    os.makedirs(work)
    me = [sys.executable, os.path.abspath(__file__), '--reads', str(args.reads), '--length', str(args.length), '--dir', work, '--level', str(args.level), '--host-level', str(args.host_level)]
    res = {'bench': 'deflate', 'level': args.level, 'host_zlib_level': args.host_level, 'workload': '%d x %d bp synth-v1 (seed %d), BGZF members of %d bytes; synthetic reads compress unlike real ones'
           % (args.reads, args.length, SEED, CHUNK)}
    try:
        m = last_json(child(me + ['--make'], 900).stdout, '"make"')
        res.update(m['make'])
        uq_file = os.path.join(work, 'reads.uQ')
        child([sys.executable, '-m', 'uq_amd.uq', '-i', m['plain'], '-o', uq_file, '--quiet'], 900)
        os.remove(m['plain'])
        env = dict(os.environ, UQ_TIMING='1')
        py = sys.executable
        plain = os.path.join(work, 'decoded.fastq')
        runs = {'decode': '%s -m uq_amd.uq -i %s --decode --quiet > %s' % (py, uq_file, plain),
                'decode_bgzf': '%s -m uq_amd.uq -i %s --decode --bgzf --bgzf-level %d --quiet > %s' % (py, uq_file, args.level, os.path.join(work, 'gpu.fastq.gz')),
                'decode_host_zlib1_16t': '%s -m uq_amd.uq -i %s --decode --quiet | %s %s --host-level %d --bgzf-writer %s' % (
                    py, uq_file, py, os.path.abspath(__file__), args.host_level, os.path.join(work, 'host.fastq.gz'))}
        for name, cmd in runs.items():
            t0 = time.perf_counter()
            r = child(cmd, 900, env, shell=True)
            res[name + '_cli'] = {'work_s': last_json(r.stderr, 'uq_timing')['work_s'], 'wall_s': round(time.perf_counter() - t0, 2)}
        res['gpu_bgzf_bytes'] = os.path.getsize(os.path.join(work, 'gpu.fastq.gz'))
        res['host_zlib1_bgzf_bytes'] = os.path.getsize(os.path.join(work, 'host.fastq.gz'))
        res['bgzf_vs_host_zlib1_wall'] = round(res['decode_host_zlib1_16t_cli']['wall_s'] / res['decode_bgzf_cli']['wall_s'], 2)
        res['bgzf_vs_host_zlib1_work'] = round(res['decode_host_zlib1_16t_cli']['work_s'] / res['decode_bgzf_cli']['work_s'], 2)
        res.update(ratios(plain))
        k = last_json(child(me + ['--kernel', plain, '--reps', str(args.reps)], 600).stdout, '"kernel"')
        res['kernel'] = k['kernel']
        if args.rocprof:
            prof = os.path.join(work, 'prof')
            child(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', prof, '-o', 'deflate', '--'] + me +
                  ['--kernel', plain, '--reps', str(args.reps)], 600)
            import csv
            for f in glob.glob(os.path.join(prof, '**', '*kernel_stats.csv'), recursive=True):
                for row in csv.DictReader(open(f)):
                    for kn in ('bgzf_deflate_kernel', 'bgzf_place_kernel'):
                        if kn in row.get('Name', ''):
                            res[kn + '_rocprof'] = {'calls': int(row['Calls']), 'avg_ms': round(float(row['AverageNs']) / 1e6, 3),
                                                    'total_ms': round(float(row.get('TotalDurationNs') or 0) / 1e6, 3)}
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
