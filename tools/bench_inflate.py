#!/usr/bin/env python3
"""gzip input: the device inflate of BGZF members against the host zlib path, on bench.py's workload.

    python tools/bench_inflate.py [--reads 10000000] [--dir /dev/shm] [--reps 10] [--rocprof]

bench.py's reads (synth-v1, seed 20261005, 150 bp) are written as plain FASTQ and as BGZF at levels 1 and 6 (a 16-thread pool, bgzip's
65 280-byte members), plus the level-6 members without their BSIZE field (the same deflate data as a plain multi-member gzip, which
was the host zlib path's file and now takes the chunked device path), a true single-member level-6 file written the way pigz writes one
(16 threads deflate 128 KiB pieces, each with the previous 32 KiB as its dictionary, Z_SYNC_FLUSH between them: real cross-piece
back-references), and a plain single-threaded gzip.compress stream of the first --slice bytes (dynamic headers with no empty stored
blocks to help the finder).  Because synth-v1's random qualities compress only 1.9x, the same number of reads is also written with
Illumina-style names and binned qualities (binned_fastq: level 6 gives about 4x, like a real run) as a pigz-style member.  Then, each GPU step in a child process under its own time limit, stopping at the first failure:
  kernel   the compressed file read into HBM (timed), the member scan (timed), uq_inflate_members over --reps warm repetitions timed
           by events, the output compared with the plain file on the device;
  stream   the chunked inflate (uq_gzip_stream_*) of the single-member and slice files: one warm run, then --reps timed by events; the
           finder / decode / finish times, chunks, rounds and re-decodes it reports; the output compared with the plain file;
  cli      `python -m uq_amd.uq` with UQ_TIMING=1 on every file: work_s (interpreter and device set-up excluded); the single-member file
           also with --host-inflate (host zlib);
  rocprof  (--rocprof) the kernel and stream steps once more under `rocprofv3 --kernel-trace --stats`: the kernels' own times.
One JSON line.  Synthetic reads compress unlike real ones (random bases and qualities): the ratios here are not a real file's.
"""
import argparse
import glob
import gzip
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
    t0 = time.perf_counter()
    parts = pigz_member(data, 6)
    out['single6_compress_s_16_threads'] = round(time.perf_counter() - t0, 2)
    files['single6'] = os.path.join(args.dir, 'reads.l6.single.fastq.gz')
    with open(files['single6'], 'wb') as f:
        for p in parts: f.write(p)
    del parts
    out['single6_bytes'] = os.path.getsize(files['single6'])
    out['single6_ratio'] = round(len(data) / out['single6_bytes'], 3)
    binned = binned_fastq(args.reads, SEED)
    files['binned'] = os.path.join(args.dir, 'reads.binned.fastq')
    with open(files['binned'], 'wb') as f: f.write(binned)
    parts = pigz_member(binned, 6)
    files['binned6'] = os.path.join(args.dir, 'reads.binned.l6.single.fastq.gz')
    with open(files['binned6'], 'wb') as f:
        for p in parts: f.write(p)
    del parts
    out['binned_fastq_bytes'] = len(binned)
    out['binned6_bytes'] = os.path.getsize(files['binned6'])
    out['binned6_ratio'] = round(len(binned) / out['binned6_bytes'], 3)
    del binned
    sl = bytes(mv[:min(len(data), args.slice)])
    files['slice6'] = os.path.join(args.dir, 'reads.slice.l6.fastq.gz')
    with open(files['slice6'], 'wb') as f: f.write(gzip.compress(sl, 6))
    out['slice6_in_bytes'] = len(sl)
    out['slice6_bytes'] = os.path.getsize(files['slice6'])
    print(json.dumps({'make': out, 'files': files}))


def binned_fastq(n, seed, p_other=0.15, length=150):
    """FASTQ that compresses like a real run's: Illumina-style names, uniform random bases, qualities binned to four values (mostly 'F',
    the others with probability p_other, in runs), so that level 6 gives a ratio of about 3.5 - 5 where synth-v1's random qualities give 1.9."""
    import numpy as np
    rng = np.random.default_rng(seed)
    name = b'@SIM:7:HXY2KDSXX:1:'
    w = len(name) + 15
    rec = np.empty((n, w + 1 + length + 3 + length + 1), dtype=np.uint8)
    rec[:, :len(name)] = np.frombuffer(name, dtype=np.uint8)
    idx = np.arange(n, dtype=np.int64)
    tile, x, y = 1101 + idx // 1000000 % 100, idx * 7 % 32000, idx * 13 % 36000
    for col, (val, nd) in enumerate(((tile, 4), (x, 5), (y, 5))):
        base = len(name) + [0, 5, 11][col]
        for d in range(nd):
            rec[:, base + d] = 48 + (val // 10 ** (nd - 1 - d)) % 10
        if col < 2: rec[:, base + nd] = ord(':')
    rec[:, w] = 10
    rec[:, w + 1:w + 1 + length] = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, (n, length))]
    q0 = w + 1 + length
    rec[:, q0:q0 + 3] = np.frombuffer(b'\n+\n', dtype=np.uint8)
    q = np.full((n, length), ord('F'), dtype=np.uint8)
    flip = rng.random((n, length)) < p_other / 3
    run = flip | np.roll(flip, 1, axis=1) | np.roll(flip, 2, axis=1)
    q[run] = np.frombuffer(b',:#', dtype=np.uint8)[rng.integers(0, 3, int(run.sum()))]
    rec[:, q0 + 3:q0 + 3 + length] = q
    rec[:, -1] = 10
    return rec.tobytes()


def pigz_member(data, level, piece=128 << 10, threads=16):
    """One gzip member the way pigz writes it: pieces deflated in parallel, each primed with the previous 32 KiB, joined by Z_SYNC_FLUSH."""
    mv = memoryview(data)

    def one(i):
        kw = {'zdict': bytes(mv[max(0, i - 32768):i])} if i else {}
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, **kw)
        return c.compress(mv[i:i + piece]) + c.flush(zlib.Z_SYNC_FLUSH if i + piece < len(data) else zlib.Z_FINISH)
    with ThreadPoolExecutor(threads) as pool:
        body = list(pool.map(one, range(0, len(data), piece)))
    return [b'\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03'] + body + [struct.pack('<II', zlib.crc32(data), len(data) & 0xFFFFFFFF)]


def stream(args):
    """Child step: the chunked device inflate of a non-BGZF file: warm run, then --reps timed by events; compared with the plain file."""
    import torch
    from uq_amd import ops, uq
    from uq_amd.device import Context
    from uq_amd.hostio import Staging
    ctx = Context(0)
    io = Staging(ctx)
    d_comp = io.file_to_device(args.stream)
    chunk = args.chunk or uq.GZIP_STREAM_CHUNK
    out, info = ops.gzip_stream_to_device(ctx, d_comp, chunk)
    ok = True
    if args.plain:
        ref = io.file_to_device(args.plain)
        # the slice file holds a prefix of the plain file; the others all of it
        ok = (args.prefix or out.numel() == ref.numel()) and out.numel() <= ref.numel() and torch.equal(out, ref[:out.numel()])
        del ref
    del out
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    infos = []
    for _ in range(args.reps):
        o, i2 = ops.gzip_stream_to_device(ctx, d_comp, chunk)
        infos.append(i2)
        del o
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / args.reps
    med = lambda k: round(sorted(i[k] for i in infos)[len(infos) // 2], 2)
    print(json.dumps({'stream': {'file': os.path.basename(args.stream), 'comp_bytes': d_comp.numel(), 'out_bytes': info['out_bytes'],
                                 'chunk_bytes': chunk, 'chunks': info['chunks'], 'starts': info['starts'], 'rounds': info['rounds'],
                                 'redecoded': info['redecoded'], 'overflows': info['overflows'], 'resolve_rounds': info['resolve_rounds'],
                                 'find_ms': med('find_ms'), 'decode_ms': med('decode_ms'), 'finish_ms': med('finish_ms'),
                                 'total_ms_events': round(ms, 2), 'out_GBps': round(info['out_bytes'] / ms / 1e6, 2), 'reps': args.reps,
                                 'output_equals_plain': bool(ok)}}))


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
    ap.add_argument('--slice', type=int, default=256 << 20, help='bytes of the plain gzip.compress stream')
    ap.add_argument('--chunk', type=int, default=0, help='chunk bytes of the device path (default: uq.GZIP_STREAM_CHUNK)')
    ap.add_argument('--plain', help=argparse.SUPPRESS)
    ap.add_argument('--stream', help=argparse.SUPPRESS)
    ap.add_argument('--prefix', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--skip-bgzf', action='store_true', help='only the non-BGZF files (stream step and CLI)')
    args = ap.parse_args()
    if args.make: return make(args)
    if args.kernel: return kernel(args)
    if args.stream: return stream(args)

    work = os.path.join(args.dir, 'uq_bench_inflate_%d' % os.getpid())
    os.makedirs(work)
    me = [sys.executable, os.path.abspath(__file__), '--reads', str(args.reads), '--length', str(args.length), '--dir', work,
          '--slice', str(args.slice), '--chunk', str(args.chunk)]
    res = {'bench': 'inflate', 'workload': '%d x %d bp synth-v1 (seed %d), BGZF members of %d bytes; synthetic reads compress unlike real ones'
           % (args.reads, args.length, SEED, CHUNK)}
    try:
        m = last_json(child(me + ['--make'], 900).stdout, '"make"')
        files = m['files']
        res.update(m['make'])
        for name, plain in (('single6', 'plain'), ('binned6', 'binned'), ('slice6', 'plain')):
            k = last_json(child(me + ['--stream', files[name], '--plain', files[plain], '--reps', str(args.reps)] + (['--prefix'] if name == 'slice6' else []),
                                600).stdout, '"stream"')
            res[name + '_stream'] = k['stream']
        for name in () if args.skip_bgzf else ('bgzf1', 'bgzf6'):
            k = last_json(child(me + ['--kernel', files[name], '--plain', files['plain'], '--reps', str(args.reps)], 600).stdout, '"kernel"')
            res[name + '_kernel'] = k['kernel']
        env = dict(os.environ, UQ_TIMING='1')
        runs = [('plain', []), ('gzip6', []), ('single6', []), ('single6_host_inflate', ['--host-inflate']), ('binned', []), ('binned6', []),
                ('binned6_host_inflate', ['--host-inflate'])]
        if not args.skip_bgzf: runs[1:1] = [('bgzf1', []), ('bgzf6', [])]
        for name, flags in runs:
            t0 = time.perf_counter()
            r = child([sys.executable, '-m', 'uq_amd.uq', '-i', files[name.split('_')[0]], '-o', os.path.join(work, 'out.uQ'), '--quiet'] + flags,
                      900, env)
            res[name + '_cli'] = {'work_s': last_json(r.stderr, 'uq_timing')['work_s'], 'wall_s': round(time.perf_counter() - t0, 2)}
        if not args.skip_bgzf:
            res['gpu_bgzf6_vs_device_gzip6_work'] = round(res['gzip6_cli']['work_s'] / res['bgzf6_cli']['work_s'], 2)
        res['single6_device_vs_host_inflate_work'] = round(res['single6_host_inflate_cli']['work_s'] / res['single6_cli']['work_s'], 2)
        res['binned6_device_vs_host_inflate_work'] = round(res['binned6_host_inflate_cli']['work_s'] / res['binned6_cli']['work_s'], 2)
        if args.rocprof:
            prof = os.path.join(work, 'prof')
            steps = [('single6', ['--stream', files['single6'], '--reps', '3'])]
            if not args.skip_bgzf: steps.insert(0, ('bgzf6', ['--kernel', files['bgzf6'], '--reps', str(args.reps)]))
            for name, step in steps:
                child(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', prof + name, '-o', 'inflate', '--'] + me + step, 600)
                for f in glob.glob(os.path.join(prof + name, '**', '*kernel_stats.csv'), recursive=True):
                    import csv
                    for row in csv.DictReader(open(f)):
                        kn = row.get('Name', '')
                        for key in ('inflate_members_kernel', 'gzs_find_kernel', 'gzs_decode_kernel', 'gzs_compact_kernel', 'gzs_resolve_kernel',
                                    'gzs_crc_pieces_kernel', 'gzs_crc_members_kernel'):
                            if key in kn:
                                res['%s_rocprof_%s' % (name, key)] = {'calls': int(row['Calls']), 'avg_ms': round(float(row['AverageNs']) / 1e6, 3),
                                                                      'min_ms': round(float(row.get('MinNs', 0)) / 1e6, 3)}
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
