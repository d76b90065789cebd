#!/usr/bin/env python3
"""BGZF-compressed containers (`--gz`): sizes, the parts entry against what it replaces, the CLI both ways, the host routes.

    python tools/bench_container.py [--reads 10000000] [--binned-reads 2000000] [--dir /dev/shm] [--reps 5] [--skip-gzip6] [--level {1,2}]

Two corpora, each encoded with all tables raw: bench.py's reads (synth-v1, 150 bp) and the `binned_fastq` corpus of tools/bench_inflate.py,
whose ratios are the realistic ones.  Every GPU step runs in a child process under its own time limit; the first failure stops the run.
  make     the FASTQ files (synth-v1 on the device, binned on the host);
  cli      UQ_TIMING work_s of: encode plain / --gz, decode from plain / --gz / `gzip -6` (one member); the best of --reps runs each;
  kernel   per member: bytes as written by --gz, and zlib levels 1 and 6 over the same 65 280-byte blocks; uq_bgzf_compress_parts (events)
           against the sum over the members of a device header || payload copy + uq_bgzf_compress; uq_inflate_members (events) on the
           --gz file;
  verdicts one PASS / FAIL per bar of DESIGN.md section 17 (in the JSON under "verdicts", and on stderr as the run goes);
  host     the routes a user takes without --gz: the plain encode, then a 16-thread zlib level-1 BGZF writer over the tar; 16 threads of
           zlib over the BGZF members into a file in --dir, then the plain decode.
--level: the compressor level of --gz and of the kernel step (`--bgzf-level`).  One JSON line.
"""
import argparse
import json
import os
import struct
import subprocess
import sys
import tarfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'tools'))

SEED = 20261003 + 2          # bench.py's workload
CHUNK = 65280
EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')
RAW = ['--raw', 'DNA', 'QUAL', 'QNAME']


def bgzf_member(chunk, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8)
    d = c.compress(chunk) + c.flush()
    return (b'\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00' + struct.pack('<H', 18 + len(d) + 8 - 1) + d +
            struct.pack('<II', zlib.crc32(chunk), len(chunk)))


def make(args):
    from bench_inflate import binned_fastq
    from uq_amd import ops, synth
    from uq_amd.device import Context
    ctx = Context(0)
    d = ops.synth_fastq(ctx, synth.Spec(SEED, args.length), 0, args.reads)
    with open(os.path.join(args.dir, 'synth.fastq'), 'wb') as f: f.write(d.cpu().numpy().tobytes())
    with open(os.path.join(args.dir, 'binned.fastq'), 'wb') as f: f.write(binned_fastq(args.binned_reads, 20261016, length=args.length))
    print(json.dumps({'make': {c: os.path.getsize(os.path.join(args.dir, c + '.fastq')) for c in ('synth', 'binned')}}))


def tar_members(path):
    """[(name, .npy header length, payload offset, payload bytes)] of a plain container."""
    import numpy as np
    out = []
    with tarfile.open(path, 'r:') as t, open(path, 'rb') as f:
        for m in t.getmembers():
            hdr = 0
            if m.name != 'config.json':
                f.seek(m.offset_data)
                np.lib.format.read_magic(f); np.lib.format.read_array_header_1_0(f)
                hdr = f.tell() - m.offset_data
            out.append((m.name, hdr, m.offset_data + hdr, m.size - hdr))
    return out


def kernel(args):
    import numpy as np
    import torch
    from uq_amd import ops
    from uq_amd.device import Context
    from uq_amd.hostio import Staging
    ctx = Context(0)
    plain, gz = args.kernel, args.kernel + '.gz'
    tar = np.memmap(plain, dtype=np.uint8, mode='r')
    d_tar = Staging(ctx).file_to_device(plain)
    parts, names = [], []
    for name, hdr, off, n in tar_members(plain):
        parts.append((tar[off - hdr:off].tobytes(), d_tar[off:off + n].clone())); names.append(name)
    del d_tar
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        fn()
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(args.reps): fn()
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / args.reps

    # both sides into one preallocated output, through the library's entries: only the device work and its host round trips are timed
    import ctypes as C
    from uq_amd._lib import call
    blob, sizes = ops.bgzf_compress_parts(ctx, parts, level=args.level)
    flags = ops.bgzf_level_flags(args.level)
    arr, keep = ops._bgzf_parts_arg(parts)
    out = torch.empty(ops.bgzf_parts_bound(parts), dtype=torch.uint8, device=ctx.device)
    ps, nout = (C.c_uint64 * len(parts))(), C.c_uint64()
    ptr = lambda t_: C.c_void_p(t_.data_ptr())

    def by_parts():
        call('uq_bgzf_compress_parts', ctx.h, arr, len(parts), ptr(out), out.numel(), ps, C.byref(nout), flags)
    by_parts()
    same = nout.value == blob.numel() and torch.equal(out[:nout.value], blob)
    # what it replaces: per member, a device-side header || payload copy, then uq_bgzf_compress on it (headers uploaded beforehand)
    d_hdr = [ctx.bytes_to_device(h) if h else None for h, _ in parts]
    cat = torch.empty(max(len(h) + d.numel() for h, d in parts), dtype=torch.uint8, device=ctx.device)

    def per_member():
        total = 0
        for (h, d), dh in zip(parts, d_hdr):
            n = len(h) + d.numel()
            if dh is not None: cat[:len(h)].copy_(dh)
            cat[len(h):n].copy_(d)
            call('uq_bgzf_compress', ctx.h, ptr(cat), n, ptr(out[total:]), out.numel() - total, C.byref(nout), flags)
            total += nout.value
        return total
    same = same and per_member() == blob.numel() and torch.equal(out[:blob.numel()], blob)
    # alternating, the best of each
    parts_ms = member_ms = None
    for _ in range(3):
        a_ms, b_ms = timed(by_parts), timed(per_member)
        parts_ms = a_ms if parts_ms is None else min(parts_ms, a_ms)
        member_ms = b_ms if member_ms is None else min(member_ms, b_ms)
    del out, cat
    del blob
    members = {}
    with ThreadPoolExecutor(16) as pool:
        for name, (h, d), size in zip(names, parts, sizes):
            whole = h + d.cpu().numpy().tobytes()
            mv = memoryview(whole)
            row = {'bytes': len(whole), 'gz_bytes': size, 'ratio': round(len(whole) / max(size, 1), 4)}
            for level in (1, 6):
                row['zlib%d_bytes' % level] = sum(pool.map(lambda i: len(bgzf_member(mv[i:i + CHUNK], level)), range(0, len(whole), CHUNK)))
            members[name] = row
    del parts
    d_comp = Staging(ctx).file_to_device(gz)
    kind, m, total, _ = ops.gzip_scan(np.memmap(gz, dtype=np.uint8, mode='r'))
    d_m = ctx.to_device(np.ascontiguousarray(m).view(np.uint8))
    out, bad = ops.inflate_members(ctx, d_comp, m, total, d_members=d_m)
    # the two files come from two encode runs: their tar headers differ in mtime, so the members are compared, not the stream
    host_out = out.cpu().numpy()
    ok = kind == ops.GZIP_BGZF and bad is None and total == tar.size and all(
        np.array_equal(host_out[off - hdr:off + n], tar[off - hdr:off + n]) for _, hdr, off, n in tar_members(plain))
    del host_out
    del out
    inflate_ms = timed(lambda: ops.inflate_members(ctx, d_comp, m, total, d_members=d_m))
    print(json.dumps({'kernel': {'members': members, 'tar_bytes': int(tar.size), 'gz_file_bytes': os.path.getsize(gz),
                                 'parts_ms_events': round(parts_ms, 3), 'per_member_copy_and_compress_ms_events': round(member_ms, 3),
                                 'parts_over_per_member': round(parts_ms / member_ms, 4), 'same_bytes': bool(same),
                                 'inflate_members_ms_events': round(inflate_ms, 3), 'gz_members': len(m),
                                 'device_inflate_equals_tar_members': bool(ok), 'reps': args.reps, 'level': args.level}}))


def bgzf_write(src, dst):
    """The host route of the encoder: the tar -> BGZF level 1 on 16 threads -> file.  Seconds."""
    t0 = time.perf_counter()
    with open(src, 'rb') as inp, open(dst, 'wb') as f, ThreadPoolExecutor(16) as pool:
        while True:
            buf = inp.read(CHUNK * 256)
            if not buf: break
            mv = memoryview(buf)
            for m in pool.map(lambda i: bgzf_member(mv[i:i + CHUNK], 1), range(0, len(buf), CHUNK)): f.write(m)
        f.write(EOF)
    return time.perf_counter() - t0


def bgzf_read(src, dst):
    """The host route of the decoder: the BGZF members inflated by zlib on 16 threads into a file.  Seconds."""
    import numpy as np
    from uq_amd import ops
    t0 = time.perf_counter()
    comp = np.memmap(src, dtype=np.uint8, mode='r')
    kind, m, total, _ = ops.gzip_scan(comp)
    assert kind == ops.GZIP_BGZF
    spans = [(int(a), int(b)) for a, b in zip(m['data_offset'], m['comp_bytes'])]
    with open(dst, 'wb') as f, ThreadPoolExecutor(16) as pool:
        for lo in range(0, len(spans), 1024):
            for b in pool.map(lambda s: zlib.decompress(comp[s[0]:s[0] + s[1]], -15), spans[lo:lo + 1024]): f.write(b)
    return time.perf_counter() - t0


def progress(what):
    print('step: ' + what, file=sys.stderr, flush=True)


def child(cmd, limit, env=None):
    progress(' '.join(cmd[-5:]))
    r = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=HERE)
    if r.returncode != 0:
        print(json.dumps({'failed': ' '.join(cmd[-6:]), 'rc': r.returncode, 'stderr': r.stderr[-2000:], 'stdout': r.stdout[-500:]}))
        sys.exit(1)
    return r


def last_json(text, key):
    for line in reversed(text.strip().split('\n')):
        if line.startswith('{') and key in line: return json.loads(line)
    raise RuntimeError('no %s line in %r' % (key, text[-500:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=10_000_000)
    ap.add_argument('--binned-reads', type=int, default=2_000_000)
    ap.add_argument('--length', type=int, default=150)
    ap.add_argument('--dir', default='/dev/shm')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip-gzip6', action='store_true')
    ap.add_argument('--level', type=int, choices=[1, 2], default=1)
    ap.add_argument('--make', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--kernel', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.make: return make(args)
    if args.kernel: return kernel(args)
    me = [sys.executable, os.path.abspath(__file__), '--reads', str(args.reads), '--binned-reads', str(args.binned_reads), '--length',
          str(args.length), '--dir', args.dir, '--reps', str(args.reps), '--level', str(args.level)]
    env = dict(os.environ, UQ_TIMING='1', PYTHONPATH=HERE)
    result = last_json(child(me + ['--make'], 300).stdout, 'make')

    def cli(argv):
        best = None
        for _ in range(max(args.reps, 1)):
            w = last_json(child([sys.executable, '-m', 'uq_amd.uq', '--quiet'] + argv, 300, env=env).stderr, 'uq_timing')['work_s']
            best = w if best is None else min(best, w)
        return best
    made = []
    try:
        for corpus in ('synth', 'binned'):
            p = lambda ext: os.path.join(args.dir, corpus + ext)
            made += [p(e) for e in ('.fastq', '.uQ', '.uQ.gz', '.gzip6.uQ.gz', '.host.uQ.gz', '.host.uQ', '.out.fastq')]
            r = {}
            r['encode_plain_work_s'] = cli(['-i', p('.fastq'), '-o', p('.uQ')] + RAW)
            r['encode_gz_work_s'] = cli(['-i', p('.fastq'), '-o', p('.uQ.gz'), '--gz', '--bgzf-level', str(args.level)] + RAW)
            r.update(last_json(child(me + ['--kernel', p('.uQ')], 600).stdout, 'kernel')['kernel'])
            # the decoder writes to stdout: into a file in --dir
            def decode(src):
                best = None
                for _ in range(max(args.reps, 1)):
                    progress('decode ' + src)
                    with open(p('.out.fastq'), 'wb') as f:
                        q = subprocess.run(['timeout', '-k', '10', '300', sys.executable, '-m', 'uq_amd.uq', '--quiet', '-i', src, '--decode'],
                                           stdout=f, stderr=subprocess.PIPE, text=True, env=env, cwd=HERE)
                    if q.returncode != 0:
                        print(json.dumps({'failed': 'decode ' + src, 'rc': q.returncode, 'stderr': q.stderr[-2000:]})); sys.exit(1)
                    w = last_json(q.stderr, 'uq_timing')['work_s']
                    best = w if best is None else min(best, w)
                return best
            r['decode_plain_work_s'] = decode(p('.uQ'))
            r['decode_gz_work_s'] = decode(p('.uQ.gz'))
            if not args.skip_gzip6:
                progress('gzip -6 of ' + p('.uQ'))
                t0 = time.perf_counter()
                c = zlib.compressobj(6, zlib.DEFLATED, 31)
                with open(p('.uQ'), 'rb') as f, open(p('.gzip6.uQ.gz'), 'wb') as g:
                    while True:
                        buf = f.read(8 << 20)
                        if not buf: break
                        g.write(c.compress(buf))
                    g.write(c.flush())
                r['gzip6_host_s_one_thread'] = round(time.perf_counter() - t0, 2)
                r['gzip6_bytes'] = os.path.getsize(p('.gzip6.uQ.gz'))
                r['decode_gzip6_work_s'] = decode(p('.gzip6.uQ.gz'))
            # host routes
            progress('host routes')
            r['host_bgzf_writer_s_16_threads'] = round(min(bgzf_write(p('.uQ'), p('.host.uQ.gz')) for _ in range(2)), 3)
            r['host_bgzf_writer_bytes'] = os.path.getsize(p('.host.uQ.gz'))
            r['host_bgzf_reader_s_16_threads'] = round(min(bgzf_read(p('.uQ.gz'), p('.host.uQ')) for _ in range(2)), 3)
            r['encode_host_route_s'] = round(r['encode_plain_work_s'] + r['host_bgzf_writer_s_16_threads'], 3)
            r['decode_host_route_s'] = round(r['decode_plain_work_s'] + r['host_bgzf_reader_s_16_threads'], 3)
            r['encode_gz_bar_s'] = round(1.25 * (r['encode_plain_work_s'] + r['parts_ms_events'] / 1e3), 3)
            r['decode_gz_bar_s'] = round(r['decode_plain_work_s'] + 1.25 * r['inflate_members_ms_events'] / 1e3, 3)
            r['encode_host_route_over_gz'] = round(r['encode_host_route_s'] / r['encode_gz_work_s'], 3)
            r['decode_host_route_over_gz'] = round(r['decode_host_route_s'] / r['decode_gz_work_s'], 3)
            # the bars of DESIGN.md section 17, each with its verdict
            r['verdicts'] = {
                'parts_not_slower_than_per_member': r['parts_over_per_member'] <= 1.0,
                'encode_gz_within_1.25x_of_plain_plus_parts': r['encode_gz_work_s'] <= r['encode_gz_bar_s'],
                'encode_gz_beats_host_route': r['encode_gz_work_s'] < r['encode_host_route_s'],
                'decode_gz_within_plain_plus_1.25x_inflate': r['decode_gz_work_s'] <= r['decode_gz_bar_s'],
                'decode_gz_beats_host_route (reported, no bar)': r['decode_gz_work_s'] < r['decode_host_route_s']}
            for k, v in r['verdicts'].items(): progress('%s %s: %s' % (corpus, k, 'PASS' if v else 'FAIL'))
            result[corpus] = r
    finally:
        for f in made:
            if os.path.exists(f): os.remove(f)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
