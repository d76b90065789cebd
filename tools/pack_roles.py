#!/usr/bin/env python3
"""Where a tile's time goes in the fused pack + statistics + QNAME kernel, per role: the bench step's pack call alone (as tools/packkernel_time.py
runs it) with a library whose pack.hip was built with -DPK_ROLE_CLOCK:
    tools/variants.sh pack.hip clock -DPK_ROLE_CLOCK
    UQ_LIB_PATH=uq_amd/_variants/libuqhip_clock.so python tools/pack_roles.py [reads] [noqn]
Every wave sums, over its tiles, the cycles from barrier 1 to its arrival at barrier 2 (phase B: the packing or the parsing, with the request for the
next tile), its wait at barrier 2, its wait for the next tile's bytes, the copy-out (C), and from there to behind the next tile's barrier 1 (A).  Printed
per tile and role, in cycles and in microseconds (the counter's rate is taken from the kernel's own duration by the stream's events)."""
import ctypes as C
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from uq_amd import _lib, ops, synth
from uq_amd.device import Context, SideContext

lib = C.CDLL(_lib.LIB_PATH)
if not hasattr(lib, 'uq_pack_role_clock'):
    sys.exit('%s was not built with -DPK_ROLE_CLOCK' % _lib.LIB_PATH)
ctx = Context(0)
side = SideContext(ctx)
n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10_000_000
qn = 'noqn' not in sys.argv
d_buf = ops.synth_fastq(ctx, synth.Spec(20261005, 150), 0, n)
nbytes = d_buf.numel()
RUNS, WARM = 10, 2
ms = []
out = (C.c_ulonglong * 16)()
for it in range(RUNS):
    st = ops.stats_new(ctx)
    census = ops.ChunkedCensus(ctx, d_buf); census.chunk(0, nbytes); census.end_async()
    guess, rpb = ops.head_guess(side, d_buf, notricks=False, head_bytes=ops.HEAD_BYTES_SMALL, head_reads=ops.HEAD_READS_INDEXED)
    cap = int(nbytes * rpb * 1.02) + 1024
    guess.avg_record_bytes = int(1.0 / rpb)
    fq = None
    if qn:
        fq = ops.FusedQname(ctx, cap); ops.qname_guess_async(ctx, d_buf, None, fq)
    if it == WARM:
        torch.cuda.synchronize()
        assert lib.uq_pack_role_clock(None, 1) == 0
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(); sp = ops.pack_stats_async(ctx, d_buf, None, cap, guess, st=st, fq=fq); e1.record()
    census.wait(); torch.cuda.synchronize()
    if it >= WARM: ms.append(e0.elapsed_time(e1))
    del sp, fq, st
assert lib.uq_pack_role_clock(out, 0) == 0
launches = RUNS - WARM
call_ms = sum(ms) / len(ms)
names = ['A + barrier 1', 'B (work)', 'wait at barrier 2', 'wait for next tile', 'C (copy-out)']
try: print('tile geometry:', ops.pack_tile_geometry(guess, stats=True, qname=qn, lists=True))
except AttributeError: print('tile geometry: not reported (a library from before uq_pack_tile_geometry)')
print('%s: %d reads, pack + statistics%s call %.4f ms (min %.4f) over %d launches' % (os.path.basename(_lib.LIB_PATH), n, ' + QNAME' if qn else '', call_ms, min(ms), launches))
# a wave's five sums add up to its whole tile loop, which is the launch but for its prologue and epilogue: cycles per microsecond from that
pack_total = sum(out[k] for k in range(5)) / max(out[6], 1)
rate = pack_total / (call_ms * 1e3)
print('counter: %.0f cycles per wave and launch, ~%.0f cycles per microsecond of the call' % (pack_total, rate))
for role, base in (('pack waves', 0), ('parser wave', 8)):
    tiles, waves = out[base + 5], out[base + 6]
    if not tiles: continue
    tot = sum(out[base + k] for k in range(5))
    print('%s: %d waves and %d wave-tiles per launch, %.0f cycles (%.2f us) per tile' % (role, waves // launches, tiles // launches, tot / tiles, tot / tiles / rate))
    for k in range(5):
        print('    %-20s %8.0f cycles  %6.2f us  %5.1f %%' % (names[k], out[base + k] / tiles, out[base + k] / tiles / rate, 100.0 * out[base + k] / tot))
