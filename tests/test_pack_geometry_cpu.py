"""The pack kernels' tile geometry (uq_amd/csrc/pack_geometry.h) through the library's query, ops.pack_tile_geometry -- no GPU:
the flagship's parameters get the 64-read tile at three lanes a read and four workgroups per CU; where 64 reads do not fit (the 36 - 301 bp
workloads, a longer record) the geometry is what it was, i.e. what tests/test_gpu_pack_roles.py's tile_reads() restates; and over a sweep of record
lengths, row sizes, average records and kernel forms every geometry keeps what the kernel relies on.  The same sweep runs once more in a stand-alone
program (tools/pack_geometry_check.cpp) under the address and undefined-behaviour sanitizers.

(On the sweep's stage bound: a tile sized from the AVERAGE record holds R records of the longest kind only by luck -- that is what the pieces of Rs
reads are for, and the 36 - 301 bp geometries this file pins have R x longest > stage.  So the bound is asserted for Rs at every point, and for R
wherever R is not taken from an average: the 64-read tile, and every point with the average unknown or equal to the longest.)"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_gpu_pack_roles import decide, tile_reads
from uq_amd import ops, synth
from uq_amd._lib import PackParams

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024
FORMS = [dict(stats=False), dict(stats=True), dict(stats=True, qname=True), dict(stats=True, lists=True), dict(stats=True, qname=True, lists=True)]


def flagship_params(n=8192):
    """What the benchmark's head guess gives the pack kernel: 150 bp, "synth-v1" seed 20261005, decided from the first reads."""
    host = synth.fastq_array(synth.Spec(20261003 + 2, 150), n)
    return decide(host, n)[3]


def test_flagship_gets_64_reads_three_lanes_four_workgroups():
    p = flagship_params()
    assert (p.bits_per_base, p.bits_per_quality, p.dna_bytes_per_row, p.quality_bytes_per_row, p.variable) == (2, 6, 38, 113, 0)
    g = ops.pack_tile_geometry(p, stats=True, qname=True, lists=True)           # the step's kernel
    assert g.tiled and g.tile64
    assert (g.R, g.Rs, g.P, g.G, g.wg_per_cu, g.copies) == (64, 64, 3, 19, 4, 4)
    assert g.stage_bytes == 22 * 1024 + 32 and g.lds_bytes == 40192 and g.lds_bytes <= LDS_PER_CU // 4
    assert 64 * p.max_record_bytes + 47 <= g.stage_bytes
    gi = ops.pack_tile_geometry(p, stats=True, qname=True)                       # the indexed form with the QNAME phase: the same tile
    assert (gi.R, gi.P, gi.tile64, gi.wg_per_cu) == (64, 3, 1, 4)
    # without the QNAME phase and without an N-trick base the kernel is not one of those built for four workgroups per CU: the tile it had
    for form in (dict(stats=True, lists=True), dict(stats=True)):
        g0 = ops.pack_tile_geometry(p, **form)
        assert g0.tiled and not g0.tile64 and g0.R == tile_reads(p) == 48 and g0.P == 256 // 48 and g0.copies == 4
    g0 = ops.pack_tile_geometry(p, stats=False)                                  # (the plain pack kernel: a 20 KiB stage, no count table)
    assert g0.tiled and not g0.tile64 and (g0.R, g0.stage_bytes, g0.copies) == (56, 5 * 4096 + 32, 0)


@pytest.mark.parametrize('notricks', [True, False], ids=['var-notricks', 'var-ntrick'])
def test_the_36_301_bp_workloads_keep_their_geometry(notricks):
    n = 4000
    host = synth.fastq_array(synth.Spec(20261003 + 5, (36, 301), n_rate=1), n)
    p = decide(host, n, notricks=notricks)[3]
    assert p.variable and p.dna_max == 301 and p.dna_bytes_per_row + p.quality_bytes_per_row == (341 if notricks else 303)      # (3-bit / 2-bit bases)
    for form in FORMS[1:]:                                  # (tile_reads() restates the fused kernels' arithmetic: a 16 KiB stage)
        g = ops.pack_tile_geometry(p, **form)
        assert g.tiled and not g.tile64 and g.R == tile_reads(p), (form, g)
        assert g.stage_bytes == 4 * 4096 + 32
    g = ops.pack_tile_geometry(p, stats=False)
    assert g.tiled and not g.tile64 and g.stage_bytes == 5 * 4096 + 32
    g = ops.pack_tile_geometry(p, stats=True, qname=True, lists=True)
    assert g.copies == (8 if p.bits_per_base == 2 else 4) and g.P == (256 - 64) // g.R


def test_a_record_too_long_for_64_keeps_the_geometry():
    p = flagship_params()
    fits = (22 * 1024 + 32 - 47) // 64                      # the longest record of which 64 fit the stage
    assert p.max_record_bytes <= fits
    p.max_record_bytes = fits
    assert ops.pack_tile_geometry(p, stats=True, qname=True, lists=True).R == 64
    for rec in (fits + 1, 400, 1000, 7400):
        p.max_record_bytes = rec
        for avg in (0, 330):
            p.avg_record_bytes = avg
            g = ops.pack_tile_geometry(p, stats=True, qname=True, lists=True)
            assert g.tiled and not g.tile64 and g.copies == 8 and g.R == tile_reads(p), (rec, avg, g)
    p.max_record_bytes = 16384 - 64 + 1                    # fits no tile at all: the exact kernel, no fused form
    g = ops.pack_tile_geometry(p, stats=True, qname=True, lists=True)
    assert not g.tiled and g.R == 0


def bare_params(ntrick):
    p = PackParams()
    dna = np.full(256, -1, dtype=np.int16); nq = np.full(256, -1, dtype=np.int32)
    dna[list(b'ACGT')] = np.arange(4)
    if ntrick: nq[ord('N')] = 0
    C.memmove(p.dna_code, dna.ctypes.data, 512); C.memmove(p.qual_code, dna.ctypes.data, 512); C.memmove(p.n_qual, nq.ctypes.data, 1024)
    return p


def test_sweep_through_the_query():
    """Longest record 8 .. 20 000 bytes, rows up to 400 bytes, average record 0 (unknown) .. longest, every form of the kernel."""
    points = tiled = big = 0
    ps = [bare_params(False), bare_params(True)]
    recs = list(range(8, 420, 7)) + [351, 352, 353] + list(range(420, 20001, 611)) + [16320, 16321, 20000]
    for rec in recs:
        lmax = (rec - 6) // 2
        for L in sorted({1, 36, 150, lmax} & set(range(1, lmax + 1))):
            for variable in (0, 1):
                for bd in (2, 3):
                    for bq in (1, 6, 8):
                        Cd, Cq = (bd * (L + variable) + 7) // 8, (bq * (L + variable) + 7) // 8
                        if Cd + Cq > 400: continue
                        for p in ps:
                            p.bits_per_base, p.bits_per_quality, p.variable, p.dna_max = bd, bq, variable, L
                            p.dna_bytes_per_row, p.quality_bytes_per_row, p.max_record_bytes = Cd, Cq, rec
                        for avg in (0, 4, rec // 3, rec // 2, rec - rec // 8, rec - 1, rec):
                            for nt, p in enumerate(ps):
                                p.avg_record_bytes = avg
                                for form in FORMS:
                                    g = ops.pack_tile_geometry(p, **form)
                                    points += 1
                                    cap = (4 if form['stats'] else 5) * 4096
                                    assert bool(g.tiled) == (rec + 64 <= cap), (rec, form, g)
                                    if not g.tiled: continue
                                    tiled += 1
                                    where = (rec, avg, L, variable, bd, bq, nt, form, g)
                                    assert 1 <= g.wg_per_cu and g.lds_bytes <= LDS_PER_CU // g.wg_per_cu, where
                                    assert g.Rs * rec + 47 <= g.stage_bytes, where
                                    if g.tile64 or avg < 4 or avg >= rec: assert g.R * rec + 47 <= g.stage_bytes, where
                                    assert 1 <= g.P <= g.G == (L + variable + 7) // 8, where
                                    assert 1 <= g.Rs <= g.R <= 64, where
                                    assert g.P * g.R <= (192 if form.get('qname') else 256), where
                                    if g.tile64:
                                        big += 1
                                        assert g.R == 64 and g.wg_per_cu == 4 and bd == 2 and form['stats'] and (form.get('qname') or nt), where
                                    else:
                                        assert 4 * g.R + 1 <= 256 and g.stage_bytes == cap + 32, where
    assert points > 100_000 and big > 1000 and tiled > big


def test_sweep_stand_alone_under_the_sanitizers(tmp_path):
    gxx = next((p for p in (shutil.which(c) for c in ('g++', 'c++', 'clang++')) if p), None)
    if gxx is None:
        pytest.skip('no host C++ compiler')
    exe = tmp_path / 'pack_geometry_check'
    subprocess.check_call([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                           os.path.join(REPO, 'uq_amd', 'csrc'), os.path.join(REPO, 'tools', 'pack_geometry_check.cpp'), '-o', str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'ok' in r.stdout
