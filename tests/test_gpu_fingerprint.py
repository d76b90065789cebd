"""GPU: uq_fingerprint_accumulate against the plain-Python statement of the fingerprint (tests/fingerprint_ref.py), exactly, on all nine fields.

The kernel stages the stream in tiles of TILE = 16 368 bytes (csrc/fingerprint.hip: FP_TILE) cut at 16-byte-aligned addresses from the
start of each group of records; a word belongs to the tile that holds its first byte.  The inputs below are built from that number: short
records (a group is a fraction of a tile), records of a few tiles whose lines start and end at every byte phase around a tile boundary, one
70 000-base read between short ones, a line longer than a tile at either end of the buffer, buffers misaligned by 1-7 bytes."""
import os
import random
import re

import numpy as np
import pytest

import fingerprint_ref as F
from uq_amd import ops

pytestmark = pytest.mark.gpu

TILE = 16368
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def text_of(records):
    return b''.join(b'\n'.join(r) + b'\n' for r in records)


def line(rnd, L, alphabet=None):
    if alphabet: return bytes(rnd.choice(alphabet) for _ in range(L))
    return bytes(rnd.randrange(33, 127) for _ in range(L))


def on_device(ctx, text, mis=0):
    """(the text as a device tensor whose address is `mis` bytes past a 16-byte boundary, its record index built on the host)"""
    a = np.frombuffer(text, dtype=np.uint8)
    whole = ctx.torch.zeros(len(a) + 16, dtype=ctx.torch.uint8, device=ctx.device)
    off = (-whole.data_ptr()) % 16 + mis
    buf = whole[off:off + len(a)]
    buf.copy_(ctx.to_device(a))
    assert buf.data_ptr() % 16 == mis % 16
    ls = ctx.to_device(ops.host_line_starts(text).view(np.int64))
    return buf, ls


def device_fp(ctx, text, pieces=None, mis=0):
    buf, ls = on_device(ctx, text, mis)
    n = (ls.numel() - 1) // 4
    d = ops.fingerprint_new(ctx)
    for first, cnt, base in (pieces if pieces is not None else [(0, n, 0)]):
        ops.fingerprint_accumulate(ctx, d, buf, ls, first, cnt, base)
    return ops.fingerprint_fetch(ctx, d)


def test_the_tile_size_is_the_kernels():
    src = open(os.path.join(REPO, 'uq_amd', 'csrc', 'fingerprint.hip')).read()
    assert int(re.search(r'FP_TILE = (\d+);', src).group(1)) == TILE


def test_known_answers(ctx):
    from test_fingerprint_cpu import V1, V2, V3, KNOWN1, KNOWN2, KNOWN3_ORDERED
    assert device_fp(ctx, V1) == KNOWN1
    assert device_fp(ctx, V2) == KNOWN2
    assert device_fp(ctx, V3, pieces=[(0, 1, 1)])['ordered'] == KNOWN3_ORDERED


def test_every_length_from_0_to_17(ctx):
    """All three hashed lines at every length 0..17 (empty lines, one byte, a word less one, a word, a word and one, two words and one),
    in one file and one record at a time."""
    rnd = random.Random(11)
    recs = [(line(rnd, a), line(rnd, b), b'+', line(rnd, c)) for a in range(18) for b in range(18) for c in (0, 1, 7, 8, 9, 16, 17)]
    recs += [(line(rnd, L), line(rnd, L), b'+', line(rnd, L)) for L in range(18)]
    text = text_of(recs)
    assert device_fp(ctx, text) == F.fingerprint(text)
    for L in range(18):
        one = text_of([(line(rnd, L), line(rnd, (L * 5) % 18), b'+', line(rnd, 17 - L))])
        assert device_fp(ctx, one) == F.fingerprint(one), L


@pytest.mark.parametrize('mis', range(1, 8))
def test_misaligned_buffer(ctx, mis):
    """The buffer starts 1-7 bytes past a 16-byte boundary: the first tile begins before the buffer, and nothing outside it may be read
    (the tensor ends with the text)."""
    rnd = random.Random(mis)
    recs = [(b'@m:%d' % i, line(rnd, rnd.randint(0, 60), b'ACGTN'), b'+', line(rnd, rnd.randint(0, 60))) for i in range(300)]
    recs.insert(150, (b'@long', line(rnd, TILE + 5 + mis, b'ACGT'), b'+', line(rnd, TILE + 5 + mis)))
    text = text_of(recs)
    assert device_fp(ctx, text, mis=mis) == F.fingerprint(text)


def aligned_record(rnd, q, s, p, ulen):
    """The record with a QUAL line of ulen..ulen + 15 bytes, so that its length is a multiple of 16: in a file of such records every record
    starts at a 16-byte-aligned address and its tile boundaries lie exactly TILE, 2 TILE, ... bytes behind its first byte."""
    fixed = len(q) + len(s) + len(p) + 4
    return (q, s, p, line(rnd, ulen + (-(fixed + ulen)) % 16))


def test_lines_straddle_every_tile_boundary(ctx):
    """Records of three tiles, each 16-byte aligned and fingerprinted by a call of its own (one record = one group, tiles counted from its
    first byte): the SEQ line starts -9..+9 bytes around the first tile boundary and ends -9..+9 around the second one, the QUAL line
    starts right behind it and ends in the third tile -- so a line start, a line end, a newline and every byte of a word meet a boundary."""
    rnd = random.Random(12)
    recs = []
    for d in range(-9, 10):
        for e in (-9 + (d + 9) % 19, 9 - (d + 9) % 19):
            q = b'@' + line(rnd, TILE + d - 2)                    # TILE + d - 1 bytes + newline: SEQ starts at offset TILE + d of the record
            recs.append(aligned_record(rnd, q, line(rnd, TILE + e - d, b'ACGT'), b'+', 500))     # ... and its newline sits at offset 2 TILE + e
    text = text_of(recs)
    starts = ops.host_line_starts(text)
    assert all(int(starts[4 * i]) % 16 == 0 for i in range(len(recs)))
    assert sorted({int(starts[4 * i + 1] - starts[4 * i]) - TILE for i in range(len(recs))}) == list(range(-9, 10))
    assert sorted({int(starts[4 * i + 2] - starts[4 * i]) - 1 - 2 * TILE for i in range(len(recs))}) == list(range(-9, 10))
    want = F.fingerprint(text)
    assert device_fp(ctx, text, pieces=[(i, 1, i) for i in range(len(recs))]) == want
    assert device_fp(ctx, text) == want                       # and as one call: groups of one record each
    # the first boundary inside the third line, with and without text, and on its newline
    recs = [aligned_record(rnd, b'@p%d' % d, line(rnd, TILE - 8 + d, b'ACGT'), b'+' if d % 2 else b'+p%d' % d, 40) for d in range(0, 10)]
    text = text_of(recs)
    starts = ops.host_line_starts(text)
    assert sorted({int(starts[4 * i + 2] - starts[4 * i]) - TILE for i in range(len(recs))}) == list(range(-3, 7))
    assert device_fp(ctx, text, pieces=[(i, 1, i) for i in range(len(recs))]) == F.fingerprint(text)


def test_many_short_records(ctx):
    """140 000 records of about 20 bytes: groups of the largest size (63 records), more groups than the persistent grid has workgroups, so
    that workgroups walk over several; a group's last record and the file's last group are partial."""
    rnd = random.Random(13)
    bases = [line(rnd, rnd.randint(0, 9), b"ACGT") for _ in range(997)]
    recs = [(b'@%x' % (i * 2654435761 % 2 ** 20), bases[i % 997], b'+', bases[(i * 7) % 997][::-1]) for i in range(140000)]
    text = text_of(recs)
    assert 18 <= len(text) / len(recs) <= 22
    assert device_fp(ctx, text) == F.fingerprint(text)


def test_long_read_between_short_ones_and_long_lines_at_both_ends(ctx):
    rnd = random.Random(14)
    short = lambda i: (b'@s:%d' % i, line(rnd, 100 + i % 50, b'ACGT'), b'+', line(rnd, 100 + i % 50))
    recs = [short(i) for i in range(40)]
    recs.insert(20, (b'@ont:1', line(rnd, 70000, b'ACGTN'), b'+', line(rnd, 70000)))
    text = text_of(recs)
    assert device_fp(ctx, text) == F.fingerprint(text)
    # a line longer than a tile is the buffer's first line, another one its last
    recs = [(b'@' + line(rnd, TILE + 100), b'ACGT', b'+', b'IIII')] + [short(i) for i in range(5)] + [(b'@end', b'AC', b'+', line(rnd, TILE + 100))]
    text = text_of(recs)
    for mis in (0, 5):
        assert device_fp(ctx, text, mis=mis) == F.fingerprint(text)


@pytest.mark.parametrize('edge', [2 ** 31, 2 ** 32])
def test_stream_offsets_past_2_31_and_2_32(ctx, edge):
    """The text lies across byte 2^31 / 2^32 of a larger buffer (the index says where; nothing else of the buffer is read): groups of several
    records and of several tiles on either side of the edge and across it."""
    rnd = random.Random(edge % 97)
    recs = []
    for i in range(240):
        L = TILE + 300 if i % 40 == 17 else rnd.randint(30, 300)
        recs.append((b'@far:%d' % i, line(rnd, L, b'ACGT'), b'+', line(rnd, L)))
    text = text_of(recs)
    start = edge - len(text) // 2 - 5
    whole = ctx.torch.empty(start + len(text), dtype=ctx.torch.uint8, device=ctx.device)
    whole[start:].copy_(ctx.to_device(np.frombuffer(text, dtype=np.uint8)))
    starts = ops.host_line_starts(text) + np.uint64(start)
    assert int(starts[0]) < edge - 3 * TILE and int(starts[-1]) > edge + 3 * TILE
    ls = ctx.to_device(starts.view(np.int64))
    d = ops.fingerprint_new(ctx)
    ops.fingerprint_accumulate(ctx, d, whole, ls, 0, len(recs))
    want = F.fingerprint(text)
    assert ops.fingerprint_fetch(ctx, d) == want
    d = ops.fingerprint_new(ctx)
    for a, b in ((100, 240), (0, 100)): ops.fingerprint_accumulate(ctx, d, whole, ls, a, b - a, a)
    assert ops.fingerprint_fetch(ctx, d) == want


def test_pieces_in_any_order_equal_one_call(ctx):
    rnd = random.Random(15)
    recs = [(b'@q:%d' % i, line(rnd, rnd.randint(1, 300), b'ACGT'), b'+', line(rnd, rnd.randint(1, 300))) for i in range(2000)]
    text = text_of(recs)
    want = F.fingerprint(text)
    cuts = [0, 1, 2, 65, 700, 701, 1999, 2000]
    pieces = [(a, b - a, a) for a, b in zip(cuts, cuts[1:])]
    rnd.shuffle(pieces)
    assert device_fp(ctx, text, pieces=pieces) == want
    assert device_fp(ctx, text) == want
    # a piece with an index base of its own is that piece of a longer file
    part = device_fp(ctx, text, pieces=[(700, 1, 12345)])
    assert part == F.fingerprint(text, 700, 1, read_index_base=12345)


def test_line_3_with_text(ctx):
    rnd = random.Random(16)
    recs = [(b'@r%d' % i, line(rnd, 50, b'ACGT'), b'+' if i % 3 else b'+r%d' % i, line(rnd, 50)) for i in range(500)]
    recs[7] = (recs[7][0], recs[7][1], b'-', recs[7][3])               # one byte, not a '+'
    recs[8] = (recs[8][0], recs[8][1], b'', recs[8][3])
    text = text_of(recs)
    got = device_fp(ctx, text)
    assert got == F.fingerprint(text) and got['plus_text'] == 167 + 2
    plain = text_of([(q, s, b'+', u) for q, s, _, u in recs])
    assert {k for k in F.FIELDS if device_fp(ctx, plain)[k] != got[k]} == {'plus_text'}
