"""The plain deflate reader of the compressor's tests (deflate_reader.py) against zlib, and its two references against brute force."""
import random
import zlib

import pytest

import deflate_reader as R
from deflate_writer import crafted_invalid, crafted_members
from uq_amd import synth


def _zlib_inflate(raw):
    d = zlib.decompressobj(-15)
    out = d.decompress(raw) + d.flush()
    assert d.eof
    return out, len(raw) - len(d.unused_data)


def _replay(blocks):
    out = bytearray()
    for b in blocks:
        if b['btype'] == 0: out += b['stored']
        for t in b['tokens']:
            if isinstance(t, tuple):
                for _ in range(t[0]): out.append(out[-t[1]])
            else:
                out.append(t)
    return bytes(out)


@pytest.mark.parametrize('level', [0, 1, 6, 9])
def test_reader_equals_zlib_on_zlib_streams(level):
    rnd = random.Random(level)
    texts = [b'', b'a', synth.fastq(5, 60, (30, 80)), bytes(rnd.getrandbits(8) for _ in range(3000)), b'ab' * 700 + b'\x00' * 300,
             bytes(rnd.choice(b'ACGT') for _ in range(5000))]
    seen = set()
    for text in texts:
        for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY):
            c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
            raw = c.compress(text[:len(text) // 2]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(text[len(text) // 2:]) + c.flush()
            data, blocks, end = R.inflate(raw)
            want, used = _zlib_inflate(raw)
            assert data == want == text and (end + 7) // 8 == used == len(raw)
            assert _replay(blocks) == text and blocks[-1]['final'] and not any(b['final'] for b in blocks[:-1])
            for b in blocks:
                seen.add(b['btype'])
                if b['btype'] != 2: continue
                assert len(b['llens']) == b['hlit'] and len(b['dlens']) == b['hdist'] and len(b['clens_written']) == b['hclen']
                assert sum(n for _, _, _, n in R.run_spans(b)) == b['hlit'] + b['hdist']
    assert seen == ({0, 1, 2} if level else {0})            # zlib wrote every block type the level has


def test_reader_equals_zlib_on_crafted_members():
    members = crafted_members()
    assert len(members) > 40
    for name, raw, data in members:
        got, blocks, end = R.inflate(raw)
        want, used = _zlib_inflate(raw)
        assert got == want == data and (end + 7) // 8 == used, name
        assert _replay(blocks) == data, name


def test_reader_refuses_what_zlib_refuses():
    refused = 0
    for name, raw, *_ in crafted_invalid():
        d = zlib.decompressobj(-15)
        try:
            d.decompress(raw); ok = d.eof
        except zlib.error:
            ok = False
        if ok: continue
        with pytest.raises(R.DeflateError):
            R.inflate(raw)
        refused += 1
    assert refused > 5
    # over-subscribed and incomplete codes, one of each kind
    for lens, kind in (([1, 1, 1], 'litlen'), ([2, 2, 2], 'litlen'), ([1, 2], 'dist'), ([1], 'codelen'), ([2, 2, 2, 3], 'codelen')):
        with pytest.raises(R.DeflateError):
            R.Code(lens, kind)
    R.Code([1, 0, 0], 'dist'); R.Code([0, 1], 'litlen'); R.Code([0, 0], 'dist'); R.Code([1, 2, 2], 'codelen')


def test_package_merge_equals_brute_force():
    rnd = random.Random(20261019)
    cases = [[1, 1], [1, 1, 1], [1, 1, 2, 3, 5, 8], [1, 2, 4, 8, 16, 32, 64], [5] * 7, [1, 1, 1, 1, 100], [3, 0, 0, 9], [7], []]
    for _ in range(150):
        m = rnd.randrange(2, 8)
        cases.append([rnd.choice([1, 1, 2, 3, 10, 100, rnd.randrange(1, 1000)]) for _ in range(m)])
    checked = 0
    for w in cases:
        m = sum(1 for f in w if f)
        lo = max(1, (m - 1).bit_length())
        for limit in range(lo, min(lo + 3, 6) + 1):
            if m > 6 and limit > 4: continue                # 5^7 assignments and up: enough is covered below that
            assert R.package_merge_cost(w, limit) == R.brute_force_cost(w, limit), (w, limit)
            checked += 1
    assert checked > 300
    # a limit that does not bind gives Huffman's cost; a tighter one costs more
    for w in cases:
        if sum(1 for f in w if f) < 2: continue
        d = R.huffman_depths(w)
        free = sum(w[s] * l for s, l in d.items())
        assert R.package_merge_cost(w, max(d.values())) == free == R.package_merge_cost(w, 15)
        if max(d.values()) > (len(d) - 1).bit_length() and max(d.values()) > 1:
            assert R.package_merge_cost(w, max(d.values()) - 1) >= free


def test_unlimited_depth_on_known_trees():
    fib = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584]
    for k in range(2, len(fib) + 1):
        assert R.unlimited_depth(fib[:k]) == k - 1
    assert R.unlimited_depth([1 << i for i in range(20)]) == 19
    assert R.unlimited_depth([7] * 16) == 4 and R.unlimited_depth([7] * 17) == 5
    assert R.unlimited_depth([0, 9, 0]) == 1 and R.unlimited_depth([]) == 0 and R.unlimited_depth([0, 0]) == 0
    # the tie rule: a leaf goes before an internal node of the same weight, so 1 1 2 2 is two levels deep for all, not three
    assert R.huffman_depths([1, 1, 2, 2]) == {0: 2, 1: 2, 2: 2, 3: 2}
