"""The deflate decoders (inflate_core.h through uq_inflate_member_host, inflate_stream.h through uq_gzip_stream_host) on valid deflate
that zlib's compressor never writes, and on its nearest invalid neighbours: the streams of tests/deflate_writer.py, each checked there
against zlib's inflate."""
import random
import re
import zlib

import pytest

from deflate_writer import behind_valid_front, crafted_invalid, crafted_members, crafted_streams, gzip_wrap
from uq_amd import ops

CHUNKS = [256, 1 << 10, 3000, 1 << 14]


def test_case_lists_cover_what_they_claim():
    members, streams, invalid = crafted_members(), crafted_streams(), crafted_invalid()
    assert len(members) > 220 and len(streams) > 55 and len(invalid) >= 12
    assert all(len(data) <= 65536 for _, _, data in members) and max(len(data) for _, _, data in members) == 65536
    assert max(len(data) for _, _, data in streams) < 330000
    for names in ([n for n, _, _ in members], [n for n, _, _ in streams], [c[0] for c in invalid]):
        assert len(set(names)) == len(names)
    import deflate_writer
    have = {c[0] for lst in (members, streams, invalid) for c in lst}
    table = deflate_writer.__doc__.split('crafted_invalid = I):')[1]
    named = [w for w in re.split(r'[\s,():]+', table) if '_' in w and w == w.lower() and w not in ('w_size', '_7')]
    assert len(named) > 40 and not [w for w in named if w not in have]


def test_host_member_decoder_on_crafted_members():
    for name, raw, data in crafted_members():
        st, out = ops.inflate_member_host(raw, len(data), zlib.crc32(data))
        assert (st, out) == (0, data), (name, st)


@pytest.mark.parametrize('chunk', CHUNKS)
def test_host_stream_decoder_on_crafted_streams(chunk):
    for name, blob, data in crafted_streams():
        out, info = ops.gzip_stream_host(blob, chunk)
        assert out == data, (name, chunk)
        assert info['out_bytes'] == len(data)


@pytest.mark.parametrize('chunk', CHUNKS)
def test_host_stream_decoder_on_crafted_streams_with_wrong_starts(chunk):
    rnd = random.Random(23 + chunk)
    for name, blob, data in crafted_streams():
        nb = 8 * len(blob)
        starts = [rnd.randrange(1, nb) << 2 | rnd.randrange(3) for _ in range(30)]
        assert ops.gzip_stream_host(blob, chunk, starts=starts)[0] == data, (name, chunk)


def test_crafted_members_as_one_gzip_file_each():
    # the chunk decoder on the member cases too (a chunk that starts at a member header knows its window: bytes from the start)
    for name, raw, data in crafted_members()[::3]:
        assert ops.gzip_stream_host(gzip_wrap(raw, data), 256)[0] == data, name


@pytest.mark.parametrize('case', crafted_invalid(), ids=lambda c: c[0])
def test_host_decoders_refuse_invalid_neighbours(case):
    name, raw, isize, want = case
    st, _ = ops.inflate_member_host(raw, isize, 0)
    assert st == want, (name, st)
    blob = gzip_wrap(raw, b'')[:-4] + isize.to_bytes(4, 'little')
    # alone in a gzip member the fault's status is the member decoder's, except that the stream decoder has no bound on a member's
    # output, so a member that is longer than its ISIZE says is a mismatch (9) there and an overflow (8) here
    stream_want = {8: 9}.get(want, want)
    for chunk in (64, 256, 1 << 14):
        with pytest.raises(ops.GzipStreamError) as e:
            ops.gzip_stream_host(blob, chunk)
        assert e.value.status == stream_want, (name, chunk, e.value.status)
    if isize == 0:                                              # a fault in a block header: the same wherever the block stands
        blob = behind_valid_front(raw)
        for chunk in (64, 256, 1 << 10):
            with pytest.raises(ops.GzipStreamError) as e:
                ops.gzip_stream_host(blob, chunk)
            assert e.value.status == want and e.value.offset > 3000, (name, chunk, e.value.status)
