"""The deflate compressor's code builder past its length limits, on the MI355X.

On the device the rebuild loop of uq_def_huffman is a handshake of the whole workgroup: all threads rank the symbols, thread 0 builds
the tree and sets `done`, everybody reads it between two barriers, in scratch that shares its LDS with the hash table and the parse
window.  The blocks of deflate_limit_inputs.py make that loop go round (test_deflate_limits_cpu.py proves it for each of them, on the
host build of the same code); here the device's bytes are the host build's, byte for byte: every block alone, the full blocks in the
middle of one launch between ordinary ones, as parts, through the sizer, and read back by the device's own inflate."""
import numpy as np
import pytest

from deflate_limit_inputs import BLOCK, fastq_blocks, header_blocks, limit_blocks
from test_deflate_limits_cpu import LEVELS, analysed
from uq_amd import ops

pytestmark = pytest.mark.gpu


def _host(name, level):
    return analysed(name, level)[0]


def _stream(level):
    """(the eight blocks, their host members): ordinary, lit15, ordinary, clen7, lit15, ordinary, clen7, ordinary"""
    full = {}
    for name, b in limit_blocks():
        if len(b) == BLOCK: full.setdefault(name.split('/')[0], []).append((name, b))
    fq = fastq_blocks(4)
    lit, clen = full['lit15'], full['clen7']
    order = [fq[0], lit[0], fq[1], clen[0], lit[1], fq[2], clen[1], fq[3]]
    members = [ops.bgzf_block_host(b, level=level) if isinstance(b, bytes) else _host(b[0], level) for b in order]
    return [b if isinstance(b, bytes) else b[1] for b in order], members


@pytest.mark.parametrize('level', LEVELS)
def test_every_named_block_alone(ctx, level):
    for name, b in limit_blocks() + header_blocks():
        got = ctx.to_numpy(ops.bgzf_compress(ctx, ctx.bytes_to_device(b), eof=False, level=level)).tobytes()
        assert got == (_host(name, level) if b else b''), name


@pytest.mark.parametrize('level', LEVELS)
def test_limit_blocks_between_ordinary_ones_in_one_launch(ctx, level):
    blocks, members = _stream(level)
    assert len(blocks) == 8 and all(len(b) == BLOCK for b in blocks)
    data = b''.join(blocks)
    d_data = ctx.bytes_to_device(data)
    d_blob = ops.bgzf_compress(ctx, d_data, eof=False, level=level)
    blob = ctx.to_numpy(d_blob).tobytes()
    for k, m in enumerate(members):                         # member by member, so that a failure names the block
        at = sum(len(x) for x in members[:k])
        assert blob[at:at + len(m)] == m, 'block %d of the stream' % k
    assert blob == b''.join(members)
    # the sizer: the same plan without the emit pass
    want = ops.deflate_size_host(data, level=level)
    assert want == len(blob)
    assert ops.deflate_size(ctx, b'', d_data, level=level) == want
    assert ops.deflate_size(ctx, data[:3], d_data[3:], level=level) == want
    # and the device's own inflate reads it back (it checks every member's CRC-32)
    kind, m, total, err = ops.gzip_scan(np.frombuffer(blob, dtype=np.uint8))
    assert kind == ops.GZIP_BGZF and err is None and total == len(data) and len(m) == 8
    out, bad = ops.inflate_members(ctx, d_blob, m, total)
    assert bad is None and ctx.torch.equal(out, d_data)


@pytest.mark.parametrize('level', LEVELS)
def test_limit_blocks_as_parts(ctx, level):
    host_parts, dev = [], []
    for k, (name, b) in enumerate(limit_blocks()):
        cut = (0, 3, 17)[k % 3]                             # some of the block comes from the part's host prefix
        host_parts.append((b[:cut], b[cut:]))
        dev.append((b[:cut], ctx.bytes_to_device(b[cut:])))
    out, sizes = ops.bgzf_compress_parts(ctx, dev, level=level)
    want, want_sizes = ops.bgzf_compress_parts_host(host_parts, level=level)
    assert sizes == want_sizes == [len(_host(name, level)) for name, _ in limit_blocks()]
    assert ctx.to_numpy(out).tobytes() == want == b''.join(_host(name, level) for name, _ in limit_blocks())
    for (prefix, d), n in zip(dev, sizes):
        assert ops.deflate_size(ctx, prefix, d, level=level) == n
