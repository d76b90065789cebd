"""The byte source of a .uQ container on the decode side, and the member-aligned BGZF layout of the encode side.

A container is a tar.  On disk it is either that tar, or the tar as BGZF (`--gz`, or `bgzip reads.uQ`), or the tar behind any other gzip.
The decoder addresses the *inflated* tar: a source serves byte ranges of it,

    read_host(offset, n)   -> bytes         (tar and .npy headers)
    to_device(offset, n)   -> uint8 tensor  (payloads; a fresh, aligned allocation)
    total                                    the inflated size

and there are three of them: PlainSource (the file itself), BgzfSource (random access: only the members that cover a range are
uploaded and inflated) and BufferSource (the whole inflated stream in HBM: other gzip, and BGZF after verify_all()).

The tar is untrusted input: walk_tar() checks every offset and size against `total` before anything is addressed.
"""
import json
import tarfile

import numpy as np

from .errors import error as _error

BGZF_BLOCK = 65280
BLOCKSIZE, RECORDSIZE = tarfile.BLOCKSIZE, tarfile.RECORDSIZE

PLAIN, BGZF, GZIP = 'plain', 'bgzf', 'gzip'
OTHER_MAGIC = ((b'BZh', 'bzip2'), (b'\xfd7zXZ\x00', 'xz'), (b'\x28\xb5\x2f\xfd', 'zstd'))




def sniff(path):
    """The container's outer format by its first bytes: PLAIN or 'gzip' (BGZF or not is the scan's business).  bzip2 / xz / zstd are
    refused by name: tarfile would open the first two transparently and the decoder would then address the compressed file."""
    with open(path, 'rb') as f:
        head = f.read(8)
    for magic, name in OTHER_MAGIC:
        if head.startswith(magic):
            _error('ERROR: %s is %s-compressed: decompress it first (compressed containers are read as gzip / BGZF only)' % (path, name))
    return GZIP if head[:2] == b'\x1f\x8b' else PLAIN


# ---------------------------------------------------------------------------------------------------------------- sources
class PlainSource:
    kind = PLAIN

    def __init__(self, path, io):
        import os
        self.path, self.io, self.total = path, io, os.path.getsize(path)

    def _check(self, offset, n):
        if offset < 0 or n < 0 or offset + n > self.total:
            _error('ERROR: bytes %d..%d lie outside this uQ file of %d bytes' % (offset, offset + n, self.total))

    def read_host(self, offset, n):
        self._check(offset, n)
        with open(self.path, 'rb') as fh:
            fh.seek(offset)
            return fh.read(n)

    def to_device(self, offset, n):
        self._check(offset, n)
        return self.io.file_to_device(self.path, offset, n)


class BufferSource:
    """The whole inflated stream as one uint8 device tensor."""
    kind = GZIP

    def __init__(self, ctx, d_buf):
        self.ctx, self.d_buf, self.total = ctx, d_buf, int(d_buf.numel())

    def _check(self, offset, n):
        if offset < 0 or n < 0 or offset + n > self.total:
            _error('ERROR: bytes %d..%d lie outside the %d inflated bytes of this uQ file' % (offset, offset + n, self.total))

    def read_host(self, offset, n):
        self._check(offset, n)
        return self.d_buf[offset:offset + n].cpu().numpy().tobytes()

    def to_device(self, offset, n):
        self._check(offset, n)
        return self.d_buf[offset:offset + n].clone()


def member_error(path, k, members, status):
    from .ops import INFLATE_STATUS
    _error('ERROR: %s: gzip member %d (deflate data at byte %d): %s' % (path, k, int(members[k]['data_offset']),
                                                                       INFLATE_STATUS.get(status, 'status %d' % status)))


class BgzfSource:
    """Random access into a BGZF file through its member table (ops.gzip_scan).  comp: the compressed file as a host uint8 array (a memmap:
    read_host touches the covering members only).  device_inflate(k0, k1) -> uint8 device tensor of the output of members [k0, k1), or
    None for a source that serves the host only.  `inflated`: the indices of the members inflated for the device so far."""
    kind = BGZF

    def __init__(self, comp, members, total, device_inflate=None, name='input'):
        self.comp, self.members, self.total, self.name = comp, members, int(total), name
        self.device_inflate = device_inflate
        self.out_offset = np.ascontiguousarray(members['out_offset']).astype(np.uint64)
        self.inflated = set()
        self.whole = None                      # verify_all(): the inflated stream, kept

    @property
    def inflated_members(self):
        return len(self.inflated)

    def _check(self, offset, n):
        if offset < 0 or n < 0 or offset + n > self.total:
            _error('ERROR: bytes %d..%d lie outside the %d inflated bytes of this uQ file' % (offset, offset + n, self.total))

    def cover(self, offset, n):
        """[k0, k1): the smallest run of members whose output covers inflated bytes [offset, offset + n) -- its first and last member
        both hold a byte of the range.  (0, 0) for an empty range."""
        self._check(offset, n)
        if n == 0: return 0, 0
        k0 = int(np.searchsorted(self.out_offset, np.uint64(offset), 'right')) - 1
        k1 = int(np.searchsorted(self.out_offset, np.uint64(offset + n), 'left'))
        return k0, k1

    def selected(self, offset, n):
        """The members of cover() that have output (empty members inside the run are left out)."""
        k0, k1 = self.cover(offset, n)
        return [k for k in range(k0, k1) if self.members[k]['isize']]

    def read_host(self, offset, n):
        from .ops import inflate_member_host
        k0, k1 = self.cover(offset, n)
        if k1 == k0: return b''
        if self.whole is not None: return self.whole[offset:offset + n].cpu().numpy().tobytes()
        parts = []
        for k in range(k0, k1):
            m = self.members[k]
            if not m['isize']: continue
            lo = int(m['data_offset'])
            st, out = inflate_member_host(self.comp[lo:lo + int(m['comp_bytes'])].tobytes(), int(m['isize']), int(m['crc32']))
            if st: member_error(self.name, k, self.members, st)
            parts.append(out)
        skip = offset - int(self.out_offset[k0])
        return b''.join(parts)[skip:skip + n]

    def to_device(self, offset, n):
        k0, k1 = self.cover(offset, n)
        if self.whole is not None: return self.whole[offset:offset + n].clone()
        if k1 == k0: return self.device_inflate(0, 0)[:0]
        self.inflated.update(k for k in range(k0, k1) if self.members[k]['isize'])
        skip = offset - int(self.out_offset[k0])
        return self.device_inflate(k0, k1)[skip:skip + n].clone()

    def verify_all(self):
        """Every member inflated (length and CRC-32 checked) into one buffer that serves all later reads: what the single-GPU decoder does
        before it writes anything."""
        if self.whole is None:
            self.whole = self.device_inflate(0, len(self.members))
            self.inflated.update(range(len(self.members)))
        return self


def device_inflater(ops, ctx, fetch, members, name='input'):
    """device_inflate for BgzfSource: fetch(lo, n) -> the compressed bytes [lo, lo + n) as a uint8 device tensor (for a file: file ->
    pinned -> HBM); the members [k0, k1) inflate there on a member table rebased to the span (uq_inflate_members)."""
    def inflate(k0, k1):
        if k1 <= k0: return ctx.empty(0)
        sub = members[k0:k1].copy()
        lo = int(sub['data_offset'][0])
        hi = int(sub['data_offset'][-1]) + int(sub['comp_bytes'][-1])
        out_lo = int(sub['out_offset'][0])
        total = int(sub['out_offset'][-1]) + int(sub['isize'][-1]) - out_lo
        sub['data_offset'] -= np.uint64(lo)
        sub['out_offset'] -= np.uint64(out_lo)
        d_out, bad = ops.inflate_members(ctx, fetch(lo, hi - lo), sub, total)
        if bad is not None: member_error(name, k0 + bad[0], members, bad[1])
        return d_out
    return inflate


def open_source(session, path):
    """The source for `path`, sniffed by content.  BGZF: a BgzfSource (nothing inflated yet).  Other gzip: inflated now, whole, on the
    device in parallel chunks (or on the host with --host-inflate)."""
    ops, ctx = session.ops, session.ctx
    if sniff(path) == PLAIN: return PlainSource(path, session.io)
    comp = np.memmap(path, dtype=np.uint8, mode='r')
    kind, members, total, err = ops.gzip_scan(comp)
    if kind == ops.GZIP_MALFORMED:
        _error('ERROR: %s is not a readable gzip file: %s (gzip member at byte %d)' % (path, err[0], err[1]))
    if kind == ops.GZIP_BGZF:
        if len(members) == 0 or int(members[-1]['isize']) != 0:
            session.say('Warning: %s has no BGZF EOF member; it may be truncated' % path)
        return BgzfSource(comp, members, total, device_inflater(ops, ctx, lambda lo, n: session.io.file_to_device(path, lo, n), members, path), name=path)
    del comp
    if session.args.host_inflate:
        import zlib
        try:
            return BufferSource(ctx, session.io.gzip_to_device(path))
        except (zlib.error, EOFError) as e:
            _error('ERROR: %s is not a readable gzip file: %s' % (path, e))
    from .uq import GZIP_STREAM_CHUNK
    d_comp = session.io.file_to_device(path)
    try:
        d_buf, _ = ops.gzip_stream_to_device(ctx, d_comp, GZIP_STREAM_CHUNK)
    except ops.GzipStreamError as e:
        _error('ERROR: %s is not a readable gzip file: %s' % (path, e))
    return BufferSource(ctx, d_buf)


# ---------------------------------------------------------------------------------------------------------------- the tar walk
NOT_A_TAR = 'ERROR: Sorry, the path you have provided as input is a file, but not a tar file, and therefore cannot be a .uq file!'
NO_CONFIG = 'ERROR: No config.json file was found in your input path! I cannot decode data without it!'


def walk_tar(source):
    """name -> (payload offset, size) of the regular members of the tar `source` serves, by its header fields.  Every header block and
    every payload lies inside source.total, or the walk raises UqError.  The end is two zero blocks (one is accepted) or the end of the
    stream on a block boundary; a stream that stops inside a header block is damaged.  Plain ustar / GNU headers of regular files are
    understood (what this project and the reference write); GNU long-name and pax records are passed over, not applied."""
    total = source.total
    members, pos, first = {}, 0, True
    while pos + BLOCKSIZE <= total:
        block = source.read_host(pos, BLOCKSIZE)
        if len(block) != BLOCKSIZE: _error('ERROR: this uQ file is damaged: short read of the tar header at byte %d' % pos)
        if block == b'\0' * BLOCKSIZE: break
        try:
            ti = tarfile.TarInfo.frombuf(block, tarfile.ENCODING, 'surrogateescape')
        except tarfile.HeaderError as e:
            if first: _error(NOT_A_TAR)
            _error('ERROR: this uQ file is damaged: the tar header at byte %d is unreadable (%s)' % (pos, e))
        first = False
        size, data = int(ti.size), pos + BLOCKSIZE
        if size < 0 or data + size > total:
            _error('ERROR: this uQ file is damaged: member %r claims bytes %d..%d of a tar of %d bytes' % (ti.name, data, data + size, total))
        if ti.isreg(): members[ti.name] = (data, size)
        pos = data + size + (-size % BLOCKSIZE)
    if first: _error(NOT_A_TAR)
    if pos > total or 0 < total - pos < BLOCKSIZE:
        _error('ERROR: this uQ file is damaged: the tar stops inside the block at byte %d (%d bytes in all)' % (pos - pos % BLOCKSIZE if pos <= total else total - total % BLOCKSIZE, total))
    return members


def read_config(source, members):
    if 'config.json' not in members: _error(NO_CONFIG)
    offset, size = members['config.json']
    try:
        return json.loads(source.read_host(offset, size).decode())
    except (ValueError, UnicodeDecodeError) as e:
        _error('ERROR: config.json of this uQ file is unreadable: %s' % e)


# ---------------------------------------------------------------------------------------------------------------- the --gz layout
def tar_header(name, size, mtime):
    ti = tarfile.TarInfo(name); ti.size = size; ti.mtime = mtime
    return ti.tobuf(tarfile.DEFAULT_FORMAT, tarfile.ENCODING, 'surrogateescape')


def framing_pieces(entries, mtime):
    """entries: [(name, member size)] in tar order.  Returns len(entries) + 1 byte strings: piece k is the zero padding that closes member
    k - 1 followed by the tar header of member k; the last one is the closing padding and the end-of-archive zeros up to RECORDSIZE."""
    pieces, pos, pad = [], 0, 0
    for name, size in entries:
        pieces.append(b'\0' * pad + tar_header(name, size, mtime))
        pos += pad + BLOCKSIZE + size
        pad = -size % BLOCKSIZE
    pos += pad
    end = 2 * BLOCKSIZE
    end += -(pos + end) % RECORDSIZE
    pieces.append(b'\0' * (pad + end))
    return pieces


def member_aligned_layout(frame_sizes, part_sizes):
    """The compressed (offset, length) of every framing piece and data part of a member-aligned file: [{'frame': (o, n), 'data': (o, n)}]
    per member, then {'frame': ..., 'data': None} for the closing piece; the EOF member follows."""
    layout, pos = [], 0
    for k, f in enumerate(frame_sizes):
        entry = {'frame': (pos, f), 'data': None}
        pos += f
        if k < len(part_sizes):
            entry['data'] = (pos, part_sizes[k]); pos += part_sizes[k]
        layout.append(entry)
    return layout


def member_aligned_host(tar_bytes, level=1):
    """The member-aligned BGZF of an existing plain tar, built on the host with the device compressor's code at that level (the host twin
    of the --gz writer).  Returns (bytes, layout, names)."""
    from . import ops

    class Host:
        total = len(tar_bytes)

        def read_host(self, offset, n): return tar_bytes[offset:offset + n]
    members = walk_tar(Host())
    order = sorted(members, key=lambda k: members[k][0])
    out, frames, parts, pos = [], [], [], 0
    for name in order + [None]:
        end = members[name][0] if name else len(tar_bytes)
        piece = ops.bgzf_block_host(tar_bytes[pos:end], level=level)
        out.append(piece); frames.append(len(piece))
        if name is None: break
        offset, size = members[name]
        blob, sizes = ops.bgzf_compress_parts_host([(b'', tar_bytes[offset:offset + size])], level=level)
        out.append(blob); parts.append(sizes[0])
        pos = offset + size
    out.append(ops.BGZF_EOF)
    return b''.join(out), member_aligned_layout(frames, parts), order
