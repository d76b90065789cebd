"""stdin -> BGZF on stdout, on the CPU, through the compressor the GPU runs (uq_bgzf_compress_block_host: deflate_core.h).

    python -m uq_amd.bgzf_host [--no-eof] < file > file.gz

One member per 65 280 bytes of input, then the 28-byte BGZF EOF member unless --no-eof.  With --no-eof the output's length is the size
`uq --test --device-compressor` reports for the same bytes, so `--compressor "python -m uq_amd.bgzf_host --no-eof"` reproduces the
device sizer's numbers without a GPU.  The library is loaded without torch or a device: only the host entry is called.
"""
import ctypes as C
import sys

from ._lib import LIB_PATH

BLOCK = 65280
EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')


def compress(data, eof=True):
    """The BGZF stream of `data` (bytes)."""
    lib = C.CDLL(LIB_PATH)
    fn = lib.uq_bgzf_compress_block_host
    fn.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    fn.restype = C.c_int
    out = C.create_string_buffer(65536)
    nout, st = C.c_uint64(), C.c_uint32()
    parts = []
    for at in range(0, len(data), BLOCK):
        block = data[at:at + BLOCK]
        if fn(block, len(block), out, 65536, C.byref(nout), C.byref(st)) or st.value:
            raise RuntimeError('uq_bgzf_compress_block_host failed on the block at byte %d' % at)
        parts.append(out.raw[:nout.value])
    if eof: parts.append(EOF)
    return b''.join(parts)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if any(a != '--no-eof' for a in argv):
        print(__doc__, file=sys.stderr)
        return 2
    sys.stdout.buffer.write(compress(sys.stdin.buffer.read(), eof='--no-eof' not in argv))
    return 0


if __name__ == '__main__':
    sys.exit(main())
