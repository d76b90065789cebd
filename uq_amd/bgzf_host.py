"""stdin -> BGZF on stdout, on the CPU, through the compressor the GPU runs (uq_bgzf_compress_block_host: deflate_core.h).

    python -m uq_amd.bgzf_host [--no-eof] [--level {1,2}] < file > file.gz

One member per 65 280 bytes of input, then the 28-byte BGZF EOF member unless --no-eof.  With --no-eof the output's length is the size
`uq --test --device-compressor` reports for the same bytes, so `--compressor "python -m uq_amd.bgzf_host --no-eof"` reproduces the
device sizer's numbers without a GPU (with --level 2, those of --bgzf-level 2).  The library is loaded without torch or a device: only the host entry is called.
"""
import ctypes as C
import sys

from ._lib import LIB_PATH

BLOCK = 65280
EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')


def compress(data, eof=True, level=1):
    """The BGZF stream of `data` (bytes) at compressor level 1 or 2."""
    if level not in (1, 2): raise ValueError('the BGZF compressor has levels 1 and 2, not %r' % (level,))
    lib = C.CDLL(LIB_PATH)
    argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    if level == 1:
        fn = lib.uq_bgzf_compress_block_host
        fn.argtypes = argtypes
        fn.restype = C.c_int
    else:
        host_l = lib.uq_bgzf_compress_block_host_l
        host_l.argtypes = argtypes + [C.c_uint32]
        host_l.restype = C.c_int
        fn = lambda *a: host_l(*a, 2)                   # UQ_BGZF_LEVEL2
    out = C.create_string_buffer(65536)
    nout, st = C.c_uint64(), C.c_uint32()
    parts = []
    for at in range(0, len(data), BLOCK):
        block = data[at:at + BLOCK]
        if fn(block, len(block), out, 65536, C.byref(nout), C.byref(st)) or st.value:
            raise RuntimeError('the host compressor failed on the block at byte %d' % at)
        parts.append(out.raw[:nout.value])
    if eof: parts.append(EOF)
    return b''.join(parts)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    eof, level, k = True, 1, 0
    while k < len(argv):
        if argv[k] == '--no-eof': eof = False
        elif argv[k] == '--level' and k + 1 < len(argv) and argv[k + 1] in ('1', '2'):
            k += 1
            level = int(argv[k])
        else:
            print(__doc__, file=sys.stderr)
            return 2
        k += 1
    sys.stdout.buffer.write(compress(sys.stdin.buffer.read(), eof=eof, level=level))
    return 0


if __name__ == '__main__':
    sys.exit(main())
