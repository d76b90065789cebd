"""The decoder's QNAME rendering against exact integer arithmetic.

Four pieces of device code print QNAME lines (emit.hip): the field loop of emit_tile_kernel (text and packed form), its inlined copy in
decode_stream_kernel (behind the staging test, with a wave-per-line fallback), emit_qname_direct under direct_tiles_kernel, and
emit_sizes_kernel, which must agree with all of them on every field's length.  Through encoded FASTQ files they only ever see small
numbers.  Here each of them gets hand-built layouts (qname_layouts.py): every column dtype at its largest value, results at both sides
of every digit-count boundary, of 2**32, 2**63 and at 2**64 - 1, offsets down to -2**63, string tables with empty and 300-byte strings,
prefixes and suffixes of 256 bytes, 0 to 32 columns -- and every byte of the text is compared with O.decode, which computes
`str(int(v) + min)` in Python integers.

Every layout goes through both decoders (ops.decode_fastq; ops.unpack + ops.emit_fastq) on the table geometries uq_decode_fastq
dispatches on:
  S        variable lengths, ACGT at 2 bits, one contiguous quality range                 decode_stream_kernel
  T40      fixed 40 bp, the same alphabets: one chunk per lane                            emit_tile_kernel<true, 5, false, 1>
  T100     fixed 100 bp: pieces of DE_K chunks per lane                                   emit_tile_kernel<true, 5, false, DE_K>
  Gfixed   --notricks with N (3-bit bases) and qualities with gaps: through the tables    emit_tile_kernel<true> (generic)
  Gvar     the same, variable lengths (a contiguous range would take the stream kernel)   emit_tile_kernel<true> (generic)
  D        Gvar's alphabets; one read of 6 000 bases among 96 of 15 - 25: its tile is
           beyond the LDS image                                                           direct_tiles_kernel<true> / <false>
The second decoder runs emit_tile_kernel<false> (and direct_tiles_kernel<false> on D) on every geometry."""
import gzip
import io

import numpy as np
import pytest

import qname_layouts as QL
import uq_oracle as O
from uq_amd import ops, uq

pytestmark = pytest.mark.gpu
GEOMS = ['S', 'T40', 'T100', 'Gfixed', 'Gvar', 'D']


def _assert_geometry(geom):
    """The table properties each case relies on to reach its kernel: a change of the generator must not quietly move it elsewhere."""
    cfg, members, n = QL.tables(geom)
    if geom in ('S', 'T40', 'T100'):
        assert cfg['bits_per_base'] == 2 and cfg['N_qual'] == {} and QL.contiguous(cfg['qualities']) and cfg['bits_per_quality'] == 5
    else:
        assert cfg['bits_per_base'] == 3 and cfg['N_qual'] == {} and not QL.contiguous(cfg['qualities'])
    assert cfg['variable_read_lengths'] == (geom in ('S', 'Gvar', 'D'))
    if geom == 'T40': assert cfg['dna_max'] == 40               # (40 + 14) / 8 = 6 chunks a line: fewer than 2 DE_K
    if geom == 'T100': assert cfg['dna_max'] == 100             # 14 chunks a line: pieces of DE_K
    if geom == 'D':
        L = _seq_lengths(geom)
        # 12 000 bytes of SEQ and QUAL in a tile whose image was sized for the average record: well under 200 bytes + the QNAME line
        assert cfg['dna_max'] == 6000 and L[30] == 6000 and sorted(L)[-2] <= 25 and n == 97
    else:
        assert n > 3 * 64 and n % 64 and n % 63                 # several tiles and a ragged last one


_bare = {}


def _bare_records(geom):
    """Lines 2 - 4 of every record (O.decode with an empty QNAME layout), computed once per geometry."""
    if geom not in _bare:
        text = O.decode(*QL.craft(geom, QL.layout('', '', [])))
        lines = text.split('\n')[:-1]
        assert len(lines) == 4 * QL.tables(geom)[2] and not any(lines[0::4])
        _bare[geom] = [lines[i + 1:i + 4] for i in range(0, len(lines), 4)]
    return _bare[geom]


def _seq_lengths(geom):
    return [len(r[0]) for r in _bare_records(geom)]


class Tables:
    """The packed tables of a geometry on the device, and (lazily) what uq_unpack makes of them."""

    def __init__(self, ctx, geom):
        self.ctx, self.geom = ctx, geom
        self.cfg, members, self.n = QL.tables(geom)
        self.dna = ctx.to_device(np.load(io.BytesIO(members['DNA.raw'])).reshape(-1))
        self.qual = ctx.to_device(np.load(io.BytesIO(members['QUAL.raw'])).reshape(-1))
        self._text = None

    def decode(self, cfg, cols, want_bytes):
        # the size pass first, on its own: the text kernels are only started on record offsets that are right
        size, bad = ops.decode_fastq(self.ctx, cfg, cols, self.dna, self.qual, self.n, size_only=True)
        assert bad is None and size == want_bytes, 'decode_fastq: the size pass reports %d bytes, the oracle\'s text has %d' % (size, want_bytes)
        text, bad = ops.decode_fastq(self.ctx, cfg, cols, self.dna, self.qual, self.n)
        assert bad is None
        return self.ctx.to_numpy(text).tobytes()

    def emit(self, cfg, cols, want_bytes):
        if self._text is None:
            seq, qt, ln, bad = ops.unpack(self.ctx, self.dna, self.qual, self.n, ops.make_unpack_params(self.cfg))
            assert ops.bad_index(bad) is None
            self._text = (seq, qt, ln)
        size = ops.emit_fastq(self.ctx, cfg, cols, *self._text, self.n, size_only=True)
        assert size == want_bytes, 'emit_fastq: the size pass reports %d bytes, the oracle\'s text has %d' % (size, want_bytes)
        return self.ctx.to_numpy(ops.emit_fastq(self.ctx, cfg, cols, *self._text, self.n)).tobytes()

    def both(self, lay, want_bytes):
        cfg, _ = QL.craft(self.geom, lay)
        cols = [self.ctx.to_device(a) for _, a in lay['columns']]
        return [('decode_fastq', self.decode(cfg, cols, want_bytes)), ('unpack + emit_fastq', self.emit(cfg, cols, want_bytes))]


def _same(got, want, what):
    """got == want, with the first differing line in the message."""
    if got == want: return
    g, w = got.split(b'\n'), want.split(b'\n')
    k = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
    show = lambda lines: lines[k][:120].decode('latin-1') if k < len(lines) else '<end of text>'
    raise AssertionError('%s: %d bytes against the oracle\'s %d; line %d of read %d is %r, the oracle has %r'
                         % (what, len(got), len(want), k % 4 + 1, k // 4, show(g), show(w)))


def _check_layouts(ctx, geom, layouts):
    _assert_geometry(geom)
    tab = Tables(ctx, geom)
    for name, lay in layouts.items():
        want = O.decode(*QL.craft(geom, lay)).encode('latin-1')
        for decoder, got in tab.both(lay, len(want)):
            _same(got, want, '%s, %s, layout %s' % (geom, decoder, name))


@pytest.mark.parametrize('geom', GEOMS)
def test_integer_columns_print_exactly(ctx, geom):
    """1(a): uint8 .. uint64 columns, without offset and with `min` from -2**63 to 2**63 - 1; the printed results include `min` itself, the
    dtype's largest value, -1 / 0 / 1, 10**k - 1 and 10**k up to k = 19, 2**32 - 1, 2**32, 2**63 - 1, 2**63 and 2**64 - 1, all inside
    [-2**63, 2**64).  Four columns side by side (a lane per field) and nine (the looped field passes), different separators."""
    _check_layouts(ctx, geom, QL.integer_layouts(QL.tables(geom)[2]))


@pytest.mark.parametrize('geom', GEOMS)
def test_mapping_columns_copy_their_strings(ctx, geom):
    """1(b): tables with the empty string, strings of 1, 16, 17 and 300 bytes, a table of one string, uint8 codes and uint16 codes into 300
    entries; every code addresses its table."""
    _check_layouts(ctx, geom, QL.mapping_layouts(QL.tables(geom)[2]))


@pytest.mark.parametrize('geom', GEOMS)
def test_layout_edges(ctx, geom):
    """1(c): prefixes of 0, 1, 255 and 256 bytes, suffixes of 0 and 256, 0 / 1 / 5 / 32 columns.  No columns: the QNAME is prefix + suffix (a
    branch of its own in both tile kernels); 5 and 32 columns: more (record, field) items in a tile than lanes."""
    _check_layouts(ctx, geom, QL.edge_layouts(QL.tables(geom)[2]))


def test_stream_kernel_staging_boundary(ctx):
    """1(d): geometry S, one mapping column whose strings all have the same length, once for every length from 1 to 80: somewhere on the
    way the QNAME lines of a full tile outgrow the stream kernel's staging area and it writes them a wave per line instead.  Every
    length decodes exactly, the last that is staged and the first that is not included."""
    _assert_geometry('S')
    tab = Tables(ctx, 'S')
    for length in range(1, 81):
        lay = QL.sweep_layout(tab.n, length)
        cfg, members = QL.craft('S', lay)
        cols = [ctx.to_device(a) for _, a in lay['columns']]
        want = O.decode(cfg, members).encode('latin-1')
        _same(tab.decode(cfg, cols, len(want)), want, 'S, decode_fastq, strings of %d bytes' % length)


@pytest.mark.parametrize('geom', ['S', 'T40', 'Gvar'])
def test_values_beyond_the_recorded_max_keep_the_text_whole(ctx, geom):
    """1(e): a damaged container may store integers above the `max` its config records.  The size pass and the render pass share
    field_from_raw, so such a value still prints as itself: the text has the length of its lines, every SEQ / QUAL line is intact,
    and every field reads back as stored + min."""
    _assert_geometry(geom)
    tab = Tables(ctx, geom)
    n = tab.n
    stored = {'uint8': 255, 'uint16': 65535, 'uint32': 2 ** 32 - 1, 'uint64': 2 ** 64 - 2}
    recorded = [('uint8', None, 9), ('uint16', -25, 100), ('uint32', None, 99), ('uint64', 1, 1000)]
    cols = []
    for j, (dt, off, mx) in enumerate(recorded):
        a = np.array([(i * 7 + j) % (mx - (off or 0) + 1) for i in range(n)], dtype=dt)
        a[j::5] = stored[dt]                                                         # every fifth read, a different one per column
        a[64 + j] = stored[dt] - 1
        cols.append(({'format': 'integers', 'dtype': dt, 'offset': off is not None, 'min': off or 0, 'max': mx}, a))
    lay = QL.layout('@d', '#', cols)
    assert all(int(a.max()) + (c['min'] if c['offset'] else 0) > c['max'] for c, a in lay['columns'])
    names = ['@d' + ''.join(str(int(a[i]) + (c['min'] if c['offset'] else 0)) + (QL.SEPS[k] if k < 3 else '') for k, (c, a) in enumerate(lay['columns'])) + '#'
             for i in range(n)]
    bare = _bare_records(geom)
    for decoder, got in tab.both(lay, sum(len(nm) + 1 + sum(len(x) + 1 for x in rec) for nm, rec in zip(names, bare))):
        lines = got.decode('latin-1').split('\n')
        assert len(lines) == 4 * n + 1 and lines[-1] == '', decoder
        for i in range(n):
            assert lines[4 * i + 1:4 * i + 4] == bare[i], (decoder, i)
            assert lines[4 * i] == names[i], (decoder, i)


# ---- through the CLI: containers written with O.write_tar from hand-built layouts
def _cli_decode(ctx, path, flags):
    args = uq.build_parser().parse_args(['-i', str(path), '--decode', '--quiet'] + flags)
    uq.validate_args(args)
    out = io.BytesIO()
    s = uq.Session(args, ctx=ctx)
    s.decode(out=out)
    return out.getvalue(), s


@pytest.mark.parametrize('case', ['u8-offset-minus-25', 'u1-offset-2**63+1', 'u2-offset-2**64+1'])
def test_cli_decodes_offsets_at_the_contract_edges(ctx, tmp_path, case):
    """4: (i) a uint64 column with `min` = -25 stays on the device and prints -25 for a stored 0; (ii) / (iii) offsets no int64 holds take the
    host path (qname.decode_names).  Plain, --two-pass-decode and --bgzf all give the oracle's text."""
    import random
    rnd = random.Random(4)
    n = QL.tables('S')[2]
    dtype, mn = {'u8-offset-minus-25': ('uint64', -25), 'u1-offset-2**63+1': ('uint8', 2 ** 63 + 1), 'u2-offset-2**64+1': ('uint16', 2 ** 64 + 1)}[case]
    lay = QL.layout('@cli.', ' end', [QL.int_column('uint8', None, n, rnd), QL.int_column(dtype, mn, n, rnd, beyond=mn > 0)])
    cfg, members = QL.craft('S', lay)
    path = tmp_path / 'crafted.uQ'
    O.write_tar(str(path), cfg, members)
    want = O.decode(cfg, members).encode('latin-1')
    on_device = case == 'u8-offset-minus-25'
    plain, s = _cli_decode(ctx, path, [])
    assert uq.Session.device_text_possible(s.open_container()[1]) == on_device
    _same(plain, want, case)
    _same(_cli_decode(ctx, path, ['--two-pass-decode'])[0], want, case + ' --two-pass-decode')
    _same(gzip.decompress(_cli_decode(ctx, path, ['--bgzf'])[0]), want, case + ' --bgzf')
    first = want.split(b'\n')[::4][list(lay['columns'][1][1]).index(0)]
    assert first.endswith(b'%d end' % mn)                       # the read that stores 0 prints `min` itself
