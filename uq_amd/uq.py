#!/usr/bin/env python3
"""uq -- FASTQ <-> uQ (tar of .npy arrays + config.json) on MI355X.  Drop-in for the reference script:

    python -m uq_amd.uq -i reads.fastq [--sort DNA|QUAL|QNAME|None] [--raw DNA QUAL QNAME] [--pattern a b]
                        [--notricks] [--pad] [--peek] [--test [--compressor CMD | --device-compressor]] [-o out.uQ] [--temp DIR]
    python -m uq_amd.uq -i reads.fastq.uQ --decode > reads.fastq

Same thirteen flags and validation as uq.py:21-71, same container (uq.py:897-913), same function names
for the seams of the hot path -- `encoder_fixed`, `encoder_variable`, `write_pattern`, `write_out`,
`test_patterns`, `run_mix`, `encode_dna_qual`, `encode_qname`, `load_from_tar`, `split_bits` -- as
methods of `Session` (the reference keeps their shared state in module globals).  Every O(N*L) step
runs on the GPU through the C ABI (uq_amd._lib); there is no CPU fallback.  Between the passes the
tables stay in HBM (the reference parks them in <temp>/*.temp files to save RAM, uq.py:710-711, 734).

Deliberate fixes of reference defects: Q5 private temp dir, Q6 members written
and decoded in numeric order, Q4 compressors spawned on demand, Q13/Q21 clear errors, Q17 stable ties,
Q19/Q25 decoder works on codes.
"""
import argparse
import io
import json
import os
import shutil
import subprocess
import sys
import tarfile
import tempfile
import time

import numpy as np

from .errors import UqError, error

# compressed bytes per chunk of a gzip file that is not BGZF, inflated on the device
GZIP_STREAM_CHUNK = 1 << 18

PATTERNS = ['0.1', '1.1', '2.1', '3.1', '0.2', '1.2', '2.2', '3.2']


def whole_records(nlines, what=None):
    """The reads of a text of `nlines` lines, or the refusal of a line count that is not whole records (uq.py:85-87, its missing spaces
    included); `what` names the text where a session holds more than one."""
    if nlines % 4 != 0:
        if what is None: error('ERROR: The FASTQ file provided contains' + str(nlines) + 'rows, which is not divisible by 4!')
        error('ERROR: %s contains %d rows, which is not divisible by 4!' % (what, nlines))
    if nlines == 0: error('ERROR: empty input')
    return nlines // 4


def build_parser():
    p = argparse.ArgumentParser(description='This tool converys FASTQ files to microq (uQ) files and back.')
    p.add_argument('-i', '--input', required=True, help='Required. Input FASTQ/uQ file path.')
    p.add_argument('-o', '--output', help='Optional. FASTQ->uQ only. Default is to append .uQ to input filename.')
    p.add_argument('--compressor', action='store', help='Optional. Path to compression program that accepts data on stdin and prints to stdout/pipe)')
    p.add_argument('--sort', action='store', help='Optional. [DNA/QUAL/QNAME/None] Resort FASTQ. See output of --test for optimium method.')
    p.add_argument('--raw', nargs='+', metavar='file name', help='Optional. [DNA/QUAL/QNAME/None] Store tables raw rather than unique & sorted + key.')
    p.add_argument('--pattern', nargs='+', metavar='pattern', help='Optional. [0.1/0.2/1.1/1.2/2.1/2.2/3.1/3.2] x2 (DNA|QUAL) See output of --test for optimium.')
    p.add_argument('--temp', help='Optional. Directory to write temporary files to. Default is OS dependant.')
    p.add_argument('--test', action='store_true', default=False, help='Optional. Try all possible sort/raw/pattern combinations.')
    p.add_argument('--notricks', action='store_true', default=False, help='Optional. Prevents conversion of N to the most popular base.')
    p.add_argument('--pad', action='store_true', default=False, help='Optional. Pads DNA/QUAL to the nearest 2/4/8 bits.')
    p.add_argument('--peek', action='store_true', default=False, help='Optional. No output files are created, the input is just scanned.')
    p.add_argument('--decode', action='store_true', default=False, help='Requred if you want to convert a .uQ back to .fastq')
    p.add_argument('--device', type=int, default=int(os.environ.get('LOCAL_RANK', '0')), help='GPU index (extension)')
    p.add_argument('--quiet', action='store_true', default=False, help='suppress the analysis report (extension)')
    p.add_argument('--host-qname', action='store_true', default=False, help='run the QNAME passes sequentially on the host (extension)')
    p.add_argument('--host-inflate', action='store_true', default=False,
                   help='inflate gzip input that is not BGZF on the host (zlib, one thread) instead of in parallel chunks on the GPU (extension)')
    p.add_argument('--exact-qname', action='store_true', default=False,
                   help='run the QNAME passes as kernels of their own (layout, then tokeniser) instead of inside the pack kernel (extension)')
    p.add_argument('--multi-pass', action='store_true', default=False,
                   help='census, record index, statistics and pack as separate passes over the stream; the default counts the statistics in the pack kernel, '
                        'packing speculatively with decisions guessed from the head of the file and verified afterwards (extension)')
    p.add_argument('--two-pass-decode', action='store_true', default=False,
                   help='decode through the fixed-pitch text arrays (uq_unpack + uq_emit_fastq) instead of the fused kernel (extension)')
    p.add_argument('--bgzf', action='store_true', default=False,
                   help='with --decode: write BGZF-compressed FASTQ (what bgzip writes), deflated on the GPU (extension)')
    p.add_argument('--gz', action='store_true', default=False,
                   help='write the container BGZF-compressed (reads.fastq.uQ.gz), its tables deflated on the GPU; --decode reads such a file, and '
                        'any gzip of a .uQ, by its content (extension)')
    p.add_argument('--device-compressor', action='store_true', default=False,
                   help='with --test: size every candidate on the GPU with the built-in deflate sizer (its size as BGZF from this '
                        "project's own compressor) instead of piping it through --compressor (extension)")
    p.add_argument('--bgzf-level', type=int, default=None, metavar='{1,2}',
                   help='the level of the GPU deflate compressor under --decode --bgzf, --gz and --test --device-compressor: 1 (the default, '
                        'fast) or 2 (more match candidates and a lazy parse: smaller, slower) (extension)')
    p.add_argument('--verify', action='store_true', default=False,
                   help='after the container is written: read it back from the disk, decode it on the GPU and compare the record fingerprint of the '
                        'decoded text with the input\'s -- the same reads in the same order, or with --sort the same reads as a multiset; exit '
                        'status 1 and a diagnosis if not (extension)')
    p.add_argument('--fingerprint', action='store_true', default=False,
                   help='print the record fingerprint (uqfp1, DESIGN.md section 19: not cryptographic) of the input FASTQ as one JSON line and '
                        'write no container; with --decode: of the decoded text, and write no text (extension)')
    p.add_argument('--qc', action='store_true', default=False,
                   help='print the per-cycle base and quality tables, the read-length, mean-quality and GC histograms (uqqc1, DESIGN.md section 24) of '
                        'the input FASTQ as one JSON line and write no container; with --bin-qual: of the binned text; with --decode: of the decoded '
                        'text, and write no text (extension)')
    p.add_argument('--qc-cycles', type=int, default=None, metavar='N',
                   help='with --qc: the number of exact cycles, 1 .. 1024 (the default); positions from N on are counted together under "beyond" (extension)')
    from . import binqual
    p.add_argument('--bin-qual', action='store', default=None, metavar='SPEC', help=binqual.HELP)
    from . import recfilter
    p.add_argument('--filter', action='store', default=None, metavar='SPEC', help=recfilter.HELP)
    from . import rectrim
    p.add_argument('--trim', action='store', default=None, metavar='SPEC', help=rectrim.HELP)
    from . import adapters
    p.add_argument('--adapter', action='store', default=None, metavar='SPEC', help=adapters.HELP)
    from . import recdedup
    p.add_argument('--dedup', action='store', default=None, metavar='SPEC', help=recdedup.HELP)
    p.add_argument('--mate2', action='store', default=None, metavar='R2.fastq',
                   help='paired-end input: -i is R1, this is R2 (plain, BGZF or other gzip, each by its content).  The read counts must be equal and '
                        'read r of R2 must be the mate of read r of R1 (same QNAME up to the first space or tab, /1 with /2 allowed); the two '
                        'files are interleaved on the GPU (R1 record, its R2 record, ...) and the container is the plain encode of that '
                        'text, with a "paired" key in config.json (DESIGN.md section 25) (extension)')
    p.add_argument('--interleaved', action='store_true', default=False,
                   help='paired-end input in one file that already alternates R1 and R2: the mates are checked on the GPU and config.json '
                        'gets the "paired" key (extension)')
    p.add_argument('--split-mates', nargs=2, default=None, metavar=('OUT1', 'OUT2'),
                   help='with --decode of a paired container: write mate 1 (the even records) to OUT1 and mate 2 (the odd records) to OUT2 '
                        'instead of the interleaved text to stdout; with --bgzf both BGZF-compressed (extension)')
    return p


def validate_args(args):
    """uq.py:52-71, including the case quirks of Q1."""
    if args.pattern:
        if len(args.pattern) != 2: error('ERROR: There must be 2 values for --pattern!')
        elif not all(p in PATTERNS for p in args.pattern): error('ERROR: Pattern values are incorrect!')
    if args.sort:
        if args.sort.lower() not in ['dna', 'qual', 'qname', 'none']: error('ERROR: --sort value is incorrect!')
        if args.sort.lower() == 'none': args.sort = (None,)
    if args.raw:
        if not all(r.lower() in ['dna', 'qual', 'qname', 'none'] for r in args.raw): error('ERROR: --raw values are incorrect!')
        args.raw = set(args.raw)
        if 'none' in args.raw:
            args.raw.add(None); args.raw.discard('none')
    if args.bgzf and not args.decode: error('ERROR: --bgzf compresses decoded FASTQ: use it together with --decode')
    if args.gz:
        if args.decode: error('ERROR: --gz compresses the container the encoder writes: --decode recognises a compressed container by itself')
        if args.peek: error('ERROR: --gz compresses the container the encoder writes: --peek writes none')
    if args.device_compressor:
        if args.compressor: error('ERROR: --device-compressor and --compressor are two ways to size the same candidates: give one of them')
        if not args.test: error('ERROR: --device-compressor sizes the candidates of --test: use it together with --test')
    if args.bgzf_level is not None:
        if args.bgzf_level not in (1, 2): error('ERROR: --bgzf-level is 1 or 2')
        if not ((args.bgzf and args.decode) or args.gz or (args.device_compressor and args.test)):
            error('ERROR: --bgzf-level sets the level of the GPU deflate compressor: use it together with --decode --bgzf, --gz or '
                  '--test --device-compressor')
    if args.verify:
        if args.decode: error('ERROR: --verify checks the container an encode writes: it does not go with --decode')
        if args.peek: error('ERROR: --verify reads back the container the encoder writes: --peek writes none')
        if args.test: error('ERROR: --verify does not go with --test: encode with the parameters --test found, then verify that file')
        if args.fingerprint: error('ERROR: --fingerprint writes no container, so there is nothing for --verify to read back')
    if args.fingerprint:
        if args.bgzf: error('ERROR: --fingerprint writes no text, so there is nothing for --bgzf to compress')
        if args.gz or args.peek or args.test or args.output:
            error('ERROR: --fingerprint only reads: it does not go with --gz, --peek, --test or -o')
    if args.qc_cycles is not None:
        if not args.qc: error('ERROR: --qc-cycles sets the number of exact cycles of --qc: use it together with --qc')
        if not 1 <= args.qc_cycles <= 1024: error('ERROR: --qc-cycles is 1 .. 1024')
    if args.qc:
        if args.bgzf: error('ERROR: --qc writes no text, so there is nothing for --bgzf to compress')
        if args.verify: error('ERROR: --qc writes no container, so there is nothing for --verify to read back')
        if args.fingerprint: error('ERROR: --qc and --fingerprint each print their own line: run them one after the other')
        if args.gz or args.peek or args.test or args.output:
            error('ERROR: --qc only reads: it does not go with --gz, --peek, --test or -o')
    if args.bin_qual is not None:
        if args.decode: error('ERROR: --bin-qual changes the qualities an encode stores: the text --decode writes is what the container holds')
        bin_qual_table(args.bin_qual)
    if args.filter is not None:
        if args.decode: error('ERROR: --filter drops reads before an encode stores them: the text --decode writes is what the container holds')
        filter_criteria(args.filter)
    if args.trim is not None:
        if args.decode: error('ERROR: --trim cuts reads before an encode stores them: the text --decode writes is what the container holds')
        trim_steps(args.trim)
    if args.adapter is not None:
        if args.decode: error('ERROR: --adapter cuts reads before an encode stores them: the text --decode writes is what the container holds')
        if adapter_criteria(args.adapter)[0]['seq2'] is not None and args.mate2 is None and not args.interleaved:
            error('ERROR: --adapter %s: seq2 is the second mates\' adapter: use it together with --mate2 or --interleaved' % args.adapter)
    if args.dedup is not None:
        if args.decode: error('ERROR: --dedup drops reads before an encode stores them: the text --decode writes is what the container holds')
        dedup_criteria(args.dedup)
    mate2, interleaved, split = args.mate2, args.interleaved, args.split_mates
    if mate2 is not None and interleaved:
        error('ERROR: --mate2 and --interleaved are two forms of the same input: give R1 with -i and R2 with --mate2, or one interleaved file with --interleaved')
    if mate2 is not None or interleaved:
        flag = '--mate2' if mate2 is not None else '--interleaved'
        if args.decode: error('ERROR: %s describes the FASTQ an encode reads: it does not go with --decode (a paired container says so itself; see --split-mates)' % flag)
        if isinstance(args.sort, str) and args.sort.lower() in ('dna', 'qual', 'qname'):
            error('ERROR: --sort %s tears mates apart: a paired container keeps R1 and R2 of a pair next to each other, so %s does not go with --sort' % (args.sort, flag))
    if split is not None:
        if not args.decode: error('ERROR: --split-mates writes the two mates of a paired container: use it together with --decode')
        if args.fingerprint or args.qc: error('ERROR: --fingerprint and --qc write no text, so there is nothing for --split-mates to split')
        if os.path.abspath(split[0]) == os.path.abspath(split[1]): error('ERROR: --split-mates needs two different output files')
    if not os.path.isfile(args.input): error('ERROR: Sorry, the input path you have specified is not a file!')
    if mate2 is not None and not os.path.isfile(mate2): error('ERROR: Sorry, the --mate2 path you have specified is not a file!')
    return args


def bin_qual_table(spec):
    """--bin-qual SPEC -> (the 256-byte table, the explicit form of the spec); a bad spec is a UqError."""
    from . import binqual
    return binqual.parse(spec), binqual.explicit(spec)


def filter_criteria(spec):
    """--filter SPEC -> (the criteria of uq_filter_params, the explicit form of the spec); a bad spec is a UqError."""
    from . import recfilter
    return recfilter.parse(spec), recfilter.explicit(spec)


def dedup_criteria(spec):
    """--dedup SPEC -> (prefix and flags of uq_dedup_params, the explicit form of the spec); a bad spec is a UqError."""
    from . import recdedup
    return recdedup.parse(spec), recdedup.explicit(spec)


def trim_steps(spec):
    """--trim SPEC -> (the steps of uq_trim_params, the explicit form of the spec); a bad spec is a UqError."""
    from . import rectrim
    return rectrim.parse(spec), rectrim.explicit(spec)


def adapter_criteria(spec):
    """--adapter SPEC -> (seq, seq2, err, overlap as adapters.parse gives them, the explicit form of the spec); a bad spec is a UqError."""
    from . import adapters
    return adapters.parse(spec), adapters.explicit(spec)


def npy_header(shape, fortran_order, dtype):
    """The .npy v1.0 header numpy.save writes for this array (uq.py:263-274 via numpy)."""
    f = io.BytesIO()
    np.lib.format.write_array_header_1_0(f, {'descr': np.lib.format.dtype_to_descr(np.dtype(dtype)),
                                             'fortran_order': bool(fortran_order), 'shape': tuple(int(s) for s in shape)})
    return f.getvalue()


def pattern_header(rows, cols, pattern):
    """Shape / fortran_order of numpy.save(asXarray(rot90(table, k))) -- SURVEY.md A.4, Q22."""
    k = int(pattern[0])
    shape = (rows, cols) if k % 2 == 0 else (cols, rows)
    fortran = pattern.endswith('.2') and min(shape) > 1     # 1-wide arrays are C- and F-contiguous: numpy says False
    return npy_header(shape, fortran, np.uint8)


class Session:
    """One encode (or decode) run: the reference's module-level state as an object."""

    def __init__(self, args, ctx=None, out=sys.stdout):
        from . import ops
        from .device import Context
        self.ops = ops
        self.args = args
        self.ctx = ctx or Context(args.device)
        from .hostio import Staging
        self.io = Staging(self.ctx)
        self.out = out
        self.members = {}          # name -> (npy header bytes, payload: device tensor or numpy array), uq.py:272-274
        self.tables = {}           # 'DNA' / 'QUAL' -> (device tensor, rows, cols); 'QNAME' -> [device column tensors]
        self.columns = []
        self.config = {}
        self.t0 = time.time()
        self.split = self.t0
        self.last_subprocess_used = 0
        self.tar_mtime = None      # the mtime of the tar headers write_container writes (None: now)
        self.gz_bytes = None       # --gz: the bytes of the file written
        self.gz_layout = None      # --gz: name -> {'frame': (offset, bytes), 'data': (offset, bytes)} in the compressed file
        self.tar_path = None
        self.source = None         # decode: the container's byte source (uq_amd/container.py)
        self.path = None           # the plain FASTQ file `load` read (None: no file holds the bytes of d_buf)
        self._host = None          # host copy of the FASTQ bytes, made on first use (`host`)
        self.side = None           # the second context the head guess runs on, made by the first queued load and kept
        self.index_only = False    # --fingerprint / --qc: the load stops at the line count
        self.pairing = None        # --mate2 / --interleaved: config.json's "paired" value
        self.bin_qual_ranges = None    # --bin-qual: the explicit form of the spec
        self.binned_changed = 0    # --bin-qual: quality characters this session's binning changed
        self.filtering = None      # --filter: config.json's "filter" value (spec, criteria, unit, report)
        self.deduping = None       # --dedup: config.json's "dedup" value (spec, criteria, unit, seed, report)
        self.trimming = None       # --trim: config.json's "trim" value (spec, criteria, report)
        self.adapting = None       # --adapter: config.json's "adapter" value (spec, criteria, report)
        self._pre_index = None     # --trim, --filter: (reads, record index) of the buffer a paired loader or trim_records hands on, until the next step of load_device takes it
        self.d_buf = None          # the FASTQ text in HBM (uint8 device tensor)
        self.total = 0             # reads in d_buf
        self.d = None              # analyse: the decisions of analysis.decide_from_stats
        self.hs = None             # analyse: the host copy of the statistics (ops.HostStats)
        self.qname_arrays = []     # analyse: one array of values per QNAME column
        self.load_path = None      # which pipeline load_device took
        self.pack_path = None      # 'speculative' (the load's tables were kept) or 'plain'
        self.qname_path = None     # 'fused', 'device', 'host-native' or 'host-python'
        self.gzip_path = None      # gzip input: how it was inflated
        self.gzip_stream_info = None   # gzip input that is not BGZF: what ops.gzip_stream_to_device reports
        self._reset_load_state()

    def _reset_load_state(self):
        """What one load leaves for analyse and pack, back to empty: load_device does this first."""
        self._d_ls = None          # the record index (`d_ls`), expanded on first use
        self._spec = None          # (guessed uq_pack_params, dna, qual, bad) of a speculative pack, until _encode takes or drops it
        self._fq = None            # the ops.FusedQname the pack kernel filled, until analyse_qname takes it
        self._guess_shared = False  # the QNAME guess has been handed to share_qname_guess in this load
        self.d_stats = None        # the statistics in HBM (device uq_stats)
        self.load_path = None

    def say(self, *a):
        if not self.args.quiet:
            print(*a, file=self.out)

    def split_time(self):
        now = time.time(); d = now - self.split; self.split = now
        return '(' + str(d / 60) + ' minutes)'

    last_params = None         # uq_pack_params of the previous encode in this process

    # ------------------------------------------------------------------ passes 1-2 (analysis)
    def load(self, path):
        """Read the FASTQ, put it in HBM, build the record index.  Replaces `wc -l` + line iteration."""
        ops, ctx = self.ops, self.ctx
        if os.path.getsize(path) == 0: error('ERROR: empty input')
        if ops.is_gzip(path): return self.load_gzip(path)
        self.path, self._host = path, None
        # pinned, chunked, file reads overlapped with the PCIe copies; the newline census of a chunk is queued right behind its
        # copy (row f2), so that only the scan of the per-tile counts is left when the last byte lands
        census = {}

        def on_chunk(d, lo, n):
            if 'c' not in census: census['c'] = ops.ChunkedCensus(ctx, d)
            census['c'].chunk(lo, n)
        chunked = self.io.chunk % (16 << 10) == 0
        self.d_buf = self.io.file_to_device(path, on_chunk=on_chunk if chunked else None)
        self.load_device(census=census.get('c'))       # (the text is handed over in `d_buf`, no name of it kept here: --filter frees it)

    def load_gzip(self, path):
        """gzip input (an extension: the reference reads plain text only), recognised by its magic bytes: gzip_to_device, then load_device."""
        self.d_buf = self.gzip_to_device(path)
        self.path, self._host = None, None             # the file holds compressed bytes: the host copy (`host`) comes from d_buf
        self.load_device()

    def gzip_to_device(self, path):
        """A gzip file's text as a device buffer.  BGZF (every member carries its
        compressed size): the compressed file goes to HBM, the member headers are walked on the host, every member inflates on the device
        into its slice of one buffer (uq_inflate_members).  Any other gzip goes to HBM compressed and inflates there in parallel chunks
        (uq_gzip_stream_*, GZIP_STREAM_CHUNK bytes each); --host-inflate: on the host (zlib), streamed to HBM."""
        ops, ctx = self.ops, self.ctx
        kind, members, total, err = ops.gzip_scan(np.memmap(path, dtype=np.uint8, mode='r'))
        if kind == ops.GZIP_MALFORMED: error('ERROR: %s is not a readable gzip file: %s' % (path, err[0]))
        if kind == ops.GZIP_BGZF:
            self.gzip_path = 'BGZF, %d members inflated on the device' % len(members)
            d_comp = self.io.file_to_device(path)
            d_buf, bad = ops.inflate_members(ctx, d_comp, members, total)
            del d_comp
            if bad is not None:
                k, st = bad
                error('ERROR: %s: gzip member %d (deflate data at byte %d): %s' % (path, k, int(members[k]['data_offset']),
                                                                                  ops.INFLATE_STATUS.get(st, 'status %d' % st)))
        elif self.args.host_inflate:
            self.gzip_path = 'gzip inflated on the host'
            import zlib
            try:
                d_buf = self.io.gzip_to_device(path)
            except (zlib.error, EOFError) as e:
                error('ERROR: %s is not a readable gzip file: %s' % (path, e))
        else:
            d_comp = self.io.file_to_device(path)
            try:
                d_buf, info = ops.gzip_stream_to_device(ctx, d_comp, GZIP_STREAM_CHUNK)
            except ops.GzipStreamError as e:
                error('ERROR: %s is not a readable gzip file: %s' % (path, e))
            finally:
                del d_comp
            self.gzip_stream_info = info
            self.gzip_path = 'gzip, %d chunks inflated on the device' % info['chunks']
        if d_buf.numel() == 0: error('ERROR: empty input')
        return d_buf

    def text_to_device(self, path):
        """One input file of either kind -> its FASTQ text in HBM, without load_device (the paired loader: the single-input path keeps its
        chunked census behind the PCIe copies, `load`)."""
        if os.path.getsize(path) == 0: error('ERROR: empty input')
        return self.gzip_to_device(path) if self.ops.is_gzip(path) else self.io.file_to_device(path)

    # ------------------------------------------------------------------ paired-end input
    def load_input(self):
        """The input of an encode (or of --fingerprint / --qc) in HBM: one file, two mates interleaved on the device, or one interleaved file."""
        args = self.args
        if args.mate2 is not None: return self.load_pairs(args.input, args.mate2)
        if args.interleaved and (args.filter is not None or args.dedup is not None): return self.load_interleaved_filtered(args.input)
        self.load(args.input)
        if args.interleaved: self.check_interleaved()

    def load_interleaved_filtered(self, path):
        """--interleaved --filter (or --dedup): the mates are checked on the input as it is given, BEFORE load_device drops reads: text to HBM, index, even
        read count, uq_mate_check, then load_device (which filters, and checks the mates of what is left once more)."""
        d_buf = self.text_to_device(path)
        n, ls = self.indexed(d_buf, None)
        if n % 2: error('ERROR: --interleaved: the input holds %d reads, an odd number: R1 and R2 do not alternate' % n)
        self.require_mates(d_buf, ls, 0, 2, d_buf, ls, 1, 2, n // 2)
        self.path, self._host = None, None
        self._pre_index = (n, ls)
        self.d_buf = d_buf
        del d_buf, ls
        self.load_device()

    def indexed(self, d_buf, what):
        """(reads, record index) of a text in HBM."""
        nlines = self.ops.count_lines(self.ctx, d_buf)
        return whole_records(nlines, what), self.ops.index_lines(self.ctx, d_buf, nlines)

    def require_mates(self, d_a, ls_a, first_a, step_a, d_b, ls_b, first_b, step_b, npairs):
        """uq_mate_check over the pairs; a pair that does not match is a refusal, with its two QNAME lines fetched from HBM."""
        ops, ctx = self.ops, self.ctx
        d_rep = ops.mate_report_new(ctx)
        ops.mate_check(ctx, d_rep, d_a, ls_a, first_a, step_a, d_b, ls_b, first_b, step_b, npairs)
        rep = ops.mate_report_fetch(ctx, d_rep)
        if rep['mismatches']:
            k = rep['first_mismatch']

            def qname_line(d, ls, r):
                lo, hi = (int(v) for v in ctx.to_numpy(ls[4 * r:4 * r + 2], np.uint64))
                return ctx.to_numpy(d[lo:hi - 1]).tobytes().decode('latin-1')
            error('ERROR: pair %d: %s and %s are not mates (%d of %d pairs differ)' % (
                k, qname_line(d_a, ls_a, first_a + k * step_a), qname_line(d_b, ls_b, first_b + k * step_b), rep['mismatches'], rep['pairs']))
        self.pairing = {'layout': 'interleaved', 'pairs': rep['pairs'], 'slash_pairs': rep['slash_pairs']}

    def load_pairs(self, path1, path2):
        """-i R1 --mate2 R2: both files to HBM by the loaders of their kinds, lines counted and indexed, equal read counts, uq_mate_check,
        uq_interleave_records into a new buffer (the inputs are freed), then load_device as for a file with those bytes."""
        ops, ctx = self.ops, self.ctx
        d_1 = self.text_to_device(path1)
        d_2 = self.text_to_device(path2)
        n1, ls_1 = self.indexed(d_1, 'R1 (%s)' % path1)
        n2, ls_2 = self.indexed(d_2, 'R2 (%s)' % path2)
        if n1 != n2: error('ERROR: R1 holds %d reads, R2 holds %d' % (n1, n2))
        self.require_mates(d_1, ls_1, 0, 1, d_2, ls_2, 0, 1, n1)
        d_out = ctx.empty(d_1.numel() + d_2.numel())
        ops.interleave_records(ctx, d_1, ls_1, d_2, ls_2, 0, n1, out=d_out)
        ctx.sync()
        del d_1, d_2, ls_1, ls_2
        self.path, self._host = None, None             # no file holds the interleaved bytes: the host copy (`host`) comes from d_buf
        self.d_buf = d_out
        del d_out
        self.load_device()

    def check_interleaved(self):
        """--interleaved, behind `load`: an even read count, and record 2i + 1 the mate of record 2i (one buffer, nothing copied)."""
        if self.total % 2: error('ERROR: --interleaved: the input holds %d reads, an odd number: R1 and R2 do not alternate' % self.total)
        self.require_mates(self.d_buf, self.d_ls, 0, 2, self.d_buf, self.d_ls, 1, 2, self.total // 2)

    def load_device(self, d_buf=None, census=None):
        """The same for FASTQ bytes that are already in HBM (a uint8 device tensor; `census`: an ops.ChunkedCensus of it whose chunks have
        all been queued -- load() queues them behind the PCIe copies).  --trim, --filter, --dedup, --bin-qual first, in that order; then the line count alone (--fingerprint, --qc),
        or the queued step bench.py times, or -- where that does not hold for this file -- the same two reads with the record index,
        or -- where that has no kernel either, and under --multi-pass -- the plain statistics pass.  Same results whichever path."""
        self._reset_load_state()
        if d_buf is not None: self.d_buf = d_buf         # (the loaders of this class leave the text in `d_buf` and pass none: --filter can then free it)
        del d_buf
        if self.args.trim is not None or self.args.adapter is not None:
            self.trim_records(census)
            census = None                                # (the trimmed reads in a buffer of their own; the census of the untrimmed text has been closed)
        if self.args.filter is not None:
            self.filter_records(census)
            census = None                                # (the kept reads in a buffer of their own; the census of the unfiltered text has been closed)
        if self.args.dedup is not None:
            self.dedup_records(census)
            census = None                                # (likewise)
        trimmed = None
        if self._pre_index is not None:                  # --trim without --filter or --dedup: the index uq_trim_records wrote is the trimmed text's
            (n, ls), self._pre_index = self._pre_index, None
            trimmed = (4 * n, ls)
            del ls
        d_buf = self.d_buf
        binned = self.bin_qualities(census) if self.args.bin_qual is not None else trimmed      # (line count, record index)
        del trimmed
        if binned is not None: census = None             # (its census has been closed; the step below runs its own: one more census per encode, with the flag only)
        if self.index_only: return self._load_index_only(census, binned)
        if binned is not None: self._d_ls = binned[1]
        self.load_path = 'multi-pass'
        if self.args.multi_pass or not d_buf.numel():
            self.total = whole_records(census.end() if census is not None else self.ops.count_lines(self.ctx, d_buf))
        elif self._load_queued(census) is None:
            self._load_indexed()
        if self._spec is None: self._load_plain_stats()

    def _load_index_only(self, census, binned):
        """--fingerprint, --qc: the line count and (on first use) the record index, no statistics, no pack."""
        self.load_path = 'index only'
        if binned is not None: nlines, self._d_ls = binned
        else: nlines = census.end() if census is not None else self.ops.count_lines(self.ctx, self.d_buf)
        self.total = whole_records(nlines)

    def _load_queued(self, census):
        """The default, the step bench.py times, queued back to back: the census's closing scan (the line count
        stays on the device) -> the QNAME layout guess from a sample of the reads -> pack + pass-1 statistics + QNAME fields in ONE
        kernel, with decisions guessed from the head of the file (a second context's stream works them out beside the census) and verified
        afterwards against the whole file's counts.  NO record index is written: the kernels walk the census's newline lists; `d_ls` is
        expanded on first use by whatever still wants it (the exact QNAME kernels, the plain packers, the N-trick's first occurrences).
        The stream is read twice.  Sets `total`; returns None, with nothing kept, when the queued form does not hold for this file."""
        ops, ctx, args, d_buf = self.ops, self.ctx, self.args, self.d_buf
        nbytes = int(d_buf.numel())
        if census is None:
            ctx.sync()                                   # (whoever made the buffer may still be writing it: the guess's stream does not wait for this one)
            census = ops.ChunkedCensus(ctx, d_buf)
            census.chunk(0, nbytes)
        census.end_async()
        if self.side is None:
            from .device import SideContext
            self.side = SideContext(ctx)                # the guess's small census / index / statistics must not touch the queued census's state
        g = ops.head_guess(self.side, d_buf, notricks=args.notricks, pad=args.pad, head_bytes=ops.HEAD_BYTES_SMALL, head_reads=ops.HEAD_READS_INDEXED)
        queued, fq, cap = None, None, 0
        if g is not None:
            guess, rpb = g
            cap = int(nbytes * rpb * 1.02) + 1024
            guess.avg_record_bytes = int(1.0 / rpb)
            if self.fused_qname_enabled():
                fq = ops.FusedQname(ctx, cap)
                if self.owns_qname_guess(): ops.qname_guess_async(ctx, d_buf, None, fq)
                self.share_qname_guess(fq)
            queued = ops.pack_stats_async(ctx, d_buf, None, cap, guess, fq=fq)
            if queued is not None and fq is not None: ops.qname_fused_finish(ctx, fq)
        nlines, ok = census.wait()
        if not ok:                                       # a tile with more newlines than a list holds (lines of a few bytes): the bitmap form
            nlines, queued = ops.count_lines(ctx, d_buf), None
        n = self.total = whole_records(nlines)
        if queued is None or n > cap: return None
        self._spec = (guess, queued[0][:n * guess.dna_bytes_per_row], queued[1][:n * guess.quality_bytes_per_row], queued[2])
        self.d_stats = queued[3]
        self.load_path = 'two reads (census; pack + statistics), queued, no record index'
        self._fq = fq
        return self._spec

    def _load_indexed(self):
        """The queued form does not hold for this file (more reads than the head promised, a head without a whole record, a census list
        overflow, an alphabet without a fused kernel): the same two reads through the plain calls, with the record index.  Leaves `_spec`
        None when there is no fused kernel for this file either."""
        ops, ctx, args = self.ops, self.ctx, self.args
        guess = ops.head_guess_indexed(ctx, self.d_buf, self.d_ls, self.total, args.notricks, args.pad)
        if guess is None: return
        fq = None
        if self.fused_qname_enabled() and not self._guess_shared:
            fq = ops.FusedQname(ctx, self.total)
            if self.owns_qname_guess(): ops.qname_guess(ctx, self.d_buf, self.d_ls, self.total, fq)
            self.share_qname_guess(fq)
        res = ops.pack_stats(ctx, self.d_buf, self.d_ls, 0, self.total, guess, fq=fq)
        if res is None: return
        self._spec = (guess,) + res[:3]
        self.d_stats = res[3]
        self.load_path = 'two reads (census; pack + statistics)'
        if fq is not None:
            ops.qname_fused_finish(ctx, fq)
            self._fq = fq

    def _load_plain_stats(self):
        """--multi-pass, and whatever the speculative forms left: the statistics as a pass of their own over the record index."""
        self.d_stats = self.ops.stats_new(self.ctx)
        self.ops.stats_accumulate(self.ctx, self.d_stats, self.d_buf, self.d_ls, 0, self.total)

    def filter_records(self, census=None):
        """--filter, at the head of load_device, in front of bin_qualities (the mean quality is judged on the qualities as given): the records
        of self.d_buf get their verdicts (uq_filter_mark), the kept units their places (uq_filter_plan; a unit is a pair under --mate2 /
        --interleaved) and are copied back to back into a new buffer (uq_compact_records), which replaces self.d_buf; the old one is freed.
        Needs the record index (the census, closed here if load() had begun one, + uq_index_lines -- or what a paired loader left in
        `_pre_index`).  Nothing kept is a refusal before anything is written.  Of a paired text the mates are checked once more on what is
        left, and that report is what `pairing` holds."""
        ops, ctx, args = self.ops, self.ctx, self.args
        d_buf = self.d_buf
        criteria, explicit = filter_criteria(args.filter)
        unit = 2 if (args.mate2 is not None or args.interleaved) else 1
        if self._pre_index is not None: (n, ls), self._pre_index = self._pre_index, None
        else:
            nlines = census.end() if census is not None else (ops.count_lines(ctx, d_buf) if d_buf.numel() else 0)
            if census is not None: census.buf = None     # (closed: it lets go of the unfiltered text)
            n = whole_records(nlines)
            ls = ops.index_lines(ctx, d_buf, nlines)
        if n % unit: error('ERROR: --interleaved: the input holds %d reads, an odd number: R1 and R2 do not alternate' % n)
        d_report = ops.filter_report_new(ctx)
        verdict = ops.filter_mark(ctx, d_report, d_buf, ls, 0, n, ops.filter_params(unit=unit, **criteria))
        src, dst, kept, size = ops.filter_plan(ctx, d_report, ls, 0, n, unit, verdict)
        report = ops.filter_report_fetch(ctx, d_report)
        if kept == 0: error('ERROR: --filter %s keeps none of the %d reads' % (args.filter, n))
        d_out = ops.compact_records(ctx, d_buf, src, dst, kept, out_bytes=size)
        ctx.sync()
        self.d_buf = d_out
        del d_buf, src, dst, verdict, ls               # the unfiltered text is freed here: the loaders of this class keep no name of it (a caller that passed its own tensor to load_device keeps that)
        self.path, self._host = None, None             # no file holds the filtered bytes: the host copy (`host`) comes from d_buf
        self.filtering = {'spec': args.filter, 'criteria': explicit, 'unit': unit, 'report': report}
        if unit == 2:
            nk, ls_k = self.indexed(d_out, None)
            self.require_mates(d_out, ls_k, 0, 2, d_out, ls_k, 1, 2, nk // 2)

    def dedup_records(self, census=None):
        """--dedup, behind filter_records and in front of bin_qualities (duplicates are judged on the reads as trimmed, cut and filtered; keep=best
        on the qualities as given): the units of self.d_buf get their sort keys (uq_dedup_keys), the keys are sorted (uq_argsort_rows), hash-equal
        neighbours are compared byte for byte (uq_dedup_mark) -- with the next seed while two different sequences shared a hash (ops.dedup_verdicts)
        -- and the units that repeat no earlier one are copied back to back into a new buffer (uq_filter_plan with a scratch report,
        uq_compact_records), which replaces self.d_buf; the old one is freed, by the rules filter_records states.  Needs the record index
        (`_pre_index` if the trimmer left one, else the census, closed here, + uq_index_lines).  Of a paired text the mates are checked once
        more on what is left, and that report is what `pairing` holds."""
        ops, ctx, args = self.ops, self.ctx, self.args
        d_buf = self.d_buf
        criteria, explicit = dedup_criteria(args.dedup)
        unit = 2 if (args.mate2 is not None or args.interleaved) else 1
        if self._pre_index is not None: (n, ls), self._pre_index = self._pre_index, None
        else:
            nlines = census.end() if census is not None else (ops.count_lines(ctx, d_buf) if d_buf.numel() else 0)
            if census is not None: census.buf = None     # (closed: it lets go of the text with its duplicates)
            n = whole_records(nlines)
            ls = ops.index_lines(ctx, d_buf, nlines)
        if n % unit: error('ERROR: --interleaved: the input holds %d reads, an odd number: R1 and R2 do not alternate' % n)

        def run_seed(seed):
            params = ops.dedup_params(unit=unit, prefix=criteria['prefix'], flags=criteria['flags'], seed=seed)
            d_report = ops.dedup_report_new(ctx)
            keys = ops.dedup_keys(ctx, d_report, d_buf, ls, 0, n, params)
            perm = ops.argsort_rows(ctx, keys, n // unit, 16)
            verdict = ops.dedup_mark(ctx, d_report, d_buf, ls, 0, n, params, keys, perm)
            return verdict, ops.dedup_report_fetch(ctx, d_report)
        verdict, report, seed = ops.dedup_verdicts(run_seed)
        src, dst, kept, size = ops.filter_plan(ctx, ops.filter_report_new(ctx), ls, 0, n, unit, verdict)
        d_out = ops.compact_records(ctx, d_buf, src, dst, kept, out_bytes=size)
        ctx.sync()
        self.d_buf = d_out
        del d_buf, src, dst, verdict, ls               # the text with its duplicates is freed here (see filter_records)
        self.path, self._host = None, None             # no file holds the deduplicated bytes: the host copy (`host`) comes from d_buf
        self.deduping = {'spec': args.dedup, 'criteria': explicit, 'unit': unit, 'seed': seed, 'report': report}
        if unit == 2:
            nk, ls_k = self.indexed(d_out, None)
            self.require_mates(d_out, ls_k, 0, 2, d_out, ls_k, 1, 2, nk // 2)

    def trim_records(self, census=None):
        """--trim and --adapter, at the head of load_device, in front of filter_records and bin_qualities (the filter judges the reads as trimmed; the
        qualities are judged as given): the records of self.d_buf get their windows (uq_trim_mark under --trim; narrowed by uq_adapter_mark
        under --adapter, which starts from whole lines when there is no --trim) and their places (uq_trim_plan) and are
        copied, cut, back to back into a new buffer (uq_trim_records), which replaces self.d_buf; the old one is freed, by the rules
        filter_records states.  Needs the record index (the census, closed here if load() had begun one, + uq_index_lines -- or what a
        paired loader left in `_pre_index`); the index of the trimmed text, which the copy writes, is handed on in `_pre_index`: --filter
        takes it and censuses nothing.  Reads left without bases are a refusal before anything is written, unless --filter drops them."""
        ops, ctx, args = self.ops, self.ctx, self.args
        d_buf = self.d_buf
        adapter = args.adapter
        if args.trim is not None: steps, explicit = trim_steps(args.trim)
        if adapter is not None: a_criteria, a_explicit = adapter_criteria(adapter)
        if self._pre_index is not None: (n, ls), self._pre_index = self._pre_index, None
        else:
            nlines = census.end() if census is not None else (ops.count_lines(ctx, d_buf) if d_buf.numel() else 0)
            if census is not None: census.buf = None     # (closed: it lets go of the untrimmed text)
            n = whole_records(nlines)
            ls = ops.index_lines(ctx, d_buf, nlines)
        window, report, a_report = None, None, None
        if args.trim is not None:
            d_report = ops.trim_report_new(ctx)
            window = ops.trim_mark(ctx, d_report, d_buf, ls, 0, n, ops.trim_params(**steps))
        if adapter is not None:                         # behind the trimmer's four steps: it narrows their windows (a poly-G tail no longer hides the adapter in front of it)
            paired = args.mate2 is not None or args.interleaved
            flags = (ops.ADAPTER_FRESH if window is None else 0) | (ops.ADAPTER_PAIRED if paired else 0)
            d_areport = ops.adapter_report_new(ctx)
            window = ops.adapter_mark(ctx, d_areport, d_buf, ls, 0, n, ops.adapter_params(
                a_criteria['seq'], (a_criteria['seq2'] or a_criteria['seq']) if paired else None, a_criteria['err'], a_criteria['overlap'], flags), window)
        dst, size = ops.trim_plan(ctx, ls, 0, n, window)
        if args.trim is not None: report = ops.trim_report_fetch(ctx, d_report)
        if adapter is not None: a_report = ops.adapter_report_fetch(ctx, d_areport)
        keeps_bases = args.filter is not None and filter_criteria(args.filter)[0]['min_len'] >= 1
        if report is not None and report['emptied'] and not keeps_bases:
            error('ERROR: --trim %s leaves %d reads without bases; add --filter min-len=1 (or higher)' % (args.trim, report['emptied']))
        if a_report is not None and a_report['emptied'] and not keeps_bases:
            error('ERROR: --adapter %s leaves %d reads without bases; add --filter min-len=1 (or higher)' % (adapter, a_report['emptied']))
        d_out, ls_out = ops.trim_records(ctx, d_buf, ls, 0, n, window, dst, out_bytes=size, index=True)
        ctx.sync()
        self.d_buf = d_out
        del d_buf, window, dst, ls                      # the untrimmed text is freed here (see filter_records)
        self.path, self._host = None, None              # no file holds the trimmed bytes: the host copy (`host`) comes from d_buf
        if report is not None: self.trimming = {'spec': args.trim, 'criteria': explicit, 'report': report}
        if a_report is not None: self.adapting = {'spec': adapter, 'criteria': a_explicit, 'report': a_report}
        self._pre_index = (n, ls_out)

    def bin_qualities(self, census=None):
        """--bin-qual, at the head of load_device: the table of the spec applied to every quality line of self.d_buf, in place
        (uq_requantise_qualities), before the head guess, the statistics, the pack or a fingerprint see the text -- every path works on the
        binned stream only.  Needs the record index (the census, closed here if load() had begun one, + uq_index_lines); newlines do not
        move, so the index stays valid and is handed back: (line count, index); the index is None, and nothing is binned, when the lines
        are not whole records (load_device reports that)."""
        ops, ctx = self.ops, self.ctx
        d_buf = self.d_buf
        lut, self.bin_qual_ranges = bin_qual_table(self.args.bin_qual)
        nlines = census.end() if census is not None else (ops.count_lines(ctx, d_buf) if d_buf.numel() else 0)
        if nlines == 0 or nlines % 4 != 0: return nlines, None
        ls = ops.index_lines(ctx, d_buf, nlines)
        d_changed = ops.changed_new(ctx)
        ops.requantise_qualities(ctx, d_buf, ls, 0, nlines // 4, lut, d_changed)
        self.binned_changed = int(ctx.to_numpy(d_changed).view(np.uint64)[0])
        return nlines, ls

    def binned_changed_in_file(self):
        return self.binned_changed

    # the fused QNAME pass's seams (the sharded session overrides the last two: rank 0's guess is every rank's)
    def fused_qname_enabled(self):
        return not self.args.multi_pass and not self.args.host_qname and not self.args.exact_qname

    def owns_qname_guess(self):
        return True

    def share_qname_guess(self, fq):
        """One GPU: nothing to share (and a fallback may guess again).  The sharded session broadcasts rank 0's structure here -- once per load,
        which is what `_guess_shared` records."""

    @property
    def d_ls(self):
        """The record index (uint64 offset of every line start), expanded when somebody asks for it: the default encode never does."""
        if self._d_ls is None:
            self._d_ls = self.ops.index_lines(self.ctx, self.d_buf, 4 * self.total)
        return self._d_ls

    @d_ls.setter
    def d_ls(self, value):
        self._d_ls = value

    @property
    def host(self):
        """Host copy of the FASTQ bytes: only the sequential QNAME fallback needs it."""
        # (under --bin-qual the file still holds the qualities as given while d_buf holds the binned ones: this copy is read for its QNAME
        # lines only, which binning does not touch)
        if self._host is None:
            self._host = np.fromfile(self.path, dtype=np.uint8) if self.path else self.ctx.to_numpy(self.d_buf)
        return self._host

    # small seams the sharded session (uq_amd/dist_encode.py) overrides
    def fetch_stats(self):
        hs = self.ops.stats_fetch(self.ctx, self.d_stats)
        if hs.incomplete:                        # the speculative pass could not count everything: plain statistics pass
            self._spec = None
            self._load_plain_stats()
            hs = self.ops.stats_fetch(self.ctx, self.d_stats)
        return hs

    def starts_with_at(self):
        return int(self.d_buf[0]) == ord('@')

    def first_seen(self):
        return self.ops.first_occurrence(self.ctx, self.d_buf, self.d_ls, 0, self.total)

    def reads_in_file(self):
        return self.total

    def analyse_qname(self):
        """QNAME passes 1 / 2 / 4: per-read work on the device (qname_device), or -- for QNAMEs outside the
        subset that path reproduces exactly, and with --host-qname -- sequentially on the host."""
        from . import qname, qname_device
        self.qname_path = 'fused'
        fq, self._fq = self._fq, None
        res = qname_device.analyse_fused(self.ctx, fq, self.total) if fq is not None else None
        del fq
        if res is None:
            self.qname_path = 'device'
            res = None if self.args.host_qname else qname_device.analyse_device(self.ctx, self.d_buf, self.d_ls, self.total)
        if res is None:
            self.qname_path = 'host-native'
            h_ls = self.ctx.to_numpy(self.d_ls, np.uint64)
            res = qname.analyse_native(self.host, h_ls, self.total)               # C++ host path
            if res is None:                                                        # regex-special separators etc.: Python path
                self.qname_path = 'host-python'
                res = qname.analyse(qname.qname_lines(self.host, h_ls, self.total))
        return res

    def analyse(self):
        """Pass 1 (histogram, lengths, QNAME layout), the N-trick / width decisions, pass 2 (QNAME typing)."""
        from . import analysis, qname
        args = self.args
        hs = self.fetch_stats()
        if not self.starts_with_at(): error('ERROR: This does not look like a FASTA/FASTQ file! (first line does not start with @)')
        if hs.bad_plus is not None:
            error('ERROR: For entry' + str(hs.bad_plus) + 'the third line does not start with +')
        if hs.bad_len is not None:
            error('ERROR: Length of DNA does not match the length of the quality scores for entry ' + str(hs.bad_len))
        self.hs = hs
        d = analysis.decide_from_stats(hs, notricks=args.notricks, pad=args.pad, first_seen=self.first_seen)
        self.d = d
        try:
            prefix, suffix, separators, columns, arrays = self.analyse_qname()
        except qname.QnameError as e:
            error(str(e))
        self.columns = columns
        self.qname_arrays = arrays
        binning = None
        if args.bin_qual is not None:
            binning = {'spec': args.bin_qual, 'ranges': self.bin_qual_ranges or bin_qual_table(args.bin_qual)[1],
                       'changed': self.binned_changed_in_file()}
            self.say('Binned qualities (%s): %d of %d quality characters changed' % (args.bin_qual, binning['changed'], sum(d['qual_distribution'].values())))
        if self.trimming is not None:
            from . import rectrim
            self.say(rectrim.report_line(self.trimming['report']))
        if self.adapting is not None:
            from . import adapters
            self.say(adapters.report_line(self.adapting['report']))
        if self.filtering is not None:
            from . import recfilter
            self.say(recfilter.report_line(self.filtering['report']))
        if self.deduping is not None:
            from . import recdedup
            self.say(recdedup.report_line(self.deduping['report']))
        self.report(prefix, suffix, separators)
        self.config = {
            'base_distribution': d['base_distribution'], 'qual_distribution': d['qual_distribution'],
            'reads': self.reads_in_file(), 'bases': d['bases'], 'qualities': d['qualities'],
            'variable_read_lengths': d['variable_read_lengths'], 'bits_per_base': d['bits_per_base'],
            'bits_per_quality': d['bits_per_quality'], 'N_qual': d['N_qual'], 'dna_max': d['dna_max'],
            'QNAME_prefix': prefix, 'QNAME_suffix': suffix, 'QNAME_separators': separators, 'QNAME_columns': columns,
        }
        if binning is not None: self.config['quality_binning'] = binning
        if self.trimming is not None: self.config['trim'] = dict(self.trimming)
        if self.adapting is not None: self.config['adapter'] = dict(self.adapting)
        if self.filtering is not None: self.config['filter'] = dict(self.filtering)
        if self.deduping is not None: self.config['dedup'] = dict(self.deduping)
        if self.pairing is not None: self.config['paired'] = dict(self.pairing)

    def report(self, prefix, suffix, separators):
        """The analysis printout of uq.py:459-545 (condensed: same facts, fewer bar charts)."""
        d, say = self.d, self.say
        total_bases = float(sum(d['base_distribution'].values()))
        say('Finished analysing file!', self.split_time())
        say('    - total reads:', self.reads_in_file())
        say('    - total bases:', int(total_bases))
        say('\nQNAME Analysis:')
        if prefix: say('    - all QNAMEs prefixed with:', prefix)
        if suffix: say('    - all QNAMEs suffixed with:', suffix)
        if separators: say('    - QNAME field separators:', separators, '(', len(separators), 'symbols )')
        say('\nDNA Analysis:')
        bases_all = sorted(d['base_distribution'])
        say('    - DNA sequences contained the following characters:', ' '.join(bases_all), '(' + str(len(bases_all)) + ' in total)')
        for b in bases_all:
            pct = d['base_distribution'][b] / total_bases * 100
            say('     ', b, '|' + ('#' * int(pct / 2)).ljust(50) + '|', ('%.3f' % pct).rjust(7) + '%', str(d['base_distribution'][b]).rjust(12))
        for b, code in d['N_qual'].items():
            say('    - The base', b, 'consistently had the same quality value; it is encoded as', d['bases'][0], 'with quality code', code)
        say('    - this means we will store each letter of DNA in', d['bits_per_base'], 'bits.')
        if d['dna_min'] == d['dna_max']: say('    - all DNA sequences are', d['dna_min'], 'bases long')
        else:
            say('    - the largest DNA sequence is', d['dna_max'], 'bases long')
            say('    - the smallest DNA sequence is', d['dna_min'], 'bases long')
        say('    - we will use', d['dna_bytes_per_row'], 'bytes per unique DNA sequence.\n')
        say('QUAL Analysis:')
        quals_all = sorted(d['qual_distribution'])
        for b in bases_all:                                                     # uq.py:520-526: the per-base breakdown
            say('  [Breakdown for "' + b + '"]')
            row = self.hs.counts[ord(b)]
            for q in np.flatnonzero(row):
                pct = int(row[q]) / float(d['base_distribution'][b]) * 100
                say('     ', chr(q), '|' + ('#' * int(pct / 2)).ljust(50) + '|', ('%.3f' % pct).rjust(7) + '%', str(int(row[q])).rjust(12))
            say('')
        say('  [Total distribution]')
        say('    - the following values were seen as quality scores:', ' '.join(quals_all), '(' + str(len(quals_all)) + ' in total)')
        say('    - There distribution is:')
        for q in quals_all:                                                     # uq.py:531-532
            pct = d['qual_distribution'][q] / total_bases * 100
            say('     ', q, '|' + ('#' * int(pct / 2)).ljust(50) + '|', ('%.3f' % pct).rjust(7) + '%', str(d['qual_distribution'][q]).rjust(12))
        nnew = len([c for c in d['N_qual'].values() if c >= len(d['qualities'])])
        if nnew: say('    - as mentioned above,', nnew, 'unique quality scores will be added to the', len(quals_all), 'above.')
        say('    - this means we will store each quality symbol in', d['bits_per_quality'], 'bits.')
        say('    - we will use', d['quality_bytes_per_row'], 'bytes per unique quality sequence.\n')
        for idx, c in enumerate(self.columns):
            say('    - Column', idx + 1, 'is type', c['format'], 'stored as', c['dtype'])

    # ------------------------------------------------------------------ pass 3: the packers
    def _encode(self, variable):
        ops, ctx, d = self.ops, self.ctx, self.d
        p = ops.make_pack_params(d['bases'], d['qualities'], d['N_qual'], d['bits_per_base'], d['bits_per_quality'],
                                 variable, d['dna_bytes_per_row'], d['quality_bytes_per_row'], d['dna_max'], self.hs.max_record_bytes,
                                 avg_record_bytes=self.d_buf.numel() // max(self.total, 1))
        spec, self._spec = self._spec, None
        self.pack_path = 'speculative' if (spec is not None and ops.same_pack_params(p, spec[0])) else 'plain'
        if self.pack_path == 'speculative':
            dna, qual, bad = spec[1:]            # packed while the statistics were counted: the guess was right
        else:
            del spec
            dna, qual, bad = ops.pack(ctx, self.d_buf, self.d_ls, 0, self.total, p)
        Session.last_params = p
        b = ops.bad_index(bad) if bad is not None else None      # (the speculative kernel flags its statistics instead)
        if b is not None: error('ERROR: read %d holds a symbol with no code (internal inconsistency)' % b)
        return ((dna, self.total, d['dna_bytes_per_row']), (qual, self.total, d['quality_bytes_per_row']))

    def encoder_fixed(self):
        """uq.py:108-182 on the session's resident buffer.  Returns ((dna tensor, rows, cols), (qual tensor, rows, cols)).
        The module-level `encoder_fixed(...)` / `encoder_variable(...)` keep the reference's ten-argument signature and
        its `((array, ptr), (array, ptr), lib)` return."""
        return self._encode(False)

    def encoder_variable(self):
        """uq.py:188-254 (adds the sentinel bit above each read's most significant symbol)."""
        return self._encode(True)

    def pack(self):
        """uq.py:705-736: pass 3, and pass 4's column arrays moved to the device."""
        arrays = self.encoder_variable() if self.d['variable_read_lengths'] else self.encoder_fixed()
        self.tables['DNA'], self.tables['QUAL'] = arrays
        self.tables['QNAME'] = [a if self.ctx.torch.is_tensor(a) else self.ctx.to_device(a) for a in self.qname_arrays]

    # ------------------------------------------------------------------ writers
    def write_pattern(self, table, filename):
        """uq.py:257-270.  `table` = (device tensor, rows, cols)."""
        args = self.args
        if args.pattern is None: pattern = '0.1'; args.pattern = ['0.1', '0.1']
        elif filename.startswith('DNA'): pattern = args.pattern[0]
        elif filename.startswith('QUAL'): pattern = args.pattern[1]
        else: error('ERROR: This should never happen!')
        t, rows, cols = table
        payload = t[:rows * cols] if pattern == '0.1' else self.ops.pattern(self.ctx, t, rows, cols, pattern)   # 0.1 is the table itself
        self.members[filename] = (pattern_header(rows, cols, pattern), payload)      # stays in HBM until write_container streams it

    def write_out(self, array, filename, dtype=None):
        """uq.py:272-274: a 1-D array (key or QNAME column) as a .npy member.  `array`: device tensor (with the
        numpy dtype its bytes stand for) or numpy."""
        if isinstance(array, np.ndarray):
            self.members[filename] = (npy_header(array.shape, False, array.dtype), array)
        else:
            self.members[filename] = (npy_header((array.numel(),), False, dtype or self._npdtype(array.element_size())), array)

    def member_bytes(self, name):
        """One member as the bytes numpy.save would have written (tests, --test sizing)."""
        header, payload = self.members[name]
        if not isinstance(payload, np.ndarray): payload = self.ctx.to_numpy(payload)
        return header + payload.tobytes()

    @property
    def device_sizer(self):
        return bool(self.args.device_compressor)

    @property
    def bgzf_level(self):
        """--bgzf-level: the level of every run of the device compressor and of its host twin (1 when not given)."""
        return self.args.bgzf_level or 1

    @property
    def has_compressor(self):
        """--compressor CMD or --device-compressor: the candidates of --test are sized by something."""
        return self.args.compressor is not None or self.device_sizer

    def compressed_size(self, data, tensor=None):
        """uq.py:277-285 (Q4/Q26 fixed: spawn on demand, serialise first, surface errors).  The device form, compressed_size(header,
        tensor): the member is the .npy header `data` followed by the bytes of a device tensor, which stay where they are -- with
        --device-compressor its size as BGZF (uq_deflate_size), otherwise the member goes to the host and through the command."""
        if tensor is not None:
            if self.device_sizer: return self.ops.deflate_size(self.ctx, data, tensor, level=self.bgzf_level)
            data = data + self.ctx.to_numpy(tensor).tobytes()
        if not self.args.compressor: return len(data)
        p = subprocess.run(self.args.compressor + ' | wc -c', shell=True, input=data, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
        if p.returncode != 0: error('ERROR: the compressor command failed')
        self.last_subprocess_used += 1
        return int(p.stdout.split()[0])

    def test_patterns(self, table, filename):
        """uq.py:290-334: size of each candidate layout -> [size, pattern] of the smallest."""
        args = self.args
        t, rows, cols = table
        if not self.has_compressor: return [rows * cols, '0.1']
        if filename.startswith('DNA'): pattern = None if args.pattern is None else args.pattern[0]
        elif filename.startswith('QUAL'): pattern = None if args.pattern is None else args.pattern[1]
        else: error('ERROR: This should never happen!')
        results = []
        pats = PATTERNS if pattern is None else [pattern]
        if self.device_sizer:
            # every layout into the one table-sized buffer and sized there, queued back to back; the totals come back together
            sizes = self.ops.DeflateSizes(self.ctx, len(pats), level=self.bgzf_level)
            payload = self.ctx.empty(rows * cols)
            for pat in pats:
                self.ops.pattern(self.ctx, t, rows, cols, pat, out=payload)
                sizes.add(pattern_header(rows, cols, pat), payload)
            return sorted([size, pat] for size, pat in zip(sizes.fetch(), pats))[0]
        for pat in pats:
            payload = self.ops.pattern(self.ctx, t, rows, cols, pat)
            blob = pattern_header(rows, cols, pat) + self.ctx.to_numpy(payload).tobytes()
            results.append([self.compressed_size(blob), pat])
        return sorted(results)[0]

    # ------------------------------------------------------------------ table builds
    def _npdtype(self, itemsize):
        return {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[itemsize]

    def encode_dna_qual(self, sort_order, table_name, raw, test):
        """uq.py:765-805.  sort_order: None = no sort, False = compute and return, tensor = apply."""
        ops, ctx = self.ops, self.ctx
        t, rows, cols = self.tables[table_name]
        if raw:
            out_name = table_name + '.raw'
            if sort_order is None:
                table = (t, rows, cols)
            else:
                if sort_order is False: sort_order = ops.argsort_rows(ctx, t, rows, cols)       # uq.py:773-775
                table = (ops.gather_rows(ctx, t, rows, cols, sort_order), rows, cols)            # uq.py:777
            if test: test[out_name] = self.test_patterns(table, out_name)
            else: self.write_pattern(table, out_name)
        else:
            out_name = table_name + '.key'
            perm, key, skey, uniq, nu = ops.unique_rows(ctx, t, rows, cols, want_key=sort_order is not False,
                                                        want_sorted_key=sort_order is False)    # uq.py:784-789
            isz = ops.key_itemsize(nu - 1)                                                       # uq.py:790
            if sort_order is None:
                k = ops.narrow(ctx, key, isz)
            elif sort_order is False:
                sort_order = perm                                                                # == argsort(key), stable (uq.py:796)
                k = ops.narrow(ctx, skey, isz)
            else:
                k = ops.narrow(ctx, ops.gather_rows(ctx, key.view(ctx.torch.uint8), rows, 4, sort_order).view(ctx.torch.int32), isz)
            if test: test[out_name] = self.compressed_size(npy_header((k.numel(),), False, self._npdtype(isz)), k)
            else: self.write_out(k, out_name, self._npdtype(isz))
            table = (uniq, nu, cols)
            if test: test[table_name] = self.test_patterns(table, table_name)
            else: self.write_pattern(table, table_name)
        return sort_order

    def encode_qname(self, sort_order, raw, test):
        """uq.py:808-851 on the device: columns stacked into big-endian rows, then the row kernels."""
        ops, ctx, columns = self.ops, self.ctx, self.columns
        cols_d = self.tables['QNAME']
        n = self.total
        common = max(c.element_size() for c in cols_d)
        ncols = len(cols_d)

        def emit(name, tensor, dtype):
            if test: test[name] = self.compressed_size(npy_header((tensor.numel(),), False, np.dtype(dtype)), tensor)
            else: self.write_out(tensor, name, np.dtype(dtype))

        if raw:
            if sort_order is False:
                rows = ops.stack_columns(ctx, cols_d, common)                                    # uq.py:814-815
                sort_order = ops.argsort_rows(ctx, rows, n, ncols * common)                      # uq.py:816
            for idx, column in enumerate(columns):
                c = cols_d[idx]
                if sort_order is not None:
                    c = ops.gather_rows(ctx, c.view(ctx.torch.uint8), n, c.element_size(), sort_order).view(c.dtype)
                emit(column['name'] + '.raw', c, column['dtype'])
        else:
            rows = ops.stack_columns(ctx, cols_d, common)                                        # uq.py:828-829
            perm, key, skey, uniq, nu = ops.unique_rows(ctx, rows, n, ncols * common, want_key=sort_order is not False,
                                                        want_sorted_key=sort_order is False)    # uq.py:830
            isz = ops.key_itemsize(nu - 1)                                                       # uq.py:832
            if sort_order is False:
                sort_order = perm                                                                # uq.py:833
                k = ops.narrow(ctx, skey, isz)
            elif sort_order is None:
                k = ops.narrow(ctx, key, isz)
            else:
                k = ops.narrow(ctx, ops.gather_rows(ctx, key.view(ctx.torch.uint8), n, 4, sort_order).view(ctx.torch.int32), isz)
            emit('QNAME.key', k, self._npdtype(isz))
            for idx, column in enumerate(columns):                                               # uq.py:845-847
                col = ops.unstack_column(ctx, uniq, nu, ncols, common, idx, np.dtype(column['dtype']).itemsize)
                emit(column['name'], col, column['dtype'])
        return sort_order

    def run_mix(self, sorted_on, raw_tables, test):
        """uq.py:739-762: the order of the three table builds and who produces / consumes sort_order."""
        if test: test = {'sorted_on': sorted_on, 'raw_tables': raw_tables}
        if sorted_on in ['DNA', 'QUAL']:
            not_sorted_on = 'DNA' if sorted_on == 'QUAL' else 'QUAL'
            sort_order = self.encode_dna_qual(False, sorted_on, sorted_on in raw_tables, test)
            self.encode_dna_qual(sort_order, not_sorted_on, not_sorted_on in raw_tables, test)
            self.encode_qname(sort_order, 'QNAME' in raw_tables, test)
        elif sorted_on == 'QNAME':
            sort_order = self.encode_qname(False, 'QNAME' in raw_tables, test)
            self.encode_dna_qual(sort_order, 'DNA', 'DNA' in raw_tables, test)
            self.encode_dna_qual(sort_order, 'QUAL', 'QUAL' in raw_tables, test)
        else:
            self.encode_qname(None, 'QNAME' in raw_tables, test)
            self.encode_dna_qual(None, 'DNA', 'DNA' in raw_tables, test)
            self.encode_dna_qual(None, 'QUAL', 'QUAL' in raw_tables, test)
        if test:
            total_size = 0
            for key, value in test.items():
                if key.startswith('QNAME') or key.endswith('key'): total_size += value
                elif key.startswith('DNA') or key.startswith('QUAL'): total_size += value[0]
            test['total_size'] = total_size
        return test

    def run_tests(self):
        """uq.py:855-889: the (raw set x sort) grid, best-of by total size."""
        args, say = self.args, self.say
        all_results = []
        say('Starting tests...')
        say('Time:                       Sort:      Raw Tables:                      Patterns:')
        self.split_time()
        raw_grid = [('DNA', 'QUAL', 'QNAME'), ('DNA', 'QUAL'), ('QUAL', 'QNAME'), ('DNA', 'QNAME'), ('DNA',), ('QUAL',), ('QNAME',), (None,)]
        for raw_tables in (raw_grid if args.raw is None else [args.raw]):
            if not self.has_compressor: args.sort = (None,)
            for to_sort in (['DNA', 'QUAL', 'QNAME', None] if args.sort is None else [args.sort]):
                all_results.append(self.run_mix(to_sort, raw_tables, True))
                say(self.split_time().ljust(27), str(to_sort).ljust(10), str(tuple(raw_tables)).ljust(32), 'All' if args.raw is None else str(args.pattern))
        best = sorted(all_results, key=lambda k: k['total_size'])[0]
        args.sort = best['sorted_on']
        args.raw = best['raw_tables']
        args.pattern = (best['DNA.raw'][1] if 'DNA.raw' in best else best['DNA'][1],
                        best['QUAL.raw'][1] if 'QUAL.raw' in best else best['QUAL'][1])
        say('\nAll done!')
        say('Size (compressed)    Sort:    Raw Tables:                 Raw stats:' if self.has_compressor else
            '             Size    Sort:    Raw Tables:                 Raw stats:')
        for result in sorted(all_results, key=lambda k: k['total_size']):
            rest = {k: v for k, v in result.items() if k not in ('total_size', 'sorted_on', 'raw_tables')}
            say(str(result['total_size']).rjust(17) + '   ', str(result['sorted_on']).ljust(8), str(tuple(result['raw_tables'])).ljust(27),
                ' '.join(str(k) + ':' + str(v) for k, v in rest.items()))
        # uq.py:885-889 (py2 `print x,` soft spaces kept: the line reads the same)
        line = 'Parameters found to be the best for this data type:\n  '
        if args.sort is not None and args.sort != (None,): line += '  --sort ' + str(args.sort)
        if args.raw is not None: line += '  --raw ' + ' '.join(map(str, args.raw))
        if args.pattern is not None: line += '  --pattern ' + ' '.join(map(str, args.pattern))
        say(line)
        return all_results

    # ------------------------------------------------------------------ container
    def closing_config(self):
        """uq.py:897-900: config.json with the parameters of the tables as it is written, and the member names in their order (numeric, Q6)."""
        args = self.args
        cfg = dict(self.config)
        cfg['sort'] = args.sort if isinstance(args.sort, str) else [None]
        cfg['raw'] = sorted(args.raw, key=str) if args.raw else [None]
        cfg['pattern'] = list(args.pattern) if args.pattern else None
        self.config = cfg

        def order(name):
            base = name.split('.')[0]
            if base.startswith('QNAME_'): return (3, int(base[6:]), name)
            return ({'DNA': 0, 'QUAL': 1, 'QNAME': 2}.get(base, 4), 0, name)
        return json.dumps(cfg, indent=4, sort_keys=True).encode(), sorted(self.members, key=order)

    def write_container(self, path):
        """uq.py:897-913: config.json + members into an uncompressed tar."""
        args = self.args
        blob, names = self.closing_config()
        # private temp dir (Q5); beside the output unless --temp says otherwise, so the final move is a rename
        tmpdir = tempfile.mkdtemp(prefix='uq_', dir=args.temp if args.temp else (os.path.dirname(os.path.abspath(path)) or None))

        def pwrite_all(fd, data, pos):
            mv = memoryview(data).cast('B')
            done = 0
            while done < len(mv): done += os.pwrite(fd, mv[done:], pos + done)

        entries = [('config.json', (blob, np.zeros(0, np.uint8)))] + [(k, self.members[k]) for k in names]
        mtime = int(time.time()) if self.tar_mtime is None else int(self.tar_mtime)
        try:
            tmp = os.path.join(tmpdir, 'temp.uq')
            # The tar stream tarfile.open(mode='w').addfile() would write (header block, data, padding to 512,
            # two zero blocks, padding to RECORDSIZE), with the payloads streamed HBM -> pinned -> pwrite.
            fd = os.open(tmp, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            try:
                if args.gz: self.write_gz(fd, entries, mtime, pwrite_all)
                else: self.write_plain(fd, entries, mtime, pwrite_all)
            finally:
                os.close(fd)
            shutil.move(tmp, path)
        finally:
            shutil.rmtree(tmpdir, ignore_errors=True)

    def write_plain(self, fd, entries, mtime, pwrite_all):
        pos = 0
        for name, (header, payload) in entries:
            nbytes = payload.nbytes if isinstance(payload, np.ndarray) else payload.numel() * payload.element_size()
            ti = tarfile.TarInfo(name); ti.size = len(header) + nbytes; ti.mtime = mtime
            head = ti.tobuf(tarfile.DEFAULT_FORMAT, tarfile.ENCODING, 'surrogateescape') + header
            pwrite_all(fd, head, pos); pos += len(head)
            if isinstance(payload, np.ndarray):
                if nbytes: pwrite_all(fd, np.ascontiguousarray(payload), pos)
            else:
                self.io.device_to_fd(payload, fd, pos)
            pos += nbytes
            pad = -ti.size % tarfile.BLOCKSIZE
            if pad: pwrite_all(fd, b'\0' * pad, pos); pos += pad
        end = 2 * tarfile.BLOCKSIZE
        end += -(pos + end) % tarfile.RECORDSIZE
        pwrite_all(fd, b'\0' * end, pos)

    def write_gz(self, fd, entries, mtime, pwrite_all):
        """--gz: the same tar as member-aligned BGZF.  Every member's .npy header + payload is one data part, cut
        into 65 280-byte blocks from its own start and deflated on the device, all parts in one uq_bgzf_compress_parts call; the tar
        framing between the parts (padding + the next header; at the end the closing zeros) is one small member each, compressed on
        the host by the same code.  So a part's bytes in the file are exactly what --test --device-compressor reports for it."""
        from . import container
        ops, ctx = self.ops, self.ctx
        parts, sizes = [], []
        for name, (header, payload) in entries:
            if isinstance(payload, np.ndarray):                # host payloads (config.json's is empty) go up as they are
                payload = ctx.to_device(np.ascontiguousarray(payload).reshape(-1).view(np.uint8)) if payload.nbytes else None
            if len(header) > 256:                              # config.json: all "header", no payload -- it is the part's data
                if payload is not None: error('ERROR: member %s has a header of %d bytes; --gz takes .npy headers of at most 256' % (name, len(header)))
                header, payload = b'', ctx.bytes_to_device(header)
            parts.append((header, payload))
            sizes.append(len(header) + (0 if payload is None else payload.numel() * payload.element_size()))
        frames = [ops.bgzf_block_host(f, level=self.bgzf_level) for f in container.framing_pieces([(e[0], n) for e, n in zip(entries, sizes)], mtime)]
        d_out, part_bytes = ops.bgzf_compress_parts(ctx, parts, level=self.bgzf_level)
        layout = container.member_aligned_layout([len(f) for f in frames], part_bytes)
        src = 0
        for k, entry in enumerate(layout):
            pwrite_all(fd, frames[k], entry['frame'][0])
            if entry['data'] is not None:
                o, n = entry['data']
                if n: self.io.device_to_fd(d_out[src:src + n], fd, o)
                src += n
        end = layout[-1]['frame'][0] + layout[-1]['frame'][1]
        pwrite_all(fd, ops.BGZF_EOF, end)
        self.gz_layout = {e[0]: lay for e, lay in zip(entries, layout)}
        self.gz_layout[None] = layout[-1]
        self.gz_bytes = end + len(ops.BGZF_EOF)

    # ------------------------------------------------------------------ whole encode
    def encode(self):
        args = self.args
        if args.output is None: args.output = args.input + ('.uQ.gz' if args.gz else '.uQ')
        self.say('Warming up...')
        self.load_input()
        self.encode_loaded()
        return self.verify() if args.verify else True

    # ------------------------------------------------------------------ the record fingerprint
    def indexed_input(self):
        """The input FASTQ (plain, BGZF or other gzip) in HBM as for an encode, only the record index built: what ops.fingerprint and ops.qc take."""
        self.index_only = True
        self.load_input()
        return self.ctx, self.d_buf, self.d_ls, self.total

    def fingerprint_input(self):
        """--fingerprint: one JSON line, no container."""
        fp = self.ops.fingerprint(*self.indexed_input())
        print(self.ops.fingerprint_json(fp), file=self.out)
        return fp

    def fingerprint_decoded(self, show=True):
        """--decode --fingerprint: the fingerprint of the text --decode would write (the text stays in HBM)."""
        fp = self.ops.fingerprint(self.ctx, self.decode_to_device())
        if show: print(self.ops.fingerprint_json(fp), file=self.out)
        return fp

    # ------------------------------------------------------------------ the per-cycle tables
    def qc_input(self):
        """--qc: the input FASTQ goes to HBM as for --fingerprint (with --bin-qual it is binned there first); one kernel, one JSON line, no container."""
        qc = self.ops.qc(*self.indexed_input(), ncycles=self.args.qc_cycles or self.ops.QC_MAX_CYCLES)
        print(self.ops.qc_json(qc), file=self.out)
        return qc

    def qc_decoded(self):
        """--decode --qc: the tables of the text --decode would write (the text stays in HBM)."""
        qc = self.ops.qc(self.ctx, self.decode_to_device(), ncycles=self.args.qc_cycles or self.ops.QC_MAX_CYCLES)
        print(self.ops.qc_json(qc), file=self.out)
        return qc

    VERIFY_DECODE_ERRORS = (UqError, RuntimeError, ValueError, IndexError, KeyError, OverflowError, OSError, EOFError)

    def verify(self):
        """--verify: args.output is reopened through the normal decode path -- the bytes on the disk, a --gz file's members and CRCs included
        -- decoded to a device tensor and fingerprinted; the result against the fingerprint of the input text, which is still in HBM.  Without a
        sort `ordered` must be equal, with --sort X `records` (the same reads as a multiset); `reads` and `bases` in both cases.  One line
        either way, also under --quiet; False = not verified (exit status 1), with what the components say about the cause.  The container
        stays where it was written."""
        ops, ctx, args = self.ops, self.ctx, self.args
        show = lambda *a: print(*a, file=self.out)
        want = ops.fingerprint(ctx, self.d_buf, self.d_ls, self.total)
        resorted = args.sort in ('DNA', 'QUAL', 'QNAME')                        # (Q1: any other spelling passes validation and sorts nothing)
        self.members, self.tables = {}, {}                                      # the tables have been written: their HBM is the decoder's now
        dargs = argparse.Namespace(**dict(vars(args), input=args.output, output=None, decode=True, bgzf=False, gz=False, verify=False, quiet=True))
        try:
            got = Session(dargs, ctx=ctx, out=self.out).fingerprint_decoded(show=False)
        except self.VERIFY_DECODE_ERRORS as e:
            show('VERIFY FAILED: %s does not decode: %s' % (args.output, str(e) or type(e).__name__))
            show('    (one known cause: an N-trick base that took a quality code of its own, SURVEY.md Q9 -- encode such a file with --notricks)')
            return False
        self.verify_fingerprints = (want, got)
        hx = lambda v: '%016x' % v
        key = 'records' if resorted else 'ordered'
        if all(want[k] == got[k] for k in ('reads', 'bases', key)):
            line = 'Verified: %s decodes to the same %d reads %s (%s; records %s)' % (
                args.output, want['reads'], 'as a multiset, resorted by --sort ' + args.sort if resorted else 'in the same order',
                key + ' fingerprint equal', hx(got['records']))
            if want['plus_text']: line += '; the text after the + of %d third lines is not kept by the format' % want['plus_text']
            if self.pairing is not None: line += '; %d pairs, mates interleaved' % self.pairing['pairs']
            if self.trimming is not None:                     # `want` was taken from the trimmed text in HBM
                line += '; gives back the reads as --trim %s cut them, %d of %d bases' % (
                    self.trimming['criteria'], self.trimming['report']['bases_out'], self.trimming['report']['bases_in'])
            if self.adapting is not None:                     # ... and cut at the adapters
                line += '; gives back the reads as --adapter %s cut them, %d of %d bases' % (
                    self.adapting['criteria'], self.adapting['report']['bases_out'], self.adapting['report']['bases_in'])
            if self.filtering is not None:                    # `want` was taken from the filtered text in HBM
                line += '; gives back the %d reads --filter kept of %d' % (self.filtering['report']['reads_out'], self.filtering['report']['reads_in'])
            if self.deduping is not None:                     # ... and from the deduplicated text
                line += '; gives back the %d reads --dedup kept of %d' % (
                    self.deduping['report']['reads_in'] - self.deduping['report']['dup_reads'], self.deduping['report']['reads_in'])
            if args.bin_qual is not None:                     # `want` was taken from the binned stream in HBM: the container gives back the binned reads
                line += '; qualities binned by --bin-qual %s, %d characters changed' % (args.bin_qual, self.binned_changed_in_file())
            show(line)
            return True
        show('VERIFY FAILED: %s does not decode to the reads of %s (%s %s, decoded %s)' % (args.output, args.input, key, hx(want[key]), hx(got[key])))
        if want['reads'] != got['reads'] or want['bases'] != got['bases']:
            show('    - the input holds %d reads / %d bases, the decoded text %d / %d' % (want['reads'], want['bases'], got['reads'], got['bases']))
        elif want['pairs'] == got['pairs'] and want['qname'] != got['qname']:
            show('    - the sequence and quality lines are verified (pairs %s); the QNAME lines are not reproduced byte for byte:' % hx(got['pairs']))
            show('      integer QNAME fields are stored as numbers, so leading zeros, a + sign and spaces around them are lost (SURVEY.md Q12)')
        else:
            for k, what in (('dna', 'sequence'), ('qual', 'quality')):
                if want[k] != got[k]: show('    - the %s lines differ (%s %s, decoded %s)' % (what, k, hx(want[k]), hx(got[k])))
            if want['qname'] != got['qname']: show('    - the QNAME lines differ (qname %s, decoded %s)' % (hx(want['qname']), hx(got['qname'])))
            if want['dna'] == got['dna'] and want['qual'] == got['qual'] and want['pairs'] != got['pairs']:
                show('    - every sequence and every quality line is there, but not with its partner (pairs %s, decoded %s)' % (hx(want['pairs']), hx(got['pairs'])))
            elif want['pairs'] == got['pairs'] and want['qname'] == got['qname'] and want['records'] != got['records']:
                show('    - every line is there, but the QNAME lines do not sit on their reads (records %s, decoded %s)' % (hx(want['records']), hx(got['records'])))
        if not resorted and want['records'] == got['records']:
            show('    - the same reads, reordered: the container stores them in another order than the input')
        show('    the container stays where it was written.')
        return False

    def encode_loaded(self, write=True):
        """Everything after the FASTQ is in HBM (`load` / `load_device`).  write=False: stop before the container is
        written -- the members stay in `self.members` (header bytes, device payload)."""
        args = self.args
        self.analyse()
        if args.peek:
            self.say('The config.json would look like:')
            self.say(json.dumps(self.config, indent=4, sort_keys=True))
            return
        self.pack()
        if args.test: self.run_tests()
        if args.sort is None: args.sort = (None,)                                               # uq.py:893-895
        if args.raw is None: args.raw = (None,)
        self.members = {}
        self.run_mix(args.sort, args.raw, False)
        if not write: return
        self.say('\nWriting final config...')
        self.say('Archiving results and cleaning up temp directory...')
        self.write_container(args.output)
        self.say('All Done! :) ')

    # ------------------------------------------------------------------ decode (uq.py:926-1058)
    def load_from_tar(self, members, file_name, pattern='0.1', rows=None):
        """uq.py:943-945 on the device: payload -> table.  `members`: name -> (offset, size) inside the tar
        `self.tar_path`; the payload streams file -> pinned -> HBM.  Returns (device tensor, rows, cols) for
        2-D members; for 1-D ones a device tensor typed by width (its bytes are the member's dtype).
        `rows` = (lo, hi): only that range of rows / elements (the sharded decoder; a row-major payload is read
        as a slice of the file, any other layout whole)."""
        offset, size = members[file_name]
        f = io.BytesIO(self.source.read_host(offset, min(size, 65536)))
        version = np.lib.format.read_magic(f)
        shape, fortran, dtype = np.lib.format.read_array_header_1_0(f) if version == (1, 0) else np.lib.format.read_array_header_2_0(f)
        hdr = f.tell()
        # a .uQ file is untrusted input: the payload must be exactly what the header promises (numpy.load raises on a
        # short member, uq.py:944-945) before any of it is addressed on the device
        want = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize if len(shape) else np.dtype(dtype).itemsize
        if len(shape) not in (1, 2) or hdr + want != size:
            error('ERROR: member %s of this uQ file is damaged (header says %s x %s = %d bytes, the member holds %d)'
                  % (file_name, tuple(shape), np.dtype(dtype).name, want, size - hdr))
        if len(shape) == 1:
            tt = self.ctx.torch
            isz = np.dtype(dtype).itemsize
            lo, hi = rows if rows is not None else (0, shape[0])
            d_pay = self.source.to_device(offset + hdr + lo * isz, (hi - lo) * isz)
            return d_pay.view({1: tt.uint8, 2: tt.int16, 4: tt.int32, 8: tt.int64}[isz])
        k = int(pattern[0])
        nrows, cols = (shape if k % 2 == 0 else shape[::-1])
        if rows is not None and pattern == '0.1':
            lo, hi = rows
            return (self.source.to_device(offset + hdr + lo * cols, (hi - lo) * cols), hi - lo, cols)
        d_pay = self.source.to_device(offset + hdr, size - hdr)
        # numpy flags 1-wide arrays as C order whatever the pattern asked for: the byte stream is the same
        t = d_pay if pattern == '0.1' else self.ops.unpattern(self.ctx, d_pay, nrows, cols, pattern)   # 0.1 is the table itself
        if rows is not None:
            lo, hi = rows
            return (t[lo * cols:hi * cols].contiguous(), hi - lo, cols)
        return (t, nrows, cols)

    def split_bits(self, dna, qual, config):
        """uq.py:1002-1007 + 1031-1054 on the device: rows -> characters (fixed pitch) + lengths."""
        p = self.ops.make_unpack_params(config)
        n = dna[1]
        seq, qt, ln, bad = self.ops.unpack(self.ctx, dna[0], qual[0], n, p)
        b = self.ops.bad_index(bad)
        if b is not None: error('ERROR: row %d of the DNA table carries no length sentinel; is this a uQ file?' % b)
        return seq, qt, ln

    def open_container(self):
        """Tar members (name -> (payload offset, size)) and config.json of args.input."""
        from . import container
        args = self.args
        if self.source is None or self.tar_path != args.input: self.source = container.open_source(self, args.input)
        self.tar_path = args.input
        if self.source.kind != container.PLAIN:
            # a compressed container: the tar is walked by its header fields through the source
            members = container.walk_tar(self.source)
            return members, container.read_config(self.source, members)
        if not tarfile.is_tarfile(args.input):
            error(container.NOT_A_TAR)
        with tarfile.open(args.input) as t:
            members = {m.name: (m.offset_data, m.size) for m in t.getmembers()}
            if 'config.json' not in members: error(container.NO_CONFIG)
            config = json.loads(t.extractfile('config.json').read().decode())
        return members, config

    @property
    def inflated_members(self):
        """BGZF containers: how many of the file's members this session has inflated on the device so far (None for other sources)."""
        return getattr(self.source, 'inflated_members', None)

    def load_tables(self, members, config, rows=None, mate=None):
        """uq.py:943-973 on the device: the DNA / QUAL tables as (tensor, reads, row bytes) and the QNAME columns, in
        stored read order; `rows` = (lo, hi) restricts all of them to that range of reads (keys are sliced, the
        tables they index are loaded whole).  `mate` = 0 / 1 (--split-mates): the even / the odd reads only -- a raw table is
        gathered with a stride-2 index (uq_gather_rows), a key or a raw column is sliced with that stride before it is used."""
        ops, ctx = self.ops, self.ctx
        pat = config['pattern'] or ['0.1', '0.1']

        def half(d):                                                                               # a key or a column: every second element
            return d if mate is None else d[mate::2].contiguous()

        def table(name, pattern):
            if name + '.raw' in members:
                t, nrows, cols = self.load_from_tar(members, name + '.raw', pattern, rows)
                if mate is None: return (t, nrows, cols)
                d_idx = ctx.torch.arange(mate, nrows, 2, dtype=ctx.torch.int64, device=ctx.device)
                return (ops.gather_rows(ctx, t, nrows, cols, d_idx), d_idx.numel(), cols)
            if name in members and name + '.key' in members:
                t, nrows, cols = self.load_from_tar(members, name, pattern)
                d_key = half(self.load_from_tar(members, name + '.key', rows=rows))
                self.check_index(d_key, nrows, name + '.key')
                return (ops.gather_rows(ctx, t, nrows, cols, d_key), d_key.numel(), cols)          # uq.py:953, 957
            error('ERROR: No ' + name + ' data was found in this uQ file?!')

        DNA = table('DNA', pat[0])
        QUAL = table('QUAL', pat[1])
        ncols = len(config['QNAME_columns'])
        u8 = ctx.torch.uint8
        if 'QNAME.key' in members:
            d_key = half(self.load_from_tar(members, 'QNAME.key', rows=rows))
            d_cols = []
            for i in range(ncols):                                                                # uq.py:973, numeric order (Q6)
                c = self.load_from_tar(members, 'QNAME_%d' % (i + 1))
                if i == 0: self.check_index(d_key, c.numel(), 'QNAME.key')
                d_cols.append(ops.gather_rows(ctx, c.view(u8), c.numel(), c.element_size(), d_key).view(c.dtype))
        else:
            d_cols = [half(self.load_from_tar(members, 'QNAME_%d.raw' % (i + 1), rows=rows)) for i in range(ncols)]
        for i, c in enumerate(config['QNAME_columns']):                                           # uq.py:1016 `column['map'][row[i]]`
            if c['format'] == 'mapping': self.check_index(d_cols[i], len(c['map']), 'QNAME column %d' % (i + 1))
        if len({DNA[1], QUAL[1]} | {c.numel() for c in d_cols}) != 1:
            error('ERROR: the tables of this uQ file do not hold the same number of reads')
        return DNA, QUAL, d_cols

    def check_index(self, d_index, limit, what):
        """A stored key / mapping code must address its table: numpy raises IndexError in the reference (uq.py:953-973,
        1016); here the device check runs before the gather / the text kernels use the value."""
        bad = self.ops.check_index_range(self.ctx, d_index, limit)
        if bad is not None:
            error('ERROR: %s of this uQ file is damaged: entry %d points beyond its table of %d rows' % (what, bad, limit))

    @staticmethod
    def device_text_possible(config):
        """Can the device kernels write this file's QNAME lines?  At most 32 columns, prefix and suffix of at most 256 bytes, and integer
        columns they print exactly: stored value + offset inside [-2**63, 2**64), the offset itself an int64.  Other files take
        qname.decode_names (Python integers)."""
        for c in config['QNAME_columns']:
            if c['format'] == 'mapping': continue
            if c.get('offset') and not -2 ** 63 <= int(c['min']) < 2 ** 63: return False
            if int(c.get('max', 0)) >= 2 ** 64: return False
        return len(config['QNAME_columns']) <= 32 and len(config['QNAME_prefix']) <= 256 and len(config['QNAME_suffix']) <= 256

    def decode_text(self, config, DNA, QUAL, d_cols):
        """uq.py:1002-1058 on the device: the FASTQ text of these reads as one uint8 device tensor."""
        ops, ctx, n = self.ops, self.ctx, DNA[1]
        if self.args.two_pass_decode:
            seq, qt, ln = self.split_bits(DNA, QUAL, config)
            return ops.emit_fastq(ctx, config, d_cols, seq, qt, ln, n)
        # rows -> text in one kernel (uq_decode_fastq)
        text, bad = ops.decode_fastq(ctx, config, d_cols, DNA[0], QUAL[0], n)
        if bad is not None: error('ERROR: row %d of the DNA table carries no length sentinel; is this a uQ file?' % bad)
        return text

    def decode_tables(self):
        """The container of args.input opened and checked, its tables in HBM: (config, DNA, QUAL, QNAME columns)."""
        members, config = self.decode_open()
        return (config,) + tuple(self.load_tables(members, config))

    def decode_open(self):
        """The container of args.input opened and checked: (members, config)."""
        from . import container
        # a compressed container is verified whole (every member's length and CRC-32) before the first byte of text leaves
        self.source, self.tar_path = container.open_source(self, self.args.input), self.args.input
        if self.source.kind == container.BGZF: self.source.verify_all()
        return self.open_container()

    def host_text_records(self, config, DNA, QUAL, d_cols):
        """The text of a file whose QNAME lines the device kernels cannot write (device_text_possible), record by record: sequence and quality
        characters from the device, names from qname.decode_names (Python integers)."""
        from . import qname
        ctx, n = self.ctx, DNA[1]
        seq, qt, ln = self.split_bits(DNA, QUAL, config)
        dmax = config['dna_max']
        S = ctx.to_numpy(seq).reshape(n, dmax); Q = ctx.to_numpy(qt).reshape(n, dmax); L = ctx.to_numpy(ln, np.uint32)
        cols = [ctx.to_numpy(c, np.dtype(cc['dtype'])) for c, cc in zip(d_cols, config['QNAME_columns'])]
        names = qname.decode_names(config, cols)
        for r in range(n):
            l = int(L[r])
            yield names[r].encode('latin-1') + b'\n' + S[r, :l].tobytes() + b'\n+\n' + Q[r, :l].tobytes() + b'\n'

    def decode_to_device(self):
        """The decoded FASTQ text as one uint8 device tensor, whichever way the QNAME lines are made: the bytes `decode` writes."""
        config, DNA, QUAL, d_cols = self.decode_tables()
        if self.device_text_possible(config): return self.decode_text(config, DNA, QUAL, d_cols)
        return self.ctx.bytes_to_device(b''.join(self.host_text_records(config, DNA, QUAL, d_cols)))

    def decode(self, out=None):
        out = out or sys.stdout
        config, DNA, QUAL, d_cols = self.decode_tables()
        self.write_text(config, DNA, QUAL, d_cols, out.buffer if hasattr(out, 'buffer') else out)

    def decode_split(self, out1, out2):
        """--decode --split-mates OUT1 OUT2: the even reads of a paired container to OUT1, the odd ones to OUT2.  The two halves of every
        table are made on the device (load_tables with `mate`); each goes through the unchanged text path into its own file."""
        members, config = self.decode_open()
        if 'paired' not in config:
            error('ERROR: --split-mates needs a paired container and the config.json of %s has no "paired" key: if its reads alternate R1 and R2, '
                  'decode it and encode the text again with --interleaved' % self.args.input)
        if config['reads'] % 2: error('ERROR: this uQ file says it is paired and holds %d reads, an odd number' % config['reads'])
        for mate, path in enumerate((out1, out2)):
            DNA, QUAL, d_cols = self.load_tables(members, config, mate=mate)
            tmp = path + '.tmp%d' % os.getpid()
            try:
                with open(tmp, 'wb') as w: self.write_text(config, DNA, QUAL, d_cols, w)
                os.replace(tmp, path)
            finally:
                if os.path.exists(tmp): os.remove(tmp)
            del DNA, QUAL, d_cols

    def write_text(self, config, DNA, QUAL, d_cols, w):
        """The FASTQ text of these tables into the binary stream w (--bgzf: BGZF-compressed)."""
        ctx = self.ctx
        bgzf = self.args.bgzf
        if self.device_text_possible(config):
            # the text streams out through the pinned buffers (--bgzf: deflated on the device first)
            text = self.decode_text(config, DNA, QUAL, d_cols)
            self.io.device_to_stream(self.ops.bgzf_compress(ctx, text, level=self.bgzf_level) if bgzf else text, w)
        else:
            sink = io.BytesIO() if bgzf else w
            for record in self.host_text_records(config, DNA, QUAL, d_cols): sink.write(record)
            if bgzf:
                # the host-built text goes up to the device and is deflated there like the device text
                self.io.device_to_stream(self.ops.bgzf_compress(ctx, ctx.bytes_to_device(sink.getvalue()), level=self.bgzf_level), w)


# ---------------------------------------------------------------------- the packers with the reference's own signature
class DeviceLib:
    """What the reference's third return value (`lib`, the cffi handle of libc) is used for: `lib.free(ptr)`
    (uq.py:712-713).  Here `ptr` is a device address; free() drops the torch tensor that owns it."""

    def __init__(self):
        self._owned = {}

    def _own(self, tensor):
        self._owned[tensor.data_ptr()] = tensor
        return tensor.data_ptr()

    def free(self, ptr):
        self._owned.pop(int(ptr), None)
        return 0


def _encoder(variable, total_reads, bases, qualities, N_qual, dna_bytes_per_row, quality_bytes_per_row, status, file_path,
             bits_per_base, bits_per_quality, ctx=None):
    from . import ops
    from .device import Context
    from .hostio import Staging
    ctx = ctx or Context(0)
    d_buf = Staging(ctx).file_to_device(file_path)
    nlines = ops.count_lines(ctx, d_buf)
    if nlines // 4 != total_reads: error('ERROR: %s holds %d reads, not %d' % (file_path, nlines // 4, total_reads))
    d_ls = ops.index_lines(ctx, d_buf, nlines)
    st = ops.stats_new(ctx)
    ops.stats_accumulate(ctx, st, d_buf, d_ls, 0, total_reads)                # dna_max and the tile sizing (the reference
    hs = ops.stats_fetch(ctx, st)                                             # closes over the global `dna_max`, uq.py:128)
    p = ops.make_pack_params(bases, qualities, N_qual, bits_per_base, bits_per_quality, variable, dna_bytes_per_row,
                             quality_bytes_per_row, hs.len_max, hs.max_record_bytes, avg_record_bytes=d_buf.numel() // max(total_reads, 1))
    dna, qual, bad = ops.pack(ctx, d_buf, d_ls, 0, total_reads, p)
    b = ops.bad_index(bad)
    if b is not None: error('ERROR: read %d holds a symbol that is in neither alphabet nor N_qual' % b)
    if status is not None: status.current = total_reads                      # uq.py:176
    lib = DeviceLib()
    return ((dna.view(total_reads, dna_bytes_per_row), lib._own(dna)),
            (qual.view(total_reads, quality_bytes_per_row), lib._own(qual)), lib)


def encoder_fixed(total_reads, bases, qualities, N_qual, dna_bytes_per_row, quality_bytes_per_row, status, file_path,
                  bits_per_base, bits_per_quality, ctx=None):
    """uq.py:108-182 with its argument list and its return value `((dna_array, dna_ptr), (qual_array, qual_ptr), lib)`:
    the arrays are uint8[total_reads][bytes_per_row] DEVICE tensors (the reference's numpy views of malloc'd memory,
    uq.py:178-181), the pointers their device addresses, and `lib.free(ptr)` releases them (uq.py:712-713)."""
    return _encoder(False, total_reads, bases, qualities, N_qual, dna_bytes_per_row, quality_bytes_per_row, status, file_path,
                    bits_per_base, bits_per_quality, ctx)


def encoder_variable(total_reads, bases, qualities, N_qual, dna_bytes_per_row, quality_bytes_per_row, status, file_path,
                     bits_per_base, bits_per_quality, ctx=None):
    """uq.py:188-254, same contract as `encoder_fixed` (rows carry the length sentinel)."""
    return _encoder(True, total_reads, bases, qualities, N_qual, dna_bytes_per_row, quality_bytes_per_row, status, file_path,
                    bits_per_base, bits_per_quality, ctx)


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        validate_args(args)
        s = Session(args, out=sys.stdout)
        t_ready = time.perf_counter()                                # interpreter, torch and the device context are up
        ok = True
        if args.decode:
            if args.fingerprint: s.fingerprint_decoded()
            elif args.qc: s.qc_decoded()
            elif args.split_mates: s.decode_split(*args.split_mates)
            else: s.decode()
        elif args.fingerprint:
            s.fingerprint_input()
        elif args.qc:
            s.qc_input()
        else:
            ok = s.encode()
        if os.environ.get('UQ_TIMING'):
            s.ctx.sync()
            print(json.dumps({'uq_timing': 'uq', 'work_s': round(time.perf_counter() - t_ready, 3)}), file=sys.stderr, flush=True)
    except UqError as e:
        print(e)
        return 1
    return 0 if ok else 1                                            # --verify: 1 = the container was written and does not give the input back


if __name__ == '__main__':
    sys.exit(main())
