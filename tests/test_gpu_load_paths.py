"""GPU: the four pipelines of `Session.load_device` (index only, the queued speculative step, the indexed fallback, --multi-pass), each
held to the sequence of `ops` calls it makes while the input is loaded and to the `load_path` it reports; whatever the path, the members
are those of the --multi-pass encode of the same input."""
import io
import os

import numpy as np
import pytest

from uq_amd import ops, synth, uq

pytestmark = pytest.mark.gpu

QUEUED = 'two reads (census; pack + statistics), queued, no record index'
INDEXED = 'two reads (census; pack + statistics)'

# What the recording proxy below noted on commit dc3da93 (the parent of the commit that split load_device into named steps), pasted in
# as recorded (the run of the queued step, which three of them share, written once): the names of the `ops` attributes called inside
# load_input() / load_device().
QUEUED_CALLS = ['ChunkedCensus', 'head_guess', 'FusedQname', 'qname_guess_async', 'pack_stats_async', 'qname_fused_finish']
EXPECTED = {
    'default': (QUEUED, ['is_gzip'] + QUEUED_CALLS),
    'multi-pass': ('multi-pass', ['is_gzip', 'ChunkedCensus', 'stats_new', 'index_lines', 'stats_accumulate']),
    'exact-qname': (QUEUED, ['is_gzip', 'ChunkedCensus', 'head_guess', 'pack_stats_async']),
    # (on the binned text neither pack_stats_async nor pack_stats has a fused kernel to offer: the queued step and the indexed fallback
    # both stand down, and the plain statistics pass runs)
    'bin-qual': ('multi-pass', ['is_gzip', 'ChunkedCensus', 'index_lines', 'changed_new', 'requantise_qualities', 'ChunkedCensus', 'head_guess',
                                'FusedQname', 'qname_guess_async', 'pack_stats_async', 'head_guess_indexed', 'FusedQname', 'qname_guess', 'pack_stats',
                                'stats_new', 'stats_accumulate']),
    'multi-pass, no census begun': ('multi-pass', ['count_lines', 'stats_new', 'index_lines', 'stats_accumulate']),
    'index only': ('index only', ['is_gzip', 'ChunkedCensus']),
    'census list overflow': (INDEXED, QUEUED_CALLS + ['count_lines', 'index_lines', 'head_guess_indexed', 'FusedQname', 'qname_guess', 'pack_stats',
                                                      'qname_fused_finish']),
    'more reads than the head promises': (INDEXED, QUEUED_CALLS + ['index_lines', 'head_guess_indexed', 'FusedQname', 'qname_guess', 'pack_stats',
                                                                   'qname_fused_finish']),
}


class Recorder:
    """`session.ops` behind a proxy that notes the name of every attribute of it that is called (functions and the classes it constructs;
    what those call inside the module is theirs)."""

    def __init__(self, module):
        self._module, self.calls = module, []

    def __getattr__(self, name):
        value = getattr(self._module, name)
        if not callable(value) or (isinstance(value, type) and issubclass(value, BaseException)): return value

        def noted(*a, **kw):
            self.calls.append(name)
            return value(*a, **kw)
        return noted


def _session(ctx, path, flags):
    args = uq.validate_args(uq.build_parser().parse_args(['-i', str(path), '--quiet'] + flags))
    s = uq.Session(args, ctx=ctx, out=io.StringIO())
    s.ops = Recorder(ops)
    return s


def _members(s):
    s.encode_loaded(write=False)
    return {name: s.member_bytes(name) for name in s.members}, s.config


def _file_case(ctx, tmp_path, flags):
    """64 reads x 40 bp in a file, through load_input(): (session, calls noted during the load)."""
    p = tmp_path / 'in.fastq'
    p.write_bytes(synth.fastq(20261020, 64, 40))
    s = _session(ctx, p, flags)
    s.load_input()
    return s, list(s.ops.calls)


@pytest.mark.parametrize('case,flags', [('default', []), ('multi-pass', ['--multi-pass']), ('exact-qname', ['--exact-qname']),
                                        ('bin-qual', ['--bin-qual', 'illumina8'])], ids=['default', 'multi-pass', 'exact-qname', 'bin-qual'])
def test_load_input_paths(ctx, tmp_path, case, flags):
    s, calls = _file_case(ctx, tmp_path, flags)
    assert (s.load_path, calls) == EXPECTED[case]
    assert s.total == 64 and s.path == str(tmp_path / 'in.fastq')
    want, _ = _file_case(ctx, tmp_path, ['--multi-pass'] + (flags if case == 'bin-qual' else []))       # (binning changes the members: both runs bin)
    assert _members(s) == _members(want)


def test_index_only_path(ctx, tmp_path):
    p = tmp_path / 'in.fastq'
    fq = synth.fastq(20261020, 64, 40)
    p.write_bytes(fq)
    s = _session(ctx, p, ['--fingerprint'])
    fp = s.fingerprint_input()
    assert s.load_path == EXPECTED['index only'][0]
    assert s.ops.calls == EXPECTED['index only'][1] + ['index_lines', 'fingerprint', 'fingerprint_json']     # (d_ls is expanded for the fingerprint)
    assert s.total == 64 and fp == ops.fingerprint_host(fq)


def _short_lines():
    """Reads of one base: more than 1 024 newlines in a 16 KiB census tile, as in test_queued_census_list_overflow_stands_down."""
    return synth.fastq_array(synth.Spec(20261021, 1), 2000)


def _dense_tail():
    """4 MiB of 508 bp reads (all the head guess looks at), then 24 bp reads: many more reads per byte than the head promised."""
    spec_long, spec_short = synth.Spec(20261022, 508), synth.Spec(20261022, 24)
    return np.concatenate([synth.fastq_array(spec_long, 4100), synth.fastq_array(spec_short, 12000, first=4100)])


@pytest.mark.parametrize('case,text,reads', [('census list overflow', _short_lines, 2000), ('more reads than the head promises', _dense_tail, 16100)],
                         ids=['census-list-overflow', 'dense-tail'])
def test_load_device_fallback_paths(ctx, case, text, reads):
    host = text()
    runs = {}
    for flags in ([], ['--multi-pass']):
        s = _session(ctx, os.path.abspath(__file__), flags)          # -i only has to be a file
        s.load_device(ctx.to_device(host))
        runs[bool(flags)] = (s, list(s.ops.calls))
    s, calls = runs[False]
    assert (s.load_path, calls) == EXPECTED[case]
    assert s.total == reads and s.path is None
    assert (runs[True][0].load_path, runs[True][1]) == EXPECTED['multi-pass, no census begun']
    assert _members(s) == _members(runs[True][0])
