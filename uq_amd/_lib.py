"""ctypes binding of libuqhip.so (the C ABI declared in include/uqhip.h).

There is no CPU fallback: if the shared library is missing or a call fails, this raises.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('UQ_LIB_PATH') or os.path.join(HERE, 'libuqhip.so')       # UQ_LIB_PATH: A/B builds of the kernels (tuning)
UQ_NONE = (1 << 64) - 1
ABI_VERSION = 1


class UqHipError(RuntimeError):
    pass


class Stats(C.Structure):
    _fields_ = [('counts', C.c_uint64 * 65536), ('bad_plus', C.c_uint64), ('bad_len', C.c_uint64),
                ('len_min', C.c_uint32), ('len_max', C.c_uint32), ('max_record_bytes', C.c_uint32),
                ('reserved', C.c_uint32)]


class PackParams(C.Structure):
    _fields_ = [('dna_code', C.c_int16 * 256), ('qual_code', C.c_int16 * 256), ('n_qual', C.c_int32 * 256),
                ('bits_per_base', C.c_int32), ('bits_per_quality', C.c_int32), ('variable', C.c_int32),
                ('dna_bytes_per_row', C.c_int32), ('quality_bytes_per_row', C.c_int32),
                ('max_record_bytes', C.c_int32), ('dna_max', C.c_int32), ('avg_record_bytes', C.c_int32)]


class PackTileGeom(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ('tiled', 'tile64', 'R', 'Rs', 'P', 'G', 'stage_bytes', 'out_bytes', 'copies', 'lds_bytes', 'wg_per_cu',
                                          'reserved')]

    def __repr__(self):
        return 'PackTileGeom(%s)' % ', '.join('%s=%d' % (k, getattr(self, k)) for k, _ in self._fields_[:-1])


class UnpackParams(C.Structure):
    _fields_ = [('base_char', C.c_uint8 * 256), ('qual_char', C.c_uint8 * 256), ('qual_n_base', C.c_uint8 * 256),
                ('bits_per_base', C.c_int32), ('bits_per_quality', C.c_int32), ('variable', C.c_int32),
                ('dna_bytes_per_row', C.c_int32), ('quality_bytes_per_row', C.c_int32), ('dna_max', C.c_int32)]


class EmitParams(C.Structure):
    _fields_ = [('prefix', C.c_uint8 * 256), ('suffix', C.c_uint8 * 256), ('separators', C.c_uint8 * 32),
                ('prefix_len', C.c_int32), ('suffix_len', C.c_int32), ('ncols', C.c_int32), ('dna_max', C.c_int32),
                ('itemsize', C.c_int32 * 32), ('add', C.c_int64 * 32)]


class QnameLayoutResult(C.Structure):
    _fields_ = [('min_lcp', C.c_uint32), ('min_lcs', C.c_uint32), ('flags', C.c_uint32), ('nch', C.c_uint32),
                ('entry', C.c_uint64 * 64), ('lastviol', C.c_uint64 * 64), ('ch', C.c_uint8 * 64)]


class QnameColsResult(C.Structure):
    _fields_ = [('first_nonint', C.c_uint64 * 32), ('vmin', C.c_int64 * 32), ('vmax', C.c_int64 * 32),
                ('any_long', C.c_uint32 * 32), ('flags', C.c_uint32), ('reserved', C.c_uint32)]


class QnameFused(C.Structure):
    _fields_ = [('ok', C.c_uint32), ('plen', C.c_uint32), ('slen', C.c_uint32), ('nsep', C.c_uint32), ('l1len', C.c_uint32),
                ('flags', C.c_uint32), ('sample_step', C.c_uint32), ('nth', C.c_uint32),
                ('line1', C.c_uint8 * 256), ('seps', C.c_uint8 * 32), ('inset', C.c_uint8 * 256),
                ('vmin', C.c_uint32 * 8), ('vmax', C.c_uint32 * 8), ('undetermined', C.c_uint32 * 8),
                ('nreads', C.c_uint64), ('thresholds', C.c_uint64 * 24), ('counts', (C.c_uint64 * 24) * 8)]


class StatsCompact(C.Structure):
    _fields_ = [('n', C.c_uint32), ('len_min', C.c_uint32), ('len_max', C.c_uint32), ('max_record_bytes', C.c_uint32), ('reserved', C.c_uint32),
                ('pad', C.c_uint32), ('bad_plus', C.c_uint64), ('bad_len', C.c_uint64), ('key', C.c_uint32 * 2048), ('count', C.c_uint64 * 2048)]


class Decisions(C.Structure):
    _fields_ = [('status', C.c_uint32), ('nbases', C.c_uint32), ('nquals', C.c_uint32), ('nall', C.c_uint32), ('nnq', C.c_uint32), ('ncand', C.c_uint32),
                ('bases', C.c_uint8 * 256), ('qualities', C.c_uint8 * 256), ('all_bases', C.c_uint8 * 256),
                ('nq_base', C.c_uint8 * 256), ('nq_code', C.c_int32 * 256),
                ('total_quals', C.c_int32), ('bits_per_base', C.c_int32), ('bits_per_quality', C.c_int32), ('variable', C.c_int32),
                ('dna_max', C.c_int32), ('dna_min', C.c_int32), ('dna_bytes_per_row', C.c_int32), ('quality_bytes_per_row', C.c_int32),
                ('base_tot', C.c_uint64 * 256), ('qual_tot', C.c_uint64 * 256)]


class QnameColumns(C.Structure):
    _fields_ = [('status', C.c_uint32), ('ncols', C.c_uint32), ('itemsize', C.c_uint32 * 8), ('offset', C.c_uint32 * 8),
                ('from_mapping', C.c_uint32 * 8), ('vmin', C.c_uint32 * 8), ('vmax', C.c_uint32 * 8)]


class GzipStreamInfo(C.Structure):
    _fields_ = [('chunks', C.c_uint64), ('starts', C.c_uint64), ('rounds', C.c_uint64), ('redecoded', C.c_uint64),
                ('overflows', C.c_uint64), ('resolve_rounds', C.c_uint64), ('members', C.c_uint64), ('out_bytes', C.c_uint64),
                ('find_ms', C.c_double), ('decode_ms', C.c_double), ('finish_ms', C.c_double)]


class GzipMember(C.Structure):
    _fields_ = [('data_offset', C.c_uint64), ('comp_bytes', C.c_uint64), ('out_offset', C.c_uint64), ('isize', C.c_uint32),
                ('crc32', C.c_uint32)]


class BgzfPart(C.Structure):
    _fields_ = [('h_prefix', C.c_void_p), ('prefix_bytes', C.c_uint32), ('reserved', C.c_uint32), ('d_data', C.c_void_p),
                ('nbytes', C.c_uint64)]


class Fingerprint(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ('reads', 'bases', 'plus_text', 'qname', 'dna', 'qual', 'pairs', 'records', 'ordered')]


class MateReport(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ('pairs', 'mismatches', 'first_mismatch', 'slash_pairs')]


class FilterParams(C.Structure):
    _fields_ = [('min_len', C.c_uint32), ('max_len', C.c_uint32), ('max_n', C.c_uint32), ('min_mean_q', C.c_uint32),
                ('sample_threshold', C.c_uint64), ('seed', C.c_uint64), ('unit', C.c_uint32), ('flags', C.c_uint32)]


class FilterReport(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ('reads_in', 'bases_in', 'bytes_in', 'reads_out', 'bases_out', 'bytes_out',
                                          'fail_min_len', 'fail_max_len', 'fail_max_n', 'fail_mean_q', 'fail_sample', 'fail_mate')]


class TrimParams(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ('head', 'tail', 'crop', 'polyg', 'q5', 'q3', 'flags', 'reserved')]


class TrimReport(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ('reads_in', 'bases_in', 'bytes_in', 'reads_trimmed', 'bases_out', 'bytes_out',
                                          'cut_fixed', 'cut_polyg', 'cut_q5', 'cut_q3', 'cut_n', 'emptied', 'len_mismatch')]


class AdapterParams(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ('len1', 'len2', 'overlap', 'err_pct', 'flags')] + [('reserved', C.c_uint32 * 3),
                                                                                             ('seq1', C.c_uint8 * 64), ('seq2', C.c_uint8 * 64)]


class AdapterReport(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ('reads_in', 'bases_in', 'bases_out', 'reads_cut', 'full', 'partial', 'mate2', 'emptied', 'len_mismatch')]


class DedupParams(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ('unit', 'prefix', 'hash_bits', 'flags')] + [('seed', C.c_uint64)]


class DedupReport(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ('reads_in', 'bases_in', 'units_in', 'classes', 'dup_units', 'dup_reads', 'dup_bases', 'collisions')]


class SynthSpec(C.Structure):
    _fields_ = [('seed', C.c_uint64), ('len_lo', C.c_int32), ('len_hi', C.c_int32), ('n_rate', C.c_int32),
                ('n_qual_exclusive', C.c_int32), ('dup', C.c_int32), ('dup_templates', C.c_int32),
                ('skip_len_mod4', C.c_int32), ('reserved', C.c_int32)]


_vp, _u64, _u32, _int, _sz = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_size_t
_P = C.POINTER

# name -> argtypes (every function returns int except uq_last_error)
SIGNATURES = {
    'uq_abi_version': [],
    'uq_device_count': [_P(_int)],
    'uq_ctx_create': [_int, _vp, _P(_vp)],
    'uq_ctx_destroy': [_vp],
    'uq_ctx_reserve': [_vp, _sz],
    'uq_ctx_sync': [_vp],
    'uq_dev_alloc': [_vp, _sz, _P(_vp)],
    'uq_dev_free': [_vp, _vp],
    'uq_h2d': [_vp, _vp, _vp, _sz],
    'uq_d2h': [_vp, _vp, _vp, _sz],
    'uq_memset': [_vp, _vp, _int, _sz],
    'uq_timer_start': [_vp],
    'uq_timer_stop': [_vp, _P(C.c_float)],
    'uq_count_lines': [_vp, _vp, _u64, _P(_u64)],
    'uq_count_lines_begin': [_vp, _vp, _u64],
    'uq_count_lines_chunk': [_vp, _vp, _u64, _u64, _u64],
    'uq_count_lines_end': [_vp, _vp, _u64, _P(_u64)],
    'uq_count_lines_end_async': [_vp, _vp, _u64],
    'uq_index_lines_async': [_vp, _vp, _u64, _u64, _vp],
    'uq_count_lines_wait': [_vp, _vp, _u64, _P(_u64), _P(_int)],
    'uq_index_lines': [_vp, _vp, _u64, _u64, _vp],
    'uq_stats_init': [_vp, _vp],
    'uq_stats_fetch': [_vp, _vp, _vp],
    'uq_stats_fetch_compact': [_vp, _vp, _vp],
    'uq_stats_accumulate': [_vp, _vp, _vp, _u64, _u64, _vp],
    'uq_stats_export': [_vp, _vp, _u32, _u32, _u64, _vp],
    'uq_stats_import': [_vp, _vp, _u32, _vp],
    'uq_first_occurrence': [_vp, _vp, _vp, _u64, _u64, _u64, _vp],
    'uq_fingerprint_init': [_vp, _vp],
    'uq_fingerprint_accumulate': [_vp, _vp, _vp, _u64, _u64, _u64, _vp],
    'uq_fingerprint_host': [_vp, _vp, _u64, _u64, _u64, _P(Fingerprint)],
    'uq_qc_init': [_vp, _vp, _u32],
    'uq_qc_accumulate': [_vp, _vp, _vp, _u64, _u64, _u32, _vp],
    'uq_qc_host': [_vp, _vp, _u64, _u64, _u32, _vp],
    'uq_requantise_qualities': [_vp, _vp, _vp, _u64, _u64, _vp, _vp],
    'uq_requantise_qualities_host': [_vp, _vp, _u64, _u64, _vp, _P(_u64)],
    'uq_interleave_records': [_vp, _vp, _vp, _vp, _vp, _u64, _u64, _vp, _u64],
    'uq_interleave_records_host': [_vp, _vp, _vp, _vp, _u64, _u64, _vp, _u64],
    'uq_mate_report_init': [_vp, _vp],
    'uq_mate_check': [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _u64, _u64, _u64, _u64, _vp],
    'uq_mate_check_host': [_vp, _vp, _u64, _u64, _vp, _vp, _u64, _u64, _u64, _u64, _P(MateReport)],
    'uq_filter_report_init': [_vp, _vp],
    'uq_filter_report_init_host': [_P(FilterReport)],
    'uq_filter_mark': [_vp, _vp, _vp, _u64, _u64, _u64, _P(FilterParams), _vp, _vp],
    'uq_filter_mark_host': [_vp, _vp, _u64, _u64, _u64, _P(FilterParams), _vp, _P(FilterReport)],
    'uq_filter_plan': [_vp, _vp, _u64, _u64, _u32, _vp, _vp, _vp, _vp, _P(_u64), _P(_u64)],
    'uq_filter_plan_host': [_vp, _u64, _u64, _u32, _vp, _vp, _vp, _P(FilterReport), _P(_u64), _P(_u64)],
    'uq_compact_records': [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64],
    'uq_compact_records_host': [_vp, _u64, _vp, _vp, _u64, _vp, _u64],
    'uq_trim_report_init': [_vp, _vp],
    'uq_trim_report_init_host': [_P(TrimReport)],
    'uq_trim_mark': [_vp, _vp, _vp, _u64, _u64, _P(TrimParams), _vp, _vp],
    'uq_trim_mark_host': [_vp, _vp, _u64, _u64, _P(TrimParams), _vp, _P(TrimReport)],
    'uq_trim_plan': [_vp, _vp, _u64, _u64, _vp, _vp, _P(_u64)],
    'uq_trim_plan_host': [_vp, _u64, _u64, _vp, _vp, _P(_u64)],
    'uq_trim_records': [_vp, _vp, _u64, _vp, _u64, _u64, _vp, _vp, _vp, _u64, _vp],
    'uq_trim_records_host': [_vp, _u64, _vp, _u64, _u64, _vp, _vp, _vp, _u64, _vp],
    'uq_adapter_report_init': [_vp, _vp],
    'uq_adapter_report_init_host': [_P(AdapterReport)],
    'uq_adapter_mark': [_vp, _vp, _vp, _u64, _u64, _P(AdapterParams), _vp, _vp],
    'uq_adapter_mark_host': [_vp, _vp, _u64, _u64, _P(AdapterParams), _vp, _P(AdapterReport)],
    'uq_dedup_report_init': [_vp, _vp],
    'uq_dedup_report_init_host': [_P(DedupReport)],
    'uq_dedup_keys': [_vp, _vp, _vp, _u64, _u64, _u64, _P(DedupParams), _vp, _vp],
    'uq_dedup_keys_host': [_vp, _vp, _u64, _u64, _u64, _P(DedupParams), _vp, _P(DedupReport)],
    'uq_dedup_mark': [_vp, _vp, _vp, _u64, _u64, _u64, _P(DedupParams), _vp, _vp, _vp, _vp],
    'uq_dedup_mark_host': [_vp, _vp, _u64, _u64, _u64, _P(DedupParams), _vp, _vp, _vp, _P(DedupReport)],
    'uq_pack': [_vp, _vp, _vp, _u64, _u64, _P(PackParams), _vp, _vp, _vp],
    'uq_pack_stats': [_vp, _vp, _vp, _u64, _u64, _P(PackParams), _vp, _vp, _vp, _vp, _P(_int)],
    'uq_pack_stats_async': [_vp, _vp, _vp, _u64, _P(PackParams), _vp, _vp, _vp, _vp, _P(_int)],
    'uq_pack_tile_geometry': [_P(PackParams), _u32, _P(PackTileGeom)],
    'uq_pattern': [_vp, _vp, _u64, _u32, _int, _vp],
    'uq_unpattern': [_vp, _vp, _u64, _u32, _int, _vp],
    'uq_argsort_rows': [_vp, _vp, _u64, _u32, _vp],
    'uq_lower_bound_rows': [_vp, _vp, _u64, _u32, _vp, _u64, _vp],
    'uq_gather_rows': [_vp, _vp, _u64, _u32, _vp, _int, _u64, _vp],
    'uq_check_index_range': [_vp, _vp, _int, _u64, _u64, _P(_u64)],
    'uq_unique_rows': [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _P(_u64)],
    'uq_key_itemsize': [_u64],
    'uq_narrow': [_vp, _vp, _u64, _int, _vp],
    'uq_stack_columns': [_vp, _P(_vp), _P(_int), _int, _u64, _int, _vp],
    'uq_unstack_column': [_vp, _vp, _u64, _int, _int, _int, _int, _vp],
    'uq_unpack': [_vp, _vp, _vp, _u64, _P(UnpackParams), _vp, _vp, _vp, _vp],
    'uq_qname_analyse': [_vp, _vp, _u64, _P(_vp), _P(_int)],
    'uq_qname_json': [_vp, _P(C.c_char_p)],
    'uq_qname_column': [_vp, _int, _vp, _u64],
    'uq_qname_free': [_vp],
    'uq_qname_layout': [_vp, _vp, _vp, _u64, _u64, _vp, _u32, _P(QnameLayoutResult)],
    'uq_qname_tokenise': [_vp, _vp, _vp, _u64, _u32, _u32, _vp, _u32, _P(_vp), _P(_vp), _P(QnameColsResult)],
    'uq_prefix_distinct': [_vp, _vp, _int, _vp, _u64, _P(_u64), _int, _P(_u64)],
    'uq_int_prefix_distinct': [_vp, _vp, _u64, C.c_int64, _u64, _u64, _P(_u64), _int, _P(_u64)],
    'uq_encode_int': [_vp, _vp, _u64, C.c_int64, _int, _vp],
    'uq_unique_sorted_rows': [_vp, _vp, _u64, _u32, _vp, _vp, _P(_u64)],
    'uq_unique_rows_of_groups': [_vp, _vp, _u64, _u32, _vp, _vp, _u64, _vp],
    'uq_partition_order': [_vp, _vp, _u64, _u32, _vp, _vp, _P(_u64)],
    'uq_partition_rows': [_vp, _vp, _u32, _u32, _vp, _u64, _u64, _u64, _vp],
    'uq_owner_of_rows': [_vp, _vp, _u64, _P(C.c_int64), _u32, _vp],
    'uq_index_affine': [_vp, _vp, _int, _u64, C.c_int64, _vp, _int],
    'uq_invert_permutation': [_vp, _vp, _int, _u64, C.c_int64, _vp, _P(_u64)],
    'uq_scatter_rows': [_vp, _vp, _u64, _u32, _vp, _int, C.c_int64, _u64, _vp, _P(_u64)],
    'uq_qname_guess': [_vp, _vp, _vp, _u64, _vp],
    'uq_qname_guess_async': [_vp, _vp, _vp, _vp],
    'uq_pack_stats_qname': [_vp, _vp, _vp, _u64, _u64, _P(PackParams), _vp, _vp, _vp, _vp, _vp, _vp, _u64, _P(_int)],
    'uq_pack_stats_qname_async': [_vp, _vp, _vp, _u64, _P(PackParams), _vp, _vp, _vp, _vp, _vp, _vp, _u64, _P(_int)],
    'uq_qname_fused_finish': [_vp, _vp, _vp, _u64],
    'uq_qname_fused_fetch': [_vp, _vp, _P(QnameFused)],
    'uq_qname_fused_first_seen': [_vp, _vp, _u64, _u64, _u64, _P(_u32), _P(_u32), _int, _vp],
    'uq_encode_u32': [_vp, _vp, _u64, _u32, _int, _vp],
    'uq_encode_u32_columns': [_vp, _vp, _u64, _u64, _int, _P(_u32), _P(_int), _P(_vp)],
    'uq_decide_from_stats': [_vp, _vp, _u32, _u32, _int, _int, _vp, _P(Decisions)],
    'uq_make_pack_params': [C.c_char_p, _u32, C.c_char_p, _u32, C.c_char_p, _P(C.c_int32), _u32] + [C.c_int32] * 8 + [_P(PackParams)],
    'uq_same_pack_params': [_P(PackParams), _P(PackParams), _P(_int)],
    'uq_qname_fused_columns': [_P(QnameFused), _u64, _P(QnameColumns)],
    'uq_emit_fastq': [_vp, _P(EmitParams), _P(_vp), _P(_vp), _P(_vp), _vp, _vp, _vp, _u64, _vp, _vp, _u64, _P(_u64)],
    'uq_debug_scribble_lds': [_vp, C.c_uint32],
    'uq_sort_config': [_vp, C.c_int64, _P(_int), _int],
    'uq_sort_counters': [_vp, _P(_u64), _P(_u64)],
    'uq_decode_fastq': [_vp, _P(EmitParams), _P(UnpackParams), _P(_vp), _P(_vp), _P(_vp), _vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _P(_u64), _P(_u64)],
    'uq_synth_size': [_vp, _P(SynthSpec), _u64, _u64, _P(_u64)],
    'uq_synth_fastq': [_vp, _P(SynthSpec), _u64, _u64, _vp, _u64],
    'uq_gzip_scan': [_vp, _u64, _vp, _u64, _P(_u64), _P(_u64), _P(_int), _P(_u64)],
    'uq_inflate_members': [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp],
    'uq_inflate_member_host': [_vp, _u64, _vp, _u64, _u32, _P(_u32)],
    'uq_gzip_stream_begin': [_vp, _vp, _u64, _u64, _vp, _u64, _P(_vp), _P(_u64), _P(_u32), _P(_u64)],
    'uq_gzip_stream_finish': [_vp, _vp, _u64, _P(_u32), _P(_u64)],
    'uq_gzip_stream_get_info': [_vp, _P(GzipStreamInfo)],
    'uq_gzip_stream_free': [_vp],
    'uq_gzip_stream_host': [_vp, _u64, _u64, _vp, _u64, _vp, _u64, _P(_u64), _P(_u32), _P(_u64), _P(GzipStreamInfo)],
    'uq_bgzf_bound': [_u64, _P(_u64)],
    'uq_bgzf_compress': [_vp, _vp, _u64, _vp, _u64, _P(_u64), _u32],
    'uq_bgzf_compress_parts': [_vp, _P(BgzfPart), _u32, _vp, _u64, _P(_u64), _P(_u64), _u32],
    'uq_bgzf_parts_bound': [_P(BgzfPart), _u32, _P(_u64)],
    'uq_bgzf_compress_block_host': [_vp, _u64, _vp, _u64, _P(_u64), _P(_u32)],
    'uq_bgzf_compress_block_host_l': [_vp, _u64, _vp, _u64, _P(_u64), _P(_u32), _u32],
    'uq_deflate_size': [_vp, _vp, _u32, _vp, _u64, _vp, _vp],
    'uq_deflate_size_host': [_vp, _u32, _vp, _u64, _P(_u64)],
    'uq_deflate_size_l': [_vp, _vp, _u32, _vp, _u64, _vp, _vp, _u32],
    'uq_deflate_size_host_l': [_vp, _u32, _vp, _u64, _P(_u64), _u32],
}

# the entry points that return a value, not a status: name -> (restype, argtypes)
VALUE_SIGNATURES = {
    'uq_qc_words': (_u64, [_u32]),
}

_lib = None
MISSING = []


def load():
    """Load libuqhip.so (once).  Raises UqHipError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise UqHipError('%s not found: build it with `python -m uq_amd.build` (hipcc, gfx950). '
                         'There is no CPU fallback.' % LIB_PATH)
    try:
        # one HIP runtime per process: torch ships its own libamdhip64; loading it first makes libuqhip.so bind to the
        # same one (loaded the other way round, the two runtimes disagree about the visible devices)
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    lib.uq_last_error.restype = C.c_char_p
    lib.uq_last_error.argtypes = []
    for name, args in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            MISSING.append(name)
            continue
        fn.argtypes = args
        fn.restype = C.c_int
    for name, (res, args) in VALUE_SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            MISSING.append(name)
            continue
        fn.argtypes = args
        fn.restype = res
    if lib.uq_abi_version() != ABI_VERSION:
        raise UqHipError('libuqhip.so ABI %d != binding ABI %d' % (lib.uq_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def call(name, *args):
    """Call an int-returning entry point; non-zero -> UqHipError(uq_last_error())."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise UqHipError('%s: %s' % (name, lib.uq_last_error().decode('utf-8', 'replace')))
    return rc
