/* uqhip.h -- C ABI of libuqhip.so: the MI355X (gfx950) implementation of the uQ encode/decode
 * hot path.  This is the drop-in boundary: every entry point replaces one numpy / per-base-loop
 * site of the reference (JohnLonginotto/uq, `uq.py`), cited as `uq.py:<lines>` on each.
 *
 * Conventions
 *   - Every function returns 0 on success, non-zero on failure; the message is `uq_last_error()`
 *     (thread-local).  Nothing throws across the ABI.
 *   - `uq_ctx` binds one HIP device and one stream.  It is NOT thread-safe: the caller serialises,
 *     as the single-threaded reference does.  Calls enqueue on the context's stream and are
 *     synchronous at return only where they hand a value back to the host (`h_*` out-parameters).
 *   - `d_*` pointers are device memory (from `uq_dev_alloc`, hipMalloc, or a torch tensor's
 *     data_ptr()); `h_*` are host.  Buffers are caller-owned.  Scratch memory is owned by the
 *     context and grows on demand (`uq_ctx_reserve` pre-sizes it).
 *   - Tables are row-major `uint8[rows][cols]`, as the reference's numpy arrays (uq.py:178-181).
 *   - Row permutations and keys are `uint32` on the device (< 2^32 rows per GPU); the host mirror
 *     widens them where numpy would give int64.
 */
#ifndef UQHIP_H
#define UQHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UQ_ABI_VERSION 1
#define UQ_NONE UINT64_MAX

typedef struct uq_ctx uq_ctx;

/* ---- context, memory, errors.  Replaces cffi -> libc malloc/free (uq.py:111-126, 712-713). */
const char* uq_last_error(void);
int uq_abi_version(void);
int uq_device_count(int* h_count);
/* `stream` = an existing hipStream_t (e.g. torch's current stream) or NULL for a private one. */
int uq_ctx_create(int device, void* stream, uq_ctx** out);
int uq_ctx_destroy(uq_ctx* ctx);
int uq_ctx_reserve(uq_ctx* ctx, size_t scratch_bytes);
int uq_ctx_sync(uq_ctx* ctx);
int uq_dev_alloc(uq_ctx* ctx, size_t bytes, void** d_out);
int uq_dev_free(uq_ctx* ctx, void* d_ptr);
int uq_h2d(uq_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int uq_d2h(uq_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);
/* Test aid: overwrite the LDS of every CU with `pattern`-derived words (LDS survives between launches, which hides
 * reads of LDS a kernel never wrote).  No effect on results. */
int uq_debug_scribble_lds(uq_ctx* ctx, uint32_t pattern);
int uq_memset(uq_ctx* ctx, void* d_dst, int value, size_t bytes);
/* Device-side timing on the context's stream (hipEvents), for bench.py's roofline leg. */
int uq_timer_start(uq_ctx* ctx);
int uq_timer_stop(uq_ctx* ctx, float* h_ms);

/* ---- record index.  Replaces `wc -l` (uq.py:85) and the `next(f)` line iteration (uq.py:132-137).
 * uq_count_lines: number of '\n' in d_buf[0, nbytes).
 * uq_index_lines: d_line_start[k] = offset of the first byte of line k, k in [0, nlines];
 *                 d_line_start[nlines] = offset one past the last '\n'.  nlines from uq_count_lines. */
int uq_count_lines(uq_ctx* ctx, const uint8_t* d_buf, uint64_t nbytes, uint64_t* h_nlines);
int uq_index_lines(uq_ctx* ctx, const uint8_t* d_buf, uint64_t nbytes, uint64_t nlines, uint64_t* d_line_start);
/* uq_count_lines in pieces, for a buffer that is still being filled (a file streaming into HBM chunk by chunk, SURVEY.md 8
 * row f2): _begin once, _chunk for every byte range [first_byte, first_byte + chunk_bytes) as it lands -- ranges are whole
 * 16 KiB tiles of the 16-byte-aligned address space (any multiple of 16 KiB from an aligned base), the last one ends with the
 * buffer; every byte is covered exactly once, in any order -- and _end = the line count, exactly what uq_count_lines returns for
 * the whole buffer (uq_index_lines then reuses the census the same way). */
int uq_count_lines_begin(uq_ctx* ctx, const uint8_t* d_buf, uint64_t nbytes);
int uq_count_lines_chunk(uq_ctx* ctx, const uint8_t* d_buf, uint64_t nbytes, uint64_t first_byte, uint64_t chunk_bytes);
int uq_count_lines_end(uq_ctx* ctx, const uint8_t* d_buf, uint64_t nbytes, uint64_t* h_nlines);
/* The same census, the record index and the fused pack + statistics pass QUEUED one behind the other, without the host round trip that
 * `wc -l` (uq.py:85) puts between counting and reading: _end_async queues the closing scan and leaves the line count on the device,
 * uq_index_lines_async (d_line_start holds capacity_lines + 1 entries) and uq_pack_stats_async (below) read it there, and
 * uq_count_lines_wait hands it to the host once everything has been queued.  *h_ok = 0: more lines than capacity_lines, or a 16 KiB
 * tile with more newlines than its list holds -- the index (and what was packed from it) is not usable, take uq_count_lines +
 * uq_index_lines.  Between _end_async and _wait the context must not start another census. */
int uq_count_lines_end_async(uq_ctx* ctx, const uint8_t* d_buf, uint64_t nbytes);
int uq_index_lines_async(uq_ctx* ctx, const uint8_t* d_buf, uint64_t nbytes, uint64_t capacity_lines, uint64_t* d_line_start);
int uq_count_lines_wait(uq_ctx* ctx, const uint8_t* d_buf, uint64_t nbytes, uint64_t* h_nlines, int* h_ok);

/* ---- a1: pass-1 statistics.  Replaces uq.py:366-375, 382, 388, 415-425.
 * counts[base * 256 + qual] over every (base, quality) pair of reads [0, nreads); DNA length range;
 * the first record (if any) whose third line does not start with '+' or whose SEQ/QUAL lengths
 * differ.  The struct lives in device memory; the caller zero-initialises it with uq_stats_init
 * (so that several calls / shards accumulate) and copies it back with uq_d2h. */
typedef struct uq_stats {
    uint64_t counts[256 * 256];
    uint64_t bad_plus;          /* smallest read index with a bad '+' line, or UQ_NONE   (uq.py:382) */
    uint64_t bad_len;           /* smallest read index with len(SEQ) != len(QUAL)        (uq.py:388) */
    uint32_t len_min, len_max;  /* uq.py:416-417 */
    uint32_t max_record_bytes;  /* longest record (4 lines), sizing hint for the pack tiles */
    uint32_t reserved;          /* uq_pack_stats only: non-zero = the counts above are incomplete, run uq_stats_accumulate */
} uq_stats;
int uq_stats_init(uq_ctx* ctx, uq_stats* d_stats);
/* The device struct copied to the host (synchronous).  Same bytes as uq_d2h of the whole struct, but a file touches a few hundred
 * of the 65 536 counters: they travel as a short list through the context's pinned buffer instead of 512 KiB to pageable memory. */
int uq_stats_fetch(uq_ctx* ctx, const uq_stats* d_stats, uq_stats* h_stats);
/* The same statistics as the list of their non-zero counters (a file uses a few hundred of the 65 536): key = base * 256 + quality, in
 * no particular order.  n > UQ_STATS_COMPACT_CAP: the list is cut short, take uq_stats_fetch.  What the host decisions of
 * uq.py:448-545 need, without 512 KiB crossing PCIe and being cleared and copied on the host for every shard. */
#define UQ_STATS_COMPACT_CAP 2048u
typedef struct uq_stats_compact {
    uint32_t n, len_min, len_max, max_record_bytes, reserved, pad;
    uint64_t bad_plus, bad_len;
    uint32_t key[UQ_STATS_COMPACT_CAP];
    uint64_t count[UQ_STATS_COMPACT_CAP];
} uq_stats_compact;
int uq_stats_fetch_compact(uq_ctx* ctx, const uq_stats* d_stats, uq_stats_compact* h_out);
int uq_stats_accumulate(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start,
                        uint64_t first_read, uint64_t nreads, uq_stats* d_stats);
/* Multi-GPU: a uq_stats as ONE summable buffer of 65536 + 6 * world int64 words.  uq_stats_export writes the
 * counts and, in this rank's six slots, bad_plus / bad_len (made file-wide by adding read_offset; sign bit flipped so that
 * signed order == unsigned order), len_min, len_max, max_record_bytes and the `reserved` flag; the other ranks' slots are 0.
 * After an all-reduce SUM of the buffer (RCCL), uq_stats_import folds everybody's slots with MIN / MAX back into d_stats:
 * one collective per statistics exchange. */
int uq_stats_export(uq_ctx* ctx, const uq_stats* d_stats, uint32_t rank, uint32_t world, uint64_t read_offset, int64_t* d_words);
int uq_stats_import(uq_ctx* ctx, const int64_t* d_words, uint32_t world, uq_stats* d_stats);
/* First occurrence of each base byte: d_first[b] = min over pairs of (read_index << 32 | position),
 * or UQ_NONE, read_index = read_index_base + the read's number among [first_read, first_read + nreads): exact order
 * for every read length a uint32 holds and read numbers below 2^32 (as everywhere in this ABI); shards combine
 * with MIN.  Only needed to order N-trick candidates as the reference's dict does (uq.py:480). */
int uq_first_occurrence(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start,
                        uint64_t first_read, uint64_t nreads, uint64_t read_index_base, uint64_t* d_first /*[256], pre-set to UQ_NONE*/);

/* ---- the record fingerprint `uqfp1` (an extension: the reference cannot tell whether a container gives its FASTQ back; DESIGN.md
 * section 19).  Nine u64 sums over records, all arithmetic mod 2^64.  K = 0x9E3779B97F4A7C15;
 *   mix(x):  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
 *   line hash LH(tag, b) of a line b[0, L) without its '\n':  w_k = the little-endian u64 of b[8k, 8k + 8), zero-padded, k in [0, ceil(L / 8));
 *       acc = SUM_k mix(w_k + K (k + 1))  (0 for an empty line);  LH = mix(acc + K L + tag)
 *   record r (global index, 0-based) with lines q, s, p, u:  hq = LH(1, q), hs = LH(2, s), hu = LH(4, u);
 *       pair = mix(hs + mix(hu)),  rec = mix(hq + pair),  ord = mix(rec + K (r + 1))
 * reads; bases = SUM len(s); plus_text = the records whose line 3 is not exactly "+" (line 3 enters nothing else: the format does not store
 * it); qname = SUM hq, dna = SUM hs, qual = SUM hu, pairs = SUM pair, records = SUM rec, ordered = SUM ord.  Two texts with equal `ordered`
 * (and reads, bases) hold the same reads in the same order, with equal `records` the same reads as a multiset; the other sums say which
 * line class differs.  The sums commute: pieces and shards add.  NOT cryptographic: it catches accidents, not adversaries.
 * uq_fingerprint_init zeroes *d_fp (device, 8-byte aligned).  uq_fingerprint_accumulate ADDS the records [first_read, first_read + nreads)
 * of d_buf (any alignment; d_line_start as uq_index_lines writes it; lines shorter than 2^32 bytes) into *d_fp, record first_read + i with the
 * global index read_index_base + i (uq_first_occurrence's convention): one read of the stream, nothing written but the nine sums; queued on
 * the context's stream.  uq_fingerprint_host: the same, sequentially, on host memory (ADDS into *h_fp; needs no GPU). */
typedef struct uq_fingerprint { uint64_t reads, bases, plus_text, qname, dna, qual, pairs, records, ordered; } uq_fingerprint;
int uq_fingerprint_init(uq_ctx* ctx, uq_fingerprint* d_fp);
int uq_fingerprint_accumulate(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start,
                              uint64_t first_read, uint64_t nreads, uint64_t read_index_base, uq_fingerprint* d_fp);
int uq_fingerprint_host(const uint8_t* h_buf, const uint64_t* h_line_start,
                        uint64_t first_read, uint64_t nreads, uint64_t read_index_base, uq_fingerprint* h_fp);

/* ---- the per-cycle quality control tables `uqqc1` (`--qc`; an extension: the reference says nothing about what a file holds; DESIGN.md
 * section 24).  One flat array of u64 counters, C = ncycles, 1 <= C <= UQ_QC_MAX_CYCLES.  For a record with the sequence line s (length Ls)
 * and the quality line u (length Lu), both without their '\n', each line taken at its own length:
 *   cls(b):  A/a -> 0, C/c -> 1, G/g -> 2, T/t -> 3, N/n -> 4, every other byte -> 5
 *   q(b):    clamp((int)b - 33, 0, 93); a byte outside 33 .. 126 is clamped and also counted in qual_out_of_range
 *   row(p):  min(p, C) -- rows 0 .. C - 1 are exact cycles, row C is the tail and takes every position >= C
 * The array, in this order:
 *   [0 .. 8)                reads, bases = SUM Ls, qual_chars = SUM Lu, qual_out_of_range, len_mismatch = #records with Ls != Lu, three reserved words (0)
 *   base_by_cycle[C + 1][6]   [row(p)][cls(s[p])] += 1 for every p < Ls
 *   qual_by_cycle[C + 1][94]  [row(p)][q(u[p])] += 1 for every p < Lu
 *   length_hist[C + 1]        [min(Ls, C)] += 1 per record
 *   mean_qual_hist[94]        if Lu > 0: [floor(SUM_p q(u[p]) / Lu)] += 1
 *   gc_hist[101]              if Ls > 0: [floor(100 * #{p : cls(s[p]) in {1, 2}} / Ls)] += 1
 * uq_qc_words(C) = 8 + 100 (C + 1) + (C + 1) + 94 + 101, or 0 for an invalid C.  Every field is a sum over records: calls and shards add.
 * SUM base_by_cycle = bases, SUM qual_by_cycle = qual_chars, SUM length_hist = reads.
 * uq_qc_init zeroes d_qc[0, uq_qc_words(C)) (device, 8-byte aligned; queued on the context's stream).  uq_qc_accumulate ADDS the records
 * [first_read, first_read + nreads) of d_buf (any alignment; d_line_start as uq_index_lines writes it; lines shorter than 2^32 bytes; 64-bit
 * offsets) into d_qc: one read of the stream, nothing written but d_qc, nothing read back; nreads == 0 is a no-op.  uq_qc_host: the same,
 * sequentially, on host memory (ADDS into h_qc; needs no GPU). */
#define UQ_QC_MAX_CYCLES 1024u
#define UQ_QC_NBASE 6u
#define UQ_QC_NQUAL 94u
uint64_t uq_qc_words(uint32_t ncycles);
int uq_qc_init(uq_ctx* ctx, uint64_t* d_qc, uint32_t ncycles);
int uq_qc_accumulate(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start,
                     uint64_t first_read, uint64_t nreads, uint32_t ncycles, uint64_t* d_qc);
int uq_qc_host(const uint8_t* h_buf, const uint64_t* h_line_start,
               uint64_t first_read, uint64_t nreads, uint32_t ncycles, uint64_t* h_qc);

/* ---- quality binning (`--bin-qual`; an extension: the reference stores the qualities it is given).  LOSSY by request:
 * a byte table applied to the quality lines of a FASTQ text before anything else looks at it.
 * uq_requantise_qualities applies lut[] to every byte of line 4 (the quality line, without its '\n') of the records
 * [first_read, first_read + nreads) of d_buf, in place.  No other byte of d_buf is written.  d_line_start as uq_index_lines writes it.
 * h_lut: 256 bytes on the host, no entry may be '\n' (refused with an error: line ends must stay where they are, so the index stays valid) -- except
 * lut['\n'] itself, which no line ever looks up, so that the identity table passes.
 * d_changed (may be NULL): device u64, 8-byte aligned; the number of bytes whose value changed is ADDED to it (calls and shards add).
 * Queued on the context's stream; nothing is read back.  Any buffer alignment; lines shorter than 2^32 bytes; offsets are 64-bit everywhere.
 * The kernel reads the quality lines and 16 B of line starts per record, and writes the quality lines; an item stores only bytes of its
 * own line (whole 16-byte vectors and dwords inside a line, single bytes at its ends), so lines that share a vector do not race.
 * uq_requantise_qualities_host: the same, sequentially, on host memory (needs no GPU; ADDS into *h_changed, which may be NULL). */
int uq_requantise_qualities(uq_ctx* ctx, uint8_t* d_buf, const uint64_t* d_line_start,
                            uint64_t first_read, uint64_t nreads, const uint8_t* h_lut, uint64_t* d_changed);
int uq_requantise_qualities_host(uint8_t* h_buf, const uint64_t* h_line_start,
                                 uint64_t first_read, uint64_t nreads, const uint8_t* h_lut, uint64_t* h_changed);

/* ---- paired-end input (`--mate2`, `--interleaved`; an extension: the reference reads one stream).  A paired container
 * is the plain encode of the interleaved text: R1 record, its R2 record, the next R1 record, and so on.
 * uq_interleave_records: d_ls_a / d_ls_b are the record indexes of d_a / d_b as uq_index_lines writes them.  With A(r) = the bytes
 * [ls_a[4r], ls_a[4r + 4]) of d_a and B(r) likewise, writes A(first_pair) B(first_pair) A(first_pair + 1) B(first_pair + 1) ... for npairs
 * pairs to d_out, from byte 0 on: with base = ls_a[4 first_pair] + ls_b[4 first_pair], A(r) lands at ls_a[4r] + ls_b[4r] - base and B(r) at
 * ls_a[4r + 4] + ls_b[4r] - base.  The size, (ls_a[4 (first_pair + npairs)] - ls_a[4 first_pair]) + the same of b, is read back first:
 * out_capacity below it is an error before anything is launched on the buffers.  Nothing outside [0, size) of d_out is written; npairs == 0
 * is a no-op.  Any buffer alignment (the stores are 16-byte vectors at aligned addresses, single bytes at the output's two ends); lines
 * shorter than 2^32 bytes; offsets are 64-bit everywhere; queued on the context's stream.  d_out must not overlap d_a or d_b.
 * uq_mate_check: pair i, i < npairs, compares the QNAME line (line 1) of record first_a + i step_a of d_a with that of record
 * first_b + i step_b of d_b -- two files: (0, 1) and (0, 1); one interleaved buffer: the same buffer and index twice, (0, 2) and (1, 2).
 *   The id of a QNAME line, without its '\n', is its bytes up to but excluding the first ' ' or '\t'; the whole line if there is none.
 *   If the id of a ends in "/1" and the id of b ends in "/2", those two bytes are dropped from both (the other way round is not dropped).
 *   The pair matches when the two ids are then equal byte for byte.
 * uq_mate_report (device, 8-byte aligned): pairs = the pairs counted; mismatches = the pairs that do not match; first_mismatch = the lowest
 * pair_index_base + i that does not match (an atomic MIN: uq_mate_report_init sets it to UINT64_MAX and the counts to 0); slash_pairs = the
 * pairs whose "/1" and "/2" were dropped.  Calls and shards add.  The kernel reads only the QNAME lines and their line starts and writes only
 * the report; queued on the context's stream, nothing read back.
 * uq_interleave_records_host, uq_mate_check_host: the same, sequentially, on host memory (need no GPU; the report is ADDED to). */
typedef struct uq_mate_report { uint64_t pairs, mismatches, first_mismatch, slash_pairs; } uq_mate_report;
int uq_interleave_records(uq_ctx* ctx, const uint8_t* d_a, const uint64_t* d_ls_a, const uint8_t* d_b, const uint64_t* d_ls_b,
                          uint64_t first_pair, uint64_t npairs, uint8_t* d_out, uint64_t out_capacity);
int uq_interleave_records_host(const uint8_t* h_a, const uint64_t* h_ls_a, const uint8_t* h_b, const uint64_t* h_ls_b,
                               uint64_t first_pair, uint64_t npairs, uint8_t* h_out, uint64_t out_capacity);
int uq_mate_report_init(uq_ctx* ctx, uq_mate_report* d_report);
int uq_mate_check(uq_ctx* ctx, const uint8_t* d_a, const uint64_t* d_ls_a, uint64_t first_a, uint64_t step_a,
                  const uint8_t* d_b, const uint64_t* d_ls_b, uint64_t first_b, uint64_t step_b,
                  uint64_t npairs, uint64_t pair_index_base, uq_mate_report* d_report);
int uq_mate_check_host(const uint8_t* h_a, const uint64_t* h_ls_a, uint64_t first_a, uint64_t step_a,
                       const uint8_t* h_b, const uint64_t* h_ls_b, uint64_t first_b, uint64_t step_b,
                       uint64_t npairs, uint64_t pair_index_base, uq_mate_report* h_report);

/* ---- read filtering (`--filter`; an extension: the reference stores every read it is given).  A filtered container is
 * the plain encode of the filtered text.  All arithmetic is unsigned 64-bit; mix and K are the fingerprint's (uqfp1, above), cls and q the QC
 * tables' (uqqc1, above): N is cls == 4, that is 'N' or 'n', and q(b) = clamp(b - 33, 0, 93).
 * A record with the sequence line s (length Ls) and the quality line u (length Lu), both without their '\n', has the global index
 * g = read_index_base + i and belongs to unit w = g / unit; unit is 1 for single reads and 2 for interleaved pairs.  Its VERDICT is a byte,
 * the OR of
 *    1  min_len   Ls < min_len
 *    2  max_len   Ls > max_len
 *    4  max_n     #{p < Ls : cls(s[p]) == 4} > max_n
 *    8  mean_q    SUM_p q(u[p]) < min_mean_q * Lu   (an empty quality line passes)
 *   16  sample    flags & UQ_FILTER_SAMPLE and mix(seed + K (w + 1)) >= sample_threshold
 * The sample bit depends on w alone: both mates of a pair share it, and shards and pieces agree.  Criteria are switched off by min_len = 0,
 * max_len = max_n = UINT32_MAX, min_mean_q = 0 and the sample flag clear.  A unit is KEPT iff the verdicts of all its records are 0.  The
 * FILTERED TEXT is the kept units' bytes [ls[4 r0], ls[4 (r0 + unit)]), in input order, back to back from byte 0.
 * uq_filter_report (device, 8-byte aligned; uq_filter_report_init zeroes it): every field is a sum, so calls and shards add.
 * uq_filter_mark writes d_verdict[i] for record first_read + i, i < nreads, and ADDS reads_in, bases_in (SUM Ls), bytes_in and each fail_* once
 *   per record with that bit set (a record can count under several).  It reads the records and 32 B of line starts per record and writes the
 *   verdicts and the report, nothing else; queued on the context's stream, nothing read back.
 * uq_filter_plan (nreads % unit == 0) writes, for the kept units j = 0 .. kept - 1 in input order, d_src[j] = the unit's byte offset in the
 *   source, d_dst[j] = its offset in the output, and d_dst[kept] = the output's size; d_src holds nreads / unit entries, d_dst one more.  ADDS
 *   reads_out, bases_out, bytes_out and fail_mate (the records with verdict 0 whose unit is dropped) to the report; hands back the two counts
 *   (synchronises).
 * uq_compact_records copies unit j's bytes [src[j], src[j] + dst[j + 1] - dst[j]) of d_buf to d_out + dst[j] (dst[0] = 0, ascending, a unit is
 *   at least 4 bytes: what uq_filter_plan writes).  out_capacity < dst[kept_units] is an error before anything is launched on the buffers;
 *   kept_units == 0 is a no-op; d_out must not overlap d_buf.  Nothing outside [0, dst[kept_units]) of d_out is written (16-byte stores at
 *   aligned addresses, single bytes at the output's two ends), nothing outside the units -- so nothing outside [0, nbytes) -- of d_buf is read.
 * Any buffer alignment; lines shorter than 2^32 bytes; 64-bit offsets everywhere.  unit not 1 or 2, nreads or read_index_base odd with unit 2,
 * min_len > max_len and min_mean_q > 93 are errors.  The _host forms: the same, sequentially, on host memory (need no GPU). */
#define UQ_FILTER_SAMPLE 1u
typedef struct uq_filter_params { uint32_t min_len, max_len, max_n, min_mean_q; uint64_t sample_threshold, seed; uint32_t unit, flags; } uq_filter_params;
typedef struct uq_filter_report { uint64_t reads_in, bases_in, bytes_in, reads_out, bases_out, bytes_out,
                                  fail_min_len, fail_max_len, fail_max_n, fail_mean_q, fail_sample, fail_mate; } uq_filter_report;
int uq_filter_report_init(uq_ctx* ctx, uq_filter_report* d_report);
int uq_filter_report_init_host(uq_filter_report* h_report);
int uq_filter_mark(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads,
                   uint64_t read_index_base, const uq_filter_params* h_params, uint8_t* d_verdict, uq_filter_report* d_report);
int uq_filter_mark_host(const uint8_t* h_buf, const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads,
                        uint64_t read_index_base, const uq_filter_params* h_params, uint8_t* h_verdict, uq_filter_report* h_report);
int uq_filter_plan(uq_ctx* ctx, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads, uint32_t unit, const uint8_t* d_verdict,
                   uint64_t* d_src, uint64_t* d_dst, uq_filter_report* d_report, uint64_t* h_kept_units, uint64_t* h_out_bytes);
int uq_filter_plan_host(const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads, uint32_t unit, const uint8_t* h_verdict,
                        uint64_t* h_src, uint64_t* h_dst, uq_filter_report* h_report, uint64_t* h_kept_units, uint64_t* h_out_bytes);
int uq_compact_records(uq_ctx* ctx, const uint8_t* d_buf, uint64_t nbytes, const uint64_t* d_src, const uint64_t* d_dst, uint64_t kept_units,
                       uint8_t* d_out, uint64_t out_capacity);
int uq_compact_records_host(const uint8_t* h_buf, uint64_t nbytes, const uint64_t* h_src, const uint64_t* h_dst, uint64_t kept_units,
                            uint8_t* h_out, uint64_t out_capacity);

/* ---- read trimming (`--trim`; an extension: the reference stores every read as it is given).  A trimmed container is
 * the plain encode of the trimmed text.  cls and q are the QC tables' (uqqc1, above): G is cls == 2 ('G' or 'g'), N is cls == 4 ('N' or 'n'),
 * q(b) = clamp(b - 33, 0, 93).  A record has the lines qn, s, p, u without their '\n' (a '\r' in front of a '\n' is the line's last byte, as
 * everywhere), Ls = len(s), Lu = len(u).  If Ls != Lu the record is copied unchanged: its WINDOW is (0, Ls), it counts once in len_mismatch and
 * enters no cut_* sum.  Otherwise L = Ls and the window [a, b) is made in four steps, in this order:
 *   1 fixed    a = min(head, L); b = L - min(tail, L - a); if crop != UINT32_MAX: b = min(b, a + crop); cut_fixed += L - (b - a).
 *   2 poly-G   (polyg = G, 0 = off) g = the number of consecutive bytes with cls == 2 at the end of s[a, b); if G > 0 and g >= G: b -= g,
 *              cut_polyg += g.
 *   3 quality  (q3 = T3, q5 = T5, 0 = off, at most 93; the BWA / cutadapt running sum, signed 64-bit) both on the window [a, b) step 2 left,
 *              independently of each other.
 *              3' end: acc = 0, best = 0, b' = b; for i = b - 1 down to a: acc += T3 - q(u[i]); if acc < 0 stop; if acc > best: best = acc, b' = i.
 *              5' end: acc = 0, best = 0, a' = a; for i = a up to b - 1: acc += T5 - q(u[i]); if acc < 0 stop; if acc > best: best = acc, a' = i + 1.
 *              cut_q3 += b - b'; a'' = min(a', b'); cut_q5 += a'' - a; the window becomes [a'', b').
 *              In closed form, with S_i = SUM_{j = i .. b - 1} (T3 - q(u[j])): stop = the largest i in [a, b) with S_i < 0 (a - 1 if there
 *              is none); b' = the i in (stop, b) with the largest S_i > 0, the largest such i among equals (b if there is none).  The 5' form
 *              is the mirror image.
 *   4 N ends   (flags & UQ_TRIM_N) while a < b and cls(s[a]) == 4: a++; while b > a and cls(s[b - 1]) == 4: b--; cut_n += what was removed.
 * The TRIMMED RECORD is qn '\n' s[a:b] '\n' p '\n' u[a:b] '\n'; the TRIMMED TEXT is the trimmed records in input order, back to back from byte 0.
 * uq_trim_report (device, 8-byte aligned; uq_trim_report_init zeroes it): thirteen sums, so calls and shards add.  reads_trimmed = the records
 *   whose window is not (0, Ls); emptied = the records with a == b and L > 0;  bases_in - bases_out = cut_fixed + cut_polyg + cut_q5 + cut_q3
 *   + cut_n and bytes_in - bytes_out = 2 (bases_in - bases_out).
 * uq_trim_mark writes d_window[2 i] = a, d_window[2 i + 1] = b for record first_read + i, i < nreads, and ADDS every field of the report.  It
 *   reads the records and their line starts and writes the windows and the report, nothing else; queued on the context's stream, nothing
 *   read back.
 * uq_trim_plan writes d_dst[i] = the output offset of record first_read + i and d_dst[nreads] = the output's size (uq_scan_exclusive_u64), and
 *   hands the size back (one read-back; synchronises).
 * uq_trim_records writes the trimmed records to d_out (record first_read + i at d_dst[i]) and, when d_line_start_out is not NULL, the record
 *   index of the trimmed text (4 nreads + 1 entries: what uq_index_lines would write for it).  out_capacity < dst[nreads] is an error before
 *   anything is launched on the buffers; nreads == 0 is a no-op; d_out must not overlap d_buf.  Nothing outside [0, dst[nreads]) of d_out is
 *   written (16-byte stores at aligned addresses, single bytes at the output's two ends), nothing outside the records of d_buf is read.
 * Any buffer alignment; lines shorter than 2^32 bytes with their '\n'; 64-bit offsets everywhere.  q5 > 93, q3 > 93 and crop == 0 are errors.
 * A window with a > b or b > Ls (or, where Ls != Lu, another one than (0, Ls)) handed to uq_trim_plan or uq_trim_records is an error in the
 * _host forms and UNDEFINED on the device.  The _host forms: the same, sequentially, on host memory (need no GPU). */
#define UQ_TRIM_N 1u
typedef struct uq_trim_params { uint32_t head, tail, crop, polyg, q5, q3, flags, reserved; } uq_trim_params;
typedef struct uq_trim_report { uint64_t reads_in, bases_in, bytes_in, reads_trimmed, bases_out, bytes_out,
                                cut_fixed, cut_polyg, cut_q5, cut_q3, cut_n, emptied, len_mismatch; } uq_trim_report;
int uq_trim_report_init(uq_ctx* ctx, uq_trim_report* d_report);
int uq_trim_report_init_host(uq_trim_report* h_report);
int uq_trim_mark(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads,
                 const uq_trim_params* h_params, uint32_t* d_window, uq_trim_report* d_report);
int uq_trim_mark_host(const uint8_t* h_buf, const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads,
                      const uq_trim_params* h_params, uint32_t* h_window, uq_trim_report* h_report);
int uq_trim_plan(uq_ctx* ctx, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads, const uint32_t* d_window,
                 uint64_t* d_dst, uint64_t* h_out_bytes);
int uq_trim_plan_host(const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads, const uint32_t* h_window,
                      uint64_t* h_dst, uint64_t* h_out_bytes);
int uq_trim_records(uq_ctx* ctx, const uint8_t* d_buf, uint64_t nbytes, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads,
                    const uint32_t* d_window, const uint64_t* d_dst, uint8_t* d_out, uint64_t out_capacity, uint64_t* d_line_start_out);
int uq_trim_records_host(const uint8_t* h_buf, uint64_t nbytes, const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads,
                         const uint32_t* h_window, const uint64_t* h_dst, uint8_t* h_out, uint64_t out_capacity, uint64_t* h_line_start_out);

/* ---- 3' adapter removal (`--adapter`; an extension).  A marking step that NARROWS the windows of the trim section above:
 * the plan and the copy are uq_trim_plan and uq_trim_records.  cls is the QC tables' class (uqqc1, above): A 0, C 1, G 2, T 3 in either case,
 * N 4, anything else 5.  An ADAPTER A is La letters of ACGT, 1 <= La <= UQ_ADAPTER_MAX, stored as classes 0 .. 3 (lower case is folded by whoever
 * fills the structure: the library sees classes only).  A record comes with a window [a, b), a <= b <= Ls: the one uq_trim_mark wrote, or
 * (0, Ls) when UQ_ADAPTER_FRESH is set -- then d_window is not read, only written.  A record with Ls != Lu keeps (0, Ls) and counts once in
 * len_mismatch and in reads_in, with Ls added to bases_in and to bases_out.  For every other record and every p in [a, b):
 *   m(p) = min(La, b - p);
 *   p is a CANDIDATE when m(p) >= overlap and #{ j < m(p) : cls(s[p + j]) != A[j] } <= (m(p) * err_pct) / 100 (integer division); N and
 *   other bytes in the read never match (a '\r' in front of the '\n' is the line's last byte, class 5: a mismatch like any other).
 * The new window is [a, p*) for the LEFTMOST candidate p* (the rule fastp uses); it is unchanged when there is none.  The match is FULL when
 * m(p*) == La, otherwise PARTIAL; p* == a (with a < b) EMPTIES the read: an adapter dimer.  With UQ_ADAPTER_PAIRED the records with odd
 * first_read + i are matched against seq2, the others against seq1 (the interleaved layout of the pairs section); without it every record
 * uses seq1 and len2 / seq2 only have to be well-formed.  Hamming distance only: no insertions or deletions.
 * uq_adapter_report (device, 8-byte aligned; uq_adapter_report_init zeroes it): nine sums, so calls and shards add.  bases_in = SUM b - a as
 *   received, bases_out = the same sum afterwards, reads_cut = full + partial, mate2 = the cut records that used seq2, emptied = the windows
 *   that were not empty and are now.
 * uq_adapter_mark reads the records, their line starts and (without FRESH) d_window, writes d_window[2 i], d_window[2 i + 1] for every record
 *   first_read + i, i < nreads, and ADDS every field of the report, nothing else; queued on the context's stream, nothing read back.
 * Errors: null arguments, d_window not 4-byte or d_report not 8-byte aligned, len1 outside 1 .. 64, len2 > 64 (or 0 with PAIRED), a sequence
 * byte above 3, overlap outside 1 .. min(len1, len2 where PAIRED), err_pct > 30, unknown flag bits, non-zero reserved words.  A window with
 * a > b or b > Ls handed in is an error in the _host form and UNDEFINED on the device (uq_trim_plan's contract).  An error of either form
 * is raised before anything is written: windows and report are as they were.  Any buffer alignment; lines
 * shorter than 2^32 bytes with their '\n'.  The _host forms: the same, sequentially, on host memory (need no GPU). */
#define UQ_ADAPTER_MAX    64
#define UQ_ADAPTER_FRESH  1u
#define UQ_ADAPTER_PAIRED 2u
typedef struct uq_adapter_params { uint32_t len1, len2, overlap, err_pct, flags, reserved[3]; uint8_t seq1[64], seq2[64]; } uq_adapter_params;
typedef struct uq_adapter_report { uint64_t reads_in, bases_in, bases_out, reads_cut, full, partial, mate2, emptied, len_mismatch; } uq_adapter_report;
int uq_adapter_report_init(uq_ctx* ctx, uq_adapter_report* d_report);
int uq_adapter_report_init_host(uq_adapter_report* h_report);
int uq_adapter_mark(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads,
                    const uq_adapter_params* h_params, uint32_t* d_window, uq_adapter_report* d_report);
int uq_adapter_mark_host(const uint8_t* h_buf, const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads,
                         const uq_adapter_params* h_params, uint32_t* h_window, uq_adapter_report* h_report);

/* ---- duplicate removal (`--dedup`; an extension: the reference stores every read it is given).  A deduplicated container
 * is the plain encode of the deduplicated text.  The result is EXACT: no read is dropped on a hash match alone.  All arithmetic is unsigned
 * 64-bit; mix and K are the fingerprint's (uqfp1, above), q(b) = clamp(b - 33, 0, 93) the QC tables' (uqqc1, above).  A UNIT is one record
 * (unit = 1) or an interleaved pair (unit = 2); record first_read + i has the global index g = unit_index_base + i and belongs to unit
 * w = g / unit (the convention of uq_filter_mark's read_index_base), so the call's first unit is unit_index_base / unit and unit w of the
 * call holds the records first_read + w unit .. first_read + w unit + unit - 1.
 *   COMPARED TEXT of a record with the sequence line s (length Ls, without its '\n'): c = s[0, Lc), Lc = Ls if prefix == 0, else min(Ls, prefix).
 *     Bytes are compared as they are: case-sensitive, and N equals N.  Two units are EQUAL iff every record of the one has the same Lc and the
 *     same c bytes as the corresponding record of the other.  Quality and QNAME lines never enter the comparison.
 *   SEEDED LINE HASH  S = mix(seed + K); w_k = the little-endian u64 of c[8k, 8k + 8), zero-padded;
 *     acc = SUM_k mix((w_k ^ S) + K (k + 1))  (0 for an empty text);  DL(c) = mix(acc + K Lc + 2).
 *   UNIT HASH  unit 1: H = DL(c); unit 2: H = mix(DL(c1) + mix(DL(c2))); then H is masked to its low hash_bits bits (1 .. 64; 64 = no mask;
 *     fewer than 64 exist for tuning and tests only: they force collisions).
 *   SCORE  with UQ_DEDUP_BEST: min(SUM q(u[p]) over the whole quality line(s) of the unit, 2^32 - 1); otherwise 0.
 *   KEY ROW of unit w, 16 bytes in memcmp order: H big-endian (8), 0xFFFFFFFF - score big-endian (4; four zero bytes without UQ_DEDUP_BEST),
 *     w big-endian (4; unit numbers are below 2^32, as everywhere in this ABI).
 *   MARK RULE over perm, the memcmp-ascending order of the call's key rows (entries are the call's unit numbers 0 .. nreads / unit - 1; a total
 *     order, because w is in the key; what uq_argsort_rows(keys, units, 16) writes): position 0 opens a class.  For j > 0, a = perm[j - 1],
 *     b = perm[j]: H(a) != H(b): b opens a class.  H(a) == H(b) and the units are equal: b is a DUPLICATE, every record of b gets verdict 1.
 *     H(a) == H(b) and the units differ: b opens a class and collisions += 1.  Every record not marked duplicate gets verdict 0.
 *   If collisions == 0 every hash run is one class and every class lies in one run: the kept units are exactly one per distinct compared text,
 *   the first in input order, or with UQ_DEDUP_BEST the one with the highest score, ties to the lower index.  If collisions > 0 no
 *   non-duplicate was dropped but some duplicates may have been kept: the caller repeats with seed + 1.
 *   The DEDUPLICATED TEXT is the units whose records all have verdict 0, in input order, back to back: what uq_filter_plan and
 *   uq_compact_records make of the verdict array.
 * uq_dedup_report (device, 8-byte aligned; uq_dedup_report_init zeroes it): every field is a sum, so calls add.  uq_dedup_keys ADDS reads_in,
 *   bases_in (SUM Ls) and units_in; uq_dedup_mark ADDS classes, dup_units, dup_reads (the duplicates' records), dup_bases (SUM Ls of those)
 *   and collisions.
 * uq_dedup_keys writes the key row of the call's unit w to d_keys + 16 w (16-byte aligned): one read of the stream, 32 B of line starts per
 *   record; nothing else is written but the report.  uq_dedup_mark reads d_keys and d_perm (4-byte aligned), the line starts and the text of
 *   hash-equal neighbours only, and writes d_verdict[i] for EVERY record first_read + i, i < nreads, whatever it held before.  An entry of
 *   d_perm beyond the units is an error in the _host form; the device reads unit 0 for it (never out of bounds).  Both are queued on the
 *   context's stream, nothing is read back.
 * Errors: null arguments, unit not 1 or 2, nreads, first_read or unit_index_base odd with unit 2, hash_bits outside 1 .. 64, unknown flag bits,
 * more than 2^32 units (with the base), misaligned d_keys, d_perm or d_report.  Any buffer alignment; lines shorter than 2^32 bytes; 64-bit
 * offsets everywhere.  The _host forms: the same, sequentially, on host memory (need no GPU). */
#define UQ_DEDUP_BEST 1u
typedef struct uq_dedup_params { uint32_t unit, prefix, hash_bits, flags; uint64_t seed; } uq_dedup_params;
typedef struct uq_dedup_report { uint64_t reads_in, bases_in, units_in, classes, dup_units, dup_reads, dup_bases, collisions; } uq_dedup_report;
int uq_dedup_report_init(uq_ctx* ctx, uq_dedup_report* d_report);
int uq_dedup_report_init_host(uq_dedup_report* h_report);
int uq_dedup_keys(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads,
                  uint64_t unit_index_base, const uq_dedup_params* h_params, uint8_t* d_keys, uq_dedup_report* d_report);
int uq_dedup_keys_host(const uint8_t* h_buf, const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads,
                       uint64_t unit_index_base, const uq_dedup_params* h_params, uint8_t* h_keys, uq_dedup_report* h_report);
int uq_dedup_mark(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads,
                  uint64_t unit_index_base, const uq_dedup_params* h_params, const uint8_t* d_keys, const uint32_t* d_perm,
                  uint8_t* d_verdict, uq_dedup_report* d_report);
int uq_dedup_mark_host(const uint8_t* h_buf, const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads,
                       uint64_t unit_index_base, const uq_dedup_params* h_params, const uint8_t* h_keys, const uint32_t* h_perm,
                       uint8_t* h_verdict, uq_dedup_report* h_report);

/* ---- a3 / a4: the per-read packers. Replaces `encoder_fixed` (uq.py:108-182) and
 * `encoder_variable` (uq.py:188-254).  Row = sum_j code(read[j]) << (bits * (L-1-j)) [+ 1 << bits*L
 * when `variable`], big-endian, right-aligned in `*_bytes_per_row` bytes, high bytes zero. */
typedef struct uq_pack_params {
    int16_t dna_code[256];      /* bases.index(byte), or -1 when the byte is not in `bases` (uq.py:149-152) */
    int16_t qual_code[256];     /* qualities.index(byte), or -1 */
    int32_t n_qual[256];        /* N_qual[byte] for bytes with dna_code == -1, else -1 (uq.py:153) */
    int32_t bits_per_base, bits_per_quality;
    int32_t variable;           /* 0 = encoder_fixed, 1 = encoder_variable */
    int32_t dna_bytes_per_row, quality_bytes_per_row;
    int32_t max_record_bytes;   /* from uq_stats (tile sizing) */
    int32_t dna_max;            /* longest read */
    int32_t avg_record_bytes;   /* optional: mean record bytes (tile sizing for variable-length files), 0 = unknown */
} uq_pack_params;
/* Packs reads [first_read, first_read + nreads) into d_dna / d_qual rows [0, nreads).
 * *d_bad (device, 8 bytes, pre-set to UQ_NONE by the callee) = smallest local read index holding a
 * symbol with no code, else UQ_NONE. */
int uq_pack(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t first_read,
            uint64_t nreads, const uq_pack_params* h_params, uint8_t* d_dna, uint8_t* d_qual, uint64_t* d_bad);
/* a1 + a3/a4 in ONE pass over the stream: packs with GUESSED parameters (h_guess: e.g. the decisions of the previous
 * file / shard, or of a sample of this one) and accumulates the pass-1 statistics of the same reads into d_stats
 * (initialised by uq_stats_init) while the characters are in registers.  The caller then derives the real decisions
 * from d_stats (uq.py:448-545) and keeps the tables iff they equal the guess; otherwise it calls uq_pack with the
 * real ones -- nothing is assumed, the stream is just read once instead of twice when the guess holds.
 * *h_fused = 0: this geometry has no fused kernel (anything but 2-bit A/C/G/T with one contiguous quality range, the
 * Q9 carry case, records beyond one tile) and NOTHING was launched: run uq_stats_accumulate + uq_pack.
 * d_stats->reserved != 0 after the call: the counts are incomplete (a read longer than h_guess->dna_max, a record
 * longer than h_guess->max_record_bytes, SEQ / QUAL lengths differ, a symbol outside the guessed alphabets -- the kernel counts
 * on the codes the conversion produces): re-initialise and run uq_stats_accumulate.  No fused kernel either for more than 64
 * quality symbols (a count bin per byte). */
int uq_pack_stats(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t first_read,
                  uint64_t nreads, const uq_pack_params* h_guess, uint8_t* d_dna, uint8_t* d_qual, uint64_t* d_bad,
                  uq_stats* d_stats, int* h_fused);
/* uq_pack_stats of ALL reads of the buffer behind uq_count_lines_end_async + uq_index_lines_async (above): the number of reads
 * (lines / 4) is taken on the device; d_dna / d_qual hold capacity_reads rows -- more reads than that raise d_stats->reserved. */
int uq_pack_stats_async(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t capacity_reads,
                        const uq_pack_params* h_guess, uint8_t* d_dna, uint8_t* d_qual, uint64_t* d_bad,
                        uq_stats* d_stats, int* h_fused);
/* The tile geometry the pack kernels run these parameters at (csrc/pack_geometry.h; host only, no context): `form` says which kernel --
 * 0 the plain pack, UQ_PACK_FORM_STATS the fused pack + statistics kernel, with UQ_PACK_FORM_QNAME its QNAME phase, with UQ_PACK_FORM_LISTS
 * the line starts from the census's lists (d_line_start == NULL).  tiled = 0: the longest record fits no tile (the exact kernel packs; no fused
 * form) and the other fields are zero.  Else reads per tile (R) and per piece of a tile beyond the stage (Rs), lanes per read (P) over G groups of
 * eight symbols, the staging region and the out tile in bytes, the copies of the count table, the workgroup's LDS (static and dynamic) and the
 * workgroups a CU's LDS holds; tile64 = 1: the 64-read tile. */
#define UQ_PACK_FORM_STATS 1u
#define UQ_PACK_FORM_QNAME 2u
#define UQ_PACK_FORM_LISTS 4u
typedef struct uq_pack_tile_geom {
    uint32_t tiled, tile64, R, Rs, P, G, stage_bytes, out_bytes, copies, lds_bytes, wg_per_cu, reserved;
} uq_pack_tile_geom;
int uq_pack_tile_geometry(const uq_pack_params* h_params, uint32_t form, uq_pack_tile_geom* h_out);

/* ---- a9 / a11: the eight --pattern byte layouts.  Replaces numpy.rot90 + ascontiguousarray /
 * asfortranarray + the payload write of numpy.save (uq.py:263-270) and, inverse, numpy.load +
 * rot90(-k) (uq.py:943-945).  pattern_id = 2*k + (order == '.2'), k = rotations (so '0.1'=0,
 * '0.2'=1, '1.1'=2, '1.2'=3, '2.1'=4, '2.2'=5, '3.1'=6, '3.2'=7).  d_payload is the rows*cols
 * payload bytes in file order; the .npy header (shape, fortran_order) is host business. */
int uq_pattern(uq_ctx* ctx, const uint8_t* d_table, uint64_t rows, uint32_t cols, int pattern_id, uint8_t* d_payload);
int uq_unpattern(uq_ctx* ctx, const uint8_t* d_payload, uint64_t rows, uint32_t cols, int pattern_id, uint8_t* d_table);

/* ---- a5: stable argsort of rows in memcmp order.  Replaces table.view('V<C>') +
 * numpy.argsort(axis=0) (uq.py:773-775).  d_perm[j] = index of the j-th smallest row. */
int uq_argsort_rows(uq_ctx* ctx, const uint8_t* d_table, uint64_t rows, uint32_t cols, uint32_t* d_perm);
/* How the row sorts of this context run their round 0 (tuning and tests; the result is the same order either way).  Tables of
 * msd_min_rows rows and more whose heads spread take the MSD partition finished in LDS (csrc/msd.hip), the others the LSD passes
 * (csrc/radix.hip): 0 = the built-in threshold (2^18), < 0 = never.  h_level_bits[nlevels] (1 .. 10 bits a level, at most 24 in all;
 * nlevels = 0: chosen from the row count) = the digits of the partition's levels.
 * uq_sort_counters: how many sorts of this context finished round 0 the one way and the other. */
int uq_sort_config(uq_ctx* ctx, int64_t msd_min_rows, const int* h_level_bits, int nlevels);
int uq_sort_counters(uq_ctx* ctx, uint64_t* h_msd_rounds, uint64_t* h_lsd_rounds);

/* ---- multi-GPU --sort: d_pos[k] = index of the first row of the memcmp-SORTED table that is
 * >= probe row k (numpy.searchsorted(side='left') on void rows).  Splits a locally sorted shard at the
 * splitter rows of the sample sort before the all-to-all. */
int uq_lower_bound_rows(uq_ctx* ctx, const uint8_t* d_sorted_table, uint64_t rows, uint32_t cols,
                        const uint8_t* d_probes, uint64_t nprobes, uint64_t* d_pos);

/* ---- a5 / a6 / a7 / a11: out[j] = table[index[j]].  Replaces table[sort_order] (uq.py:777),
 * key[sort_order] (798), columns_data[idx][sort_order] (822), table[key] on decode (953, 957, 973).
 * index_itemsize in {1,2,4,8} (keys are stored narrowed, uq.py:790). */
int uq_gather_rows(uq_ctx* ctx, const uint8_t* d_table, uint64_t table_rows, uint32_t cols,
                   const void* d_index, int index_itemsize, uint64_t n_out, uint8_t* d_out);

/* Decode-side validation of a stored key / mapping column before it indexes a table (a .uQ file is untrusted input):
 * *h_first_bad = lowest position j with index[j] >= limit, or UQ_NONE.  The reference's numpy raises IndexError on
 * such a file (uq.py:953, 957, 973 `table[key]`; 1016 `column['map'][row[i]]`); uq_gather_rows itself reads row 0 for an
 * out-of-range index (never out of bounds), so callers that want the error check first. */
int uq_check_index_range(uq_ctx* ctx, const void* d_index, int index_itemsize, uint64_t n, uint64_t limit, uint64_t* h_first_bad);

/* ---- a6: unique rows + inverse.  Replaces numpy.unique(rows as void, return_inverse=True)
 * (uq.py:784-789).  Outputs: d_perm = stable sort order of the rows (== argsort(key, stable),
 * uq.py:796), d_key[i] = rank of row i among the distinct rows, d_sorted_key[j] = d_key[d_perm[j]]
 * (uq.py:798), d_unique = the distinct rows in memcmp order (capacity rows*cols; pass NULL to skip),
 * *h_nunique = their number.  Any of d_key / d_sorted_key / d_unique may be NULL. */
int uq_unique_rows(uq_ctx* ctx, const uint8_t* d_table, uint64_t rows, uint32_t cols,
                   uint32_t* d_perm, uint32_t* d_key, uint32_t* d_sorted_key, uint8_t* d_unique, uint64_t* h_nunique);

/* ---- a6: key narrowing.  Replaces key.astype(numpy.min_scalar_type(max(key))) (uq.py:790, 832).
 * uq_key_itemsize: 1/2/4/8 for the largest key value nunique-1.  uq_narrow: u32 -> u8/u16/u32/u64. */
int uq_key_itemsize(uint64_t max_key);
int uq_narrow(uq_ctx* ctx, const uint32_t* d_key, uint64_t n, int itemsize, void* d_out);

/* ---- a7: QNAME column tables.  Replaces numpy.dstack(cols)[0] + structured view (uq.py:814-815,
 * 828-829): rows of ncols fields, each widened to `common_itemsize` and stored BIG-endian so that
 * memcmp order == field-by-field numeric order; then the row functions above apply.
 * uq_unstack_column converts one field of such rows back to a little-endian column of out_itemsize
 * (uq.py:846-847 `[:,idx].astype(dtype)`). */
int uq_stack_columns(uq_ctx* ctx, const void* const* h_d_cols, const int* h_itemsize, int ncols,
                     uint64_t n, int common_itemsize, uint8_t* d_rows);
int uq_unstack_column(uq_ctx* ctx, const uint8_t* d_rows, uint64_t n, int ncols, int common_itemsize,
                      int col, int out_itemsize, void* d_out);

/* ---- a12: unpack.  Replaces split_bits + the per-symbol char map, N restore and sentinel strip of
 * the decoder (uq.py:1002-1007, 1031-1054).  Outputs fixed-pitch text: d_seq / d_qualtxt are
 * uint8[nreads][dna_max], left-aligned, d_len[r] = read length. */
typedef struct uq_unpack_params {
    uint8_t base_char[256];     /* bases[code] */
    uint8_t qual_char[256];     /* qualities[code] (0 where undefined) */
    uint8_t qual_n_base[256];   /* qual_N[code] = the base an N-trick quality code restores, else 0 (uq.py:999, 1036) */
    int32_t bits_per_base, bits_per_quality;
    int32_t variable;
    int32_t dna_bytes_per_row, quality_bytes_per_row;
    int32_t dna_max;
} uq_unpack_params;
int uq_unpack(uq_ctx* ctx, const uint8_t* d_dna, const uint8_t* d_qual, uint64_t nreads,
              const uq_unpack_params* h_params, uint8_t* d_seq, uint8_t* d_qualtxt, uint32_t* d_len,
              uint64_t* d_bad /* smallest row with no sentinel (variable) or UQ_NONE */);

/* ---- f1: the QNAME passes, native on the HOST (no GPU involved).  Replaces the per-line Python of
 * uq.py:348-352, 394-444 (prefix / suffix / separator inference), 555-678 (column typing) and 717-736
 * (column encoding) with the same sequential semantics.  h_buf / h_line_start are HOST copies of the
 * FASTQ bytes and of the record index.  *h_status: 0 = done (*out valid); 1 = outside what the native
 * code reproduces exactly (regex-special separators, integers beyond int64, separators out of order):
 * use the Python implementation; 2 = the reference refuses this input too (uq_last_error() has its message).
 * uq_qname_json: {"prefix","suffix","separators","columns":[...]} as config.json stores them (uq.py:692-695).
 * uq_qname_column: column `col` as little-endian unsigned integers of the column's dtype, nreads entries. */
typedef struct uq_qname uq_qname;
int uq_qname_analyse(const uint8_t* h_buf, const uint64_t* h_line_start, uint64_t nreads, uq_qname** out, int* h_status);
int uq_qname_json(const uq_qname* q, const char** h_json);
int uq_qname_column(const uq_qname* q, int col, void* h_out, uint64_t capacity_bytes);
int uq_qname_free(uq_qname* q);

/* ---- f1 on the DEVICE: the same passes as reductions + one tokenising kernel over the FASTQ already in HBM.
 * uq_qname_layout (uq.py:348-352, 394-413): per character c of the first QNAME (candidate slot k, ch[k]):
 *   entry[k]    = first record whose common prefix with line 1 is <= the last position of c in line 1
 *                 (the record at which the reference's shrinking prefix sheds a c and starts counting it; UQ_NONE = never)
 *   lastviol[k] = last record whose count of c differs from line 1's (0 = none)
 *   c survives the reference's loop  <=>  entry[k] != UQ_NONE and lastviol[k] < entry[k].
 *   min_lcp / min_lcs = lengths of the common prefix / suffix.  flags bit0: some QNAME is a proper prefix or
 *   suffix of line 1 (the reference may raise IndexError there), bit1: a QNAME longer than 255 bytes -- in
 *   both cases use uq_qname_analyse.  Sharded input: h_line1 is the first QNAME of the WHOLE file,
 *   read_index_base the file-wide number of this shard's first read (0: the shard starts with line 1 itself, which
 *   is skipped); entry / lastviol are file-wide read numbers, so ranks combine results with MIN / MAX.
 * uq_qname_tokenise (uq.py:555-565, 717-736): splits QNAME[prefix_len : len - suffix_len] of every read at the
 *   ordered separators and writes, per column c, h_d_vals[c][read] = int(field) (0 if not an integer) and
 *   h_d_strs[c][read] = the field as 8 bytes in text order, zero padded (fields longer than 8 bytes that are
 *   canonical non-negative integers: 0x80 | value, big-endian).  Reductions per column: first_nonint (UQ_NONE if
 *   every field is [+-]digits), vmin / vmax over the integer fields, any_long bit0 = a field that does not fit
 *   the 8-byte key (long and not a canonical integer, or holding NUL / non-ASCII), bit1 = long canonical integer
 *   seen, bit2 = an integer field that is not the canonical decimal of its value ('+7', '007', '-0').  flags: bit0 separators missing / out of order / extra, bit1 whitespace inside a field (Python's int()
 *   strips it), bit2 more than 18 digits, bit3 QNAME shorter than prefix + suffix -- any flag: use uq_qname_analyse.
 * uq_prefix_distinct (uq.py:609-625, the `len(map) > entries_read / 10` checkpoints): from a STABLE argsort
 *   (d_perm) and the group ids in sorted order (d_sorted_key; both from uq_unique_rows), the number of distinct
 *   rows among rows [0, T] for each threshold T.  d_perm holds, per sorted position, the file-order index of that
 *   row as uint32 (perm_itemsize 4: the local argsort) or uint64 (8: file-wide indices after a distributed sort).
 * uq_int_prefix_distinct: the same counts for a column of INTEGER fields whose text is the canonical decimal of its value
 *   (then distinct strings = distinct values) without sorting it: first[v] = lowest read holding value v in [vmin, vmin +
 *   range) via atomic minima (a private LDS table per workgroup for small ranges), then h_counts[k] = #{v: first[v] <= T_k}.
 *   d_val = uq_qname_tokenise's value array; indices are file-wide (read_index_base + i).  any_long bit 2 from
 *   uq_qname_tokenise (a non-canonical integer such as '+7', '007', '-0' was seen) rules this shortcut out.
 * uq_encode_int (uq.py:724-733): d_out[i] = (unsigned itemsize)(d_val[i] - sub). */
typedef struct uq_qname_layout_result {
    uint32_t min_lcp, min_lcs;
    uint32_t flags;
    uint32_t nch;
    uint64_t entry[64];
    uint64_t lastviol[64];
    uint8_t ch[64];
} uq_qname_layout_result;
typedef struct uq_qname_cols_result {
    uint64_t first_nonint[32];
    int64_t vmin[32], vmax[32];
    uint32_t any_long[32];
    uint32_t flags;
    uint32_t reserved;
} uq_qname_cols_result;
int uq_qname_layout(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t nreads, uint64_t read_index_base,
                    const uint8_t* h_line1, uint32_t line1_len, uq_qname_layout_result* h_out);
int uq_qname_tokenise(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t nreads, uint32_t prefix_len,
                      uint32_t suffix_len, const uint8_t* h_separators, uint32_t nsep, int64_t* const* h_d_vals,
                      uint64_t* const* h_d_strs, uq_qname_cols_result* h_out);
int uq_prefix_distinct(uq_ctx* ctx, const void* d_perm, int perm_itemsize, const uint32_t* d_sorted_key, uint64_t n,
                       const uint64_t* h_thresholds, int nthresholds, uint64_t* h_counts);
int uq_int_prefix_distinct(uq_ctx* ctx, const int64_t* d_val, uint64_t n, int64_t vmin, uint64_t range, uint64_t read_index_base,
                           const uint64_t* h_thresholds, int nthresholds, uint64_t* h_counts);
int uq_encode_int(uq_ctx* ctx, const int64_t* d_val, uint64_t n, int64_t sub, int itemsize, void* d_out);

/* ---- e: row routing of the multi-GPU table builds (the reference is one process, these stand in for "all rows are in one
 * numpy array" of uq.py:767-851).  uq_partition_rows: d_dest[r] = rank that row r of an UNSORTED shard goes to in a sample sort, from
 * nsplit = world - 1 splitter rows in ascending order: the number of splitters below the row; a value that e >= 2 splitters share (a
 * tie group heavier than a rank's share) is dealt to those e ranks by file position, d_dest = lb + floor((row_index_base + r) * e /
 * total_rows), which keeps the concatenation of the ranks the stable order.  uq_owner_of_rows: d_owner[j] = rank whose record range
 * [h_shard_starts[k], h_shard_starts[k + 1]) holds file-wide row d_row_index[j].  uq_index_affine: d_out[j] = d_in[j] + add between
 * uint32 / int64 index arrays.  uq_invert_permutation: d_inv[d_perm[j] - base] = j; *h_bad = UQ_NONE or the lowest j that points
 * outside [0, n). */
/* unique + group ids (uq.py:786) of a shard that is ALREADY in memcmp order -- what the global sort hands a rank: no sort, one comparison
 * of neighbouring rows.  d_group[j] = dense rank of row j's value (from 0), d_unique (may be NULL) = the distinct rows in order. */
int uq_unique_sorted_rows(uq_ctx* ctx, const uint8_t* d_sorted_table, uint64_t rows, uint32_t cols, uint32_t* d_group, uint8_t* d_unique,
                          uint64_t* h_nunique);
/* The distinct rows of a table from what its sort left: the order (d_perm, uq_argsort_rows / uq_unique_rows) and the group ids of the
 * sorted positions (d_group = uq_unique_rows' d_sorted_key): d_unique[g] = the first row of group g, g < nunique.  d_perm = NULL: the
 * table has been moved into sorted order already.  Replaces the table half of numpy.unique (uq.py:786); only the distinct rows move. */
int uq_unique_rows_of_groups(uq_ctx* ctx, const uint8_t* d_table, uint64_t rows, uint32_t cols, const uint32_t* d_perm, const uint32_t* d_group,
                             uint64_t nunique, uint8_t* d_unique);
/* d_order = the positions 0 .. n - 1 grouped by d_dest[position] (ndest <= 16 destinations, ascending), each group in ascending order
 * (a stable partition); d_counts[k] (DEVICE, uint64) = size of group k.  What goes in front of an all-to-all: rows by destination rank,
 * requests by owner rank.  *h_bad (may be NULL: then nothing waits for the device) = UQ_NONE or a position whose destination is >= ndest. */
int uq_partition_order(uq_ctx* ctx, const uint8_t* d_dest, uint64_t n, uint32_t ndest, uint32_t* d_order, uint64_t* d_counts, uint64_t* h_bad);
int uq_partition_rows(uq_ctx* ctx, const uint8_t* d_splitters, uint32_t nsplit, uint32_t cols, const uint8_t* d_table, uint64_t rows,
                      uint64_t row_index_base, uint64_t total_rows, uint8_t* d_dest);
int uq_owner_of_rows(uq_ctx* ctx, const int64_t* d_row_index, uint64_t n, const int64_t* h_shard_starts, uint32_t world, uint8_t* d_owner);
int uq_index_affine(uq_ctx* ctx, const void* d_in, int in_itemsize, uint64_t n, int64_t add, void* d_out, int out_itemsize);
int uq_invert_permutation(uq_ctx* ctx, const void* d_perm, int perm_itemsize, uint64_t n, int64_t base, uint32_t* d_inv, uint64_t* h_bad);
/* d_out[(d_index[j] - base) * cols ...] = d_values[j * cols ...]: rows to their places (keys back to file order, uq.py:786's inverse) in one
 * random pass; *h_bad = UQ_NONE or the lowest j whose target lies outside [0, out_rows). */
int uq_scatter_rows(uq_ctx* ctx, const uint8_t* d_values, uint64_t n, uint32_t cols, const void* d_index, int index_itemsize, int64_t base,
                    uint64_t out_rows, uint8_t* d_out, uint64_t* h_bad);

/* ---- f1 INSIDE a3 / a4: the QNAME passes in the pack kernel's read of the stream (uq.py:394-444 layout inference, 555-565 field
 * split, 717-736 int() of the fields).  The pack kernel already holds every record's QNAME line in LDS; with a uq_qname_fused it
 * also splits each line at the separators, parses the fields and writes them as uint32 columns -- against a layout GUESSED on
 * the device from a sample of the file's own reads, and VERIFIED for every read in the same pass:
 *   uq_qname_guess[_async]  line 1 of the file and the layout reductions of uq_qname_layout (min lcp / lcs, entry / lastviol per
 *       character of line 1) over a stratified pseudo-random sample of ~4096 reads -> prefix / suffix lengths and the ordered separators, left in
 *       *d_q (ok = 1), or ok = 0 when the guess declines (no separator, regex metacharacters, > UQ_QF_MAXC columns, a first line
 *       beyond 255 bytes, a digit among the separators, a separator that occurs in line 1 outside the slice the reference reads the ORDER
 *       from -- uq.py:433-436 drops the last character before the suffix, its per-read rule (410-413) counts over the whole middle: such a
 *       character is in the reference's set but not in its order, and what happens then hangs on the LAST read alone -- ...): the pack
 *       kernel then leaves the QNAME lines alone and the caller runs uq_qname_layout / _tokenise.
 *   uq_pack_stats_qname[_async]  = uq_pack_stats[_async] + per read: the line starts with line1[:plen] and ends with
 *       line1[l1len - slen:], its middle holds exactly the separators in order, every field is the canonical decimal of a value
 *       below 10^9 (digits only, no sign, no leading zero), the line is no proper prefix / suffix of line 1; d_vals[c * pitch + r]
 *       = value of field c of read r.  Anything else raises d_q->flags (bit0 separators, bit1 line > 255 bytes, bit2 > 9 digits,
 *       bit3 line shorter than prefix + suffix, bit4 field not a canonical decimal, bit5 / bit6 prefix / suffix mismatch, bit7
 *       proper prefix / suffix of line 1 (or possibly so), bit8 a tile was not visited).  With flags == 0 and nreads == the number
 *       of reads the layout IS the reference's: the sample attains the minima (so min lcp / lcs over the file are plen / slen), no
 *       guessed separator is ever violated, and every other character of line 1 was seen violated at or after its entry in the
 *       sample (which bounds the file's entry from above and its last violation from below).
 *   uq_qname_fused_finish  queued behind it: per column the number of distinct values among reads [0, T] at the checkpoints
 *       T = 10000 * 2^k <= nreads - 1 and T = nreads - 1 (uq.py:586-602, 634-638; canonical decimals: distinct strings = distinct
 *       values).  Value ranges <= 4096: all checkpoints, from first occurrences per value.  Wider ranges (up to 2^20): checkpoint by
 *       checkpoint over the first three, counts[c][k] filled up to the first k with counts[c][k] > T_k / 10 (the reference demotes
 *       the column to `integers` there and later counts do not matter) or for all of them when the file has no more;
 *       undetermined[c] = 1: not decided here (range beyond 2^20, or no checkpoint among the first three fires): sort the column.
 *   uq_qname_fused_fetch  the structure on the host (synchronises).  uq_encode_u32: d_out[i] = (unsigned itemsize)(d_val[i] - sub).
 * Exact by construction; the caller falls back to uq_qname_layout / uq_qname_tokenise on any flag. */
#define UQ_QF_MAXC 8
#define UQ_QF_MAXT 24
typedef struct uq_qname_fused {
    uint32_t ok, plen, slen, nsep, l1len;
    uint32_t flags;                         /* raised by the pack kernel */
    uint32_t sample_step, nth;
    uint8_t line1[256];
    uint8_t seps[32];
    uint8_t inset[256];
    uint32_t vmin[UQ_QF_MAXC], vmax[UQ_QF_MAXC];
    uint32_t undetermined[UQ_QF_MAXC];
    uint64_t nreads;                        /* reads the pack kernel visited */
    uint64_t thresholds[UQ_QF_MAXT];
    uint64_t counts[UQ_QF_MAXC][UQ_QF_MAXT];
} uq_qname_fused;
int uq_qname_guess(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t nreads, uq_qname_fused* d_q);
/* The two queued forms below -- and uq_pack_stats_async -- accept d_line_start == NULL: no record index is expanded at all (uq_index_lines_async is left out of the
 * step: 8 B per line written and read again).  The line starts then come from the newline lists the census queued in front left in the
 * context (uq_count_lines_end_async for the same d_buf): the pack kernel finds each tile's place in them through one record per tile
 * (a binary search over the per-tile counts, done by a small kernel in front), the QNAME sample is stratified by position in the stream
 * instead of by read number.  Same tables, statistics and field values (tests/test_gpu_pack.py, tests/test_gpu_qname.py run both forms);
 * a census whose lists overflowed (uq_count_lines_wait's *h_ok = 0) makes both stand down as the indexed forms do. */
int uq_qname_guess_async(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uq_qname_fused* d_q);
int uq_pack_stats_qname(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads,
                        const uq_pack_params* h_guess, uint8_t* d_dna, uint8_t* d_qual, uint64_t* d_bad, uq_stats* d_stats,
                        uq_qname_fused* d_q, uint32_t* d_vals, uint64_t vals_pitch, int* h_fused);
int uq_pack_stats_qname_async(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t capacity_reads,
                              const uq_pack_params* h_guess, uint8_t* d_dna, uint8_t* d_qual, uint64_t* d_bad, uq_stats* d_stats,
                              uq_qname_fused* d_q, uint32_t* d_vals, uint64_t vals_pitch, int* h_fused);
int uq_qname_fused_finish(uq_ctx* ctx, uq_qname_fused* d_q, const uint32_t* d_vals, uint64_t vals_pitch);
int uq_qname_fused_fetch(uq_ctx* ctx, const uq_qname_fused* d_q, uq_qname_fused* h_out);
/* The fused pass over SHARDS (one rank per GPU, uq_amd.qname_device.analyse_fused_sharded): rank 0's guess is broadcast, every rank's
 * pack kernel verifies and parses its own reads, flags / vmin / vmax are combined over the ranks, and the distinct counts of the
 * small-range columns (h_range[c] <= 4096 values from h_vmin[c]; 0: skip the column) come from first-occurrence tables with FILE-WIDE
 * read numbers: d_first[c * 4096 + v - h_vmin[c]] = read_offset + the shard's lowest read holding v, INT64_MAX where v does not occur;
 * int64 so that a collective's MIN over the ranks is the file's table.  Nothing waits for the device. */
int uq_qname_fused_first_seen(uq_ctx* ctx, const uint32_t* d_vals, uint64_t vals_pitch, uint64_t nreads, uint64_t read_offset,
                              const uint32_t* h_vmin, const uint32_t* h_range, int ncols, int64_t* d_first);
int uq_encode_u32(uq_ctx* ctx, const uint32_t* d_val, uint64_t n, uint32_t sub, int itemsize, void* d_out);
int uq_encode_u32_columns(uq_ctx* ctx, const uint32_t* d_vals, uint64_t vals_pitch, uint64_t n, int ncols, const uint32_t* h_sub,
                          const int* h_itemsize, void* const* h_d_outs);       /* uq_encode_u32 of the first ncols columns of a fused pass, one launch */

/* ---- the host decisions between the passes, in the library (no device, no context: plain host C++).
 * uq_decide_from_stats = uq.py:448-545 (alphabets ASCII-sorted, the N-trick, the width ladder, bytes per row), the twin of
 * uq_amd.analysis.decide_from_pairs_py.  The statistics come as h_compact (its first n distinct non-zero counters; n <= UQ_STATS_COMPACT_CAP)
 * or, when h_compact is NULL, as the dense table h_dense[65536]; the read lengths are passed on their own.  h_first_seen: NULL or
 * 256 sort keys (lower = the base appeared earlier) that order two or more N-trick candidates; ncand says whether they were needed.
 * status 1: no base counted. */
typedef struct uq_decisions {
    uint32_t status, nbases, nquals, nall, nnq, ncand;
    uint8_t bases[256], qualities[256], all_bases[256];      /* bases: the DNA alphabet left after the N-trick; all_bases: before it */
    uint8_t nq_base[256]; int32_t nq_code[256];              /* N_qual, in the order the candidates were taken */
    int32_t total_quals, bits_per_base, bits_per_quality, variable, dna_max, dna_min, dna_bytes_per_row, quality_bytes_per_row;
    uint64_t base_tot[256], qual_tot[256];
} uq_decisions;
int uq_decide_from_stats(const uq_stats_compact* h_compact, const uint64_t* h_dense, uint32_t len_min, uint32_t len_max, int notricks, int pad,
                         const uint64_t* h_first_seen, uq_decisions* h_out);
/* uq_pack_params from the decisions (ops.make_pack_params): code tables from the alphabets (a byte given twice keeps its last index),
 * n_qual from the nnq (byte, code) pairs. */
int uq_make_pack_params(const uint8_t* bases, uint32_t nbases, const uint8_t* qualities, uint32_t nquals, const uint8_t* nq_base,
                        const int32_t* nq_code, uint32_t nnq, int32_t bits_per_base, int32_t bits_per_quality, int32_t variable,
                        int32_t dna_bytes_per_row, int32_t quality_bytes_per_row, int32_t dna_max, int32_t max_record_bytes,
                        int32_t avg_record_bytes, uq_pack_params* h_out);
/* *h_same = 1: a and b describe the same encoding (everything but the two tile-sizing hints). */
int uq_same_pack_params(const uq_pack_params* a, const uq_pack_params* b, int* h_same);
/* The column typing of uq.py:586-678 from a fetched uq_qname_fused (uq_amd.qname_device.fused_columns_py is the twin): for n reads,
 * status 0 = ncols columns typed (all `integers`), 1 = decline (no guess, a flag, another read count or other checkpoints than n's, a
 * column that stays a mapping of strings), 2 = a column needs the sort-based distinct counts.  Columns are judged in order; the first
 * that declines or needs the sort decides.  from_mapping[c] = 1: the column kept the format `mapping` through every checkpoint and
 * became `integers` by its value range (its dtype follows the distinct count, not the range). */
typedef struct uq_qname_columns {
    uint32_t status, ncols;
    uint32_t itemsize[UQ_QF_MAXC], offset[UQ_QF_MAXC], from_mapping[UQ_QF_MAXC];     /* itemsize 1, 2, 4, 8 = uint8 ... uint64 */
    uint32_t vmin[UQ_QF_MAXC], vmax[UQ_QF_MAXC];
} uq_qname_columns;
int uq_qname_fused_columns(const uq_qname_fused* h_q, uint64_t n, uq_qname_columns* h_out);

/* ---- f3: FASTQ text assembled on the device.  Replaces the decoder's exec-compiled convert_qname
 * (uq.py:1010-1026) and its four prints per read (uq.py:1042-1045).  Inputs: the fixed-pitch text and
 * lengths uq_unpack produced, and the QNAME columns (device arrays, one value per read, little-endian
 * unsigned of itemsize[c] bytes).  Integer columns print str(value + add[c]) (add = 'min' when the
 * column has an offset, any int64): exact wherever value + add[c] lies in [-2^63, 2^64), at every itemsize -- the
 * caller keeps other columns (an offset beyond int64, sums from 2^64 on) away from the device; mapping columns copy string number `value` of a flattened table
 * (h_d_map_chars[c], h_d_map_offs[c][nmap + 1]; both NULL for integer columns) and pass nmap in add[c] (0 = not
 * given): a value >= nmap then reads the last string, never beyond the table -- uq_check_index_range tells the caller.
 * Record = prefix + fields joined by separators[c] + suffix '\n' SEQ '\n' '+' '\n' QUAL '\n'.
 * d_offsets: uint64[nreads + 1] workspace (record offsets on return).  With d_out == NULL only the total
 * size is computed (*h_total). */
typedef struct uq_emit_params {
    uint8_t prefix[256];
    uint8_t suffix[256];
    uint8_t separators[32];
    int32_t prefix_len, suffix_len, ncols, dna_max;
    int32_t itemsize[32];
    int64_t add[32];
} uq_emit_params;
int uq_emit_fastq(uq_ctx* ctx, const uq_emit_params* h_params, const void* const* h_d_cols, const uint8_t* const* h_d_map_chars,
                  const uint32_t* const* h_d_map_offs, const uint8_t* d_seq, const uint8_t* d_qual, const uint32_t* d_len,
                  uint64_t nreads, uint64_t* d_offsets, uint8_t* d_out, uint64_t capacity, uint64_t* h_total);

/* ---- a12 + f3 in one pass: packed DNA / QUAL rows (+ QNAME columns) -> FASTQ text.  The decoder's split_bits,
 * character maps, N restore, sentinel strip (uq.py:1002-1007, 1031-1054), convert_qname (1010-1026) and prints
 * (1042-1045) without the 2 x dna_max bytes per read of intermediate text uq_unpack + uq_emit_fastq pass through HBM.
 * Same bytes as those two calls.  Protocol: call once with d_out == NULL -- read lengths (variable-length tables:
 * d_len, uint32[nreads]; may be NULL for fixed-length tables), record offsets (d_offsets, uint64[nreads + 1]) and
 * *h_total are computed, *h_bad = lowest row without a valid length sentinel (UINT64_MAX: none; also left in
 * d_bad[0]) -- then again with the output buffer and the SAME d_len / d_offsets / d_bad, which are only read. */
int uq_decode_fastq(uq_ctx* ctx, const uq_emit_params* h_emit, const uq_unpack_params* h_unpack, const void* const* h_d_cols,
                    const uint8_t* const* h_d_map_chars, const uint32_t* const* h_d_map_offs, const uint8_t* d_dna,
                    const uint8_t* d_qual, uint64_t nreads, uint32_t* d_len, uint64_t* d_offsets, uint64_t* d_bad,
                    uint8_t* d_out, uint64_t capacity, uint64_t* h_total, uint64_t* h_bad);

/* ---- synthetic FASTQ ("synth-v1"): workload generation for tests and bench.py.
 * Byte-identical to uq_amd/synth.py.  uq_synth_size: total bytes of reads [first, first+n).
 * uq_synth_fastq: writes them to d_out (capacity >= that size). */
typedef struct uq_synth_spec {
    uint64_t seed;
    int32_t len_lo, len_hi;
    int32_t n_rate;             /* percent of bases that are 'N' */
    int32_t n_qual_exclusive;   /* 1: N <-> '!' exclusively; 0: N always '#', shared */
    int32_t dup;                /* 0 none, 1 DNA, 2 QUAL, 3 both */
    int32_t dup_templates;
    int32_t skip_len_mod4;
    int32_t reserved;
} uq_synth_spec;
int uq_synth_size(uq_ctx* ctx, const uq_synth_spec* h_spec, uint64_t first, uint64_t n, uint64_t* h_bytes);
int uq_synth_fastq(uq_ctx* ctx, const uq_synth_spec* h_spec, uint64_t first, uint64_t n, uint8_t* d_out, uint64_t capacity);

/* ---- gzip input (an extension: the reference reads plain FASTQ only).  A BGZF file (what `bgzip` writes) is a chain of independent
 * gzip members, each with its compressed size in a `BC` extra subfield (BSIZE) and at most 64 KiB of output: they inflate in parallel
 * on the device.  Any other gzip is inflated on the device in parallel chunks (uq_gzip_stream_*, below).
 * uq_gzip_scan: walks the RFC 1952 member headers of h_buf[0, nbytes) (FEXTRA, FNAME, FCOMMENT, FHCRC).  *h_kind:
 *   UQ_GZIP_BGZF       every member carries BSIZE (the 28-byte EOF block and other empty members included): h_members[k] for all of them,
 *                      out_offset = the 64-bit prefix sum of ISIZE, *h_total_out = the inflated size;
 *   UQ_GZIP_OTHER      a member without BSIZE: the walk stops at it (its end is known only by inflating it); it is the last entry, with
 *                      comp_bytes = the rest of the input and isize = crc32 = 0;
 *   UQ_GZIP_MALFORMED  a truncated header or member, no magic, a method other than deflate, reserved flags, a bad header CRC, a BSIZE past
 *                      the end, ISIZE > 65536 in a BGZF member: *h_bad_offset = the member's offset, the message in uq_last_error().
 * h_members = NULL counts only (*h_nmembers); otherwise it holds `capacity` entries.  Returns 0 whatever the class. */
#define UQ_GZIP_BGZF 1
#define UQ_GZIP_OTHER 2
#define UQ_GZIP_MALFORMED 3
typedef struct uq_gzip_member {
    uint64_t data_offset;       /* first byte of the member's deflate data in the input */
    uint64_t comp_bytes;        /* deflate bytes (BSIZE + 1 - header - trailer) */
    uint64_t out_offset;        /* where its output starts in the inflated file */
    uint32_t isize;             /* trailer: output bytes */
    uint32_t crc32;             /* trailer: CRC-32 of the output */
} uq_gzip_member;
int uq_gzip_scan(const uint8_t* h_buf, uint64_t nbytes, uq_gzip_member* h_members, uint64_t capacity, uint64_t* h_nmembers,
                 uint64_t* h_total_out, int* h_kind, uint64_t* h_bad_offset);
/* uq_inflate_members: every member of d_members[0, nmembers) (a uq_gzip_scan table, in device memory) inflated from d_comp (the whole
 * compressed input, comp_bytes) into d_out[out_offset, out_offset + isize), one wave per member, its length and CRC-32 checked on the
 * device.  d_status[k] = 0, or the UQ_INF_* code (uq_amd/csrc/inflate_core.h) that stopped member k; a member that fails writes nothing
 * to d_out.  Reads stay inside [data_offset, data_offset + comp_bytes) and writes inside [out_offset, out_offset + isize), whatever the
 * bytes; a member that is not inside d_comp / d_out gets UQ_INF_TOO_LARGE.
 * uq_inflate_member_host: the same decoder on one member's deflate data on the CPU (h_out holds isize <= 65536 bytes): *h_status as above. */
int uq_inflate_members(uq_ctx* ctx, const uint8_t* d_comp, uint64_t comp_bytes, const uq_gzip_member* d_members, uint64_t nmembers,
                       uint8_t* d_out, uint64_t out_bytes, uint32_t* d_status);
int uq_inflate_member_host(const uint8_t* h_comp, uint64_t comp_bytes, uint8_t* h_out, uint64_t isize, uint32_t crc32, uint32_t* h_status);

/* ---- gzip that is not BGZF (one member, or members without BSIZE), inflated on the device in parallel chunks: the speculative scheme of
 * rapidgzip (uq_amd/csrc/inflate_stream.h).  Chunk starts are units packed as (canonical bit position << 2) | kind,
 * kind 0 a member header, 1 a non-final stored block (position = 8 x the byte offset of LEN), 2 a dynamic-Huffman block (its header's bit).
 * uq_gzip_stream_begin: d_comp[0, comp_bytes) (device; the whole gzip file) cut into chunks of chunk_bytes whose starts the finder looks
 *   for -- or, when h_starts is not NULL, the caller's nstarts starts (host memory; wrong ones cost time, never change the output; chunk 0
 *   always starts at byte 0) -- decoded on the device in rounds until the chain of chunk ends and starts is verified.  *h_out_bytes = the
 *   inflated size, *h_stream = a handle for uq_gzip_stream_finish.  A damaged file: *h_status = its UQ_INF_* / UQ_GZS_* code (non-zero),
 *   *h_bad_offset = the byte offset named in uq_last_error(), *h_stream = NULL.  Synchronises the context's stream.
 * uq_gzip_stream_finish: the output into d_out (device, >= *h_out_bytes): chunks placed, markers resolved, every member's ISIZE and CRC-32
 *   checked.  *h_status / *h_bad_offset as above.  uq_gzip_stream_free releases the handle (and its device workspace) whatever happened.
 * uq_gzip_stream_get_info: counts and times of the run (uq_gzip_stream_info).
 * uq_gzip_stream_host: the same finder, chunk decoder, chain check and resolution on the CPU, serially: h_out receives the output when
 *   capacity >= *h_out_bytes (otherwise only *h_out_bytes is set); h_info may be NULL. */
typedef struct uq_gzip_stream uq_gzip_stream;
typedef struct uq_gzip_stream_info {
    uint64_t chunks;            /* chunks after the chain check */
    uint64_t starts;            /* chunk starts decoded in the first round (chunk 0 included) */
    uint64_t rounds;            /* decode rounds */
    uint64_t redecoded;         /* chunk decodes after the first round (chain mismatches, slot overflows) */
    uint64_t overflows;         /* slot overflows of verified chunks */
    uint64_t resolve_rounds;    /* marker resolution rounds */
    uint64_t members;
    uint64_t out_bytes;
    double find_ms, decode_ms, finish_ms;
} uq_gzip_stream_info;
int uq_gzip_stream_begin(uq_ctx* ctx, const uint8_t* d_comp, uint64_t comp_bytes, uint64_t chunk_bytes, const uint64_t* h_starts,
                         uint64_t nstarts, uq_gzip_stream** h_stream, uint64_t* h_out_bytes, uint32_t* h_status, uint64_t* h_bad_offset);
int uq_gzip_stream_finish(uq_gzip_stream* stream, uint8_t* d_out, uint64_t out_bytes, uint32_t* h_status, uint64_t* h_bad_offset);
int uq_gzip_stream_get_info(const uq_gzip_stream* stream, uq_gzip_stream_info* h_info);
int uq_gzip_stream_free(uq_gzip_stream* stream);
int uq_gzip_stream_host(const uint8_t* h_comp, uint64_t comp_bytes, uint64_t chunk_bytes, const uint64_t* h_starts, uint64_t nstarts,
                        uint8_t* h_out, uint64_t capacity, uint64_t* h_out_bytes, uint32_t* h_status, uint64_t* h_bad_offset,
                        uq_gzip_stream_info* h_info);

/* ---- BGZF output (an extension: the reference writes plain FASTQ only).  The deflate compressor is uq_amd/csrc/deflate_core.h: one
 * dynamic-Huffman block per 65 280-byte input block (a stored block where that is smaller), so every member is at most 65 311 bytes; a
 * member's bytes depend on its input bytes only.
 * uq_bgzf_bound: *h_bound = the output capacity uq_bgzf_compress needs for nbytes of input (EOF member included). */
int uq_bgzf_bound(uint64_t nbytes, uint64_t* h_bound);
/* uq_bgzf_compress: d_in[0, nbytes) (device) as a BGZF stream into d_out (device, out_capacity bytes): one member per 65 280 bytes of input,
 * compressed one workgroup per block, in chunks of blocks (the workspace, from the context's scratch pool, is bounded by the chunk); the
 * members are placed at 64-bit offsets.  flags & UQ_BGZF_EOF: the 28-byte BGZF EOF member is appended.  *h_out_bytes = the bytes written.
 * flags & UQ_BGZF_LEVEL2: the compressor's level 2 (more match candidates per position and a lazy parse: smaller members, more time);
 * without it level 1, whose bytes are what they always were.  At either level a member's bytes depend on its input bytes and the level
 * only, and the bounds hold.  Any other flag bit is an error.
 * A block that fails, or a capacity that is too small, is an error naming the block.  Synchronises the context's stream. */
#define UQ_BGZF_EOF 1u
#define UQ_BGZF_LEVEL2 2u
int uq_bgzf_compress(uq_ctx* ctx, const uint8_t* d_in, uint64_t nbytes, uint8_t* d_out, uint64_t out_capacity, uint64_t* h_out_bytes,
                     uint32_t flags);
/* uq_bgzf_compress_parts: several buffers as one run of BGZF members (what the `--gz` container writer calls once for all tar members).
 * Part k is h_prefix[0, prefix_bytes) (host, at most 256 bytes: a .npy header) followed by d_data[0, nbytes) (device, any alignment); the
 * 65 280-byte block cuts restart at every part, so part k's members are exactly uq_bgzf_compress(prefix || data) without the EOF member
 * and h_part_bytes[k] (host) = S(prefix || data) of uq_deflate_size.  One block table for all parts is built on the host and uploaded
 * once; the chunks of blocks run across the parts.  The members of all parts follow each other in d_out; *h_out_bytes = their total (plus
 * the EOF member with UQ_BGZF_EOF).  A block that fails is an error naming the part and the block; a capacity that is too small is an
 * error and nothing is written past it.  Synchronises the context's stream.
 * uq_bgzf_parts_bound: *h_bound = the capacity uq_bgzf_compress_parts needs (EOF member included). */
typedef struct uq_bgzf_part {
    const uint8_t* h_prefix;    /* host */
    uint32_t prefix_bytes;      /* <= 256 */
    uint32_t reserved;
    const uint8_t* d_data;      /* device */
    uint64_t nbytes;
} uq_bgzf_part;
int uq_bgzf_compress_parts(uq_ctx* ctx, const uq_bgzf_part* h_parts, uint32_t nparts, uint8_t* d_out, uint64_t out_capacity,
                           uint64_t* h_part_bytes, uint64_t* h_out_bytes, uint32_t flags);
int uq_bgzf_parts_bound(const uq_bgzf_part* h_parts, uint32_t nparts, uint64_t* h_bound);
/* uq_bgzf_compress_block_host: the same compressor on the CPU, on one block (nbytes <= 65 280): h_out[0, capacity) receives the member,
 * *h_out_bytes = its size.  *h_status = 0, 1 (the member needs more than `capacity` bytes: nothing but zeros written) or 2 (nbytes too large). */
int uq_bgzf_compress_block_host(const uint8_t* h_in, uint64_t nbytes, uint8_t* h_out, uint64_t capacity, uint64_t* h_out_bytes,
                                uint32_t* h_status);
/* uq_bgzf_compress_block_host_l: the same with flags: 0 (level 1) or UQ_BGZF_LEVEL2; any other bit is an error. */
int uq_bgzf_compress_block_host_l(const uint8_t* h_in, uint64_t nbytes, uint8_t* h_out, uint64_t capacity, uint64_t* h_out_bytes,
                                  uint32_t* h_status, uint32_t flags);

/* ---- the size of a buffer as BGZF, without writing it (an extension: what `--test --device-compressor` sizes its candidates with).
 * For the byte string B = prefix || data, S(B) = the sum, over the consecutive 65 280-byte blocks of B, of the size of the member
 * uq_bgzf_compress_block_host writes for the block: the length of uq_bgzf_compress's output without the EOF member.  S of nothing is 0.
 * uq_deflate_size: h_prefix[0, prefix_bytes) (host, at most 256 bytes: a .npy header) followed by d_data[0, nbytes) (device).  One
 * workgroup per block runs the compressor's size-only path (deflate_core.h: uq_deflate_block_size); S is ADDED to *d_total (device, 8-byte
 * aligned), and *d_status (device) is raised to a block's status if one fails: the caller zeroes both.  One launch whatever nbytes is, over
 * a fixed workspace from the context's scratch pool; queued on the context's stream and not synchronised, nothing is read back: calls can
 * be queued back to back and their totals fetched together. */
int uq_deflate_size(uq_ctx* ctx, const uint8_t* h_prefix, uint32_t prefix_bytes, const uint8_t* d_data, uint64_t nbytes, uint64_t* d_total,
                    uint32_t* d_status);
/* uq_deflate_size_host: the same code on the CPU over host bytes: *h_total = S(h_prefix || h_data). */
int uq_deflate_size_host(const uint8_t* h_prefix, uint32_t prefix_bytes, const uint8_t* h_data, uint64_t nbytes, uint64_t* h_total);
/* uq_deflate_size_l, uq_deflate_size_host_l: the same with flags: 0 (level 1) or UQ_BGZF_LEVEL2 (S over the members level 2 writes); any
 * other bit is an error. */
int uq_deflate_size_l(uq_ctx* ctx, const uint8_t* h_prefix, uint32_t prefix_bytes, const uint8_t* d_data, uint64_t nbytes, uint64_t* d_total,
                      uint32_t* d_status, uint32_t flags);
int uq_deflate_size_host_l(const uint8_t* h_prefix, uint32_t prefix_bytes, const uint8_t* h_data, uint64_t nbytes, uint64_t* h_total,
                           uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* UQHIP_H */
