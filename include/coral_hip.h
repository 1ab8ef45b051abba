/*
 * coral_hip.h — C ABI of libcoral_hip.so: the MI355X (gfx950) data-parallel hot path of CoRAL's
 * breakpoint-graph construction.
 *
 * The reference (suhas-r/CoRAL @ 2024-10-24) is pure Python and has no FFI of its own; the calls below
 * replace, one for one, the per-record loops the reference runs through pysam.
 * Each entry point cites the reference lines it stands in for.  INTEGRATION.md shows the ctypes
 * binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - every pointer is a plain device (HBM) or host pointer as stated; no framework types;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); launches are asynchronous
 *     unless a function says it returns a value read back from the device;
 *   - return value 0 = success, negative = error (see coral_last_error());
 *   - the library allocates nothing on the device: the caller owns all buffers and workspaces (the one exception is the
 *     query arena of the coral_*_host calls, see there);
 *   - results are integers and order-free (atomics only ever add integers), so they are bit-exact and
 *     independent of wave scheduling; compacted lists are returned unordered together with a sort key
 *     (record ordinal, within-record index) that defines the reference's iteration order.
 *
 * Record layout in HBM (structure of arrays, BAM file order = (tid, pos) order):
 *   tid, pos, end      int32   reference id, 0-based start, htslib bam_endpos
 *   flagmq             int32   flag | mapq << 16 | has_seq << 24
 *   n_cigar            int32   number of real CIGAR ops
 *   cigar_off          int64   offset (in ops) of the record's first op; ALWAYS a multiple of 4
 *   cigar              uint32  BAM-packed ops (len << 4 | op); every record is padded with op 15 to a
 *                              multiple of 4 ops so a wave reads whole 16-byte quads
 */
#ifndef CORAL_HIP_H
#define CORAL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CORAL_OK 0
#define CORAL_ERR_ARG (-1)        /* bad argument (null pointer, unsorted / overlapping segments, ...) */
#define CORAL_ERR_HIP (-2)        /* a HIP runtime call failed */
#define CORAL_ERR_CAPACITY (-3)   /* an output list overflowed; *count holds the needed size */
#define CORAL_ERR_FORMAT (-4)     /* malformed BAM / BGZF input */
#define CORAL_ERR_ZERODIV (-5)    /* a division the reference performs has a zero divisor (ZeroDivisionError there) */

typedef struct coral_records {
    int64_t n_rec;
    const int32_t *tid;
    const int32_t *pos;
    const int32_t *end;
    const int32_t *flagmq;
    const int32_t *n_cigar;
    const int64_t *cigar_off;
    const uint32_t *cigar;
} coral_records_t;

const char *coral_version(void);
const char *coral_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * coral_cigar_scan — ONE fused pass over every CIGAR op in HBM.
 *
 * Replaces the per-record `get_blocks()` walk and block loop of find_smalldel_breakpoints
 * (/root/reference/src/infer_breakpoint_graph.py:750-762), and pre-computes what the later
 * coverage calls need per record so the CIGAR bytes are streamed once.  summary[i] is one 16-byte row:
 *   [0] mbases     Σ length of M/=/X ops        (what count_coverage adds for a fully covered record,
 *                                                 infer_breakpoint_graph.py:131, :1033)
 *   [1] qinfer     Σ length of M/I/S/H/=/X ops  (pysam infer_read_length(), :1031)
 *   [2] blk_first  start of the first aligned block, [3] blk_last end of the last one (-1: none)
 *                                                (blocks[0][0], blocks[-1][1] at :760)
 * and one row (record, op index of the next block, prev block end, next block start) is appended to
 * `gaps` for every pair of consecutive blocks further apart than `min_gap` in a record with
 * mapq >= min_mapq (:754, :757-758).  `counters` are TWO device words the caller zeroes beforehand: [0] counts the
 * gap rows (rows beyond gap_cap are dropped, the counter still counts them), [1] is the kernel's work cursor.
 * summary and gaps must be 16-byte aligned.
 * ------------------------------------------------------------------------------------------------ */
int coral_cigar_scan(const coral_records_t *rec, int32_t min_gap, int32_t min_mapq, int32_t *summary /* [n_rec][4] */,
                     int32_t *gaps /* [gap_cap][4] */, uint32_t *counters /* [2] */, uint32_t gap_cap, void *stream);
/* Name of the kernel behind coral_cigar_scan as rocprofv3 prints it (reported next to the roofline figures). */
const char *coral_scan_kernel_name(void);

/* ------------------------------------------------------------------------------------------------
 * coral_segment_coverage — per-segment record count and aligned-base count.
 *
 * Replaces, for S sorted, pairwise disjoint half-open segments (seg_tid, seg_start, seg_end):
 *   n_reads[j] = #records overlapping the segment with infer_read_length() > 0
 *                (/root/reference/src/infer_breakpoint_graph.py:1031-1032)
 *   n_bases[j] = Σ of the four pysam count_coverage arrays with quality_threshold=0,
 *                read_callback='nofilter' BEFORE the non-ACGT correction (:130-132, :1033-1034):
 *                aligned (M/=/X) bases of records with SEQ that fall inside the segment.
 * Records fully inside one segment use the `summary` rows of coral_cigar_scan; only records straddling a
 * segment boundary have their CIGAR walked again.  n_reads / n_bases are ADDED to (caller zeroes).
 * `strad` is a workspace of n_rec uint32 and `strad_count` a zeroed device counter.
 * ------------------------------------------------------------------------------------------------ */
int coral_segment_coverage(const coral_records_t *rec, const int32_t *summary /* [n_rec][4] */,
                           int32_t n_seg, const int32_t *seg_tid, const int32_t *seg_start,
                           const int32_t *seg_end, unsigned long long *n_reads,
                           unsigned long long *n_bases, uint32_t *strad, uint32_t *strad_count,
                           void *stream);

/* ------------------------------------------------------------------------------------------------
 * coral_point_cover — which records cover which query points.
 *
 * Replaces the four single-position region fetches per concordant edge
 * (/root/reference/src/infer_breakpoint_graph.py:1043-1046): for P points sorted by (tid, pos) appends
 * the packed pair (point index << 32 | record ordinal) for every record with pos <= p < end.
 * *pair_count is a zeroed device counter; pairs beyond pair_cap are dropped (still counted).
 * max_span: an upper bound of end - pos over the records (the longest reference span of an alignment), which confines the
 * search to the records starting within max_span in front of a point; <= 0 = unknown (the window starts at the contig's
 * first record).  Relies on the (tid, pos) order of the record layout.
 * ------------------------------------------------------------------------------------------------ */
int coral_point_cover(const coral_records_t *rec, int32_t n_pts, const int32_t *pt_tid,
                      const int32_t *pt_pos, int32_t max_span, unsigned long long *pairs, uint32_t *pair_count,
                      uint32_t pair_cap, void *stream);

/* ------------------------------------------------------------------------------------------------
 * coral_sa_table — the chimeric-alignment table of ALL reads from the tokenised SA rows (device in, device out).
 *
 * Replaces the SA-tag half of fetch() (/root/reference/src/infer_breakpoint_graph.py:139-174: first-seen
 * de-duplication of SA entries per read name, read_length = query_length of the first record with flag < 256,
 * reads without a primary dropped) and alignment_from_satags with the nine cigar2pos* shapes
 * (/root/reference/src/cigar_parsing.py:17-269), including the stable (qs, qe) sort.
 *   inputs  rec_tid / rec_flagmq / rec_qlen (pysam query_length) / rec_name : int32[n_rec];
 *           sa int32[n_sa][8] (layout of coral_bam_decode_*), sa_nm int32[n_sa], sa_rec int32[n_sa] owner record
 *   outputs out_rows int32[<= n_sa][8] = qs, qe, tid, rint[1], rint[2], strand, mapq, NM (rows of read i are
 *           out_off[i]..out_off[i+1], sorted by (qs, qe)); out_name / out_failed int32[<= n_sa] per read (failed = the
 *           read's value is the reference's ([], [], [])); reads are in the insertion order of the reference's dict;
 *           out_read_length int32[n_names] (-1 = no primary seen);  counts (HOST) = {n_reads, n_rows}
 * `workspace` is device scratch; when it is too small the call returns CORAL_ERR_CAPACITY with counts[0] = MiB needed.
 * Errors mirror the reference: CORAL_ERR_FORMAT = SA CIGAR outside the nine shapes (KeyError, cp:255),
 * CORAL_ERR_ZERODIV = zero-length query interval (ZeroDivisionError, cp:268); when several reads offend, the error is that
 * of the first of them in table order (the reference walks its dict and raises there).  Synchronises `stream`.
 * ------------------------------------------------------------------------------------------------ */
int coral_sa_table(int32_t n_rec, const int32_t *rec_tid, const int32_t *rec_flagmq, const int32_t *rec_qlen,
                   const int32_t *rec_name, int32_t n_names, int32_t n_sa, const int32_t *sa, const int32_t *sa_nm,
                   const int32_t *sa_rec, void *workspace, int64_t workspace_bytes, int32_t *out_rows, int32_t *out_off,
                   int32_t *out_name, int32_t *out_failed, int32_t *out_read_length, int32_t *counts, void *stream);
const char *coral_sa_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * coral_hash_rows — hash_alignment_to_seg (/root/reference/src/infer_breakpoint_graph.py:181-210) on coral_sa_table's device
 * rows: for both ends of every local alignment the index of the CN segment containing it (the reference's IntervalTree
 * point queries), and the inverted index (contig, segment) -> alignments in the reference's append order.
 *   inputs  rows int32[n_rows][8] (coral_sa_table layout); the CN segments as a device table sorted by (contig id, start),
 *           pairwise disjoint: seg_tid / seg_start / seg_end (exclusive) / seg_idx (the segment's index within its contig,
 *           file order) int32[n_seg]; tid_has_segs int32[n_tid] (0: contig absent from the CN file)
 *   outputs cni0 / cni1 int32[n_rows] (-1 no segment, -3 contig absent); e_key int64[2 * n_rows] = contig << 32 | segment
 *           ascending and e_row int32[2 * n_rows] = table row — the first *n_ent (HOST) entries are valid
 * `workspace`: device scratch; too small -> CORAL_ERR_CAPACITY with *n_ent = MiB needed.  Synchronises `stream`.
 * ------------------------------------------------------------------------------------------------ */
int coral_hash_rows(int32_t n_rows, const int32_t *rows, int32_t n_seg, const int32_t *seg_tid, const int32_t *seg_start,
                    const int32_t *seg_end, const int32_t *seg_idx, const int32_t *tid_has_segs, int32_t n_tid,
                    void *workspace, int64_t workspace_bytes, int32_t *cni0, int32_t *cni1, int64_t *e_key, int32_t *e_row,
                    int32_t *n_ent, void *stream);

/* ------------------------------------------------------------------------------------------------
 * coral_*_host — the three short device queries of a graph build as ONE call each: host arguments in, host results out.
 *
 * Unlike the entry points above, these own their device scratch: a per-device query arena of the library (one pinned host
 * block, one device block, behind a mutex) that grows when a call needs more and is reused otherwise, so a query in steady
 * state allocates nothing.  A call stages its arguments through the pinned block, queues everything on `stream`, copies the
 * result back and returns after its last wait; nothing it returns points into the arena.  Results that can be large are
 * written straight into the caller's buffers (page-locked ones keep the copies asynchronous).  Errors: coral_sa_last_error().
 * coral_query_arena_release frees the arenas of all devices (tests, unload); the next query allocates again.
 *
 * coral_segment_coverage_host: coral_segment_coverage for n_seg half-open segments segs int64[n_seg][3] = (contig id, start,
 *   end) in ANY order, overlapping or not: they are split into batches of sorted, pairwise disjoint segments (first fit in
 *   (contig, start) order), all batches are uploaded with one copy, launched one after the other and fetched with one copy
 *   and ONE wait.  n_reads / n_bases int64[n_seg] (host) are set, in the caller's order.
 * coral_hash_rows_host: coral_hash_rows with the segment table seg int32[4][n_seg] (contig, start, end, index; sorted by
 *   (contig, start), disjoint) and tid_has_segs int32[n_tid] on the HOST; cni0 / cni1 int64[n_rows] and the first *n_ent of
 *   e_key / e_row int64[2 * n_rows] are written to the caller's host buffers, already widened.  Two waits: the entry count,
 *   then exactly that many entries.
 * coral_point_cover_host: coral_point_cover for n_pts host points sorted by (contig, position), distinct, followed by a
 *   device sort of the pairs: rec_out int32[<= pair_cap] (host) = the record ordinals in (point, record) order, bounds
 *   int64[n_pts + 1] (host) = the first pair of every point (bounds[n_pts] = *n_pairs).  More pairs than pair_cap:
 *   CORAL_ERR_CAPACITY with *n_pairs = the count needed, nothing else written.  Two waits: the count, then the pairs.
 * ------------------------------------------------------------------------------------------------ */
int coral_segment_coverage_host(const coral_records_t *rec, const int32_t *summary /* device [n_rec][4] */, int32_t n_seg,
                                const int64_t *segs, int64_t *n_reads, int64_t *n_bases, void *stream);
int coral_hash_rows_host(int32_t n_rows, const int32_t *rows /* device */, int32_t n_seg, const int32_t *seg,
                         const int32_t *tid_has_segs, int32_t n_tid, int64_t *cni0, int64_t *cni1, int64_t *e_key,
                         int64_t *e_row, int32_t *n_ent, void *stream);
int coral_point_cover_host(const coral_records_t *rec, int32_t n_pts, const int32_t *pt_tid, const int32_t *pt_pos,
                           int32_t max_span, uint32_t pair_cap, int32_t *rec_out, int64_t *bounds, uint32_t *n_pairs,
                           void *stream);
int coral_query_arena_release(void);

/* ------------------------------------------------------------------------------------------------
 * coral_sa_table_async — coral_sa_table and coral_bp_pair_table as one chain on `stream` WITHOUT a host wait (coral_sa_table has
 * three): the call returns when the chain is queued.  The numbers of groups, reads and rows stay in device memory for the
 * kernels that need them; grids, sorts and scans are sized by n_sa, which bounds all of them.  Inputs and workspace rule as
 * coral_sa_table (too small: CORAL_ERR_CAPACITY at once, counts[0] = MiB needed, nothing queued); chr_rank int32[n_tid] (device)
 * and the four thresholds as coral_bp_pair_table.
 *   device outputs, capacities by n_sa: out_rows int32[n_sa][8], out_off int32[n_sa + 1] (entries behind the last read =
 *           the number of rows), out_read_length int32[n_names], pairs int32[2 * n_sa][8] (slots of the first n_rows rows
 *           written), and the table in the host's layout, ready for exact-size copies: cols int64[8][n_rows] (column
 *           stride = the number of rows found: the first 8 * n_rows words of a buffer of 8 * n_sa), off_w int64[n_sa + 1],
 *           name_w int64[n_sa], failed_b uint8[n_sa] (0 / 1)
 *   counts  PAGE-LOCKED host int32[4], written by a copy at the end of the chain (valid once `stream` has passed it):
 *           n_reads, n_rows, error code (0; 3 = SA CIGAR outside the nine shapes: CORAL_ERR_FORMAT of coral_sa_table, KeyError
 *           in the reference; 4 = zero-length query interval: CORAL_ERR_ZERODIV, ZeroDivisionError; with several offending
 *           reads in a table: the code of the first of them in table order, as coral_sa_table), n_groups.  With an error code the other outputs hold nothing to be used.
 * ------------------------------------------------------------------------------------------------ */
int coral_sa_table_async(int32_t n_rec, const int32_t *rec_tid, const int32_t *rec_flagmq, const int32_t *rec_qlen,
                         const int32_t *rec_name, int32_t n_names, int32_t n_sa, const int32_t *sa, const int32_t *sa_nm,
                         const int32_t *sa_rec, void *workspace, int64_t workspace_bytes, int32_t *out_rows, int32_t *out_off,
                         int32_t *out_read_length, const int32_t *chr_rank, int32_t n_tid, int32_t min_bp_match_cutoff,
                         int32_t min_mapq, int32_t gap_, int32_t gap_mapq, int32_t *pairs, int64_t *cols, int64_t *off_w,
                         int64_t *name_w, uint8_t *failed_b, int32_t *counts, void *stream);

/* ------------------------------------------------------------------------------------------------
 * coral_bp_pair_table — the breakpoint candidate of EVERY pair of local alignments of every chimeric read (K4).
 *
 * Replaces the arithmetic of alignment2bp (/root/reference/src/breakpoint_utilities.py:70-96, called per read inside the
 * interval search, infer_breakpoint_graph.py:432-434), of alignment2bp_l (bu:129-186, infer_breakpoint_graph.py:687-688)
 * and of interval2bp (bu:289-295): which pairs yield a candidate depends on the amplicon intervals of the moment, but the
 * candidate itself and every interval-independent test are pure functions of two table rows, so they are computed once.
 *   inputs  off int32[n_reads + 1], rows int32[n_rows][8] — exactly coral_sa_table's out_off / out_rows (device);
 *           chr_rank int32[n_tid]: rank of every BAM contig in chr1..22,X,Y,M (global_names.py:13-18), -1 = other contig
 *   output  pairs int32[2 * n_rows][8] (device, 16-byte aligned).  Slot 2 * g + 0 = pair (g, g + 1), slot 2 * g + 1 = pair
 *           (g - 1, g + 1) around row g ("skip one low-MAPQ alignment"); a slot whose pair leaves the read has bits = 0.
 *           Fields: c1, p1, c2, p2, query gap, bits, row a, row b with
 *           bits: 1 valid | 2 passes the MAPQ / query-gap tests | 4 o1 is '-' | 8 o2 is '-' | 16 ends swapped by interval2bp
 *                 | 32 strands differ | 64 |gr - grr| > max(gap_, |0.2 gr|) | 128 a contig outside chr1..22,X,Y,M (KeyError
 *                 in the reference) | mapq(a) << 8 | mapq(b) << 16
 * Asynchronous on `stream`.  No limit on the number of alignments per read.
 * ------------------------------------------------------------------------------------------------ */
int coral_bp_pair_table(int32_t n_reads, int32_t n_rows, const int32_t *off, const int32_t *rows, const int32_t *chr_rank,
                        int32_t n_tid, int32_t min_bp_match_cutoff, int32_t min_mapq, int32_t gap_, int32_t gap_mapq,
                        int32_t *pairs, void *stream);

/* ------------------------------------------------------------------------------------------------
 * coral_search_* — host side of the amplicon-interval search (no device work): one step of find_interval_i
 * (infer_breakpoint_graph.py:362-434) in one call, alignment2bp_l over all reads (ibg:676-690) in another.
 *
 * coral_search_create borrows HOST arrays (they must outlive the handle): the chimeric table (off int64[n_reads + 1];
 * per row: owning read, contig id, rint[1], rint[2], CN-segment index of both ends (-1 none, -3 contig without CN
 * segments)), per read hash(read name) and name id, the inverted index of hash_alignment_to_seg (e_key = contig << 32 |
 * segment, ascending; e_row = table row), the pair table (host copy of coral_bp_pair_table's output) and the CN segments
 * of every contig in file order (seg_off int64[n_tid + 1]; start, inclusive end).
 * coral_search_params (once, before the first step): min_cluster_cutoff / max_seq_len (ibg:385-419), the arguments of
 * coral_call_breakpoints (cluster distance, match cutoff, acceptance floor) and the number of look-ahead threads.
 * coral_search_step(tid, s, e, si, ei): reach sets (ibg:369-384, replayed as CPython sets: size and iteration order),
 * segments with fewer reads than the cutoff dropped, runs of neighbouring segments (ibg:392-419), for every run alignment2bp
 * of the united set's reads, in the set's iteration order, between the run and (tid, s, e), and coral_call_breakpoints on
 * every run's candidates (ibg:436-457; sub-cluster counter not advanced, Appendix A Q4).  A step is a pure function of its arguments: coral_search_prefetch asks for it to be computed
 * ahead on a worker thread, coral_search_step then waits for / takes over / computes it; results do not depend on timing.
 * coral_search_within: alignment2bp_l of every read in table order.  coral_search_between: alignment2bp
 * of the listed reads between two intervals.  coral_search_result then gives (valid until the next call on the handle)
 *   cand int64[n_cand][13] = c1, p1, o1, c2, p2, o2, read name id, i, j, query gap, swapped, mapq a, mapq b (the 11 fields
 *        of bu:81 / bu:294-295), the runs' candidates one after the other;
 *   meta int64[n_meta] = n_groups, then per run: contig id, first segment, last segment, n candidates, n clusters, n calls,
 *        the cluster sizes, and per call: head candidate, p1, p2, flags, begin and end of its support in `sup` (head and
 *        support indices are relative to the run's first candidate; flags as coral_call_breakpoints);
 *   stats double[6 per call], sup int64[n_sup];
 *   order_off int64[n_groups + 1] / order int32[] = the reads of every run in iteration order (table indices).
 * CORAL_ERR_FORMAT: a candidate touches a contig outside chr1..22,X,Y,M (KeyError at bu:293 in the reference).
 *
 * A handle can be made in two parts.  coral_search_create_early takes what exists before hash_alignment_to_seg (table rows,
 * name ids, pair table, number of contigs), lays out the per-read pack and starts filling it without waiting (a big table on
 * threads of the handle's own).  coral_search_attach then brings the CN-segment indices, read hashes, inverted index and CN
 * segments, waits for the fill, writes the indices into the pack and reports in first_row_of_tid int64[n_tid] (may be null)
 * the first table row with cni0 != -3 per contig (-1: none).  coral_search_create is the two in a row.  Until it is attached
 * a handle answers step / prefetch / within / between / bfs with CORAL_ERR_ARG; coral_search_free is always allowed.
 *
 * The look-ahead threads and the helper threads of big steps belong to the PROCESS: the first coral_search_params with
 * n_threads > 0 starts them, later handles share them (asking for more makes the set grow; results never depend on the
 * count), coral_search_free joins nothing — it drops the handle's queued steps and waits for those being computed.
 * coral_search_shutdown joins the threads (idempotent; a later prefetch starts them again; after fork() the child starts
 * its own).  coral_search_stats: out int64[>= 7] = attached, pack fill complete when attach began, steps queued in all, steps
 * already queued when the last coral_search_bfs began (-1: none), steps computed by the caller, look-ahead / helper threads alive.
 * "Steps queued" counts each distinct key the CALLER asked for, once.  While coral_search_bfs runs, a look-ahead thread that
 * finishes a step also queues, as speculative entries behind every real one, the steps of the intervals the search will
 * probably derive from it (CORAL_SEARCH_SPECULATE=0: never; at most CORAL_SEARCH_SPECULATE_MAX per search); results never
 * depend on it.  With n_out >= 12 also: out[7] speculative entries queued, out[8] keys the caller asked for that a guess had
 * queued first, out[9] of those the ones computed already when their step was asked for, out[10] speculative entries never
 * asked for, out[11] steps computed so far by any thread.
 * ------------------------------------------------------------------------------------------------ */
void *coral_search_create_early(int64_t n_reads, int64_t n_rows, const int64_t *off, const int64_t *row_read,
                                const int64_t *row_tid, const int64_t *ra, const int64_t *rb, const int64_t *read_name,
                                const int32_t *pairs, int32_t n_tid);
int coral_search_attach(void *handle, const int64_t *cni0, const int64_t *cni1, const int64_t *read_hash, int64_t n_ent,
                        const int64_t *e_key, const int64_t *e_row, const int64_t *seg_off, const int64_t *seg_start,
                        const int64_t *seg_end, int64_t *first_row_of_tid);
int coral_search_shutdown(void);
int coral_search_stats(void *handle, int64_t *out, int32_t n_out);
void *coral_search_create(int64_t n_reads, int64_t n_rows, const int64_t *off, const int64_t *row_read, const int64_t *row_tid,
                          const int64_t *ra, const int64_t *rb, const int64_t *cni0, const int64_t *cni1,
                          const int64_t *read_hash, const int64_t *read_name, int64_t n_ent, const int64_t *e_key,
                          const int64_t *e_row, const int32_t *pairs, int32_t n_tid, const int64_t *seg_off,
                          const int64_t *seg_start, const int64_t *seg_end);
int coral_search_free(void *handle);
const char *coral_search_error(void *handle);
int coral_search_params(void *handle, double min_cluster_cutoff, int64_t max_seq_len, int64_t bp_distance_cutoff,
                        int64_t match_cutoff, double accept_floor, int32_t n_threads);
int coral_search_prefetch(void *handle, int64_t tid, int64_t s, int64_t e, int64_t si, int64_t ei);
int coral_search_step(void *handle, int64_t tid, int64_t s, int64_t e, int64_t si, int64_t ei);
int coral_search_within(void *handle, int32_t n_int, const int64_t *int_tid, const int64_t *int_start, const int64_t *int_end);
int coral_search_between(void *handle, int64_t n_sel, const int32_t *reads, int64_t t1, int64_t s1, int64_t e1, int64_t t2,
                         int64_t s2, int64_t e2);
int coral_search_result(void *handle, int64_t *n_meta, const int64_t **meta, int64_t *n_cand, const int64_t **cand,
                        int64_t *n_sup, const int64_t **sup, const double **stats, const int64_t **order_off,
                        const int32_t **order);
/* coral_search_bfs — the WHOLE interval search of a build in one call: the loop over the seed intervals and the breadth-first
 * search of find_interval_i (/root/reference/src/infer_breakpoint_graph.py:343-673) incl. its order-dependent half: addbp
 * (ibg:326-340), the refinement of the reached segments into new intervals (ibg:459-612), interval_exclusive (bu:54-67) and
 * the connection bookkeeping (ibg:614-673); the pure steps run ahead on the handle's worker threads as with
 * coral_search_prefetch / _step.  iv int64[n_seed][4] = contig id, start, end, ccid (-1) of the seeds after the CN-segment snap;
 * seg_cn / seg_ix = CN value and the reference's per-chromosome index of every CN segment (layout of seg_start / seg_end);
 * chr_rank[contig] = rank in chr1..22,X,Y,M or -1; tid_has_rows[contig] = 1 if some alignment is hashed to the contig's
 * segments; log_level 0 none, 1 warnings, 2 + debug events.  Errors: CORAL_ERR_FORMAT / -10 / -11 = the reference's KeyError
 * cases, -12 = its IndexError (coral_search_error has the text).  coral_search_bfs_get(which) returns the result arrays:
 *   0 intervals int64[n][5] (contig, start, end, ccid, start-is-a-bool — Appendix A Q2)
 *   1 breakpoints int64[n][11] (c1 p1 o1 c2 p2 o2, read name id / i / j of the head candidate, query gap, swapped)
 *   2 int64[n][4] (flags of coral_call_breakpoints, ccid, first and end chunk)   3 statistics double[n][6]
 *   4 chunks int64[n][2] (begin, end into 5 / 6 / 7)   5 / 6 / 7 support triples (read name id, i, j) — chunk 0 of a breakpoint
 *     is the set it was created with, every later chunk arrived through `|=` (ibg:330)
 *   8 connection keys int64[n][2] in insertion order   9 offsets int64[n + 1] into 10   10 breakpoint indices in order of addition
 *   11 events int64[n][6] for the log (type, arguments). */
int coral_search_bfs(void *handle, int32_t n_seed, const int64_t *iv, const double *seg_cn, const int64_t *seg_ix,
                     const int32_t *chr_rank, const uint8_t *tid_has_rows, double cn_gain, int64_t interval_delta,
                     int32_t log_level);
int coral_search_bfs_get(void *handle, int32_t which, const void **ptr, int64_t *n);

/* ------------------------------------------------------------------------------------------------
 * The candidates behind the search — HOST functions (no device work, no HIP call on any thread).
 *
 * coral_smalldel_pass: find_smalldel_breakpoints up to its breakpoint calls
 * (infer_breakpoint_graph.py:721-802 of the reference) in one pass.  gaps int64[n_gap][6] = record ordinal, op index,
 * previous block end, next block start, first block start, last block end of the record, sorted by (record, op index) — the
 * gap rows of coral_cigar_scan; h_tid / h_pos / h_end / h_name_id / h_mapq int32[n_rec] the record columns; iv
 * int64[n_int][3] = contig id, start, end (inclusive) in list order, NOT assumed sorted or disjoint.
 *   Selection (ibg:750-766): interval by interval in list order, rows in their own order inside an interval; a record
 *   overlaps when pos < e + 1 and end > s; a record inside two intervals is taken twice (Appendix A Q11).
 *   Grouping (ibg:746-762): by read-name id in order of first appearance among the selected rows, stable inside a group;
 *   k_in = the row's index in its group.
 *   Candidates (ibg:772): c1 = c2 = contig, p1 = next block start, p2 = min(previous block end, next block start) (the
 *   aliasing swap, Q7), o1 = 1, o2 = 0, read = name id, i = j = k_in, gap = swapped = 0, mapq a = mapq b = -1;
 *   then coral_call_breakpoints with advance_subcluster = 1 and the given cutoffs and floor (ibg:777-802).
 * Synchronous, needs no handle and starts no thread.  The result is read with coral_tail_result_get (which = 0 candidates
 * int64[n][13]; 1 cluster sizes int32; 2 / 3 / 4 head, p1, p2 per call; 5 statistics double[calls][6]; 6 flags int32; 7 / 8
 * support offsets and indices — 1..8 as coral_call_breakpoints; 9 name id per group; 10 group bounds int64[G + 1]; 11 rows
 * int64[n][6] = contig, next block start, previous block end, first block start, last block end, mapq in the candidates'
 * order — what large_indel_alignments holds), coral_tail_result_rc / _error, and freed with coral_tail_result_free.
 *
 * coral_search_tail_prefetch(handle, intervals, gap rows + record columns): returns at once; queues on the process's
 * look-ahead threads (a) the pass above with the handle's parameters and (b) coral_search_within of the same intervals
 * followed by coral_call_breakpoints with advance_subcluster = 1 (find_breakpoints, ibg:676-718).  The interval list is
 * copied and is the jobs' key; the other arrays are borrowed until the jobs were collected or the handle freed.
 * coral_search_tail_collect(which = 0 small deletions, 1 within): with arguments equal to the key of a queued job (and, for
 * 0, the same arrays) it waits for that job, or computes it itself if no thread has begun it; with any other arguments, or
 * with no job, it computes here and now — results never depend on the prefetch.  *result belongs to the handle until the
 * next collect of the same kind.  A handle without threads queues nothing and computes on demand.  coral_search_free drops
 * queued tail jobs and waits for those in flight, as for steps.  coral_search_tail_stats: out int64[4] = jobs queued,
 * collects served by a queued job, collects computed on demand, served ones the caller computed itself.
 * ------------------------------------------------------------------------------------------------ */
void *coral_smalldel_pass(int64_t n_gap, const int64_t *gaps, int64_t n_rec, const int32_t *h_tid, const int32_t *h_pos,
                          const int32_t *h_end, const int32_t *h_name_id, const int32_t *h_mapq, int32_t n_int, const int64_t *iv,
                          double min_cluster_cutoff, int64_t bp_distance_cutoff, int64_t match_cutoff, double accept_floor);
void coral_tail_result_free(void *result);
int coral_tail_result_rc(const void *result);
const char *coral_tail_result_error(const void *result);
int coral_tail_result_get(const void *result, int32_t which, const void **ptr, int64_t *n);
int coral_search_tail_prefetch(void *handle, int32_t n_int, const int64_t *iv, int64_t n_gap, const int64_t *gaps, int64_t n_rec,
                               const int32_t *h_tid, const int32_t *h_pos, const int32_t *h_end, const int32_t *h_name_id,
                               const int32_t *h_mapq);
int coral_search_tail_collect(void *handle, int32_t which, int32_t n_int, const int64_t *iv, int64_t n_gap, const int64_t *gaps,
                              int64_t n_rec, const int32_t *h_tid, const int32_t *h_pos, const int32_t *h_end,
                              const int32_t *h_name_id, const int32_t *h_mapq, const void **result);
int coral_search_tail_stats(void *handle, int64_t *out);

/* ------------------------------------------------------------------------------------------------
 * coral_read_counter — copy a device counter to the host (synchronises `stream`).
 * ------------------------------------------------------------------------------------------------ */
int coral_read_counter(const uint32_t *dev_counter, uint32_t *host_value, void *stream);

/* ------------------------------------------------------------------------------------------------
 * coral_cluster_first_fit — HOST function (no device work).
 *
 * Greedy first-fit clustering of one (chr1, chr2, o1, o2) group of breakpoint candidates, exactly as
 * /root/reference/src/breakpoint_utilities.py:268-282: candidate i joins the FIRST existing cluster that
 * has any member with |p1 - p1'| < cutoff and |p2 - p2'| < cutoff, else opens a new cluster.
 * cluster_of[i] receives the cluster ordinal (creation order), *n_clusters the number of clusters.
 * ------------------------------------------------------------------------------------------------ */
int coral_cluster_first_fit(int64_t n, const int64_t *p1, const int64_t *p2, int64_t cutoff,
                            int32_t *cluster_of, int32_t *n_clusters);

/* ------------------------------------------------------------------------------------------------
 * coral_first_seen_rows — HOST function.  is_first[i] = 1 iff row i of the row-major int64 matrix rows[n][ncols]
 * differs from every earlier row.  With the read-name id in column 0 and the tokenised SA entry in the others this
 * is the "if sa not in chimeric_alignments[rn]: append" de-duplication of
 * /root/reference/src/infer_breakpoint_graph.py:146-151, for all reads at once, exact (no hash-only equality).
 * ------------------------------------------------------------------------------------------------ */
int coral_first_seen_rows(int64_t n, int32_t ncols, const int64_t *rows, uint8_t *is_first);

/* ------------------------------------------------------------------------------------------------
 * coral_names_unify — HOST function: the read-name tables of `n_pieces` consecutive byte ranges of ONE BAM file (one per
 * rank, each decoded on its own GPU; piece p has n_names[p] names as blob[p] + off[p][n_names[p] + 1], numbered in order of
 * first appearance WITHIN the piece) -> the numbering a single decode of the whole file gives: name id = order of first
 * appearance over the file = insertion order of the reference's dicts keyed by query_name
 * (/root/reference/src/infer_breakpoint_graph.py:141-151).  lut[p][local id] receives the global id; out_blob (capacity:
 * the pieces' blob bytes together) / out_off (capacity: Σ n_names + 1) the global table; *n_global its size.
 * Exact: names are compared as bytes, a 64-bit hash only routes them; n_threads workers join hash partitions in parallel.
 * ------------------------------------------------------------------------------------------------ */
int coral_names_unify(int32_t n_pieces, const int64_t *n_names, const uint8_t *const *blob, const int64_t *const *off,
                      int32_t *const *lut, uint8_t *out_blob, int64_t *out_off, int64_t *n_global, int32_t n_threads);

/* ------------------------------------------------------------------------------------------------
 * coral_pyset_* — HOST functions: the iteration order of the Python sets of read names the reference builds and iterates
 * in its interval search (/root/reference/src/infer_breakpoint_graph.py:379-384 .add() per reached CN segment,
 * :405-419 `|=` unions, :428/432 iteration), obtained by replaying CPython 3.10's set algorithm on (item id, str hash)
 * pairs instead of creating the sets.  `create` builds one set per key from entries in insertion order and reports the
 * distinct counts; `union_order` returns list(set() | sets[keys[0]] | sets[keys[1]] | ...) as item ids in iteration
 * order (out_items needs room for the sum of the counts).
 * ------------------------------------------------------------------------------------------------ */
void *coral_pyset_batch_create(int64_t n_entries, const int32_t *key_of_entry, const int32_t *item,
                               const int64_t *item_hash, int32_t n_keys, int32_t *out_count);
int coral_pyset_union_order(void *handle, int32_t n_union, const int32_t *keys, int32_t *out_items, int32_t *out_n);
int coral_pyset_batch_free(void *handle);

/* Candidates -> clusters -> exact breakpoints in one call: cluster_bp_list (bu:252-286), then for every cluster the
 * sub-cluster loop of ibg:436-457 / :693-718 / :777-802 around bpc2bp (bu:299-388) and bp_match (bu:391-416).
 * field_ptr[13] / field_stride[13] (stride in elements): the candidate columns c1, p1, o1, c2, p2, o2, read, i, j, gap,
 * swapped, mapq_a, mapq_b as int64 (chromosomes as BAM tids < 64, orientation 0 '+' / 1 '-').
 * min_cluster_cutoff: minimum cluster size and first-sub-cluster support; accept_floor: support needed by later sub-clusters
 * (max(normal_cov * min_bp_cov_factor, 3)); advance_subcluster = 0 reproduces the BFS call site, which never increments its
 * sub-cluster counter (Appendix A Q4).
 * Outputs (caller allocates n entries each, call_sup_off n + 1, call_stats 6 n): cluster_size[*n_clusters] for the log;
 * for each accepted breakpoint k < *n_calls: call_head (candidate whose fields name the breakpoint), call_p1/p2 (positions),
 * call_stats[6k..] (mean p1, mean p2, sd p1, sd p2, mean mapq 1, mean mapq 2), call_flags bit0/bit1 = the sd was the
 * reference's "ValueError -> integer 0" case, and sup_idx[call_sup_off[k] .. call_sup_off[k+1]) = supporting candidates. */
int coral_call_breakpoints(int64_t n, const int64_t *const *field_ptr, const int64_t *field_stride, double min_cluster_cutoff,
                           int64_t bp_distance_cutoff, int64_t match_cutoff, double accept_floor, int32_t advance_subcluster,
                           int32_t *n_clusters, int32_t *cluster_size, int32_t *n_calls, int64_t *call_head, int64_t *call_p1,
                           int64_t *call_p2, double *call_stats, int32_t *call_flags, int64_t *call_sup_off, int64_t *sup_idx);

/* NM statistics of the mapped, non-chimeric (no SA tag) MAPQ-60 records, ibg:153-157: their count and the sums of
 * e = NM / query_length and of e * e, added in record order with one rounding per addition (the reference's sequential
 * `+=`).  Host arrays: tid / mapq / nm / qlen int32[n], sa_off int64[n + 1] (SA rows per record).
 * CORAL_ERR_ZERODIV when a counted record has query_length 0 (no SEQ): the reference raises ZeroDivisionError at ibg:154. */
int coral_nm_stats(int64_t n, const int32_t *tid, const int64_t *sa_off, const int32_t *mapq, const int32_t *nm,
                   const int32_t *qlen, int64_t *count, double *sum_e, double *sum_e2);

/* Long-read support of the concordant edges (ibg:1043-1055): for edge q, pt_rec[pt_begin[4q + d] .. pt_end[4q + d]) are the
 * record ordinals covering its position d (p, p + 1, p - 101, p + 101: coral_point_cover; the four ranges may be any slices of
 * the one int32 array pt_rec[n_pt_rec], equal points share theirs), rec_name int32[n_rec] maps records to read-name ids,
 * sup_name[sup_off[q] .. sup_off[q + 1]) are the name ids supporting a discordant edge at either node of the edge;
 * count[q] = number of distinct names covering all four positions and not among those.  Host arrays. */
int coral_concordant_counts(int32_t n_edges, const int64_t *pt_begin, const int64_t *pt_end, const int32_t *pt_rec, int64_t n_pt_rec,
                            const int32_t *rec_name, int64_t n_rec, int64_t n_names, const int64_t *sup_off, const int64_t *sup_name,
                            int64_t *count);

/* coral_independent_rows — HOST function: keep[i] = 1 for a maximal linearly independent subset of the rows of A (double[m][n],
 * taken in order; a row is kept when it is not in the span of the rows kept before it — Gram-Schmidt, re-orthogonalised once,
 * residual > tol * max(1, |row|)).  The redundant balance rows of the CN program (bg:526-541) are dropped with it before
 * coral_cn_solve.  Returns the number of rows kept, negative = bad arguments. */
int coral_independent_rows(int32_t m, int32_t n, const double *A, uint8_t *keep, double tol);

/* coral_cn_solve — HOST function: the CN assignment of one amplicon graph,  argmin Σ w_inv/x + w_lin·x − w_log·log x  s.t.
 * A x = 0, x > 0,  started at x = 1 — the program compute_cn_lr gives to cvxopt.solvers.cp (the reference's
 * src/breakpoint_graph.py:495-606; one variable per edge, one balance row per interior node).  Not convex in general (w_log = -0.5
 * on sequence and source edges); convex on the box x_j < 2 w_inv_j / |w_log_j| for those edges, and that the answer is a minimum
 * is certified by tests/test_cn_solver.py against a 50-digit solve.  A double[p][n] row-major with linearly
 * independent rows.  Infeasible-start Newton with a backtracking search on the KKT residual, until the relative step is below
 * 1e-13.  Returns 0 (x[n] and nu[p] filled, *n_iter = iterations), 1 = the reduced Newton system was singular (the caller takes
 * its general path), negative = bad arguments.  CN parity against cvxopt itself is unpinned. */
int coral_cn_solve(int32_t n, int32_t p, const double *w_inv, const double *w_lin, const double *w_log, const double *A,
                   int32_t max_iter, double *x, double *nu /* [p]: the multipliers of the balance rows */, int32_t *n_iter);

/* Reachable CN segments of one amplicon interval — the traversal of ibg:369-384 with the read-name sets replayed natively.
 * visit_rows[n_visit]: rows of the chimeric table hashed to segments si..ei of chromosome `tid`, in the reference's visiting
 * order (segment ascending, then append order).  row_read/row_tid/cni0/cni1 are per table row, off[n_reads + 1] the row
 * ranges per read, read_hash[n_reads] = hash(read name).  Every read is expanded once (first visit); it is added to the set
 * of each (chromosome, segment) it touches outside (si, ei) on `tid` (boundary segments count as outside, Appendix A Q9).
 * Returns a handle usable with coral_pyset_union_order / coral_pyset_batch_free (NULL on bad arguments); keys are numbered
 * in order of first appearance = insertion order of the reference's nested dicts. */
void *coral_reach_create(int64_t n_visit, const int64_t *visit_rows, const int64_t *row_read, const int64_t *off,
                         const int64_t *row_tid, const int64_t *cni0, const int64_t *cni1, int64_t n_reads, int64_t tid,
                         int64_t si, int64_t ei, const int64_t *read_hash, int32_t *n_keys_out);
/* codes[k] = tid << 32 | segment index, counts[k] = distinct reads of key k. */
int coral_reach_keys(void *handle, int64_t *codes, int32_t *counts);

/* ------------------------------------------------------------------------------------------------
 * coral_bam_decode_* — HOST functions: BAM/BGZF file -> structure-of-arrays records, decoded ONCE.
 *
 * Replaces pysam.AlignmentFile(path, 'rb') + the whole-file fetch() loop
 * (/root/reference/src/infer_breakpoint_graph.py:65, :140-158).  `open` inflates (n_threads zlib workers) and
 * parses the whole file; `sizes` reports {n_rec, n_cigar_words (padded), n_sa_rows, n_nonacgt, n_names,
 * names_bytes, n_ref, ref_names_bytes}; `fill` copies everything into caller-allocated arrays (read names as ONE blob of
 * names_bytes bytes without terminators + name_off[n_names + 1], name id = order of first appearance in the file, i.e. the
 * insertion order of the reference's dicts keyed by query_name, ibg:148-151; reference names as consecutive NUL-terminated
 * strings); `close` frees the handle.
 * SA rows are 8 ints: ref id, 1-based pos, strand (0 '+', 1 '-'), leading S, M, +I/-D, trailing S, mapq
 * (leading S = -2 marks a CIGAR that contains S and M but is not one of the nine shapes of
 * cigar_parsing.py:219-229).  qlen is l_seq, or the CIGAR-implied query length when SEQ is '*'.
 * ------------------------------------------------------------------------------------------------ */
int coral_bam_decode_open(const char *path, int32_t n_threads, void **handle);
int coral_bam_decode_sizes(void *handle, int64_t sizes[8]);
int coral_bam_decode_fill(void *handle, int32_t *tid, int32_t *pos, int32_t *end, int32_t *flag, int32_t *mapq,
                          int32_t *qlen, int32_t *has_seq, int32_t *nm, int32_t *name_id, int32_t *n_cigar,
                          int64_t *cigar_off, uint32_t *cigar, int64_t *sa_off, int32_t *sa, int32_t *sa_nm,
                          int64_t *nonacgt_rec, int32_t *nonacgt_pos, char *names, int64_t *name_off,
                          char *ref_names, int32_t *ref_lens);
int coral_bam_decode_close(void *handle);
/* The same for the rank-th of `world` byte ranges of the file (one process per GPU decodes only its share): the range starts
 * at the first BGZF block at or after its first byte and at the first record that starts in that block's inflated bytes or
 * later, and ends with the record that straddles into the next range; read-name ids are local to the range. */
int coral_bam_decode_range(const char *path, int32_t n_threads, int32_t rank, int32_t world, void **handle);
/* stats = compressed bytes, uncompressed bytes, BGZF blocks of the decoded range; *seconds = wall time of the decode. */
int coral_bam_decode_stats(void *handle, int64_t stats[3], double *seconds);
/* SoA records -> coordinate-sorted BAM (tests and benchmarks only; the product reads BAM).  Arrays as coral_bam_decode_fill
 * delivers them (names / ref_names: one C string per name id / contig); SEQ is hash-made ACGT with N at the listed aligned
 * positions, QUAL absent, tags NM:i, SA:Z, and CG:B,I for CIGARs of more than 65535 operations. */
int coral_bam_write(const char *path, int64_t n_rec, const int32_t *tid, const int32_t *pos, const int32_t *flag,
                    const int32_t *mapq, const int32_t *qlen, const int32_t *has_seq, const int32_t *nm, const int32_t *name_id,
                    const int32_t *n_cigar, const int64_t *cigar_off, const uint32_t *cigar, const int64_t *sa_off,
                    const int32_t *sa, const int32_t *sa_nm, int64_t n_nonacgt, const int64_t *nonacgt_rec,
                    const int32_t *nonacgt_pos, const char *const *names, int32_t n_ref, const char *const *ref_names,
                    const int32_t *ref_lens, uint32_t seed, int32_t level, int32_t n_threads);
const char *coral_bam_last_error(void);
/* What a decode is asked for besides (or instead of) the records of a byte range.  Host pointers only; the arrays are read
 * during the open call and not kept.  Every rule is checked by both pipelines alike (CORAL_ERR_ARG, coral_bam_last_error says
 * why): world >= 1 and 0 <= rank < world; spans sorted, disjoint, non-empty and inside the file; segments sorted by (tid,
 * start), disjoint, 0 <= start <= end; quality_threshold 0..255; read_callback 0 or 1; no want_index / want_qc on a span
 * decode; per_base only with segments (n_seg >= 0) of at most 2^28 positions in all; depth_bin >= 0, and with depth_bin > 0:
 * depth_min_mapq 0..255, depth_exclude_flags 0..0xffff, depth_count_deletions 0 or 1, no span decode, at most 2^28 bins over
 * the header's contigs (checked once the header is read: refused before anything is decoded or allocated); keep_min_mapq
 * 0..255, keep_min_seq_length 0..2^29, keep_require_flags and keep_exclude_flags 0..0xffff, and no active record filter together
 * with want_index; want_reads 0, 1 or 2, and with want_reads = 1 or 2: reads_exclude_flags 0..0xffff, reads_seg under the rules of
 * the coverage segments, reads_names of 1..254 bytes each, strictly ascending, and no want_index; reads_order 0 or 1, and 1 only
 * with want_reads = 2.  A span decode is not sharded: rank and world are taken as 0 and 1. */
typedef struct {
    int32_t rank, world;                       /* byte range (ignored when n_spans >= 0) */
    int32_t n_spans;                           /* -1: the byte range; >= 0: only records starting inside these spans */
    const uint64_t *span_beg, *span_end;       /* virtual offsets, sorted, disjoint, non-empty */
    int32_t n_seg;                             /* -1: no coverage request; >= 0: sorted, disjoint segments */
    const int32_t *seg_tid, *seg_start, *seg_end;
    int32_t quality_threshold, read_callback;
    int32_t want_index, want_qc;
    int32_t per_base;                          /* 0: counts per segment; else: the table per position and base (pileup) */
    int32_t depth_bin;                         /* 0: no binned-depth request; >= 1: the bin size */
    int32_t depth_min_mapq, depth_exclude_flags, depth_count_deletions;
    /* the reads request: want_reads 0 = none */
    int32_t want_reads;                        /* 1: the selected records as FASTQ text, 2: as their own bytes (coral_bam_reads_sizes / _fill) */
    int32_t reads_order;                       /* 0: file order; 1: the written records of a want_reads = 2 request ascending by
                                                *    key = (uint64)(uint32)tid << 32 | (uint64)(uint32)(pos + 1) << 1 | (flag >> 4 & 1)
                                                *    - tid = -1 is 0xffffffff: records without coordinates last; at an equal position
                                                *    forward strand first -, records with equal keys in their input order (stable) */
    int32_t reads_exclude_flags;               /* 0..0xffff  written only when (flag & it) == 0 */
    int32_t reads_n_seg;                       /* 0: no region limit; else sorted, disjoint segments, the coverage segments' rules */
    const int32_t *reads_seg_tid, *reads_seg_start, *reads_seg_end;
    int32_t reads_n_names;                     /* 0: no name limit; else names of 1..254 bytes, sorted ascending by their bytes */
    const uint8_t *reads_names;                /*    (memcmp, then length), no duplicates: one blob ...                        */
    const int64_t *reads_name_off;             /*    ... and reads_n_names + 1 offsets into it                                 */
    /* the record filter: all four 0 = none.  A record is kept when all four tests hold. */
    int32_t keep_min_mapq;                     /* 0..255    keep when mapq >= it               (samtools view -q) */
    int32_t keep_min_seq_length;               /* 0..2^29   keep when l_seq >= it              (awk 'length($10) > 1000': 1001) */
    int32_t keep_require_flags;                /* 0..0xffff keep when (flag & it) == it        (samtools view -f) */
    int32_t keep_exclude_flags;                /* 0..0xffff keep when (flag & it) == 0         (samtools view -F) */
} coral_bam_request_t;
/* coral_bam_decode_range with a request; the results that ride along are read from the handle (of this call, or of
 * coral_bamgpu_host) with coral_bam_coverage_result, coral_bam_pileup_result, coral_bam_index_sizes / _fill,
 * coral_bam_qc_sizes / _fill and coral_bam_depth_sizes / _fill.
 *
 * Spans (n_spans >= 0) - replaces htslib's hts_itr_query + bgzf_seek behind every lr_bamfh.count_coverage(chrom, w, w + window,
 * ...) of /root/reference/src/plot_amplicons.py:399-409: the records that START inside n_spans spans [span_beg, span_end) of
 * virtual offsets (the chunks of a region query).  Each span begins at a known record start (no search), ends in front of the
 * record at or behind its end, and only its blocks (plus what its last record straddles into) are inflated;
 * coral_bam_decode_stats counts the blocks inflated.
 *
 * Window coverage (n_seg >= 0) - replaces, for the coverage track of `plot`, the per-window
 * lr_bamfh.count_coverage(chrom, w, w + window, quality_threshold=..., read_callback='nofilter') calls
 * (/root/reference/src/plot_amplicons.py:399-400, :408-409; threshold from :935): pysam count_coverage summed over its four
 * arrays, for any base-quality threshold and both read callbacks.  The caller cuts its windows into n_seg sorted (by tid,
 * start), pairwise disjoint half-open segments (seg_tid, seg_start, seg_end) and sums the segments back into windows.  A
 * base counts when its record is on the segment's contig (read_callback 1 = 'all': none of the flags 0x704), has SEQ, it is
 * an aligned base of an M / = / X op (the real CIGAR: CG:B,I for the placeholder) inside the segment, its SEQ code is A, C,
 * G or T, and quality_threshold (0..255) is 0 or the record has QUAL (first byte not 0xff) with QUAL >= quality_threshold
 * there.  `coverage_result` copies the n_seg int64 counts of the handle.
 *
 * Pileup (per_base != 0, with segments) - replaces lr_bamfh.count_coverage(chrom, start, stop, ...) itself, the four per-position
 * arrays the reference sums at once (/root/reference/src/infer_breakpoint_graph.py:130-133,
 * /root/reference/src/plot_amplicons.py:399-409): the same rule split by position and base.  A counted base adds 1 to
 * counts[p][b], p = the position's place among the positions of all segments in segment order, b = 0..3 for the SEQ codes 1,
 * 2, 4, 8 (A, C, G, T).  The segments may hold at most 2^28 positions in all (4 x 2^28 counters stay int32-indexable, the
 * table is at most 4 GiB).  `pileup_result` copies the uint32 [n_pos][4] table; n_pos must be the sum of the segment lengths.
 * `coverage_result` stays valid and returns the sums of the table per segment: one result, not two rules.  Allowed on a span
 * decode, as coverage is; tables of byte ranges add up.
 *
 * BAI index (want_index; SAMv1 5.2) - replaces what the reference gets from htslib behind pysam: the "Sorted indexed" BAM it
 * opens was indexed by `samtools index` (hts_idx_push / hts_idx_finish).  Besides the records, what the byte range contributes
 * to the file's index.  index_sizes -> heads, linear-index windows, contigs, records; index_fill copies
 *            head_key / head_voff  one entry per maximal run of file-consecutive records with the same (tid, bin), in file
 *                      order: tid * 65536 + reg2bin(beg, end) (-1: a record without coordinates) and the virtual offset
 *                      (block file offset << 16 | offset in the inflated block) of the run's first record; a run's chunk
 *                      ends where the next head starts, the last one at scalars[1]
 *            lin       per contig (length >> 14) + 1 windows: smallest virtual offset of an overlapping record, ~0 = none
 *            n_mapped / n_unmapped  records per contig without / with flag 0x4 (pseudo-bin 37450)
 *            scalars   records without coordinates, virtual offset behind the range's last record (bgzf_tell's rule),
 *                      (tid, pos) of the first and of the last record as sortable words (order check across ranges)
 *          A record is indexed as [max(pos, 0), bam_endpos), one base without a reference length; a record that sorts in
 *          front of its predecessor fails the decode.  Partial results of consecutive byte ranges concatenate (a run that
 *          goes on across the boundary is one run, windows take the minimum) into the whole file's.
 *
 * Read QC (want_qc) - replaces the one pass over every read of the reference's scripts/report_nanopore_qc.py:35-48
 * (len(sequence) and np.mean(quality) per read of the FASTQ the file was aligned from) and feeds its summary,
 * scripts/report_nanopore_qc.py:70-74 (Q25 / Q50 / Q75 of both, quality_control_summary.tsv).  A READ is a record with
 * flag & 0x900 == 0 and l_seq > 0 (one per FASTQ record; mapped or not); a read whose first QUAL byte is 0xff has no quality.
 *   qc_sizes -> records, reads; qc_fill copies, per read in file order, length (l_seq), qual_sum (sum of its QUAL bytes,
 *          -1 without quality), mapq and flag; hist[256] = count of every QUAL byte value over the reads with quality;
 *          counters = records, reads, records with flag 0x100, with flag 0x800, reads with flag 0x4, primary records
 *          without SEQ, reads without quality, bases of all reads.  Integers only: mean quality of a read is
 *          qual_sum / length on the host.  Results of consecutive byte ranges concatenate / add up.
 *
 * Binned depth (depth_bin > 0) - replaces the one pass over the alignments behind the reference's scripts/call_cnvs.sh:12-17
 * (cnvkit.py batch --seq-method wgs; CNVkit's `coverage` sums depth into fixed-size bins along every contig), which yields the
 * --cn_seg file `seed` and `reconstruct` need; segmentation and normalisation stay the CN caller's.  Contig t of the header, of
 * length LN[t], has ceil(LN[t] / depth_bin) bins (a length of 0: none); bin_off is their exclusive prefix sum in tid order,
 * n_bins = bin_off[n_ref] <= 2^28.  A record takes part when 0 <= tid < n_ref, pos >= 0, its real CIGAR (CG:B,I for the
 * placeholder) has an op, flag & depth_exclude_flags == 0 and mapq >= depth_min_mapq; SEQ and QUAL are not looked at, and a
 * record with flag 0x4 that is not excluded has its CIGAR walked all the same.
 *   bases[bin_off[tid] + x / depth_bin] += 1 for every reference position x < LN[tid] covered by an M, = or X op, and by a D op
 *          when depth_count_deletions is 1; N, I, S, H, P and zero-length ops add nothing, positions at or behind LN[tid] are
 *          dropped; position arithmetic is 64-bit.
 *   reads[bin_off[tid] + pos / depth_bin] += 1 for every record that takes part and has pos < LN[tid].
 *   depth_sizes -> n_ref, n_bins; depth_fill copies bin_off (n_ref + 1 int64) and the two int64 tables (n_bins each).  Exact
 *          integers, independent of scheduling, batch size and rank count; tables of byte ranges add up.
 *
 * Record filter (any keep_* field non-zero) - replaces the single-threaded trip through SAM text between aligning and sorting
 * in the reference's scripts/align_nanopore_reads.sh:42-44 (samtools view -h | awk 'length($10) > 1000 || $1 ~ /^@/' |
 * samtools view -bSq 25: keep_min_mapq 25, keep_min_seq_length 1001).  A record is kept when mapq >= keep_min_mapq, l_seq >=
 * keep_min_seq_length, (flag & keep_require_flags) == keep_require_flags and (flag & keep_exclude_flags) == 0.  l_seq is the
 * fixed field: a record without SEQ has length 0, where awk sees `*` with length 1 - both fail any threshold of 2 or more.
 *   Every result of a filtered decode equals the result of the same request on a BAM file that holds only the kept records, in
 *   the same order: the records (read-name ids numbered by first appearance among the kept records), the non-ACGT list, window
 *   coverage, pileup, read QC including its `records` counter, and binned depth - for byte ranges (rank / world) and for span
 *   decodes.  Exception: coral_bam_decode_stats and coral_bamgpu_stats go on counting the bytes and blocks actually read.
 *   A dropped record is validated only as far as the boundary walk and its fixed fields go (block_size >= 32): its tags are
 *   not walked, so a malformed tag in a dropped record is not an error, in either pipeline.  depth_min_mapq and
 *   depth_exclude_flags stay and apply on top of the filter (a logical AND).  Not together with want_index: the virtual
 *   offsets of a file that does not exist mean nothing.
 *
 * Reads (want_reads = 1) - replaces the second pass over the file that the reference's workflow makes to get at the reads behind
 * an amplicon: `samtools view x.bam region... | samtools fastq`, or `samtools view -N names.txt` when the supporting alignment
 * is a hard-clipped supplementary and the whole read sits at its primary record elsewhere (its scripts start and end at FASTQ:
 * scripts/align_nanopore_reads.sh, scripts/report_nanopore_qc.py).  A record is WRITTEN when l_seq > 0, (flag &
 * reads_exclude_flags) == 0, with segments: tid >= 0 and [pos, bam_endpos) - [pos, pos + 1) with flag 0x4 - meets a non-empty
 * segment, with names: its read name (without the NUL) is in the list, found by an exact binary search.  Segments and names
 * intersect; neither means every read.  An active record filter acts first.  The text of a written record is exactly
 *   `@` name `\n` SEQ `\n+\n` QUAL `\n`          (2 l_seq + l_read_name + 5 bytes)
 * with SEQ characters "=ACMGRSVTWYHKDBN"[code], QUAL characters min(q, 93) + 33, l_seq times `"` (quality 1) for a record whose
 * first QUAL byte is 0xff; with flag 0x10 SEQ is reversed and complemented (the complement of a 4-bit code is its bit reversal)
 * and QUAL reversed, so the read has the orientation it was sequenced in.  Nothing is appended to the name; records come in
 * file order.  Allowed on byte ranges (the texts of consecutive ranges concatenate) and on span decodes, not with want_index.
 *   reads_sizes -> records written, text bytes; reads_fill copies the text and the n + 1 int64 offsets of the records in it.
 *   The whole result lives in host memory: meant for the reads of an amplicon; for every read of a 2 M-read file the GPU
 *   pipeline writes the same text to a file batch by batch: the CORAL_SINK_TEXT sink of coral_bamgpu_open_request.
 *
 * Records (want_reads = 2) - the same selection with the alignments kept: what `samtools view -b x.bam region... > amp.bam`
 * gets from a second pass, for a genome browser or any tool that reads BAM.  reads_exclude_flags, reads_seg_*, reads_names /
 * reads_name_off and the keep_* filter mean what they mean for want_reads = 1, with the same validation.  A record is WRITTEN
 * when (flag & reads_exclude_flags) == 0, with segments: tid >= 0 and [pos, bam_endpos) - [pos, pos + 1) with flag 0x4 - meets
 * a non-empty segment, with names: its name is listed.  Unlike FASTQ, l_seq > 0 is NOT required: a record without SEQ is still
 * a record.  An active record filter acts first.  The output is 4 + block_size bytes per written record - its block_size word
 * and the block_size bytes behind it, byte for byte the source's inflated stream (a CIGAR carried in a CG:B,I tag is copied as
 * it is) - one record after the other in file order.  Allowed on byte ranges (the outputs of consecutive ranges concatenate)
 * and on span decodes, not with want_index.
 *   reads_sizes -> records written, total bytes; reads_fill copies the bytes and the n + 1 int64 offsets of the records.
 *   The whole result lives in host memory: meant for the records of an amplicon.  coral_bgzf_write puts a header and such bytes
 *   into a BGZF / BAM file.  For a whole 2 M-read file the GPU pipeline streams the same records to disk in bounded host
 *   memory: the CORAL_SINK_BAM sink of coral_bamgpu_open_request (CORAL_SINK_RUNS: in coordinate order, for coral_bamgpu_merge_runs). */
int coral_bam_decode_request(const char *path, int32_t n_threads, const coral_bam_request_t *req, void **handle);
int coral_bam_coverage_result(void *handle, int32_t n_seg, int64_t *counts);
int coral_bam_pileup_result(void *handle, int64_t n_pos, uint32_t *counts);
int coral_bam_index_sizes(void *handle, int64_t sizes[4]);
int coral_bam_index_fill(void *handle, int64_t *head_key, uint64_t *head_voff, uint64_t *lin, int64_t *n_mapped,
                         int64_t *n_unmapped, uint64_t scalars[4]);
int coral_bam_qc_sizes(void *handle, int64_t sizes[2]);
int coral_bam_qc_fill(void *handle, int32_t *length, int64_t *qual_sum, int32_t *mapq, int32_t *flag, int64_t hist[256],
                      int64_t counters[8]);
int coral_bam_depth_sizes(void *handle, int64_t sizes[2]);
int coral_bam_depth_fill(void *handle, int64_t *bin_off, int64_t *bases, int64_t *reads);
int coral_bam_reads_sizes(void *handle, int64_t sizes[2]);
int coral_bam_reads_fill(void *handle, uint8_t *text, int64_t *rec_off);
/* n_parts byte strings (for a BAM file: the inflated header, then record bytes) -> one BGZF file at `path`.  Each part is deflated
 * into blocks of at most 0xff00 input bytes and starts a new block (the header ends a block, as htslib's does, so the first
 * record's virtual offset has a zero low half); an empty part makes no block; level 0..9; the blocks are shared out over
 * n_threads (< 1: one) and the bytes do not depend on it; the 28-byte EOF block goes last.  CORAL_ERR_ARG: level outside 0..9,
 * n_parts < 0, a missing array or part, a path that cannot be created; CORAL_ERR_FORMAT: the write failed. */
int coral_bgzf_write(const char *path, const uint8_t *const *parts, const int64_t *part_bytes, int32_t n_parts, int32_t level,
                     int32_t n_threads);
/* Records in coordinate order - what `samtools sort` does in a pass of its own (the reference's
 * scripts/align_nanopore_reads.sh:49), here inside the decode: reads_order = 1 of the request (its key and
 * tie rule stand at the field).  CORAL_ERR_ARG: reads_order outside 0..1, or 1 without want_reads = 2.  The result is read with
 * coral_bam_reads_sizes / _fill as in file order, in final order.  A byte range or span decode sorts what it selects; the sorted
 * results of consecutive ranges are joined by coral_bam_records_merge (rank order = run order).
 * coral_bam_records_merge: a stable k-way merge of n_runs sorted runs of raw records by the same key, read from the records'
 * bytes (tid at +4, pos at +8, flag at +18).  Record k of run r is data[r][off[r][k] .. off[r][k + 1]), n[r] records; on a tie
 * the earlier run wins, inside a run the order stays.  out_off gets sum(n) + 1 offsets (the first 0), out_data the bytes
 * (out_off[sum(n)] of them = the runs' bytes; the caller sizes it).  The order and the offsets are computed first, then the
 * bytes are copied by n_threads workers (< 1: one): they do not depend on n_threads.  CORAL_ERR_ARG: n_runs < 0, a missing
 * array, a negative count, offsets that decrease. */
int coral_bam_records_merge(int32_t n_runs, const uint8_t *const *data, const int64_t *const *off, const int64_t *n,
                            uint8_t *out_data, int64_t *out_off, int32_t n_threads);

/* ------------------------------------------------------------------------------------------------
 * coral_bamgpu_* — the same decode with the inflate and the record parsing ON THE GPU: the host reads the file and sends
 * COMPRESSED bytes over PCIe; BGZF blocks are inflated one per wave (k_bgzf_inflate), record boundaries found, CIGARs laid
 * out in the padded SoA form of coral_records_t directly in HBM, and only a few hundred bytes per record (fixed fields,
 * read name, SA text) come back for the host-side fields.  Same replacement as coral_bam_decode_*
 * (/root/reference/src/infer_breakpoint_graph.py:65, :140-158), same results (tests/test_bam_gpu.py), same byte-range
 * rule for rank / world.  Every inflated block's CRC-32 is checked against its BGZF trailer (k_bgzf_crc), as htslib does.
 * The library allocates no device memory: the caller provides one workspace.
 *
 *   open   parse the header, size the batches (`batch_bytes` inflated bytes per batch; 0 = default 2.52 GiB, at most 3.5 GiB, never more than
 *          the byte range needs) -> *workspace_bytes the caller must allocate on the current device (256-byte aligned)
 *   start  take the workspace, start reading / uploading / inflating
 *   next   parse the next batch up to its sizes: out[0] records, out[1] padded CIGAR words, out[2] 1 = a batch is pending
 *          (0 = the file is done), on `stream` (synchronises it)
 *   emit   write the pending batch's CIGAR words to `cigar_dst` (device, out[1] words) and, if not NULL, its batch-local
 *          op offsets to `cigar_off_dst` (device, out[0] + 1 int64); takes the batch's host-side fields in
 *   host   the host-side half of the result as a handle for coral_bam_decode_sizes / _fill / _stats (cigar: pass NULL,
 *          n_cigar_words is 0; cigar_off covers the whole decoded range); owned by the decoder, do not close it
 *   stats  stats = batches, segments whose speculative record start was replaced by the exact walk, records fetched
 *          whole for the non-ACGT list, batch capacity; seconds = total wall time, host-side field handling, file reads,
 *          set-up of pinned buffers and streams, time the caller waited for the file feeder, ... for the GPU
 *   open_request  open with a coral_bam_request_t and a coral_bam_sink_t: where the reads request's result goes (NULL, or kind
 *          CORAL_SINK_HOST with the other fields ignored: it stays in host memory; the other kinds below; an unknown kind is
 *          CORAL_ERR_ARG); *workspace_bytes is final (the requests' own arrays are part of it).
 *          Spans go through the same batches one after the other, each from its known first record to the record at or
 *          behind its end; only their blocks are read, uploaded and inflated, and statistics count every block read.
 *          Without a request no kernel is added and nothing more is allocated.  Per batch, with
 *            a coverage request  k_bam_cov_plan + k_bam_cov_count read the batch's inflated SEQ / QUAL before the slot is reused
 *                      (one wave per 16 384 query bases of a record, one 64-bit atomic per work item and segment); segments
 *                      and counters live in the workspace
 *            per_base  k_bam_cov_plan + k_bam_pileup instead (the same work items in one-wave workgroups; one no-return
 *                      32-bit atomic per counted base, no reduction: the 64 lanes of a stride are 64 different positions);
 *                      the segments' prefix offsets (int64 [n_seg + 1]) and the uint32 [n_pos][4] table live in the workspace
 *                      too, zeroed by `start`
 *            want_index  k_bam_index (one thread per record: virtual offset by binary search of the batch's block table - a
 *                      record carried in from the batch in front keeps the offset it STARTED at -, bin, run heads, 64-bit
 *                      atomicMin per overlapped window, per-contig counters, order check), one scan and k_bam_index_compact;
 *                      the host joins the runs that go on across batches
 *            want_qc     k_bam_qc_plan, one scan and k_bam_qc read the batch's QUAL before the slot is reused (one wave per
 *                      16 384 QUAL bytes of a read, aligned 16-byte loads, one 64-bit atomic per work item, the histogram in
 *                      LDS per workgroup)
 *            depth_bin   k_bam_depth walks the batch's CIGARs before the slot is reused (one wave per record in one-wave
 *                      workgroups without LDS, 64 ops at a time; lanes that hit the same bin are summed in the wave and the
 *                      run's head issues one no-return 64-bit atomic, an op that spans whole bins is spread over them by
 *                      the wave); bin_off, the contig lengths and the two int64 tables live in the workspace, zeroed by `start`
 *            keep_*      (an active record filter) k_bam_keep (one thread per record in one-wave workgroups: 0 / 1 from the fixed
 *                      fields), one scan and k_bam_keep_compact (the kept record starts, in order, into a second array of
 *                      record starts in the workspace) between the boundary walk and the record parse; the kept count is read
 *                      back (8 bytes per batch) and is the batch's record count from there on: out[0] of `next`.  A batch
 *                      whose records are all dropped is pending with out[0] = out[1] = 0 and must be emitted like any other
 *            want_reads  k_bam_reads_plan (one thread per record in one-wave workgroups: the rule, the record's text bytes and its
 *                      work items of 16 384 bases), two scans and k_bam_reads_emit (one wave per work item in at most 2 048
 *                      one-wave workgroups without LDS: a lane makes 16 consecutive output characters from the nibbles / QUAL
 *                      bytes that cover them, mirrored for flag 0x10; aligned 16-byte stores inside an item, bytes at its two
 *                      edges; no atomics) write the batch's text into a buffer of the workspace (4/3 of a batch + 256 bytes),
 *                      which is copied to the host once the next batch's emit has synchronised the stream; the segments and the
 *                      name list live in the workspace too.  The totals come back on their own (16 bytes per batch).
 *                      want_reads = 2: the plan gives 4 + block_size per written record and work items of 32 768 record bytes,
 *                      and k_bam_reads_copy takes k_bam_reads_emit's place (same launch shape: a lane stores one aligned
 *                      16-byte chunk of the output, filled from the two aligned source chunks that cover it; bytes at an
 *                      item's two edges; no LDS, no atomics); the buffer is one batch + 256 bytes
 *                      reads_order = 1 of the request: between the plan and the scans k_bam_sort_keys (one
 *                      thread per record: reads_sort_key and the record's ordinal), hipcub's stable radix sort of (key,
 *                      ordinal) and k_bam_sort_permute (the plan's lengths and item counts in sorted order); the scans run
 *                      over the permuted arrays and k_bam_reads_copy_sorted, k_bam_reads_copy with the source record looked up
 *                      through the permutation, writes the batch's records sorted: one sorted run per batch.  The sort's
 *                      arrays (40 bytes per record of a batch + hipcub's temporary storage) are carved only for such a
 *                      request.  `finish` merges the runs (coral_bam_records_merge) when there is more than one
 *   finish        after the last batch (CORAL_ERR_ARG before): waits for `stream` once and leaves what was requested in the
 *          handle of `host` (coral_bam_coverage_result, coral_bam_pileup_result - the table is copied and summed per segment
 *          here -, coral_bam_index_sizes / _fill, coral_bam_qc_sizes / _fill, coral_bam_depth_sizes / _fill, coral_bam_reads_sizes / _fill); fails when
 *          an index was requested and the records are not in coordinate order; with nothing requested it does nothing
 *   CORAL_SINK_BAM  open_request for a want_reads = 2 request in file order (reads_order = 0) whose records go to the BGZF / BAM
 *          file `path` of the sink WHILE the decode runs, deflated where they are: uncompressed record bytes never leave the device, and the
 *          host keeps two pinned buffers of one chunk whatever the file's size.  The file is exactly coral_bgzf_write_gpu's of
 *          the two parts (header, all written record bytes): each part cut at 0xff00 bytes, the header ending a block, no empty
 *          member, the EOF block last; its bytes do not depend on batch_bytes, chunk_blocks or the run.  `header`: the inflated
 *          header to write (`header_bytes` > 0); chunk_blocks: blocks per deflate launch, 0 = 1 024, at most 16 384.  Spans are
 *          allowed.  `start` creates the sink's stream and pinned buffers and deflates the header.  Per batch, behind the plan's
 *          read-back: k_bam_reads_copy_shifted puts the batch's records behind the `carry` (< 0xff00) bytes the batch in front
 *          left at the head of the buffer (0xff00 bytes larger for that), the full blocks go in chunks through
 *          k_bgzf_chunk_desc (descriptors made on the device), k_bgzf_deflate and k_bgzf_pack on the sink's stream - behind an
 *          event recorded after the copy kernel, so the slot's reuse does not wait for them -, the tail moves to the front
 *          (device to device), and the next batch's copy kernel waits for an event behind that move.  A chunk's packed bytes
 *          come back once (4 bytes for their number first) and are written while the next chunk is on the device.  A batch that
 *          writes nothing queues nothing.  `finish` deflates the carry as the last block (none when it is 0), writes the EOF
 *          block and closes the file.  The slots, packed bytes, tokens, descriptors, lengths, offsets and scan storage of one
 *          chunk are part of *workspace_bytes only for such a request.  Nothing is kept on the host: coral_bam_reads_sizes gives
 *          records written and their inflated bytes, coral_bam_reads_fill is CORAL_ERR_ARG.  On any failure the file is left
 *          without the EOF block (readers see it truncated); `close` closes it.
 *          CORAL_ERR_ARG: want_reads other than 2, reads_order other than 0, world above 1, no path, no header,
 *          chunk_blocks outside 0..16 384, a path that cannot be created (and every refusal of a request).  No file is created
 *          by an open that is refused.
 *   CORAL_SINK_TEXT  the same for FASTQ: open_request for a want_reads = 1 request whose text goes to the plain file
 *          `path` of the sink (header and chunk_blocks are ignored) - each batch's text is written where it would be appended to the host-side result (one batch later, once
 *          the next emit or `finish` has synchronised the stream); no compression, no carry, nothing new in the workspace.  The
 *          bytes are those coral_bam_reads_fill would give.  reads_sizes / reads_fill as for CORAL_SINK_BAM; `finish`
 *          closes the file.  CORAL_ERR_ARG: want_reads other than 1, world above 1, no path, a path that cannot be created.
 *   CORAL_SINK_RUNS / merge_runs  the streamed coordinate sort (coral_bamgpu_merge.h, coral_merge_plan.h), in two phases in
 *          both of which uncompressed record bytes exist only in device memory.
 *          Phase 1, CORAL_SINK_RUNS: open_request for a want_reads = 2 request with reads_order = 1 whose batches' sorted runs go
 *          to the spill file `path` of the sink (header is ignored) WHILE the decode runs.  Per batch the plan, the key sort, the permute
 *          and the two scans run as for an ordered request; k_bam_reads_copy_sorted puts the sorted records at offset 0 of the
 *          sink's buffer and ALL of their blocks are deflated right away (k_bgzf_chunk_desc, k_bgzf_deflate, k_bgzf_pack in
 *          chunks of chunk_blocks), a short last one included: every run is a whole number of BGZF members, every member but a
 *          run's last holds 0xff00 bytes, no run shares a member.  The spill file has no header and no EOF block - members only;
 *          a batch that writes nothing leaves an empty run.  The chunk in flight is written before a run begins (its file
 *          offset is then known).  Per written record its 8-byte key and its length come back, in sorted order: the host keeps 12
 *          bytes per written record (16 while coral_bamgpu_merge_runs uploads the keys: the order's 4 bytes join them, then the
 *          keys are freed), a table of the runs and the sink's two pinned chunks - not the records.  The workspace is that of an
 *          ordered request plus the sink's arrays.  coral_bam_reads_sizes gives records and bytes, coral_bam_reads_fill is
 *          CORAL_ERR_ARG, sink_stats describes the spill file.  CORAL_ERR_ARG: want_reads other than 2, reads_order other than 1,
 *          world above 1, no path, chunk_blocks outside 0..16 384, a path that cannot be created (and every refusal of open_request).
 *          run_table (after `finish`): counts = runs, written records, bytes of the spill file; table (NULL, or max_runs rows):
 *          per run its first record, records, inflated bytes, file offset.
 *          Phase 2, merge_runs, after `finish` on the same handle, with a workspace of its own of merge_workspace_bytes(handle,
 *          stage_bytes) bytes (256-byte aligned; a negative value is an error code; the record count is only known by then).
 *          Once: the keys go up in run-major order, one stable hipcub radix sort of (key, global ordinal) - a tie goes to the
 *          earlier run, inside a run to the earlier record: coral_bam_records_merge's rule -, k_bam_merge_lens (the lengths and
 *          work items of READS_COPY_SLICE bytes in final order), three scans, and the order comes back.  The host plans steps
 *          (coral_merge_plan): the longest stretch of whole records whose sources fit stage_bytes (0: one batch's capacity; at
 *          most 0xf0000000); every run gives a contiguous range of its records, rounded outwards to its 0xff00-byte blocks; a
 *          block two steps share is read and inflated twice; a record whose own blocks do not fit: CORAL_ERR_CAPACITY, nothing
 *          created.  Per step the members go spill file -> one of two pinned pieces (rewritten only after its upload has
 *          completed) -> device -> k_bgzf_inflate + k_bgzf_crc into the staging buffer (refilled only behind an event recorded
 *          after the copy kernel that read it); the status words are waited for; k_bam_merge_copy (k_bam_reads_copy_sorted's
 *          launch shape) gathers the step's records in final order behind the carry of a second file sink - behind its
 *          wait_moved -, which cuts the concatenation of all steps at 0xff00 bytes: `out_path` is coral_bgzf_write_gpu's of the
 *          two parts (header, all records in order), byte for byte.  The reader is synchronous; the sink deflates and writes
 *          beside the next step.  Device memory: about 52 bytes per record, three times stage_bytes (staging, the members, the
 *          sink's buffer) and the sink's arrays.  Fewer than 2^31 records.  A short read, a bad magic, a member reaching behind
 *          its run, a member that does not inflate to its block or fails its CRC-32: CORAL_ERR_FORMAT, and the output is
 *          removed (as after any failure behind its creation).  The library allocates no device memory.
 *          merge_stats (after a merge): stats = steps, spill members inflated, of them members shared with the step in front,
 *          records written, their bytes, bytes of the output, its members, bytes of the spill file; seconds = the call, the order,
 *          reading the spill, waiting for upload + inflate + checksums, of that the kernels, k_bam_merge_copy, the sink, 0.
 *   coral_merge_plan  the step plan alone (host only): run_records[n_runs], len[N] (run-major), perm[N] (final position ->
 *          run-major ordinal; it must keep every run's records in their order: CORAL_ERR_ARG otherwise) -> counts = steps,
 *          parts; with the three arrays given (capacities max_steps, max_parts; too short: CORAL_ERR_CAPACITY) step_j[steps + 1],
 *          step_part[steps + 1] and parts[parts][4] = run, first block, block count, staging base, per step in run order.
 *   sink_stats  of such a handle: out = records written, their inflated bytes, bytes of the file, BGZF members in it (after
 *          `finish`: the whole file, header and EOF members included; a text file: its bytes twice and 0)
 * coral_bgzf_inflate: one inflate launch over caller-provided device buffers — desc = n_blocks x {src_off, src_len,
 * dst_off, isize} uint32 (raw DEFLATE streams in `comp`, which must be readable 4096 bytes beyond the last stream);
 * status[b] = 0 or the decoder's error code.
 * ------------------------------------------------------------------------------------------------ */
enum { CORAL_SINK_HOST = 0, CORAL_SINK_TEXT = 1, CORAL_SINK_BAM = 2, CORAL_SINK_RUNS = 3 };
typedef struct {
    int32_t kind;                              /* CORAL_SINK_*: where the reads request's result goes */
    const char *path;                          /* TEXT, BAM, RUNS: the file to create */
    const uint8_t *header;                     /* BAM: the inflated header to write, copied by the open call ... */
    int64_t header_bytes;                      /*      ... and its length, > 0 */
    int32_t chunk_blocks;                      /* BAM, RUNS: blocks per deflate launch, 0 = 1 024, at most 16 384 */
} coral_bam_sink_t;
int coral_bamgpu_start(void *handle, void *workspace, int64_t workspace_bytes);
int coral_bamgpu_next(void *handle, int64_t out[4], void *stream);
int coral_bamgpu_emit(void *handle, uint32_t *cigar_dst, int64_t *cigar_off_dst, void *stream);
int coral_bamgpu_host(void *handle, void **decoded);
int coral_bamgpu_stats(void *handle, int64_t stats[4], double seconds[6]);
int coral_bamgpu_open_request(const char *path, int32_t n_threads, int64_t batch_bytes, const coral_bam_request_t *req,
                              const coral_bam_sink_t *sink, void **handle, int64_t *workspace_bytes);
int coral_bamgpu_sink_stats(void *handle, int64_t out[4]);
int coral_bamgpu_run_table(void *handle, int64_t max_runs, int64_t *table, int64_t counts[3]);
int64_t coral_bamgpu_merge_workspace_bytes(void *handle, int64_t stage_bytes);
int coral_bamgpu_merge_runs(void *handle, const char *out_path, const uint8_t *header, int64_t header_bytes, void *workspace,
                            int64_t workspace_bytes, int64_t stage_bytes, void *stream);
int coral_bamgpu_merge_stats(void *handle, int64_t stats[8], double seconds[8]);
int coral_merge_plan(int32_t n_runs, const int64_t *run_records, const uint32_t *len, const uint32_t *perm, int64_t stage_bytes,
                     int64_t max_steps, int64_t max_parts, int64_t *step_j, int64_t *step_part, int64_t *parts, int64_t counts[2]);
int coral_bamgpu_finish(void *handle, void *stream);
int coral_bamgpu_close(void *handle);
int coral_bgzf_inflate(const uint8_t *comp, const uint32_t *desc, int32_t n_blocks, uint8_t *out, int32_t *status,
                       void *stream);

/* ------------------------------------------------------------------------------------------------
 * BGZF blocks made ON THE GPU - replaces what the reference's workflow gets from htslib's bgzf_write + zlib deflate when
 * `samtools view -b` / `samtools sort` write their output (/root/reference/scripts/align_nanopore_reads.sh:44, :49).  One
 * 64-lane wave turns one input block of at most 0xff00 bytes into one complete BGZF member (k_bgzf_deflate,
 * coral_deflate_core.h): the 18-byte header with BSIZE, ONE raw DEFLATE block - dynamic Huffman, or stored when the dynamic
 * stream would not be smaller than len + 5 bytes, so a member is never longer than len + 31 bytes -, CRC-32 and ISIZE.  An
 * empty block gives a valid empty member (31 bytes).  There is one setting, no levels.  A member's bytes are a function of its
 * block's bytes alone: not of the launch, the chunking, the alignment of source or slot, or the run.  They inflate with any
 * DEFLATE decoder; they are NOT zlib's or htslib's bytes.  The library allocates no device memory.
 *
 * coral_bgzf_deflate: one launch over caller-provided device buffers, the counterpart of coral_bgzf_inflate.  desc = n_blocks x
 *   {src_off, src_len <= 0xff00, dst_off, 0} uint32 on the device: the block is in[src_off .. src_off + src_len) (any byte
 *   alignment; nothing outside it is read), its member goes to out + dst_off, a slot of 65 536 bytes all of which may be
 *   written (out 4-byte aligned, dst_off a multiple of 4; slots must not overlap), and member_bytes[b] is the member's
 *   length.  scratch: coral_bgzf_deflate_scratch_bytes(n_blocks) bytes of device memory (4-byte aligned), the tokens between
 *   the compressor's two passes, 261 120 bytes per workgroup of the launch (at most 2 048).  The descriptors are read back
 *   once (the call waits for `stream` up to there); the launch itself is asynchronous.  n_blocks = 0 is a no-op.
 *   CORAL_ERR_ARG: n_blocks < 0, a missing array, src_len > 0xff00, a misaligned dst_off or out, short scratch.
 * coral_bgzf_pack: members in slots at the fixed stride (member b at slots + b * 65 536, member_bytes[b] long) -> one contiguous
 *   byte string: offsets[0 .. n_blocks] (uint32, device) is the exclusive scan of the lengths (offsets[n_blocks]: all bytes),
 *   packed gets the members one behind the other.  slots and packed 16-byte aligned; at most 16 384 blocks per call;
 *   scratch: coral_bgzf_pack_scratch_bytes(n_blocks) bytes (hipcub's temporary storage).  Asynchronous on `stream`.
 * coral_bgzf_write_gpu: coral_bgzf_write's contract with the blocks made on the current device: every part is cut at 0xff00
 *   bytes and starts a block of its own, an empty part makes no block, the 28-byte EOF block goes last.  The parts are host
 *   memory; chunks of consecutive blocks go up through two pinned buffers (allocated and freed by the call), each chunk is
 *   deflated and packed on the device, and only the packed bytes come back, written in order.  workspace: device memory,
 *   coral_bgzf_write_gpu_workspace_bytes() for chunks of 1 024 blocks (about 0.44 GiB, more than half of it tokens); a smaller one, down
 *   to coral_bgzf_write_gpu_workspace_min_bytes() (one block per chunk), only makes the chunks smaller - the file's bytes do not
 *   depend on it.  The call returns when the file is closed; nothing of it is left on `stream`.
 *   CORAL_ERR_ARG: no path, n_parts < 0, a missing array or part, no or too small a workspace, a path that cannot be created;
 *   CORAL_ERR_HIP: a HIP call failed; CORAL_ERR_FORMAT: the write failed.
 * ------------------------------------------------------------------------------------------------ */
int coral_bgzf_deflate(const uint8_t *in, const uint32_t *desc, int32_t n_blocks, uint8_t *out, uint32_t *member_bytes,
                       void *scratch, int64_t scratch_bytes, void *stream);
int64_t coral_bgzf_deflate_scratch_bytes(int32_t n_blocks);
int coral_bgzf_pack(const uint8_t *slots, const uint32_t *member_bytes, int32_t n_blocks, uint8_t *packed, uint32_t *offsets,
                    void *scratch, int64_t scratch_bytes, void *stream);
int64_t coral_bgzf_pack_scratch_bytes(int32_t n_blocks);
int coral_bgzf_write_gpu(const char *path, const uint8_t *const *parts, const int64_t *part_bytes, int32_t n_parts,
                         void *workspace, int64_t workspace_bytes, void *stream);
int64_t coral_bgzf_write_gpu_workspace_bytes(void);
int64_t coral_bgzf_write_gpu_workspace_min_bytes(void);

/* ------------------------------------------------------------------------------------------------
 * SAM text -> BAM records (`import`): what `samtools view -bS` does to a mapper's output, by the rules of htslib's sam_parse1 +
 * bam_write1 as coral_sam_core.h states them.  The header is the text's leading '@' lines; a record line has 11 fields and its
 * tags; a line ends at '\n', the text's last one at the text's end too.
 *
 * coral_sam_header: text[0, text_bytes) begins with the header (it may hold more: the header ends in front of the first line
 *   that does not begin with '@').  sizes[0..5] = bytes of the inflated BAM header (magic, l_text, the text verbatim, n_ref, per
 *   @SQ line l_name, name + NUL, l_ref), n_ref, bytes of all names, slots of the contig table, bytes of the header's text, its
 *   lines.  With bam / names / name_off / slots given (all four, of those sizes; name_off: n_ref + 1) they are filled: the
 *   names back to back without NUL, where each starts, and an open-addressing table (a power of two of slots, 1 + the contig
 *   or 0, linear probing from FNV-1a of the name) - the contig table of the two calls below.
 *   CORAL_ERR_FORMAT: an @SQ line without SN / LN, a bad LN, a name given twice.
 * coral_sam_encode: the whole lines of text[0, text_bytes), the first of which is line `first_line` (1-based) of the file ->
 *   their records back to back at out (out_cap bytes; out == NULL: validated and counted only).  keep[4] = min_mapq,
 *   min_seq_length, require_flags, exclude_flags: the record filter (a dropped line writes nothing).  counts[0..5] = lines,
 *   records written, records dropped, record bytes, and on a refusal its line number and field (coral_sam_core.h: Field).
 *   One thread; this is the rule book the device is compared against, and `import` with device "cpu".
 *   CORAL_ERR_FORMAT: a refused line - the lowest one; the error text names the line and the field; CORAL_ERR_CAPACITY: out
 *   is too short (2 * text_bytes + 36 * lines always suffices).
 * coral_samgpu_import: the lines that fd delivers (a file or a pipe, read to its end; never seeked), in front of them the
 *   lead_bytes bytes at lead (what the caller read behind the header), as the BAM file out_path: the header `bam` in blocks of
 *   its own, all records cut at 0xff00 bytes, the EOF block - coral_bgzf_write_gpu's file of the two parts (header, records).
 *   first_line: the file's line number of the first of them.  A feeder thread reads into two pinned buffers of batch_bytes
 *   (0: 128 MiB; the call allocates and frees them), each batch is cut at its last '\n' and the partial line leads the next
 *   one.  Per batch, on `stream`: k_sam_lines (newlines -> line starts), k_sam_size (one wave per line: fields, checks, filter,
 *   bytes), a scan, k_sam_encode (one wave per line: the record at its offset), and the record sink of
 *   the CORAL_SINK_BAM sink of coral_bamgpu_open_request deflates the bytes where they are (chunk_blocks blocks per launch, 0: 1 024).  'f' values
 *   outside the exact fast path of the device come back as (text offset, output offset), are converted with strtof from the
 *   pinned text and scattered in before the batch goes to the sink.  The file's bytes depend on the text and the filter alone.
 *   workspace: coral_samgpu_workspace_bytes(batch_bytes, chunk_blocks) bytes of device memory, n_ref / n_slots being those of
 *   the contig table; the library allocates none.  stats[0..8] = lines, records written, records dropped, text bytes, record
 *   bytes, file bytes, members, batches, float fix-ups; seconds[0..3] = all, waiting for the feeder, the two per-line kernels
 *   (from events, summed over the batches).  Nothing is left on `stream` when the call returns.
 *   CORAL_ERR_FORMAT: a refused line, as coral_sam_encode (the same line and field), or a failed write; CORAL_ERR_CAPACITY: a
 *   line longer than batch_bytes, or more float fix-ups in a batch than batch_bytes / 64; the output file is removed on any error.
 * ------------------------------------------------------------------------------------------------ */
int coral_sam_header(const uint8_t *text, int64_t text_bytes, int64_t *sizes, uint8_t *bam, uint8_t *names, int64_t *name_off,
                     uint32_t *slots);
int coral_sam_encode(const uint8_t *text, int64_t text_bytes, int64_t first_line, const uint8_t *names, const int64_t *name_off,
                     const uint32_t *slots, int32_t n_ref, int32_t n_slots, const int32_t *keep, uint8_t *out, int64_t out_cap,
                     int64_t *counts);
int coral_samgpu_import(int32_t fd, const uint8_t *lead, int64_t lead_bytes, int64_t first_line, const char *out_path,
                        const uint8_t *bam, int64_t bam_bytes, const uint8_t *names, const int64_t *name_off,
                        const uint32_t *slots, int32_t n_ref, int32_t n_slots, const int32_t *keep, int64_t batch_bytes,
                        int32_t chunk_blocks, void *workspace, int64_t workspace_bytes, void *stream, int64_t *stats,
                        double *seconds);
int64_t coral_samgpu_workspace_bytes(int64_t batch_bytes, int32_t chunk_blocks, int32_t n_ref, int32_t n_slots, int64_t names_bytes);

/* ------------------------------------------------------------------------------------------------
 * Copy number from binned depth (`cnv`): a deterministic Haar-wavelet segmenter after HaarSeg (Ben-Yaacov & Eldar 2008), in
 * place of the segmentation of `cnvkit.py batch` in the reference's scripts/call_cnvs.sh.  Parity with CNVkit is not claimed;
 * the rule (coral_cn_core.h) is what both backends compute, exactly:
 *   table     n_contigs contigs; contig c has the bins bin_off[c] .. bin_off[c + 1] of bin_size bases, ceil(lengths[c] /
 *             bin_size) of them; bases[b] int64 per bin; ref_bases: the same bins of a normal sample, or NULL; centre[c] != 0:
 *             a centring contig.  At most 2^28 bins.
 *   mask      a bin is a candidate when it has the full bin size and bases > 0 (with ref_bases: and ref_bases > 0).  C = the
 *             lower median of bases over the candidate bins of the centring contigs (C_ref: of ref_bases over the same bins).
 *             A candidate is kept when bases * 32 >= C (and ref_bases * 32 >= C_ref).  No candidate to centre on: no rows.
 *   signal    s = L(bases) - L(C) [- (L(ref_bases) - L(C_ref))], L = coral_cn_log2_q16: e = the top bit of x, m = x << (63 - e),
 *             16 times m * m -> one bit (1 and m = hi when hi >= 2^63, else 0 and m = hi << 1 | lo >> 63), L = e << 16 | bits.
 *   detail    per contig over its n kept bins x, mirror-padded (x[j] = x[-j-1], x[j] = x[2n-1-j]): for level l = 1..levels,
 *             h = 2^l <= n, c_h[k] = sum x[k..k+h-1] - sum x[k-h..k-1], k = 1..n-1, c_h[0] = c_h[n] = 0; k is a peak when
 *             c[k] > 0, c[k] > c[k-1], c[k] >= c[k+1], or the mirrored test for c[k] < 0.
 *   noise     d = the lower median of |c_1[k]|, k = 1..n-1; sigma = 1.4826 * d / sqrt(2).
 *   cut       coral_cn_fdr_cut on a (contig, level)'s peak magnitudes, descending: p_i = erfc(m_i / (sqrt(2h) * sigma *
 *             sqrt(2))), the largest 1-based i with p_i <= q * i / M gives the cut m_i (INT64_MAX: none; sigma == 0: 1, every
 *             peak).  The one floating-point step; a host function for both backends.
 *   unify     levels in rising order; a peak of at least its cut is added unless the set of the earlier levels holds a
 *             breakpoint within 2^(l-1) kept bins.
 *   rows      each contig's kept bins cut at the breakpoints (k starts a segment), in order: contig, start of the first bin,
 *             end of the last, probes = bins, sum_s = the sum of s (log2 = sum_s / (probes * 65536)), sum_bases.
 * counts[0..4] (8 entries) = rows, kept bins, C, C_ref, breakpoints.
 * coral_cn_segment_host: one thread, host arrays.  coral_cn_segment_gpu: the same arrays go up to `device`; kernels k_cn_* /
 *   k_haar_* and hipcub scans and radix sorts on `stream` in `workspace` (device memory, coral_cn_workspace_bytes; the
 *   library allocates none), three host waits in all (noise and peak counts, sorted magnitudes, rows); nothing is left on
 *   `stream`.  seconds[0..5] (or NULL) = upload, centre + signal + compaction + prefix sums, noise, the levels' peaks and
 *   sorts, the cuts on the host, unify + rows + download (from events).  Identical rows and counts.
 *   CORAL_ERR_ARG: a missing array, bins that do not fit the contigs, levels outside 1..20, fdr_q outside (0, 1), too small a
 *   workspace; CORAL_ERR_CAPACITY: more rows than row_cap - counts[0] then holds a row_cap that suffices.
 * ------------------------------------------------------------------------------------------------ */
int32_t coral_cn_log2_q16(uint64_t x);
int64_t coral_cn_fdr_cut(const int64_t *mags_desc, int64_t n_peaks, int64_t h, double sigma, double q);
int coral_cn_segment_host(int32_t n_contigs, const int64_t *bin_off, const int64_t *lengths, int64_t bin_size, const int64_t *bases,
                          const int64_t *ref_bases, const uint8_t *centre, int32_t levels, double fdr_q, int64_t row_cap,
                          int32_t *row_contig, int64_t *row_start, int64_t *row_end, int64_t *row_probes, int64_t *row_sum_s,
                          int64_t *row_sum_bases, int64_t *counts);
int coral_cn_segment_gpu(int32_t device, int32_t n_contigs, const int64_t *bin_off, const int64_t *lengths, int64_t bin_size,
                         const int64_t *bases, const int64_t *ref_bases, const uint8_t *centre, int32_t levels, double fdr_q,
                         int64_t row_cap, int32_t *row_contig, int64_t *row_start, int64_t *row_end, int64_t *row_probes,
                         int64_t *row_sum_s, int64_t *row_sum_bases, int64_t *counts, void *workspace, int64_t workspace_bytes,
                         void *stream, double *seconds);
int64_t coral_cn_workspace_bytes(int64_t n_bins, int32_t n_contigs, int32_t levels, int32_t has_reference, int64_t row_cap);
/* The same with the reference's composition per bin (coral_comp_*: the gc and rmask columns of the reference table of the
 * reference's scripts/call_cnvs.sh:12-17), which takes the GC bias and the uncalled bases out in front of the cut.  gc, at:
 * uint32 per bin of the table (NULL, both: no composition - the rows and counts of the entry points above, bit for bit).
 *   mask      a candidate must also have acgt = gc + at > 0 and acgt * 1000 >= bin_size * min_called_permille (0..1000);
 *             counts[5] = the candidates lost to this.  C, the 1/32 test and s are as above, over these candidates.
 *   stratum   g = gc * gc_strata / acgt in 64-bit integers, 0..gc_strata (gc_strata in 1..1000).
 *   bias      P = the kept bins of the centring contigs; for each g the smallest w >= 0 whose strata [max(0, g - w),
 *             min(gc_strata, g + w)] hold at least min(gc_min_bins, |P|) bins of P (gc_min_bins >= 1); bias[g] = the lower median
 *             of s over those bins (0 without any).  stratum_bins[g] = the bins of P in stratum g.  gc_strata + 1 entries each.
 *   apply     s' = s - bias[g] for every kept bin of every contig; detail, noise, cut, unify and rows run on s' (sum_s too).
 * Device: one stable radix sort of (g << 32 | biased s) over P, the strata's starts by binary search, k_cn_gc_bias (a wave per
 * stratum; the pooled median by bisection on the value), k_cn_gc_apply; no host wait is added.  seconds[0..6]: the six stages
 * above, then gc.  coral_cn_workspace_gc_bytes sizes the workspace. */
int coral_cn_segment_gc_host(int32_t n_contigs, const int64_t *bin_off, const int64_t *lengths, int64_t bin_size,
                             const int64_t *bases, const int64_t *ref_bases, const uint8_t *centre, int32_t levels, double fdr_q,
                             int64_t row_cap, int32_t *row_contig, int64_t *row_start, int64_t *row_end, int64_t *row_probes,
                             int64_t *row_sum_s, int64_t *row_sum_bases, int64_t *counts, const uint32_t *gc, const uint32_t *at,
                             int32_t gc_strata, int64_t gc_min_bins, int32_t min_called_permille, int64_t *bias,
                             int64_t *stratum_bins);
int coral_cn_segment_gc_gpu(int32_t device, int32_t n_contigs, const int64_t *bin_off, const int64_t *lengths, int64_t bin_size,
                            const int64_t *bases, const int64_t *ref_bases, const uint8_t *centre, int32_t levels, double fdr_q,
                            int64_t row_cap, int32_t *row_contig, int64_t *row_start, int64_t *row_end, int64_t *row_probes,
                            int64_t *row_sum_s, int64_t *row_sum_bases, int64_t *counts, void *workspace, int64_t workspace_bytes,
                            void *stream, double *seconds, const uint32_t *gc, const uint32_t *at, int32_t gc_strata,
                            int64_t gc_min_bins, int32_t min_called_permille, int64_t *bias, int64_t *stratum_bins);
int64_t coral_cn_workspace_gc_bytes(int64_t n_bins, int32_t n_contigs, int32_t levels, int32_t has_reference, int64_t row_cap,
                                    int32_t has_composition, int32_t gc_strata);

/* ------------------------------------------------------------------------------------------------
 * The k-mers of a reference genome (`kmers`): what lines 29-30 of the reference's scripts/align_nanopore_reads.sh get from
 * `meryl count k=15 output merylDB ref.fa` and `meryl print greater-than distinct=0.9998 merylDB > repetitive_k15.txt`, the
 * list the mapper takes with -W.  Parity with meryl's rounding of distinct=, its choice between a k-mer and its reverse
 * complement and its print order is not claimed (meryl was not available); the rule (coral_kmer_core.h) is what
 * both backends compute, exactly:
 *   text      FASTA bytes, fed in pieces of any size; the result does not depend on the cuts.  A line starts at the first byte
 *             and behind every '\n'; a line whose first byte is '>' is a header: its '>' is one break, the rest up to and
 *             including its '\n' is skipped.  '\n' and '\r' are skipped anywhere; ACGTacgt are the bases 0..3; any other byte
 *             is a break.
 *   k-mers    every window of k consecutive bases without a break, 1 <= k <= 16, as a 2k-bit integer with the first base in
 *             the top bits; canonical != 0: the smaller of the window and its reverse complement.
 *   table     4^k uint32 counters (coral_kmer_table_bytes), index = the k-mer, the caller's memory, zeroed by the caller (or
 *             holding an earlier count of bases_before bases to add to).  2^32 bases or more in all: CORAL_ERR_CAPACITY, so no
 *             counter wraps.
 * A session, so that the caller owns the reading of the file:
 *   open      (lines 29-30: the count) device < 0: the host backend, one thread, `table` in host memory; staging_bytes,
 *             workspace and stream are ignored.  device >= 0: `table` and `workspace` (coral_kmer_workspace_bytes(k,
 *             staging_bytes); the library allocates no device memory) are device memory, the kernels run on `stream`; the session
 *             owns two pinned staging buffers of staging_bytes (16 .. 2^30) and a copy stream.
 *   feed      (line 29) the next n bytes.  Device: copied into a staging buffer (waiting only for that buffer's use two pieces
 *             earlier), header lines found on the host (memchr), uploaded on the copy stream beside the kernels of the piece
 *             before; then on `stream`: scan of the keep flags, k_kmer_scatter, k_kmer_count (one no-return atomicAdd per run
 *             of equal indices of a thread's 32 symbols), k_kmer_carry.  No host wait for the kernels.
 *   finish    (line 30: what `distinct=` is computed from) waits; stats[0..5] (8 entries) = n_sequences (header lines), n_bases,
 *             total (k-mers counted), distinct (non-zero entries), the number of different count values, the largest count.
 *             seconds[0..3] (or NULL) = upload, classify + compact, count (host: the whole feed), statistics.
 *   histogram (line 30) the exact histogram, rising: values[i] = a count, numbers[i] = the distinct k-mers with it; capacity
 *             below stats[4]: CORAL_ERR_CAPACITY.
 *   select    (line 30: `print greater-than`) the entries with a count above greater_than in table order: kmers[i], counts[i];
 *             *n = how many there are; *n > capacity: CORAL_ERR_CAPACITY with the first `capacity` written - ask again with *n.
 *             Device sessions: kmers and counts are device memory; a count per 4 096-entry tile, a scan, a ranked write.
 *   lookup    (line 30) counts[i] = table[indices[i]] (0 for an index outside the table); device sessions: device memory.
 *   close     frees the session (never the table or the workspace).
 * coral_kmer_geometry (lines 29-30: the kernels of both) -> geometry[0..7] = symbols per thread and threads per workgroup of
 *   k_kmer_count, entries per workgroup tile and threads of the table passes (k_kmer_stats, k_kmer_sel_*), the symbols carried
 *   between pieces, bytes per workgroup of k_kmer_scatter, the histogram bins kept in LDS, the first count that is listed
 *   rather than binned.
 * Errors go to coral_bam_last_error.
 * ------------------------------------------------------------------------------------------------ */
/* lines 29-30 of scripts/align_nanopore_reads.sh: the bytes of meryl's count table for k */
int64_t coral_kmer_table_bytes(int32_t k);
/* line 29: the device scratch of a counting session */
int64_t coral_kmer_workspace_bytes(int32_t k, int64_t staging_bytes);
/* lines 29-30: the launch geometry of the kernels behind both */
int coral_kmer_geometry(int32_t *geometry);
/* line 29 (`meryl count k=15 output merylDB ref.fa`): a counting session */
int coral_kmer_open(int32_t k, int32_t canonical, int32_t device, void *table, int64_t staging_bytes, void *workspace,
                    int64_t workspace_bytes, void *stream, int64_t bases_before, void **handle);
/* line 29: the next bytes of ref.fa */
int coral_kmer_feed(void *handle, const uint8_t *bytes, int64_t n);
/* line 30 (`distinct=0.9998` needs them): the statistics of the finished count */
int coral_kmer_finish(void *handle, int64_t *stats, double *seconds);
/* line 30: the histogram `distinct=` is resolved against (`meryl histogram`) */
int coral_kmer_histogram(void *handle, int64_t capacity, int64_t *values, int64_t *numbers);
/* line 30 (`meryl print greater-than`): the k-mers above a count */
int coral_kmer_select(void *handle, int64_t greater_than, int64_t capacity, uint64_t *kmers, uint32_t *counts, int64_t *n);
/* line 30: the counts of given k-mers */
int coral_kmer_lookup(void *handle, const uint64_t *indices, int64_t n, uint32_t *counts);
/* lines 29-30: the end of the session (merylDB has no counterpart: nothing is left on disk) */
int coral_kmer_close(void *handle);

/* ------------------------------------------------------------------------------------------------
 * The composition of a reference genome per bin (`composition`): the GC and repeat-mask columns of the reference table that
 * the reference's scripts/call_cnvs.sh:12-17 hands to `cnvkit.py batch --seq-method wgs --reference hg38full_ref_5k.cnn`,
 * counted from the FASTA file.  Parity with `cnvkit.py reference` is not claimed; the rule (coral_comp_core.h)
 * is what both backends compute, exactly:
 *   text      FASTA bytes, fed in pieces of any size; the result does not depend on the cuts.  Lines are the k-mer counter's:
 *             a line starts at the first byte and behind every '\n'; a line whose first byte is '>' is a header and starts a
 *             contig, named by the bytes behind '>' up to the first blank, tab, '\r' or '\n' (an empty name: CORAL_ERR_FORMAT).
 *             '\n' and '\r' are skipped anywhere; every other byte of a line that is no header is one position of the contig
 *             (`samtools faidx` coordinates: N, IUPAC codes, '*' and '-' too); one in front of the first header:
 *             CORAL_ERR_FORMAT.  A contig of length 0, consecutive headers, CR LF and a last line without '\n' are legal.
 *   classes   gc: GCgc; at: ATat; masked: a..z; uncalled = length - gc - at.
 *   tables    contig c has ceil(length[c] / bin_size) bins, the last one short, in file order (the bins of the binned depth);
 *             gc, at, masked: uint32 per bin, `capacity` bins each, the caller's memory, zeroed by the caller.  1 <= bin_size <=
 *             2^31 - 1; at most 2^28 bins.
 * A session, so that the caller owns the reading of the file:
 *   open      device < 0: the host backend, one thread, tables in host memory; staging_bytes, workspace and stream are ignored.
 *             device >= 0: the tables and `workspace` (coral_comp_workspace_bytes(staging_bytes); the library allocates no
 *             device memory) are device memory, the kernels run on `stream`; the session owns two pinned staging buffers of
 *             staging_bytes (16 .. 2^30) and a copy stream.
 *   feed      the next n bytes.  Device: header lines found in the caller's bytes (memchr) and blanked to '\n' in the pinned copy,
 *             which goes up with the headers' byte offsets on the copy stream beside the kernels of the piece before (a piece
 *             with more headers than geometry[3] is fed as several); then on `stream`: scan of the is-position flags,
 *             k_comp_walk (closes the contigs, carries the open one), k_comp_count (one no-return atomicAdd per table and run of
 *             lanes in the same bin).  No host wait for the kernels.
 *   finish    waits; stats[0..6] (8 entries) = contigs, positions, bins, gc, at and masked in all, the bytes of the names.
 *             seconds[0..3] (or NULL) = upload, ordinals + contigs, count (host: the whole feed), 0.  More bins than the
 *             capacity: CORAL_ERR_CAPACITY, stats filled (stats[2] bins suffice), nothing written behind the capacity.
 *   contigs   lengths[c], and names[name_off[c] .. name_off[c + 1]) (name_off: contigs + 1 entries), host arrays.
 *   close     frees the session (never the tables or the workspace).
 * coral_comp_geometry -> geometry[0..6] = bytes per thread and threads per workgroup of k_comp_count, lanes per wave, the
 *   header lines one piece holds, threads of k_comp_walk, the smallest staging size, the bytes of one load.
 * Errors go to coral_bam_last_error.
 * ------------------------------------------------------------------------------------------------ */
/* scripts/call_cnvs.sh:12-17 (the reference table's gc and rmask columns): the device scratch of a counting session */
int64_t coral_comp_workspace_bytes(int64_t staging_bytes);
/* scripts/call_cnvs.sh:12-17: the launch geometry of the kernels behind the count */
int coral_comp_geometry(int32_t *geometry);
/* scripts/call_cnvs.sh:12-17 (`--reference hg38full_ref_5k.cnn`): a counting session over the genome's FASTA */
int coral_comp_open(int64_t bin_size, int32_t device, void *gc, void *at, void *masked, int64_t capacity, int64_t staging_bytes,
                    void *workspace, int64_t workspace_bytes, void *stream, void **handle);
/* scripts/call_cnvs.sh:12-17: the next bytes of the FASTA */
int coral_comp_feed(void *handle, const uint8_t *bytes, int64_t n);
/* scripts/call_cnvs.sh:12-17: the statistics of the finished count */
int coral_comp_finish(void *handle, int64_t *stats, double *seconds);
/* scripts/call_cnvs.sh:12-17 (the table's chromosome, start and end columns): the contigs' lengths and names */
int coral_comp_contigs(void *handle, int64_t n_contigs, int64_t *lengths, int64_t names_capacity, uint8_t *names,
                       int64_t *name_off);
/* scripts/call_cnvs.sh:12-17: the end of the session */
int coral_comp_close(void *handle);

/* ------------------------------------------------------------------------------------------------
 * Read QC and a read filter from the FASTQ itself (`qc --fastq`, `filter`): what the reference's scripts/report_nanopore_qc.py:35-48
 * collects through `pysam.FastxFile` - `len(sequence)` and `np.mean(quality)` of every record that has a sequence - and the
 * filter that its argument parser promises ("Quality filter reads") and that it lacks.  pysam and kseq were not available to
 * compare with; the rule (coral_fastq_core.h) is what both backends compute, exactly:
 *   text      FASTQ bytes, fed in pieces of any size; the result does not depend on the cuts.  A line starts at the first byte
 *             and behind every '\n'; line k has phase k mod 4; four lines are one record: name, sequence, separator, quality.  A
 *             phase-0 line must start with '@', a phase-2 line with '+'; the rest of either is not looked at.  '\r' is skipped
 *             anywhere in a phase-1 or phase-3 line; every other byte of a phase-1 line is one base (length <= 2^31 - 1), every
 *             other byte of a phase-3 line one quality character q, 33 <= q <= 126: qual_sum += q - 33, hist[q - 33] += 1.  A
 *             record's quality count must equal its length.  A last line without '\n' is legal; the stream may end at a record
 *             boundary, inside a phase-3 line or right behind the '\n' of a phase-2 line (either closes the record); an empty
 *             stream is zero records.
 *   refusals  everything else is CORAL_ERR_FORMAT, with the stream offset of the first offending byte in stats[6]: a wrong first
 *             byte (blank lines, FASTA records and wrapped records are refused so) and a quality character out of range at that
 *             byte; counts that differ at the byte that closes the record (its quality line's '\n', or the end of the stream);
 *             a stream that ends inside lines 0-2 at its end.  (kseq would skip blank lines and accept wrapped records.)
 *   rows      a record of length 0 is counted (stats[2]) and not listed; every other one is a read with length, qual_sum and kept.
 *   filter    kept iff length >= min_length, (max_length == 0 or length <= max_length) and 100 * qual_sum >= min_mean_q100 *
 *             length in 64-bit integers: the arithmetic mean of the Phred values in hundredths, not a mean of error
 *             probabilities.  No thresholds: every record is kept.  With output_fd >= 0 the bytes of every kept record go to
 *             it exactly as they were read (CR LF and a missing last '\n' included), consecutive kept records in one write.
 * A session, so that the caller owns the reading of the file:
 *   open      device < 0: the host backend, one thread, `hist` (256 zeroed uint64) in host memory; staging_bytes, workspace and
 *             stream are ignored.  device >= 0: `hist` and `workspace` (coral_fastq_workspace_bytes(staging_bytes); the library
 *             allocates no device memory) are device memory, the kernels run on `stream`; the session owns two pinned staging
 *             buffers of staging_bytes (16 .. 2^30) and a copy stream.  min_mean_q100: 0 .. 9300.
 *   feed      the next n bytes.  Device: the '\n' bytes are counted in the caller's bytes (memchr), which says how many records
 *             the piece closes and where (a piece that would close more than geometry[3] is fed as several); the pinned copy goes
 *             up on the copy stream beside the kernels of the piece before; then on `stream`: scan of the is-newline flags,
 *             k_fastq_accum (one no-return atomicAdd per row column and run of lanes in the same record, the histogram through
 *             a 256-bin LDS table), k_fastq_walk (closes the records, carries the open one) and the copy of the closed rows down
 *             into the pinned buffer, where they are taken - and the kept records' bytes written - when the buffer is next
 *             used.  No host wait for the kernels; uncompressed text never comes back from the device.
 *   finish    waits; stats[0..6] (8 entries) = records, reads, records without sequence, bases, kept records (those without
 *             sequence included), kept bases, the offending offset or -1.  seconds[0..3] (or NULL) = upload, scan + walk,
 *             accumulate (host: the whole feed), write.  A refused text: CORAL_ERR_FORMAT from feed or finish, stats[6] filled.
 *   rows      length, qual_sum and kept of the listed reads in file order, host arrays of stats[1] entries.
 *   close     frees the session (never the histogram or the workspace, and the descriptor stays open).
 * coral_fastq_geometry -> geometry[0..6] = bytes per thread and threads per workgroup of k_fastq_accum, lanes per wave, the
 *   records one piece closes, the smallest staging size, the bytes of one load, threads of k_fastq_walk.
 * Errors go to coral_bam_last_error; a bad argument or an output that cannot be written is CORAL_ERR_ARG.
 * ------------------------------------------------------------------------------------------------ */
/* scripts/report_nanopore_qc.py:35-48 (`pysam.FastxFile(fastq_file)`): the device scratch of a session over the FASTQ */
int64_t coral_fastq_workspace_bytes(int64_t staging_bytes);
/* scripts/report_nanopore_qc.py:35-48: the launch geometry of the kernels behind the loop over the records */
int coral_fastq_geometry(int32_t *geometry);
/* scripts/report_nanopore_qc.py:35-48 (and the "Quality filter reads" of its line 85): a session over the FASTQ */
int coral_fastq_open(int32_t device, int64_t min_length, int64_t max_length, int64_t min_mean_q100, int32_t output_fd,
                     int64_t staging_bytes, void *hist, void *workspace, int64_t workspace_bytes, void *stream, void **handle);
/* scripts/report_nanopore_qc.py:35-48: the next bytes of the FASTQ */
int coral_fastq_feed(void *handle, const uint8_t *bytes, int64_t n);
/* scripts/report_nanopore_qc.py:35-48: the end of the stream and the counters */
int coral_fastq_finish(void *handle, int64_t *stats, double *seconds);
/* scripts/report_nanopore_qc.py:43-48 (`mean_lengths`, `mean_qualities`): length, quality sum and kept flag of every read */
int coral_fastq_rows(void *handle, int64_t n_reads, int32_t *length, int64_t *qual_sum, uint8_t *kept);
/* scripts/report_nanopore_qc.py:35-48: the end of the session */
int coral_fastq_close(void *handle);

/* ------------------------------------------------------------------------------------------------
 * The minimizer sketch of a reference genome and its seed index (`sketch`): the first stage of `winnowmap -W repetitive_k15.txt
 * -ax map-ont` of the reference's scripts/align_nanopore_reads.sh:34, and the only use repetitive_k15.txt has.  Neither winnowmap
 * nor minimap2 was available to compare with; the rule (coral_sketch_core.h) is what both backends compute, exactly:
 *   text      FASTA bytes, fed in pieces of any size; the result does not depend on the cuts.  Lines, contigs, names and the
 *             refusals (CORAL_ERR_FORMAT) are the composition session's.  Every byte of a sequence line but '\n' and '\r' is one
 *             position of its contig; ACGTacgt are the bases, any other byte is a non-base in its place.  A contig of 2^31
 *             positions or more, or 2^32 contigs or more: CORAL_ERR_CAPACITY.
 *   k-mer     1 <= k <= 16; the k bases from position p on; fwd / rev as the k-mer counter's.  Invalid with a non-base in it or
 *             with fwd == rev.  strand = rev < fwd, canon = min(fwd, rev), key = hash64(canon) | repetitive(canon) << 2k, hash64
 *             the invertible integer hash, every step taken & (4^k - 1).  `weights`: one bit per canonical k-mer, 4^k bits in
 *             uint32 words (coral_sketch_bitmap_bytes(k)), bit (canon & 31) of word canon >> 5; NULL: no k-mer is repetitive.
 *   windows   1 <= w <= 256.  A contig with n >= 1 k-mer positions has the windows of min(w, n) consecutive positions inside it;
 *             an invalid k-mer keeps its place with the key +infinity.  Position p is a minimizer iff its k-mer is valid and its
 *             key is the minimum of at least one window that holds p; tied minima all count.
 *   output    keys[i], values[i] = contig << 32 | pos << 1 | strand, uint64, in (contig, pos) order, `capacity` entries each, the
 *             caller's memory.
 * A session, so that the caller owns the reading of the file:
 *   open      device < 0: the host backend, one thread, arrays in host memory; staging_bytes, workspace and stream are ignored.
 *             device >= 0: `weights`, the arrays and `workspace` (coral_sketch_workspace_bytes(staging_bytes); the library
 *             allocates no device memory) are device memory, the kernels run on `stream`; the session owns two pinned staging
 *             buffers of staging_bytes (16 .. 2^30) and a copy stream.
 *   feed      the next n bytes.  Device: header lines found in the caller's bytes (memchr) and blanked in the pinned copy but for
 *             their '>', which goes up with the headers' byte offsets on the copy stream beside the kernels of the piece before (a
 *             piece with more headers than geometry[4] is fed as several); then on `stream`: scan of the keep flags,
 *             k_sketch_scatter (symbols behind the geometry[1] carried ones), k_sketch_walk (the table of contig starts, the
 *             decided positions), k_sketch_tile twice with a scan between (count, write: a workgroup per geometry[0] positions,
 *             keys with halos in LDS, two sliding passes), k_sketch_carry.  No host wait for the kernels.
 *   finish    waits; stats[0..6] (8 entries) = contigs, positions, minimizers, minimizers written, 0, 0, the bytes of the names.
 *             seconds[0..3] (or NULL) = upload, symbols + contig table, sketch (host: the whole feed), the last tile.  More
 *             minimizers than the capacity: CORAL_ERR_CAPACITY, stats filled (stats[2] entries suffice), nothing written
 *             behind the capacity.
 *   contigs   lengths[c], and names[name_off[c] .. name_off[c + 1]) (name_off: contigs + 1 entries), host arrays.
 *   close     frees the session (never the arrays, the weights or the workspace).
 * The index, over the two arrays (device < 0: host arrays; else device arrays, and the call waits for `stream`):
 *   sort      by key, stably, so that ties keep their (contig, pos) order; device: one radix sort over the key's 2k + 1 bits in
 *             `workspace` (coral_sketch_sort_workspace_bytes(n)).
 *   lookup    first[i], count[i] = the entries of query_keys[i] in the sorted keys (first = the insertion point for count 0).
 *   anchors   query minimizers (query, qpos, qstrand, qkey), n_queries of them: a key with more than max_occ entries is dropped,
 *             every other one gives per entry anchor_query = query << 32 | qpos and anchor_ref = the entry's value with its
 *             strand bit ^ qstrand; query order, then index order; count, scan, write in `workspace`
 *             (coral_sketch_anchors_workspace_bytes(n_queries)).  *n_anchors = how many there are; more than the capacity:
 *             CORAL_ERR_CAPACITY with the first `capacity` written - ask again with *n_anchors.
 * coral_sketch_geometry -> geometry[0..7] = positions per tile of k_sketch_tile, symbols carried between pieces, threads per
 *   workgroup, positions per thread, the header lines one piece holds, the entries of the contig table, the smallest staging size,
 *   the largest w.
 * Errors go to coral_bam_last_error.
 * ------------------------------------------------------------------------------------------------ */
/* scripts/align_nanopore_reads.sh:34 (`-W repetitive_k15.txt`): the bytes of the weights' bitmap at k */
int64_t coral_sketch_bitmap_bytes(int32_t k);
/* scripts/align_nanopore_reads.sh:34: the device scratch of a sketching session */
int64_t coral_sketch_workspace_bytes(int64_t staging_bytes);
/* scripts/align_nanopore_reads.sh:34: the launch geometry of the kernels behind the sketch */
int coral_sketch_geometry(int32_t *geometry);
/* scripts/align_nanopore_reads.sh:34 (`winnowmap -W ... ref.fa`, the mapper's indexing of the reference): a sketching session */
int coral_sketch_open(int32_t k, int32_t w, int32_t device, const void *weights, void *keys, void *values, int64_t capacity,
                      int64_t staging_bytes, void *workspace, int64_t workspace_bytes, void *stream, void **handle);
/* scripts/align_nanopore_reads.sh:34: the next bytes of the FASTA */
int coral_sketch_feed(void *handle, const uint8_t *bytes, int64_t n);
/* scripts/align_nanopore_reads.sh:34: the end of the stream and the counts */
int coral_sketch_finish(void *handle, int64_t *stats, double *seconds);
/* scripts/align_nanopore_reads.sh:34 (the @SQ lines of the mapper's output): the contigs' lengths and names */
int coral_sketch_contigs(void *handle, int64_t n_contigs, int64_t *lengths, int64_t names_capacity, uint8_t *names,
                         int64_t *name_off);
/* scripts/align_nanopore_reads.sh:34: the end of the session */
int coral_sketch_close(void *handle);
/* scripts/align_nanopore_reads.sh:34 (the mapper's hash table of the reference's minimizers): the device scratch of the sort */
int64_t coral_sketch_sort_workspace_bytes(int64_t n);
/* scripts/align_nanopore_reads.sh:34: the pairs sorted by key */
int coral_sketch_sort(int32_t device, void *keys, void *values, int64_t n, int32_t k, void *workspace, int64_t workspace_bytes,
                      void *stream);
/* scripts/align_nanopore_reads.sh:34 (a read minimizer's look-up in the table): the entries of given keys */
int coral_sketch_lookup(int32_t device, const void *sorted_keys, int64_t n, const void *query_keys, int64_t n_queries,
                        int64_t *first, int64_t *count, void *stream);
/* scripts/align_nanopore_reads.sh:34: the device scratch of the expansion */
int64_t coral_sketch_anchors_workspace_bytes(int64_t n_queries);
/* scripts/align_nanopore_reads.sh:34 (the seeds that the mapper chains): read minimizers expanded into anchors */
int coral_sketch_anchors(int32_t device, const void *sorted_keys, const void *values, int64_t n, const uint32_t *query,
                         const uint32_t *qpos, const uint8_t *qstrand, const void *qkey, int64_t n_queries, int64_t max_occ,
                         int64_t capacity, void *anchor_query, void *anchor_ref, void *workspace, int64_t workspace_bytes,
                         void *stream, int64_t *n_anchors);

#ifdef __cplusplus
}
#endif
#endif /* CORAL_HIP_H */
