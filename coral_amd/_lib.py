"""ctypes binding of libcoral_hip.so (include/coral_hip.h).  Fails loudly when the library is missing:
there is no CPU fallback on the product path."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcoral_hip.so")


class CoralHipError(RuntimeError):
    pass


class coral_records_t(C.Structure):
    _fields_ = [("n_rec", C.c_int64), ("tid", C.c_void_p), ("pos", C.c_void_p), ("end", C.c_void_p),
                ("flagmq", C.c_void_p), ("n_cigar", C.c_void_p), ("cigar_off", C.c_void_p), ("cigar", C.c_void_p)]


class coral_bam_request_t(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("n_spans", C.c_int32), ("span_beg", C.c_void_p), ("span_end", C.c_void_p),
                ("n_seg", C.c_int32), ("seg_tid", C.c_void_p), ("seg_start", C.c_void_p), ("seg_end", C.c_void_p),
                ("quality_threshold", C.c_int32), ("read_callback", C.c_int32), ("want_index", C.c_int32), ("want_qc", C.c_int32),
                ("per_base", C.c_int32), ("depth_bin", C.c_int32), ("depth_min_mapq", C.c_int32), ("depth_exclude_flags", C.c_int32),
                ("depth_count_deletions", C.c_int32), ("want_reads", C.c_int32), ("reads_order", C.c_int32), ("reads_exclude_flags", C.c_int32),
                ("reads_n_seg", C.c_int32), ("reads_seg_tid", C.c_void_p), ("reads_seg_start", C.c_void_p), ("reads_seg_end", C.c_void_p),
                ("reads_n_names", C.c_int32), ("reads_names", C.c_void_p), ("reads_name_off", C.c_void_p), ("keep_min_mapq", C.c_int32), ("keep_min_seq_length", C.c_int32),
                ("keep_require_flags", C.c_int32), ("keep_exclude_flags", C.c_int32)]


SINK_HOST, SINK_TEXT, SINK_BAM, SINK_RUNS = range(4)         # CORAL_SINK_*: coral_bam_sink_t.kind

class coral_bam_sink_t(C.Structure):
    _fields_ = [("kind", C.c_int32), ("path", C.c_char_p), ("header", C.c_void_p), ("header_bytes", C.c_int64), ("chunk_blocks", C.c_int32)]


def bam_request(rank: int = 0, world: int = 1, spans=None, coverage=None, index: bool = False, qc: bool = False,
                per_base: bool = False, depth=None, keep=None, reads=None) -> coral_bam_request_t:
    """The request of a BAM decode: ``spans`` uint64 [K][2] virtual offsets (None: the byte range), ``coverage`` = (segments int32
    [3][S], quality threshold, read_callback code) or None, ``per_base``: the coverage as the table per position and base (the
    pileup), ``depth`` = (bin size, min_mapq, exclude_flags, count_deletions) or None: the binned-depth request, ``keep`` = (min_mapq, min_seq_length, require_flags, exclude_flags) (a
    ``bam.RecordFilter`` is one) or None: the record filter, ``reads`` = (exclude_flags, segments int32 [3][S] or None, names = a list
    of bytes or None[, mode[, order]]) or None: the reads request (no segment / no name: no such limit; mode 1, the default: FASTQ
    text, 2: the records' own bytes; order 0, the default: file order, 1: coordinate order).  The struct keeps the contiguous
    arrays it points into alive; the rules are the library's to check."""
    req = coral_bam_request_t(rank=rank, world=world, n_spans=-1, n_seg=-1, want_index=int(index), want_qc=int(qc), per_base=int(per_base))
    req.arrays = []
    if depth is not None:
        req.depth_bin, req.depth_min_mapq, req.depth_exclude_flags, req.depth_count_deletions = (int(v) for v in depth)
    if keep is not None:
        req.keep_min_mapq, req.keep_min_seq_length, req.keep_require_flags, req.keep_exclude_flags = (int(v) for v in keep)

    def pointer(a, dtype):
        req.arrays.append(np.ascontiguousarray(a, dtype=dtype))
        return req.arrays[-1].ctypes.data
    if reads is not None:                    # (in front of the coverage request: its segment rows stay the last arrays)
        exclude_flags, segs, names = reads[:3]
        req.want_reads, req.reads_exclude_flags = (int(reads[3]) if len(reads) > 3 else 1), int(exclude_flags)
        req.reads_order = int(reads[4]) if len(reads) > 4 else 0
        if segs is not None:
            segs = np.asarray(segs, dtype=np.int32).reshape(3, -1)
            req.reads_n_seg = segs.shape[1]
            req.reads_seg_tid, req.reads_seg_start, req.reads_seg_end = (pointer(row, np.int32) for row in segs)
        if names is not None:
            names = [bytes(nm) for nm in names]
            req.reads_n_names = len(names)
            req.reads_names = pointer(np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8), np.uint8)
            req.reads_name_off = pointer(np.concatenate([[0], np.cumsum([len(nm) for nm in names], dtype=np.int64)]), np.int64)
    if spans is not None:
        spans = np.asarray(spans, dtype=np.uint64).reshape(-1, 2)
        req.n_spans, req.span_beg, req.span_end = len(spans), pointer(spans[:, 0], np.uint64), pointer(spans[:, 1], np.uint64)
    if coverage is not None:
        segs, req.quality_threshold, req.read_callback = coverage
        segs = np.asarray(segs, dtype=np.int32).reshape(3, -1)
        req.n_seg = segs.shape[1]
        req.seg_tid, req.seg_start, req.seg_end = (pointer(row, np.int32) for row in segs)
    return req


_lib = None

def lib():
    """Load (once) and return the shared library; raise CoralHipError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CoralHipError("libcoral_hip.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "— the product path has no CPU fallback" % LIB_PATH)
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:
        raise CoralHipError("cannot load %s: %s" % (LIB_PATH, e))
    L.coral_version.restype = C.c_char_p
    L.coral_last_error.restype = C.c_char_p
    P = C.c_void_p
    R = C.POINTER(coral_records_t)
    L.coral_cigar_scan.argtypes = [R, C.c_int32, C.c_int32, P, P, P, C.c_uint32, P]
    L.coral_scan_kernel_name.restype = C.c_char_p
    L.coral_segment_coverage.argtypes = [R, P, C.c_int32, P, P, P, P, P, P, P, P]
    L.coral_point_cover.argtypes = [R, C.c_int32, P, P, C.c_int32, P, P, C.c_uint32, P]
    L.coral_read_counter.argtypes = [P, C.POINTER(C.c_uint32), P]
    L.coral_first_seen_rows.argtypes = [C.c_int64, C.c_int32, P, P]
    L.coral_bp_pair_table.argtypes = [C.c_int32, C.c_int32, P, P, P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P, P]
    L.coral_search_create.argtypes = [C.c_int64, C.c_int64] + [P] * 9 + [C.c_int64, P, P, P, C.c_int32, P, P, P]
    L.coral_search_create.restype = C.c_void_p
    L.coral_search_create_early.argtypes = [C.c_int64, C.c_int64] + [P] * 7 + [C.c_int32]
    L.coral_search_create_early.restype = C.c_void_p
    L.coral_search_attach.argtypes = [C.c_void_p, P, P, P, C.c_int64, P, P, P, P, P, P]
    L.coral_search_shutdown.argtypes = []
    L.coral_search_stats.argtypes = [C.c_void_p, P, C.c_int32]
    L.coral_search_free.argtypes = [C.c_void_p]
    L.coral_search_error.argtypes = [C.c_void_p]
    L.coral_search_error.restype = C.c_char_p
    PI64, PF64, PI32 = C.POINTER(C.POINTER(C.c_int64)), C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.POINTER(C.c_int32))
    L.coral_search_result.argtypes = [C.c_void_p, C.POINTER(C.c_int64), PI64, C.POINTER(C.c_int64), PI64, C.POINTER(C.c_int64), PI64,
                                      PF64, PI64, PI32]
    L.coral_search_step.argtypes = [C.c_void_p] + [C.c_int64] * 5
    L.coral_search_prefetch.argtypes = [C.c_void_p] + [C.c_int64] * 5
    L.coral_search_params.argtypes = [C.c_void_p, C.c_double, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_int32]
    L.coral_search_bfs.argtypes = [C.c_void_p, C.c_int32, P, P, P, P, P, C.c_double, C.c_int64, C.c_int32]
    L.coral_search_bfs_get.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.coral_search_within.argtypes = [C.c_void_p, C.c_int32, P, P, P]
    L.coral_search_between.argtypes = [C.c_void_p, C.c_int64, P] + [C.c_int64] * 6
    L.coral_smalldel_pass.argtypes = [C.c_int64, P, C.c_int64, P, P, P, P, P, C.c_int32, P, C.c_double, C.c_int64, C.c_int64, C.c_double]
    L.coral_smalldel_pass.restype = C.c_void_p
    L.coral_tail_result_free.argtypes = [C.c_void_p]
    L.coral_tail_result_free.restype = None
    L.coral_tail_result_rc.argtypes = [C.c_void_p]
    L.coral_tail_result_error.argtypes = [C.c_void_p]
    L.coral_tail_result_error.restype = C.c_char_p
    L.coral_tail_result_get.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.coral_search_tail_prefetch.argtypes = [C.c_void_p, C.c_int32, P, C.c_int64, P, C.c_int64, P, P, P, P, P]
    L.coral_search_tail_collect.argtypes = [C.c_void_p, C.c_int32, C.c_int32, P, C.c_int64, P, C.c_int64, P, P, P, P, P, C.POINTER(C.c_void_p)]
    L.coral_search_tail_stats.argtypes = [C.c_void_p, P]
    L.coral_sa_table.argtypes = [C.c_int32, P, P, P, P, C.c_int32, C.c_int32, P, P, P, P, C.c_int64, P, P, P, P, P,
                                 C.POINTER(C.c_int32), P]
    L.coral_sa_last_error.restype = C.c_char_p
    L.coral_hash_rows.argtypes = [C.c_int32, P, C.c_int32, P, P, P, P, P, C.c_int32, P, C.c_int64, P, P, P, P, C.POINTER(C.c_int32), P]
    L.coral_segment_coverage_host.argtypes = [R, P, C.c_int32, P, P, P, P]
    L.coral_hash_rows_host.argtypes = [C.c_int32, P, C.c_int32, P, P, C.c_int32, P, P, P, P, C.POINTER(C.c_int32), P]
    L.coral_point_cover_host.argtypes = [R, C.c_int32, P, P, C.c_int32, C.c_uint32, P, P, C.POINTER(C.c_uint32), P]
    L.coral_query_arena_release.argtypes = []
    L.coral_sa_table_async.argtypes = [C.c_int32, P, P, P, P, C.c_int32, C.c_int32, P, P, P, P, C.c_int64, P, P, P, P, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_int32, P, P, P, P, P, C.POINTER(C.c_int32), P]
    L.coral_pyset_batch_create.argtypes = [C.c_int64, P, P, P, C.c_int32, P]
    L.coral_pyset_batch_create.restype = C.c_void_p
    L.coral_pyset_union_order.argtypes = [C.c_void_p, C.c_int32, P, P, C.POINTER(C.c_int32)]
    L.coral_pyset_batch_free.argtypes = [C.c_void_p]
    L.coral_call_breakpoints.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_int64, C.c_int64, C.c_double,
                                         C.c_int32] + [C.c_void_p] * 10
    L.coral_nm_stats.argtypes = [C.c_int64] + [C.c_void_p] * 8
    L.coral_reach_create.argtypes = [C.c_int64] + [C.c_void_p] * 6 + [C.c_int64] * 4 + [C.c_void_p, C.c_void_p]
    L.coral_reach_create.restype = C.c_void_p
    L.coral_reach_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.coral_concordant_counts.argtypes = [C.c_int32, P, P, P, C.c_int64, P, C.c_int64, C.c_int64, P, P, P]
    L.coral_independent_rows.argtypes = [C.c_int32, C.c_int32, P, P, C.c_double]
    L.coral_cn_solve.argtypes = [C.c_int32, C.c_int32, P, P, P, P, C.c_int32, P, P, C.POINTER(C.c_int32)]
    L.coral_cluster_first_fit.argtypes = [C.c_int64, P, P, C.c_int64, P, C.POINTER(C.c_int32)]
    L.coral_bam_decode_open.argtypes = [C.c_char_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.coral_bam_decode_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.coral_bam_decode_fill.argtypes = [C.c_void_p] + [P] * 21
    L.coral_bam_decode_close.argtypes = [C.c_void_p]
    L.coral_bam_last_error.restype = C.c_char_p
    L.coral_names_unify.argtypes = [C.c_int32, P, P, P, P, P, P, C.POINTER(C.c_int64), C.c_int32]
    L.coral_bam_decode_range.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.coral_bam_decode_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.coral_bam_write.argtypes = [C.c_char_p, C.c_int64] + [P] * 9 + [P, P, P, P, P, C.c_int64, P, P, P, C.c_int32, P, P, C.c_uint32,
                                                                        C.c_int32, C.c_int32]
    L.coral_bamgpu_start.argtypes = [C.c_void_p, P, C.c_int64]
    L.coral_bamgpu_next.argtypes = [C.c_void_p, C.POINTER(C.c_int64), P]
    L.coral_bamgpu_emit.argtypes = [C.c_void_p, P, P, P]
    L.coral_bamgpu_host.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.coral_bamgpu_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.coral_bamgpu_close.argtypes = [C.c_void_p]
    L.coral_bgzf_inflate.argtypes = [P, P, C.c_int32, P, P, P]
    Q = C.POINTER(coral_bam_request_t)
    L.coral_bam_decode_request.argtypes = [C.c_char_p, C.c_int32, Q, C.POINTER(C.c_void_p)]
    L.coral_bam_coverage_result.argtypes = [C.c_void_p, C.c_int32, P]
    L.coral_bam_pileup_result.argtypes = [C.c_void_p, C.c_int64, P]
    L.coral_bam_index_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.coral_bam_index_fill.argtypes = [C.c_void_p, P, P, P, P, P, C.POINTER(C.c_uint64)]
    L.coral_bam_qc_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.coral_bam_qc_fill.argtypes = [C.c_void_p, P, P, P, P, P, C.POINTER(C.c_int64)]
    L.coral_bam_depth_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.coral_bam_depth_fill.argtypes = [C.c_void_p, P, P, P]
    L.coral_bam_reads_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.coral_bam_reads_fill.argtypes = [C.c_void_p, P, P]
    L.coral_bgzf_write.argtypes = [C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int32]
    L.coral_bamgpu_open_request.argtypes = [C.c_char_p, C.c_int32, C.c_int64, Q, C.POINTER(coral_bam_sink_t), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.coral_bamgpu_finish.argtypes = [C.c_void_p, P]
    L.coral_bamgpu_sink_stats.argtypes =[C.c_void_p, C.POINTER(C.c_int64)]
    L.coral_bamgpu_run_table.argtypes = [C.c_void_p, C.c_int64, P, C.POINTER(C.c_int64)]
    L.coral_bamgpu_merge_workspace_bytes.argtypes = [C.c_void_p, C.c_int64]
    L.coral_bamgpu_merge_workspace_bytes.restype = C.c_int64
    L.coral_bamgpu_merge_runs.argtypes = [C.c_void_p, C.c_char_p, P, C.c_int64, P, C.c_int64, C.c_int64, P]
    L.coral_bamgpu_merge_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.coral_merge_plan.argtypes = [C.c_int32, P, P, P, C.c_int64, C.c_int64, C.c_int64, P, P, P, C.POINTER(C.c_int64)]
    L.coral_bam_records_merge.argtypes =[C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), P, P, C.c_int32]
    L.coral_bgzf_deflate.argtypes = [P, P, C.c_int32, P, P, P, C.c_int64, P]
    L.coral_bgzf_pack.argtypes = [P, P, C.c_int32, P, P, P, C.c_int64, P]
    L.coral_bgzf_write_gpu.argtypes = [C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int32, P, C.c_int64, P]
    L.coral_sam_header.argtypes = [P, C.c_int64, C.POINTER(C.c_int64), P, P, P, P]
    L.coral_sam_encode.argtypes = [P, C.c_int64, C.c_int64, P, P, P, C.c_int32, C.c_int32, P, P, C.c_int64, C.POINTER(C.c_int64)]
    L.coral_samgpu_import.argtypes = [C.c_int32, P, C.c_int64, C.c_int64, C.c_char_p, P, C.c_int64, P, P, P, C.c_int32, C.c_int32, P, C.c_int64, C.c_int32,
                                      P, C.c_int64, P, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.coral_samgpu_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64]
    L.coral_samgpu_workspace_bytes.restype = C.c_int64
    L.coral_cn_log2_q16.argtypes = [C.c_uint64]
    L.coral_cn_log2_q16.restype = C.c_int32
    L.coral_cn_fdr_cut.argtypes = [P, C.c_int64, C.c_int64, C.c_double, C.c_double]
    L.coral_cn_fdr_cut.restype = C.c_int64
    L.coral_cn_segment_host.argtypes = [C.c_int32, P, P, C.c_int64, P, P, P, C.c_int32, C.c_double, C.c_int64] + [P] * 7
    L.coral_cn_segment_gpu.argtypes = [C.c_int32] + L.coral_cn_segment_host.argtypes + [P, C.c_int64, P, P]
    L.coral_cn_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64]
    L.coral_cn_workspace_bytes.restype = C.c_int64
    gc_args = [P, P, C.c_int32, C.c_int64, C.c_int32, P, P]
    L.coral_cn_segment_gc_host.argtypes = L.coral_cn_segment_host.argtypes + gc_args
    L.coral_cn_segment_gc_gpu.argtypes = L.coral_cn_segment_gpu.argtypes + gc_args
    L.coral_cn_workspace_gc_bytes.argtypes = L.coral_cn_workspace_bytes.argtypes + [C.c_int32, C.c_int32]
    L.coral_cn_workspace_gc_bytes.restype = C.c_int64
    L.coral_kmer_table_bytes.argtypes = [C.c_int32]
    L.coral_kmer_table_bytes.restype = C.c_int64
    L.coral_kmer_workspace_bytes.argtypes = [C.c_int32, C.c_int64]
    L.coral_kmer_workspace_bytes.restype = C.c_int64
    L.coral_kmer_geometry.argtypes = [P]
    L.coral_kmer_open.argtypes = [C.c_int32, C.c_int32, C.c_int32, P, C.c_int64, P, C.c_int64, P, C.c_int64, C.POINTER(C.c_void_p)]
    L.coral_kmer_feed.argtypes = [C.c_void_p, P, C.c_int64]
    L.coral_kmer_finish.argtypes = [C.c_void_p, P, P]
    L.coral_kmer_histogram.argtypes = [C.c_void_p, C.c_int64, P, P]
    L.coral_kmer_select.argtypes = [C.c_void_p, C.c_int64, C.c_int64, P, P, C.POINTER(C.c_int64)]
    L.coral_kmer_lookup.argtypes = [C.c_void_p, P, C.c_int64, P]
    L.coral_kmer_close.argtypes = [C.c_void_p]
    L.coral_comp_workspace_bytes.argtypes = [C.c_int64]
    L.coral_comp_workspace_bytes.restype = C.c_int64
    L.coral_comp_geometry.argtypes = [P]
    L.coral_comp_open.argtypes = [C.c_int64, C.c_int32, P, P, P, C.c_int64, C.c_int64, P, C.c_int64, P, C.POINTER(C.c_void_p)]
    L.coral_comp_feed.argtypes = [C.c_void_p, P, C.c_int64]
    L.coral_comp_finish.argtypes = [C.c_void_p, P, P]
    L.coral_comp_contigs.argtypes = [C.c_void_p, C.c_int64, P, C.c_int64, P, P]
    L.coral_comp_close.argtypes = [C.c_void_p]
    L.coral_fastq_workspace_bytes.argtypes = [C.c_int64]
    L.coral_fastq_workspace_bytes.restype = C.c_int64
    L.coral_fastq_geometry.argtypes = [P]
    L.coral_fastq_open.argtypes = [C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int64, P, P, C.c_int64, P, C.POINTER(C.c_void_p)]
    L.coral_fastq_feed.argtypes = [C.c_void_p, P, C.c_int64]
    L.coral_fastq_finish.argtypes = [C.c_void_p, P, P]
    L.coral_fastq_rows.argtypes = [C.c_void_p, C.c_int64, P, P, P]
    L.coral_fastq_close.argtypes = [C.c_void_p]
    for name, args in (("coral_sketch_bitmap_bytes", [C.c_int32]), ("coral_sketch_workspace_bytes", [C.c_int64]), ("coral_sketch_sort_workspace_bytes", [C.c_int64]),
                       ("coral_sketch_anchors_workspace_bytes", [C.c_int64])):
        getattr(L, name).argtypes = args
        getattr(L, name).restype = C.c_int64
    L.coral_sketch_geometry.argtypes = [P]
    L.coral_sketch_open.argtypes = [C.c_int32, C.c_int32, C.c_int32, P, P, P, C.c_int64, C.c_int64, P, C.c_int64, P, C.POINTER(C.c_void_p)]
    L.coral_sketch_feed.argtypes = [C.c_void_p, P, C.c_int64]
    L.coral_sketch_finish.argtypes = [C.c_void_p, P, P]
    L.coral_sketch_contigs.argtypes = [C.c_void_p, C.c_int64, P, C.c_int64, P, P]
    L.coral_sketch_close.argtypes = [C.c_void_p]
    L.coral_sketch_sort.argtypes = [C.c_int32, P, P, C.c_int64, C.c_int32, P, C.c_int64, P]
    L.coral_sketch_lookup.argtypes = [C.c_int32, P, C.c_int64, P, C.c_int64, P, P, P]
    L.coral_sketch_anchors.argtypes = [C.c_int32, P, P, C.c_int64, P, P, P, P, C.c_int64, C.c_int64, C.c_int64, P, P, P, C.c_int64, P, C.POINTER(C.c_int64)]
    for name in ("coral_bgzf_deflate_scratch_bytes", "coral_bgzf_pack_scratch_bytes"):
        getattr(L, name).argtypes = [C.c_int32]
        getattr(L, name).restype = C.c_int64
    for name in ("coral_bgzf_write_gpu_workspace_bytes", "coral_bgzf_write_gpu_workspace_min_bytes"):
        getattr(L, name).argtypes = []
        getattr(L, name).restype = C.c_int64
    with open(os.path.join(os.path.dirname(_HERE), "include", "coral_hip.h")) as fp:
        for name in re.findall(r"^int (coral_\w+)\(", fp.read(), re.M):      # every prototype of the header that returns int
            getattr(L, name).restype = C.c_int
    # the interval search keeps its threads for the life of the process: join them before the interpreter is torn down, so
    # that none sleeps in the library while it goes (handles still alive then compute their steps themselves)
    import atexit
    atexit.register(L.coral_search_shutdown)
    _lib = L
    return L


def check(rc: int, what: str):
    if rc != 0:
        raise CoralHipError("%s failed (%d): %s" % (what, rc, lib().coral_last_error().decode()))


_pyset_checked = False


def check_pyset_replay():
    """The native replay of the interpreter's ``set`` (coral_pyset_* / coral_reach_*) reproduces CPython's table growth and
    probing rules; another interpreter (or a future CPython with a different set) would silently give a different — still
    valid, but not reference-identical — discordant-edge order.  So the replay is checked once per process against real sets
    of str on a few hundred seeded operations, and a mismatch is an error, not a fallback."""
    global _pyset_checked
    if _pyset_checked:
        return
    import random
    L = lib()
    rnd = random.Random(12345)
    names = ["read%07d_%d" % (rnd.randrange(10 ** 7), k) for k in range(900)]
    hashes = np.array([hash(nm) for nm in names], dtype=np.int64)
    n_keys = 7
    entries = [(rnd.randrange(n_keys), rnd.randrange(len(names))) for _ in range(2500)]
    key = np.array([k for k, _ in entries], dtype=np.int32)
    item = np.array([i for _, i in entries], dtype=np.int32)
    counts = np.zeros(n_keys, dtype=np.int32)
    h = L.coral_pyset_batch_create(len(entries), key.ctypes.data, item.ctypes.data, hashes.ctypes.data, n_keys, counts.ctypes.data)
    if not h:
        raise CoralHipError("coral_pyset_batch_create failed")
    try:
        sets = {}
        for k, i in entries:
            if k in sets:
                sets[k].add(names[i])
            else:
                sets[k] = set([names[i]])
        index = {nm: i for i, nm in enumerate(names)}
        for trial in range(6):
            ks = [rnd.randrange(n_keys) for _ in range(rnd.randrange(1, 5))]
            acc = set([])
            for k in ks:
                acc |= sets.get(k, set())
            uk = np.array(ks, dtype=np.int32)
            out = np.empty(len(names) + 1, dtype=np.int32)
            n = C.c_int32(0)
            check(L.coral_pyset_union_order(h, len(uk), uk.ctypes.data, out.ctypes.data, C.byref(n)), "coral_pyset_union_order")
            if out[:n.value].tolist() != [index[nm] for nm in acc] or [int(c) for c in counts] != [len(sets.get(k, ())) for k in range(n_keys)]:
                raise CoralHipError("the native replay of this interpreter's set iteration order does not match real sets "
                                    "(libcoral_hip replays CPython 3.10-3.12 sets); refusing to emit edges in a different order")
    finally:
        L.coral_pyset_batch_free(h)
    _pyset_checked = True
