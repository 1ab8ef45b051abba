"""Read QC and a read filter from the FASTQ itself (the `qc --fastq` and `filter` modes): the length and the quality sum of every
record, and the kept records' bytes, from one pass over the text.

The reference's scripts/report_nanopore_qc.py:35-48 reads the FASTQ through ``pysam.FastxFile`` and takes ``len(sequence)`` and
``np.mean(quality)`` of every record that has a sequence; its argument parser promises a quality filter and the script has
none.  Here ``read_qc`` streams the text through the GPU (coral_fastq.hip) or the host (``device="cpu"``, coral_fastq_host.h) and
returns a ``FastqQC``; both give the same integers and write the same bytes.  The rule is coral_fastq_core.h's, stated in
DESIGN.md §4: four lines a record, no blank lines, no wrapped records.  pysam and kseq were not available to compare with: parity
with them is not pinned.
"""
from __future__ import annotations

import ctypes as C
import numbers
import os
import time

import numpy as np

from . import _lib, bam, fasta_stream

LAST_FASTQ_QC = {}                   # seconds of the last read_qc, by stage (open: the workspace, the pinned buffers and the session)
MAX_LENGTH = (1 << 31) - 1
MAX_MEAN_Q100 = 9300
UNALIGNED_MAPQ, UNALIGNED_FLAG = 255, 4      # SAM's values for an unaligned read


def min_staging() -> int:
    """The smallest ``chunk_bytes`` (coral_fastq_geometry)."""
    g = (C.c_int32 * 8)()
    fasta_stream.check(_lib.lib().coral_fastq_geometry(g), "coral_fastq_geometry")
    return int(g[4])


def _check_arguments(chunk_bytes, min_length, max_length, min_mean_quality):
    for name, v in (("min_length", min_length), ("max_length", max_length)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= v <= MAX_LENGTH:
            raise ValueError("%s must be an integer in 0 .. 2^31 - 1, got %r" % (name, v))
    if max_length and max_length < min_length:
        raise ValueError("max_length (%d) is below min_length (%d)" % (max_length, min_length))
    if isinstance(min_mean_quality, bool) or not isinstance(min_mean_quality, numbers.Real) or not min_mean_quality >= 0:
        raise ValueError("min_mean_quality must be a number of at least 0, got %r" % (min_mean_quality,))
    q100 = int(round(min_mean_quality * 100))
    if q100 > MAX_MEAN_Q100:
        raise ValueError("min_mean_quality must be at most 93, got %r" % (min_mean_quality,))
    if isinstance(chunk_bytes, bool) or not isinstance(chunk_bytes, numbers.Integral) or chunk_bytes < min_staging():
        raise ValueError("chunk_bytes must be an integer of at least %d, got %r" % (min_staging(), chunk_bytes))
    return q100


class FastqQC(bam.ReadQC):
    """A ``bam.ReadQC`` of the FASTQ's records: one entry per READ (a record with a sequence) in file order, ``length``,
    ``qual_sum`` (sum of the quality characters - 33), ``mapq`` 255 and ``flag`` 4 for every read (SAM's values for an unaligned
    one), ``base_quality_hist`` over every quality character; ``n_records`` records, ``n_reads`` = ``n_unmapped`` listed reads,
    ``n_no_seq`` records without sequence, ``total_bases``.  It adds ``kept`` (uint8 per listed read: the filter keeps it),
    ``n_kept`` (kept records, those without sequence included) and ``kept_bases``."""

    def __init__(self, length, qual_sum, kept, base_quality_hist, n_records, n_no_seq, n_kept, kept_bases):
        length = np.ascontiguousarray(length, dtype=np.int32)
        n = len(length)
        counters = dict(n_records=n_records, n_reads=n, n_secondary=0, n_supplementary=0, n_unmapped=n, n_no_seq=n_no_seq, n_no_qual=0,
                        total_bases=int(length.sum(dtype=np.int64)))
        super().__init__(length, qual_sum, np.full(n, UNALIGNED_MAPQ, dtype=np.int32), np.full(n, UNALIGNED_FLAG, dtype=np.int32), base_quality_hist, counters)
        self.kept = np.ascontiguousarray(kept, dtype=np.uint8)
        self.n_kept, self.kept_bases = int(n_kept), int(kept_bases)


def read_qc(fastq, device="cuda:0", chunk_bytes: int = 64 << 20, *, min_length: int = 0, max_length: int = 0, min_mean_quality: float = 0.0,
            output=None) -> FastqQC:
    """The length and the quality sum of every record of the FASTQ ``fastq`` - a path (one ending in .gz is read through Python's
    ``gzip`` on the host, which is slow: inflate it beforehand for a large file) or an open binary file -> ``FastqQC``.

    A record is four lines (name, sequence, separator, quality); '\\r' is skipped in the sequence and quality lines; a record
    without sequence is counted and not listed.  With ``output`` (a path or an open binary file) the bytes of every record that
    the filter keeps are written to it exactly as they were read: ``length >= min_length``, ``max_length == 0 or length <=
    max_length`` and ``100 * qual_sum >= round(min_mean_quality * 100) * length``.  The mean is the arithmetic mean of the Phred
    values, as the reference's script takes it, not a mean of error probabilities.  With no threshold the output is the input byte
    for byte.  The file is read in pieces of ``chunk_bytes``; the result does not depend on them.  On a GPU ``device`` the pieces
    go through two pinned buffers, so that reading, the upload and the kernels (k_fastq_* of coral_fastq.hip) overlap, and the
    kept bytes are written from the pinned buffer; ``device="cpu"`` is the host backend, one thread.
    ``CoralHipError``: blank lines, FASTA or wrapped records, a quality character outside 33 .. 126, a quality line that is not as
    long as its sequence, a stream that ends inside the first three lines of a record (the message names the byte).
    ``ValueError`` before any work: negative thresholds, ``max_length`` below ``min_length``, ``chunk_bytes`` below the smallest
    staging size."""
    q100 = _check_arguments(chunk_bytes, min_length, max_length, min_mean_quality)
    import torch
    L = _lib.lib()
    on_gpu = torch.device(device).type == "cuda"
    staging = min(int(chunk_bytes), 1 << 30)
    size, _ = fasta_stream.stream_size(fastq)
    if size is not None:
        staging = max(min_staging(), min(staging, size))         # (a small file needs no large pinned buffers)
    own_fd, fd = None, -1
    if output is not None:
        if hasattr(output, "fileno"):
            output.flush()
            fd = output.fileno()
        else:
            own_fd = fd = os.open(os.fspath(output), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
    LAST_FASTQ_QC.clear()
    t_all = time.perf_counter()
    handle = C.c_void_p()
    try:
        t0 = time.perf_counter()
        if on_gpu:
            dev = torch.device(device)
            hist = torch.zeros(256, dtype=torch.int64, device=dev)
            ws, stream = fasta_stream.gpu_side(dev, int(L.coral_fastq_workspace_bytes(staging)), "coral_fastq_workspace_bytes")
            rc = L.coral_fastq_open(dev.index or 0, int(min_length), int(max_length), q100, fd, staging, hist.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream,
                                    C.byref(handle))
        else:
            hist = np.zeros(256, dtype=np.uint64)
            rc = L.coral_fastq_open(-1, int(min_length), int(max_length), q100, fd, 0, hist.ctypes.data, None, 0, None, C.byref(handle))
        fasta_stream.check(rc, "coral_fastq_open")
        open_s = time.perf_counter() - t0
        stats, secs = (C.c_int64 * 8)(), (C.c_double * 4)()
        try:
            read_s, feed_s = fasta_stream.feed_all(L.coral_fastq_feed, handle, fastq, chunk_bytes)
            t0 = time.perf_counter()
            fasta_stream.check(L.coral_fastq_finish(handle, stats, secs), "coral_fastq_finish")
            finish_s = time.perf_counter() - t0
            n_reads = int(stats[1])
            length, qual_sum, kept = np.zeros(n_reads, dtype=np.int32), np.zeros(n_reads, dtype=np.int64), np.zeros(n_reads, dtype=np.uint8)
            fasta_stream.check(L.coral_fastq_rows(handle, n_reads, length.ctypes.data, qual_sum.ctypes.data, kept.ctypes.data), "coral_fastq_rows")
        finally:
            t0 = time.perf_counter()
            L.coral_fastq_close(handle)
            close_s = time.perf_counter() - t0
    finally:
        if own_fd is not None:
            os.close(own_fd)
    host_hist = hist.cpu().numpy() if on_gpu else hist.astype(np.int64)
    LAST_FASTQ_QC.update(open=open_s, close=close_s, read=read_s, feed=feed_s, finish_wait=finish_s, upload=float(secs[0]), scan_walk=float(secs[1]), accumulate=float(secs[2]), write=float(secs[3]),
                         wall=time.perf_counter() - t_all)
    return FastqQC(length, qual_sum, kept, host_hist, int(stats[0]), int(stats[2]), int(stats[4]), int(stats[5]))
