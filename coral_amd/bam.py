"""BAM input/output for the graph-build path.

``decode_bam`` is the product path: the native multi-threaded BGZF/BAM decoder of libcoral_hip.so
(csrc/coral_bam.cpp) turns the file into the SoA ``Records`` the kernels consume — the BAM is read once.
``write_bam`` is a small pure-Python BAM writer used by tests and tools to materialise synthetic records as a
real coordinate-sorted BAM (htslib / pysam are not available offline); it is not on the hot path.
"""
from __future__ import annotations

import array
import collections
import contextlib
import ctypes as C
import gzip
import numbers
import os
import struct
import time
import zlib
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .decode_session import BamFile, DecodeSession, Runs, TextFile
from .names import NameTable
from .synth import Records, hash_u32, S_SEQ, sa_entry_string


def default_threads() -> int:
    """Decoder threads: the CPUs this process may actually use (affinity mask and, in a container, the cgroup CPU quota)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, min(64, n))


LAST_DECODE = {}      # statistics of the last decode_bam call (bench.py): seconds, compressed / uncompressed bytes, threads


class RecordFilter(collections.namedtuple("RecordFilter", "min_mapq min_seq_length require_flags exclude_flags")):
    """Which records a decode keeps (``record_filter=`` of every decode here): ``mapq >= min_mapq`` (samtools view -q), ``l_seq >=
    min_seq_length`` (the stored sequence; a record without SEQ has length 0), ``flag & require_flags == require_flags`` (-f) and
    ``flag & exclude_flags == 0`` (-F).  Every result of a filtered decode is that of the same call on a BAM file that holds only
    the kept records, in the same order; a dropped record costs nothing behind the decode's boundary walk.  The reference's
    preparation step ``samtools view -h | awk 'length($10) > 1000' | samtools view -bSq 25`` is ``RecordFilter(25, 1001)``.
    ValueError for values outside 0..255, 0..2^29, 0..0xffff, 0..0xffff."""
    __slots__ = ()

    def __new__(cls, min_mapq=0, min_seq_length=0, require_flags=0, exclude_flags=0):
        for name, v, top in (("min_mapq", min_mapq, 255), ("min_seq_length", min_seq_length, 1 << 29),
                             ("require_flags", require_flags, 0xffff), ("exclude_flags", exclude_flags, 0xffff)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral):
                raise ValueError("%s must be an integer, got %r" % (name, v))
            if not 0 <= v <= top:
                raise ValueError("%s must be in 0..%d, got %r" % (name, top, v))
        return super().__new__(cls, int(min_mapq), int(min_seq_length), int(require_flags), int(exclude_flags))

    @property
    def active(self) -> bool:
        return any(self)


def _as_filter(record_filter) -> Optional[RecordFilter]:
    """None, a RecordFilter or a 4-tuple -> a checked RecordFilter, or None when it keeps everything."""
    if record_filter is None:
        return None
    f = record_filter if isinstance(record_filter, RecordFilter) else RecordFilter(*record_filter)
    return f if f.active else None


def record_filter_from_args(args) -> RecordFilter:
    """The RecordFilter of a command line's argument object (--filter_min_mapq, --filter_min_length, --filter_require_flags,
    --filter_exclude_flags of CoRAL.py); an object without these attributes gives the filter that keeps everything."""
    return RecordFilter(getattr(args, "filter_min_mapq", 0), getattr(args, "filter_min_length", 0),
                        getattr(args, "filter_require_flags", 0), getattr(args, "filter_exclude_flags", 0))


def decode_bam(path: str, n_threads: Optional[int] = None, rank: int = 0, world: int = 1, *, record_filter=None) -> Records:
    """Decode the BAM file (or, with ``world`` > 1, the ``rank``-th of ``world`` byte ranges of it: one process per GPU, every
    rank inflates and parses only its share; consecutive ranges neither drop nor repeat a record).  Read-name ids are local
    to the returned records.  ``record_filter``: a ``RecordFilter`` - only the records it keeps."""
    return _decode(path, "cpu", n_threads=n_threads, rank=rank, world=world, record_filter=record_filter).records


def _on_gpu(device) -> bool:
    return torch.device(device).type == "cuda" and os.environ.get("CORAL_BAM_DECODE", "gpu") != "cpu"


def load_bam(path: str, device="cuda:0", n_threads: Optional[int] = None, rank: int = 0, world: int = 1, *, regions=None,
             index=None, record_filter=None) -> Records:
    """The product's way from a BAM file to records: inflate and parse on the GPU (``decode_bam_gpu``) when ``device`` is one;
    ``CORAL_BAM_DECODE=cpu`` selects the host pipeline (``decode_bam``: same result, CIGAR words in host memory).

    ``regions`` = [(chrom, start, stop), ...]: only the records pysam's ``fetch`` returns for them (on the contig, ``pos < stop
    and end > start``), each once, in file order, read-name ids numbered by first appearance among them — through the BAI index
    ``index`` (a path, an object of ``read_index``, or None for the file next to the BAM, which must then be usable): only the
    BGZF blocks the index names are read and inflated; records a chunk carries that meet no region are dropped on the host.

    ``record_filter``: a ``RecordFilter`` - the result is that of a file holding only the records it keeps (dropped inside the
    decode; with ``regions`` the region test runs on the host afterwards, on the kept records)."""
    if regions is None:
        if _on_gpu(device):
            return decode_bam_gpu(path, device, n_threads=n_threads, rank=rank, world=world, record_filter=record_filter)
        return decode_bam(path, n_threads=n_threads, rank=rank, world=world, record_filter=record_filter)
    if world != 1:
        raise ValueError("a region decode is not sharded (world must be 1)")
    if index is False:
        raise ValueError("load_bam(regions=...) needs an index: pass its path, an object of read_index, or None for the file beside the BAM")
    names = bam_reference_names(path)
    idx = _usable_index(path, index if index is not None else _index_beside(path, must=True), len(names))
    reg = _regions_as_tids(regions, names)
    # (an empty region start == stop keeps, by the rule above, the records that span the point)
    spans = region_spans(idx, [(t, a, max(b, a + 1)) for t, a, b in reg])
    rec = _decode_spans(path, spans, device, n_threads, 0, record_filter)
    keep = np.zeros(rec.n, dtype=bool)
    tid, pos, end = rec.tid.numpy(), rec.pos.numpy(), rec.end.numpy()
    for t, a, b in reg:
        keep |= (tid == t) & (pos < b) & (end > a)
    return select_records(rec, keep)


def select_records(rec: Records, keep) -> Records:
    """The records ``rec[keep]`` (boolean mask) in their order: read-name ids renumbered by first appearance, ragged columns
    re-packed (the CIGAR words on the device they are on)."""
    keep = np.asarray(keep, dtype=bool)
    ids = np.nonzero(keep)[0]
    t = torch.from_numpy
    take = lambda x: t(np.ascontiguousarray(x.numpy()[ids]))

    def ragged(off, data, width=1):
        off = off.numpy()
        lens = off[ids + 1] - off[ids]
        new_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        src = np.repeat(off[ids] - new_off[:-1], lens) + np.arange(int(new_off[-1]), dtype=np.int64)
        return t(new_off), src
    cigar_off, cig_src = ragged(rec.cigar_off, rec.cigar)
    cigar = rec.cigar[t(cig_src).to(rec.cigar.device)] if len(cig_src) else rec.cigar[:0]
    sa_off, sa_src = ragged(rec.sa_off, rec.sa)
    na_keep = keep[rec.nonacgt_rec.numpy()] if rec.nonacgt_rec.numel() else np.zeros(0, dtype=bool)
    new_ordinal = np.cumsum(keep) - 1
    old_ids = rec.name_id.numpy()[ids]
    uniq, first, inv = np.unique(old_ids, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                     # name ids in order of first appearance among the kept
    rank_of = np.empty(len(uniq), dtype=np.int64)
    rank_of[order] = np.arange(len(uniq))
    names = rec.names
    if isinstance(names, NameTable):
        old = uniq[order]
        lens = names.off[old + 1] - names.off[old]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        src = np.repeat(names.off[old] - off[:-1], lens) + np.arange(int(off[-1]), dtype=np.int64)
        names = NameTable(names.blob[src] if len(src) else np.zeros(0, dtype=np.uint8), off)
    else:
        all_names = rec.materialise_names()
        names = [all_names[k] for k in uniq[order]]
    return Records(n=len(ids), tid=take(rec.tid), pos=take(rec.pos), end=take(rec.end), flag=take(rec.flag), mapq=take(rec.mapq),
                   qlen=take(rec.qlen), has_seq=take(rec.has_seq), nm=take(rec.nm), name_id=t(rank_of[inv].astype(np.int32)),
                   n_cigar=take(rec.n_cigar), cigar_off=cigar_off, cigar=cigar, sa_off=sa_off,
                   sa=t(np.ascontiguousarray(rec.sa.numpy()[sa_src])), sa_nm=t(np.ascontiguousarray(rec.sa_nm.numpy()[sa_src])),
                   nonacgt_rec=t(new_ordinal[rec.nonacgt_rec.numpy()[na_keep]].astype(np.int64)),
                   nonacgt_pos=t(np.ascontiguousarray(rec.nonacgt_pos.numpy()[na_keep])), n_names=len(uniq), name_gid=None, names=names,
                   header_chroms=list(rec.header_chroms), header_lens=list(rec.header_lens))


def _records_from_handle(L, h, cigar, cigar_words: int) -> Records:
    """Fill a Records object from a decode handle (coral_bam_decode_sizes / _fill).  ``cigar`` None: the handle holds the op
    words (CPU pipeline); a tensor: the ops are already on the device (GPU pipeline) and the handle holds everything else."""
    sz = (C.c_int64 * 8)()
    _lib.check(L.coral_bam_decode_sizes(h, sz), "coral_bam_decode_sizes")
    n, ncig, nsa, nna, nnames, nbytes, nref, rbytes = (int(v) for v in sz)
    i32 = lambda k: np.empty(max(k, 0), dtype=np.int32)
    tid, pos, end, flag, mapq, qlen, has_seq, nm, name_id, n_cigar = (i32(n) for _ in range(10))
    cigar_off = np.empty(n + 1, dtype=np.int64)
    host_cigar = np.empty(ncig, dtype=np.uint32) if cigar is None else None
    sa_off = np.empty(n + 1, dtype=np.int64)
    sa = np.empty((nsa, 8), dtype=np.int32)
    sa_nm = i32(nsa)
    na_rec = np.empty(nna, dtype=np.int64)
    na_pos = i32(nna)
    names_blob = np.empty(max(nbytes, 1), dtype=np.uint8)
    name_off = np.zeros(nnames + 1, dtype=np.int64)
    ref_buf = C.create_string_buffer(max(rbytes, 1))
    ref_lens = i32(nref)
    ptr = lambda a: a.ctypes.data
    _lib.check(L.coral_bam_decode_fill(h, ptr(tid), ptr(pos), ptr(end), ptr(flag), ptr(mapq), ptr(qlen), ptr(has_seq),
                                       ptr(nm), ptr(name_id), ptr(n_cigar), ptr(cigar_off), ptr(host_cigar) if host_cigar is not None else None,
                                       ptr(sa_off), ptr(sa), ptr(sa_nm), ptr(na_rec), ptr(na_pos), ptr(names_blob),
                                       ptr(name_off), C.addressof(ref_buf), ptr(ref_lens)), "coral_bam_decode_fill")
    names = NameTable(names_blob[:nbytes], name_off)                  # the names stay bytes: a str is made when one is asked for
    refs = ref_buf.raw[:rbytes].split(b"\0")[:nref]
    t = torch.from_numpy
    if cigar is None:
        cigar = t(host_cigar.view(np.int32))
    else:
        assert int(cigar_off[-1]) == cigar_words, "device CIGAR words and host offsets disagree"
    return Records(n=n, tid=t(tid), pos=t(pos), end=t(end), flag=t(flag), mapq=t(mapq), qlen=t(qlen), has_seq=t(has_seq),
                   nm=t(nm), name_id=t(name_id), n_cigar=t(n_cigar), cigar_off=t(cigar_off),
                   cigar=cigar, sa_off=t(sa_off), sa=t(sa), sa_nm=t(sa_nm), nonacgt_rec=t(na_rec),
                   nonacgt_pos=t(na_pos), n_names=nnames, name_gid=None, names=names,
                   header_chroms=[x.decode() for x in refs], header_lens=[int(x) for x in ref_lens])


def decode_bam_gpu(path: str, device="cuda:0", n_threads: Optional[int] = None, rank: int = 0, world: int = 1,
                   batch_bytes: int = 0, *, record_filter=None) -> Records:
    """The same result as ``decode_bam`` with the inflate and the record parsing on the GPU (csrc/coral_bamgpu.hip): the host
    only reads the file and uploads COMPRESSED bytes; the CIGAR words of the returned Records are a device tensor (they never
    exist in host memory), everything else is host-side as before.  ``batch_bytes``: inflated bytes per batch (0 = the default, 2.52 GiB).
    ``record_filter``: a ``RecordFilter`` (k_bam_keep / k_bam_keep_compact per batch, in front of the record parse)."""
    if torch.device(device).type != "cuda":
        raise _lib.CoralHipError("decode_bam_gpu needs a GPU device (the CPU pipeline is decode_bam)")
    return _decode_gpu(path, device, n_threads, batch_bytes, _lib.bam_request(rank, world, keep=_as_filter(record_filter)), True).records      # (whatever CORAL_BAM_DECODE says)


class DecodeResult(collections.namedtuple("DecodeResult", "records counts index qc")):
    """What _decode returns; what it was not asked for is None.  It unpacks as these four; the table of a pileup request
    (uint32 [positions][4]) is the attribute ``pileup``, the result of a binned-depth request the attribute ``depth``
    (bin_off int64 [contigs + 1], bases and reads int64 [bins]), the result of a reads request the attribute ``reads`` (text - in
    mode 2 the records' bytes - uint8, offsets int64 [records + 1])."""
    pileup = None
    depth = None
    reads = None


def _decode(path: str, device, *, n_threads: Optional[int] = None, rank: int = 0, world: int = 1, batch_bytes: int = 0, spans=None,
            coverage=None, index=False, qc=False, records=True, per_base=False, depth=None, record_filter=None, reads=None,
            sink=None) -> DecodeResult:
    """One decode of the ``rank``-th of ``world`` byte ranges, or of the records that start inside ``spans`` (uint64 [K][2] virtual
    offsets), with what rides along: ``coverage`` = (segments int32 [3][S], quality threshold, read_callback code) gives the S
    int64 ``counts``, ``index`` the partial BAI index, ``qc`` the ``ReadQC``; ``records`` False leaves the Records out.  With
    ``per_base`` the coverage is counted per position and base: ``pileup`` is the uint32 table [positions of the segments, in
    segment order][A, C, G, T] and ``counts`` its sums per segment.  ``depth`` = (bin size, min_mapq, exclude_flags,
    count_deletions) gives the binned-depth tables (``binned_depth``), ``reads`` = (exclude_flags, segments or None, sorted names or
    None[, mode]) the FASTQ text of the selected records (``extract_reads``) or, with mode 2, their own bytes (``extract_records``).  ``record_filter``: a ``RecordFilter``; every result is
    then that of a file holding only the kept records.  On the GPU pipeline when ``_on_gpu(device)``, else on the host.
    ``sink`` = BamFile(output path, inflated header, chunk_blocks): the records of a mode-2 reads request go to that BAM file while
    the decode runs (GPU pipeline only, whatever CORAL_BAM_DECODE says); ``reads`` is then (records, bytes, file bytes, members).
    ``sink`` = TextFile(output path): the FASTQ text of a mode-1 request goes to that plain file, batch by batch."""
    req = _lib.bam_request(rank, world, spans, coverage, index, qc, per_base, depth, keep=_as_filter(record_filter), reads=reads)
    if sink is not None and torch.device(device).type != "cuda":
        raise ValueError("a decode that writes its records to a file runs on a GPU device, got %r" % (device,))
    if _on_gpu(device) or sink is not None:
        return _decode_gpu(path, device, n_threads, batch_bytes, req, records, sink)
    L = _lib.lib()
    if n_threads is None:
        n_threads = default_threads()
    h = C.c_void_p()
    rc = L.coral_bam_decode_request(path.encode(), n_threads, C.byref(req), C.byref(h))
    if rc != 0:
        raise _lib.CoralHipError("coral_bam_decode_request(%s) failed (%d): %s" % (path, rc, L.coral_bam_last_error().decode()))
    try:
        _host_stats(L, h, n_threads)
        return _result_from_handle(L, h, req, records, None, 0)
    finally:
        L.coral_bam_decode_close(h)


def _host_stats(L, h, n_threads):
    st, secs = (C.c_int64 * 3)(), C.c_double(0.0)
    L.coral_bam_decode_stats(h, st, C.byref(secs))
    LAST_DECODE.clear()
    LAST_DECODE.update(seconds=float(secs.value), compressed_bytes=int(st[0]), uncompressed_bytes=int(st[1]), blocks=int(st[2]),
                       threads=int(n_threads))


def _result_from_handle(L, h, req, records: bool, cigar, cigar_words: int, reads_on_host: bool = True) -> DecodeResult:
    """What ``req`` asked for, read from a decode handle of either pipeline (``cigar``: see _records_from_handle); not the reads
    request's result when it went to a file (``reads_on_host`` False)."""
    counts = None
    if req.n_seg >= 0:
        counts = np.zeros(req.n_seg, dtype=np.int64)
        _lib.check(L.coral_bam_coverage_result(h, req.n_seg, counts.ctypes.data), "coral_bam_coverage_result")
    table = None
    if req.per_base:
        seg_start, seg_end = req.arrays[-2], req.arrays[-1]      # (bam_request puts the segment rows last)
        n_pos = int((seg_end.astype(np.int64) - seg_start).sum())
        table = np.zeros((n_pos, 4), dtype=np.uint32)
        if L.coral_bam_pileup_result(h, n_pos, table.ctypes.data) != 0:
            raise _lib.CoralHipError("coral_bam_pileup_result failed: %s" % L.coral_bam_last_error().decode())
    res = DecodeResult(_records_from_handle(L, h, cigar, cigar_words) if records else None, counts,
                       _index_partial_from_handle(L, h) if req.want_index else None, _read_qc_from_handle(L, h) if req.want_qc else None)
    res.pileup = table
    if req.depth_bin:
        sz = (C.c_int64 * 2)()
        if L.coral_bam_depth_sizes(h, sz) != 0:
            raise _lib.CoralHipError("coral_bam_depth_sizes failed: %s" % L.coral_bam_last_error().decode())
        bin_off, bases, reads = np.zeros(int(sz[0]) + 1, dtype=np.int64), np.zeros(int(sz[1]), dtype=np.int64), np.zeros(int(sz[1]), dtype=np.int64)
        if L.coral_bam_depth_fill(h, bin_off.ctypes.data, bases.ctypes.data, reads.ctypes.data) != 0:
            raise _lib.CoralHipError("coral_bam_depth_fill failed: %s" % L.coral_bam_last_error().decode())
        res.depth = (bin_off, bases, reads)
    if req.want_reads and reads_on_host:
        sz = (C.c_int64 * 2)()
        if L.coral_bam_reads_sizes(h, sz) != 0:
            raise _lib.CoralHipError("coral_bam_reads_sizes failed: %s" % L.coral_bam_last_error().decode())
        text, offsets = np.zeros(int(sz[1]), dtype=np.uint8), np.zeros(int(sz[0]) + 1, dtype=np.int64)
        if L.coral_bam_reads_fill(h, text.ctypes.data, offsets.ctypes.data) != 0:
            raise _lib.CoralHipError("coral_bam_reads_fill failed: %s" % L.coral_bam_last_error().decode())
        res.reads = (text, offsets)
    return res


def _decode_gpu(path: str, device, n_threads: Optional[int], batch_bytes: int, req, records: bool, sink=None) -> DecodeResult:
    """The GPU pipeline of _decode: one DecodeSession (``sink``: where the reads request's result goes instead of the host).  The
    CIGAR words stay on the device only when ``records`` asks for them."""
    if n_threads is None:
        n_threads = default_threads()
    with DecodeSession(path, req, device=device, n_threads=n_threads, batch_bytes=batch_bytes, sink=sink) as s:
        s.start()
        s.run(keep=records)
        dh = s.finish()
        cigar = s.cigar() if records else None
        LAST_DECODE.clear()
        LAST_DECODE.update(s.stats())
        res = _result_from_handle(s.L, dh, req, records, cigar, cigar.numel() if records else 0, reads_on_host=sink is None)
        if sink is not None:                                     # (nothing of the reads request is on the host: coral_bam_reads_fill refuses)
            res.reads = s.sink_stats()
        return res


# ----------------------------------------------------------------------------------------------
# window coverage with a base-quality threshold (the coverage track of `plot`)
# ----------------------------------------------------------------------------------------------
_READ_CALLBACKS = {"nofilter": 0, "all": 1}
_I32_MAX = (1 << 31) - 1


def bam_reference_names(path: str):
    """Contig names of a BAM file's header, in tid order (read with gzip: BGZF is a series of gzip members)."""
    with gzip.open(path, "rb") as fp:
        def take(n):
            b = fp.read(n)
            if len(b) != n:
                raise _lib.CoralHipError("%s: truncated BAM header" % path)
            return b
        if take(4) != b"BAM\x01":
            raise _lib.CoralHipError("%s: not a BAM file" % path)
        take(struct.unpack("<i", take(4))[0])
        names = []
        for _ in range(struct.unpack("<i", take(4))[0]):
            names.append(take(struct.unpack("<i", take(4))[0]).rstrip(b"\0").decode())
            take(4)
        return names


def quality_threshold_value(quality_threshold) -> int:
    """The base-quality threshold as an int in 0..255.  Integer-valued floats (``20.0``: the reference passes a float) are
    accepted; a fractional value raises ValueError (what pysam does with one is not pinned here)."""
    if isinstance(quality_threshold, numbers.Integral):
        v = int(quality_threshold)
    elif isinstance(quality_threshold, numbers.Real) and float(quality_threshold).is_integer():
        v = int(quality_threshold)
    else:
        raise ValueError("quality_threshold must be an integer in 0..255, got %r" % (quality_threshold,))
    if not 0 <= v <= 255:
        raise ValueError("quality_threshold must be an integer in 0..255, got %r" % (quality_threshold,))
    return v


def coverage_segments(windows, ref_names: Sequence[str]):
    """Windows (chrom, start, stop) -> (segments int32 [3][S]: tid, start, end of the sorted, disjoint pieces the windows are
    cut into at every start and stop; first, last int64 [W]: window w is the sum of the segments first[w]:last[w])."""
    tid_of = {c: k for k, c in enumerate(ref_names)}
    W = len(windows)
    tid, lo, hi = np.empty(W, dtype=np.int64), np.empty(W, dtype=np.int64), np.empty(W, dtype=np.int64)
    for k, w in enumerate(windows):
        if len(w) != 3:
            raise ValueError("a window is (chrom, start, stop), got %r" % (w,))
        chrom, a, b = w
        if chrom not in tid_of:
            raise ValueError("unknown contig %r" % (chrom,))
        a, b = int(a), int(b)
        if a < 0 or b < a:
            raise ValueError("bad window %r: needs 0 <= start <= stop" % (w,))
        tid[k], lo[k], hi[k] = tid_of[chrom], min(a, _I32_MAX), min(b, _I32_MAX)
    key_lo, key_hi = (tid << 32) | lo, (tid << 32) | hi
    cuts = np.unique(np.concatenate([key_lo, key_hi]))
    delta = np.zeros(len(cuts) + 1, dtype=np.int64)
    np.add.at(delta, np.searchsorted(cuts, key_lo), 1)
    np.add.at(delta, np.searchsorted(cuts, key_hi), -1)
    covered = np.cumsum(delta)[:max(len(cuts) - 1, 0)] > 0          # piece k = [cuts[k], cuts[k + 1]) lies inside some window
    keep = covered & ((cuts[:-1] >> 32) == (cuts[1:] >> 32))
    s_lo, s_hi = cuts[:-1][keep], cuts[1:][keep]
    segs = np.stack([s_lo >> 32, s_lo & 0xffffffff, s_hi & 0xffffffff]).astype(np.int32).reshape(3, -1)
    return segs, np.searchsorted(s_lo, key_lo), np.searchsorted(s_lo, key_hi)


def window_coverage(path: str, windows: Sequence[Tuple[str, int, int]], quality_threshold=0, read_callback: str = "nofilter",
                    device="cuda:0", rank: int = 0, world: int = 1, batch_bytes: int = 0, n_threads: Optional[int] = None, *,
                    index=None, record_filter=None) -> np.ndarray:
    """pysam ``AlignmentFile.count_coverage(chrom, start, stop, quality_threshold=..., read_callback=...)`` summed over its four
    arrays, for every window (chrom, start, stop) of ``windows`` (in that order, may overlap), as exact int64 — counted while
    the BAM is decoded, the only time SEQ and QUAL are at hand.

    A base counts when its read is on the window's contig (``read_callback='all'``: none of the flags 0x4 | 0x100 | 0x200 |
    0x400; ``'nofilter'``: every read), has SEQ, it is an aligned base of an M / = / X op (the CG:B,I CIGAR for the
    placeholder) inside the window, its SEQ code is A, C, G or T, and ``quality_threshold`` is 0 or the read has QUAL (first
    byte not 0xff; else pysam's query_qualities is None) with QUAL >= the threshold there.  The threshold is an integer in
    0..255 (``20.0`` is accepted; a fractional value raises ValueError — pysam's own handling of one is not pinned here).  An
    unknown contig or a window with start < 0 or stop < start raises ValueError.

    The GPU pipeline (csrc/coral_bamgpu.hip: k_bam_cov_plan / k_bam_cov_count per batch) runs on a GPU ``device``; the host
    pipeline (coral_bam_decode_request) otherwise, or with ``CORAL_BAM_DECODE=cpu``.  With ``world`` > 1 the counts are those
    of the ``rank``-th byte range; the ranges' counts add up to the whole file's.

    ``index``: a BAI index restricts the decode to the BGZF blocks it names for the windows (``region_spans``); the counts are
    the same.  None (default): the index beside the file (``path + ".bai"`` or ``path[:-4] + ".bai"``) when it is a valid BAI,
    fits the header and is not older than the BAM, else the whole file as before (``LAST_DECODE["index"]`` says which: the
    index's path, or None with ``LAST_DECODE["index_skipped"]`` giving the reason an existing file was not used); False:
    never; a path or an object of ``read_index``: must be usable, or the call raises.  With ``world`` > 1 an index raises
    ValueError (a region decode is not sharded), unless it is the default one, which is then not looked for.

    ``record_filter``: a ``RecordFilter`` - only the records it keeps are counted."""
    thr = quality_threshold_value(quality_threshold)
    if read_callback not in _READ_CALLBACKS:
        raise ValueError("read_callback must be 'nofilter' or 'all', got %r" % (read_callback,))
    cb = _READ_CALLBACKS[read_callback]
    ref_names = bam_reference_names(path)
    segs, first, last = coverage_segments(list(windows), ref_names)
    S = segs.shape[1]
    if n_threads is None:
        n_threads = default_threads()
    res = _decode_segments(path, segs, thr, cb, device, rank, world, batch_bytes, n_threads, index, len(ref_names), False, record_filter)
    counts = res.counts if res is not None else np.zeros(S, dtype=np.int64)
    csum = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    return (csum[last] - csum[first]).astype(np.int64)


def _decode_segments(path, segs, thr, cb, device, rank, world, batch_bytes, n_threads, index, n_ref, per_base, record_filter=None):
    """The decode behind ``window_coverage`` and ``pileup``: the coverage request of ``segs``, through the BAI index ``index`` (the
    rules of ``window_coverage``) when there is one.  None when the index names no block for the segments: nothing was decoded
    and every count is 0.  ``LAST_DECODE`` says which index was used."""
    idx, skipped = _index_choice(path, index, world, n_ref)
    regions = []
    if idx is not None:                                          # the segments, neighbours within one linear-index window joined
        for t, a, b in segs.T.tolist():
            if regions and regions[-1][0] == t and a - regions[-1][2] < 16384:
                regions[-1][2] = b
            else:
                regions.append([t, a, b])
    return _decode_regions(idx, skipped, regions, n_threads, lambda spans: _decode(
        path, device, n_threads=n_threads, rank=rank, world=world, batch_bytes=batch_bytes, spans=spans, coverage=(segs, thr, cb), records=False,
        per_base=per_base, record_filter=record_filter))


def _index_choice(path, index, world, n_ref):
    """Which BAI index a region decode of ``path`` uses, under the rules of ``window_coverage``: a given one (a path or an object
    of ``read_index``) must be usable and does not go with ``world`` > 1; None looks beside the file, unless ``world`` > 1, and
    takes what it finds when it is usable and not older than the BAM; False: none -> (the index or None, the reason an existing
    index beside the file was skipped or None)."""
    if index is not None and index is not False:
        if world != 1:
            raise ValueError("a region decode is not sharded: index and world > 1 do not go together")
        return _usable_index(path, index, n_ref), None
    beside = _index_beside(path) if index is None and world == 1 else None
    if beside is None:
        return None, None
    try:
        if os.path.getmtime(beside) < os.path.getmtime(path):
            raise _lib.CoralHipError("%s is older than the BAM file" % beside)
        return _usable_index(path, beside, n_ref), None
    except (_lib.CoralHipError, OSError) as e:
        return None, str(e)


def _decode_regions(idx, skipped, regions, n_threads, decode):
    """``decode(spans)`` for the spans the index ``idx`` names for ``regions`` (no index: ``decode(None)``, the whole file) -> its
    result, or None when the index names no block: nothing is decoded then.  Either way ``LAST_DECODE`` says which index was used."""
    spans = region_spans(idx, regions) if idx is not None else None
    res = None
    if spans is not None and len(spans) == 0:
        LAST_DECODE.clear()
        LAST_DECODE.update(seconds=0.0, compressed_bytes=0, uncompressed_bytes=0, blocks=0, threads=int(n_threads))
    else:
        res = decode(spans)
    if idx is not None:
        LAST_DECODE.update(index=idx.path or "<object>", spans=int(len(spans)))
    else:
        LAST_DECODE.update(index=None, index_skipped=skipped)
    return res


# ----------------------------------------------------------------------------------------------
# pileup: the bases per position (A / C / G / T), counted during the decode
# ----------------------------------------------------------------------------------------------
PILEUP_MAX_POSITIONS = 1 << 28


class Pileup:
    """pysam ``count_coverage`` itself - the four per-position arrays - for the regions of one decode (``pileup``): a stand-in for
    the reference's ``lr_bamfh`` that answers ANY window inside the loaded regions, at any resolution.  ``regions`` = the merged
    regions [(chrom, start, stop)] in (contig, start) order, ``table`` uint32 [positions of the regions, in that order][A, C, G, T]."""

    def __init__(self, regions, table, quality_threshold=0, read_callback="nofilter"):
        self.regions = [(c, int(a), int(b)) for c, a, b in regions]
        self.quality_threshold = quality_threshold_value(quality_threshold)
        self.read_callback = read_callback
        self.table = np.ascontiguousarray(table, dtype=np.uint32).reshape(-1, 4)
        self._off = np.concatenate([[0], np.cumsum([b - a for _, a, b in self.regions])]).astype(np.int64)
        if int(self._off[-1]) != len(self.table):
            raise ValueError("Pileup: the regions hold %d positions, the table %d" % (int(self._off[-1]), len(self.table)))

    def _rows(self, chrom, start, stop):
        start, stop = int(start), int(stop)
        if stop >= start:
            for k, (c, a, b) in enumerate(self.regions):
                if c == chrom and a <= start and stop <= b:
                    return self.table[self._off[k] + start - a:self._off[k] + stop - a]
        raise KeyError("%s:%d-%d is not inside one loaded region" % (chrom, start, stop))

    def counts(self, chrom, start, stop) -> np.ndarray:
        """int64 [4][stop - start]: the counted A, C, G and T bases at every position of [start, stop).  KeyError when the range
        is not inside one loaded region."""
        return np.ascontiguousarray(self._rows(chrom, start, stop).T, dtype=np.int64)

    def depth(self, chrom, start, stop) -> np.ndarray:
        """int64 [stop - start]: the sum over the four bases."""
        return self._rows(chrom, start, stop).sum(axis=1, dtype=np.int64)

    def count_coverage(self, contig, start=None, stop=None, region=None, quality_threshold=15, read_callback="all"):
        """pysam's signature and defaults: four ``array.array('L')`` (A, C, G, T) of ``stop - start`` counts.  ``region`` is a
        samtools region string ('chr:start-stop', 1-based, inclusive).  ValueError when the threshold or the callback is not
        what was counted, KeyError when the range is not inside one loaded region."""
        if quality_threshold_value(quality_threshold) != self.quality_threshold or read_callback != self.read_callback:
            raise ValueError("this Pileup was counted with quality_threshold=%d, read_callback=%r"
                             % (self.quality_threshold, self.read_callback))
        if region is not None:
            contig, span = region.rsplit(":", 1)
            a, b = span.replace(",", "").split("-")
            start, stop = int(a) - 1, int(b)
        if contig is None or start is None or stop is None:
            raise KeyError("Pileup answers (contig, start, stop) ranges only")
        return tuple(array.array("L", row.tolist()) for row in self.counts(contig, start, stop))

    def close(self):
        self.regions, self.table, self._off = [], np.zeros((0, 4), dtype=np.uint32), np.zeros(1, dtype=np.int64)


def pileup_regions(regions, ref_names: Sequence[str]):
    """Regions (chrom, start, stop), which may overlap or touch -> (the merged, non-empty regions in (contig, start) order,
    their segments int32 [3][S]).  Argument errors as ``window_coverage``."""
    reg = sorted((t, min(a, _I32_MAX), min(b, _I32_MAX)) for t, a, b in _regions_as_tids(regions, ref_names))
    merged = []
    for t, a, b in reg:
        if a == b:
            continue
        if merged and merged[-1][0] == t and a <= merged[-1][2]:
            merged[-1][2] = max(merged[-1][2], b)
        else:
            merged.append([t, a, b])
    segs = np.array(merged, dtype=np.int32).reshape(-1, 3).T.copy()
    return [(ref_names[t], a, b) for t, a, b in merged], segs


def pileup(path: str, regions: Sequence[Tuple[str, int, int]], quality_threshold=0, read_callback: str = "nofilter", device="cuda:0",
           rank: int = 0, world: int = 1, batch_bytes: int = 0, n_threads: Optional[int] = None, *, index=None,
           record_filter=None) -> Pileup:
    """pysam ``count_coverage`` per position and base for ``regions`` [(chrom, start, stop)] (they may overlap or touch and are
    merged; at most 2^28 positions in all), counted while the BAM is decoded.  The counting rule, ``quality_threshold``,
    ``read_callback``, ``index``, ``rank`` / ``world`` and the choice of the pipeline are ``window_coverage``'s: a base that
    counts there adds 1 to its position's A, C, G or T here (GPU: k_bam_cov_plan / k_bam_pileup per batch).  With ``world`` > 1
    the table is that of the ``rank``-th byte range; ``merge_pileups`` adds them.  ``record_filter``: a ``RecordFilter`` - only
    the records it keeps are counted."""
    thr = quality_threshold_value(quality_threshold)
    if read_callback not in _READ_CALLBACKS:
        raise ValueError("read_callback must be 'nofilter' or 'all', got %r" % (read_callback,))
    ref_names = bam_reference_names(path)
    merged, segs = pileup_regions(list(regions), ref_names)
    n_pos = sum(b - a for _, a, b in merged)
    if n_pos > PILEUP_MAX_POSITIONS:
        raise ValueError("the regions hold %d positions: a pileup takes at most 2^28" % n_pos)
    if n_threads is None:
        n_threads = default_threads()
    res = _decode_segments(path, segs, thr, _READ_CALLBACKS[read_callback], device, rank, world, batch_bytes, n_threads, index,
                           len(ref_names), True, record_filter)
    return Pileup(merged, res.pileup if res is not None else np.zeros((n_pos, 4), dtype=np.uint32), thr, read_callback)


def merge_pileups(parts: Sequence[Pileup]) -> Pileup:
    """The tables of byte ranges decoded by several ranks, added.  The parts must hold the same regions, counted alike."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_pileups needs at least one part")
    first = parts[0]
    total = first.table.astype(np.uint64)
    for p in parts[1:]:
        if p.regions != first.regions or p.quality_threshold != first.quality_threshold or p.read_callback != first.read_callback:
            raise ValueError("merge_pileups: the parts do not hold the same regions, threshold and read callback")
        total += p.table
    if total.size and int(total.max()) > 0xffffffff:
        raise ValueError("merge_pileups: a count does not fit 32 bits")
    return Pileup(first.regions, total.astype(np.uint32), first.quality_threshold, first.read_callback)


def count_coverage(path: str, contig: str, start: int, stop: int, quality_threshold=15, read_callback: str = "all", **kw):
    """``pysam.AlignmentFile(path).count_coverage(contig, start, stop, quality_threshold, read_callback)`` in one call: four
    ``array.array('L')``.  Keywords as ``pileup`` (device, index, record_filter, ...)."""
    p = pileup(path, [(contig, start, stop)], quality_threshold, read_callback, **kw)
    return p.count_coverage(contig, start, stop, quality_threshold=quality_threshold, read_callback=read_callback)


# ----------------------------------------------------------------------------------------------
# read QC: per-read length and base-quality statistics, counted during the decode
# ----------------------------------------------------------------------------------------------
QC_COUNTERS = ("n_records", "n_reads", "n_secondary", "n_supplementary", "n_unmapped", "n_no_seq", "n_no_qual", "total_bases")


class ReadQC:
    """What the reference's scripts/report_nanopore_qc.py looks at, from one decode of the aligned BAM.  One entry per READ (a
    record with ``flag & 0x900 == 0`` and SEQ: one per FASTQ record the file was aligned from, mapped or not), in file order:
    ``length`` int32 (``l_seq``, the stored sequence: a hard-clipped primary reports its stored length), ``qual_sum`` int64
    (sum of the read's QUAL bytes = FASTQ character - 33; -1: the read has no quality, its first QUAL byte is 0xff), ``mapq``
    and ``flag`` int32.  ``base_quality_hist`` int64 [256] counts every QUAL byte of the reads that have quality.  Counters
    (``QC_COUNTERS``, also attributes): records, reads, records with flag 0x100 / 0x800, reads with flag 0x4, primary records
    without SEQ, reads without quality, bases of all reads.  Everything is an integer until ``summary`` divides."""

    def __init__(self, length, qual_sum, mapq, flag, base_quality_hist, counters):
        self.length = np.ascontiguousarray(length, dtype=np.int32)
        self.qual_sum = np.ascontiguousarray(qual_sum, dtype=np.int64)
        self.mapq = np.ascontiguousarray(mapq, dtype=np.int32)
        self.flag = np.ascontiguousarray(flag, dtype=np.int32)
        self.base_quality_hist = np.ascontiguousarray(base_quality_hist, dtype=np.int64)
        self.counters = {k: int(counters[k]) for k in QC_COUNTERS}
        for k, v in self.counters.items():
            setattr(self, k, v)

    def mean_qualities(self) -> np.ndarray:
        """``np.mean(quality)`` of every read that has quality, in file order: qual_sum / length in float64 (the sums are far
        below 2^53, so this is the mean of the integer array bit for bit)."""
        have = self.qual_sum >= 0
        return self.qual_sum[have].astype(np.float64) / self.length[have].astype(np.float64)

    def summary(self) -> dict:
        """Q25 / Q50 / Q75 (``np.percentile``, the script's lines 70-72) and the mean (lines 58, 66) of the read lengths and of
        the reads' mean qualities, N50 and the number of bases.  The quality entries are None when no read has quality; a
        file without any read raises ValueError."""
        if len(self.length) == 0:
            raise ValueError("read QC: the file holds no read (no primary record with SEQ): there is nothing to summarise")
        lengths = self.length.astype(np.int64)
        out = {"length_Q%d" % q: float(np.percentile(lengths, q)) for q in (25, 50, 75)}
        out["mean_length"] = float(np.mean(lengths))
        mq = self.mean_qualities()
        for q in (25, 50, 75):
            out["quality_Q%d" % q] = float(np.percentile(mq, q)) if len(mq) else None
        out["mean_quality"] = float(np.mean(mq)) if len(mq) else None
        desc = np.sort(lengths)[::-1]
        out["n50"] = int(desc[np.searchsorted(2 * np.cumsum(desc), int(lengths.sum()))])      # reads this long or longer hold half the bases
        out["total_bases"] = int(lengths.sum())
        return out

    def summary_text(self) -> str:
        """The bytes of the script's ``quality_control_summary.tsv`` (``DataFrame.to_csv(sep='\\t')`` of its frame)."""
        s = self.summary()
        if s["mean_quality"] is None:
            raise ValueError("read QC: no read has base qualities: quality_control_summary.tsv cannot be written")
        row = lambda name, key: "\t".join([name] + [repr(s["%s_Q%d" % (key, q)]) for q in (25, 50, 75)]) + "\n"
        return "\tQ25\tQ50\tQ75\n" + row("mean_length", "length") + row("mean_sequence_quality", "quality")

    def write_summary(self, path: str) -> str:
        text = self.summary_text()
        with open(path, "w", newline="") as fp:
            fp.write(text)
        return path


def _read_qc_from_handle(L, h) -> ReadQC:
    sz = (C.c_int64 * 2)()
    if L.coral_bam_qc_sizes(h, sz) != 0:
        raise _lib.CoralHipError("coral_bam_qc_sizes failed: %s" % L.coral_bam_last_error().decode())
    r = int(sz[1])
    length, mapq, flag = (np.empty(r, dtype=np.int32) for _ in range(3))
    qual_sum, hist = np.empty(r, dtype=np.int64), np.zeros(256, dtype=np.int64)
    cnt = (C.c_int64 * 8)()
    if L.coral_bam_qc_fill(h, length.ctypes.data, qual_sum.ctypes.data, mapq.ctypes.data, flag.ctypes.data, hist.ctypes.data, cnt) != 0:
        raise _lib.CoralHipError("coral_bam_qc_fill failed: %s" % L.coral_bam_last_error().decode())
    return ReadQC(length, qual_sum, mapq, flag, hist, dict(zip(QC_COUNTERS, cnt)))


def read_qc(path: str, device="cuda:0", n_threads: Optional[int] = None, rank: int = 0, world: int = 1, batch_bytes: int = 0, *,
            record_filter=None) -> ReadQC:
    """Per-read length and base-quality statistics of the BAM (``ReadQC``), counted while it is decoded - the only time QUAL is
    at hand.  On the GPU pipeline when ``device`` is a GPU (k_bam_qc_plan / k_bam_qc per batch), on the host
    pipeline with ``device="cpu"`` or ``CORAL_BAM_DECODE=cpu`` (coral_bam_decode_request); the results are identical.  With
    ``world`` > 1 the result is that of the ``rank``-th byte range; ``merge_read_qc`` joins them.  ``record_filter``: a
    ``RecordFilter`` - the statistics (``n_records`` included) are those of the records it keeps."""
    bam_reference_names(path)                                    # (a clear error for something that is not a BAM file)
    return _decode(path, device, n_threads=n_threads, rank=rank, world=world, batch_bytes=batch_bytes, qc=True, records=False,
                   record_filter=record_filter).qc


def merge_read_qc(parts: Sequence[ReadQC]) -> ReadQC:
    """The results of consecutive byte ranges (in rank order) as one: rows concatenated, histograms and counters added."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_read_qc needs at least one part")
    cat = lambda k: np.concatenate([getattr(p, k) for p in parts])
    return ReadQC(cat("length"), cat("qual_sum"), cat("mapq"), cat("flag"), np.sum([p.base_quality_hist for p in parts], axis=0),
                  {k: sum(p.counters[k] for p in parts) for k in QC_COUNTERS})


# ----------------------------------------------------------------------------------------------
# binned depth: read depth per fixed-size bin of every contig, counted during the decode
# ----------------------------------------------------------------------------------------------
DEPTH_MAX_BINS = 1 << 28


class BinnedDepth:
    """Read depth summed into bins of ``bin_size`` bases along every contig of the header - the per-bin table a copy-number
    caller starts from (the reference's scripts/call_cnvs.sh runs CNVkit for it).  ``chroms`` / ``lengths``: the header's
    contigs; contig c has ceil(length / bin_size) bins, the last one ending at the contig's length.  ``bases(c)``: reference
    positions of the bin covered by M / = / X ops (and D ops with ``count_deletions``), summed over the records that take part
    (``flag & exclude_flags == 0`` and ``mapq >= min_mapq``); ``reads(c)``: such records that start in the bin.  int64, exact."""

    def __init__(self, chroms, lengths, bin_size, min_mapq, exclude_flags, count_deletions, bin_off, bases, reads):
        self.chroms, self.lengths = list(chroms), [max(int(l), 0) for l in lengths]
        self.bin_size, self.min_mapq, self.exclude_flags, self.count_deletions = int(bin_size), int(min_mapq), int(exclude_flags), bool(count_deletions)
        self.bin_off = np.ascontiguousarray(bin_off, dtype=np.int64)
        self.all_bases = np.ascontiguousarray(bases, dtype=np.int64)
        self.all_reads = np.ascontiguousarray(reads, dtype=np.int64)
        want = np.concatenate([[0], np.cumsum([(l + self.bin_size - 1) // self.bin_size for l in self.lengths], dtype=np.int64)])
        if not np.array_equal(self.bin_off, want) or len(self.all_bases) != want[-1] or len(self.all_reads) != want[-1]:
            raise ValueError("BinnedDepth: the tables do not fit the contigs and the bin size")
        self._tid = {c: k for k, c in enumerate(self.chroms)}

    @property
    def params(self):
        return (self.bin_size, self.min_mapq, self.exclude_flags, self.count_deletions)

    @property
    def n_bins(self) -> int:
        return int(self.bin_off[-1])

    def _rows(self, chrom):
        if chrom not in self._tid:
            raise KeyError("unknown contig %r" % (chrom,))
        t = self._tid[chrom]
        return slice(int(self.bin_off[t]), int(self.bin_off[t + 1])), self.lengths[t]

    def bases(self, chrom) -> np.ndarray:
        return self.all_bases[self._rows(chrom)[0]]

    def reads(self, chrom) -> np.ndarray:
        return self.all_reads[self._rows(chrom)[0]]

    def bins(self, chrom):
        """(starts, ends) int64 of the contig's bins; the last bin ends at the contig's length."""
        rows, length = self._rows(chrom)
        starts = np.arange(rows.stop - rows.start, dtype=np.int64) * self.bin_size
        return starts, np.minimum(starts + self.bin_size, length)

    def mean_depth(self, chrom) -> np.ndarray:
        """bases / bin length as float64 (the short last bin divided by its own length)."""
        starts, ends = self.bins(chrom)
        return self.bases(chrom).astype(np.float64) / (ends - starts).astype(np.float64)

    def write(self, path: str) -> str:
        """Tab-separated, one row per bin in header order, with the columns CNVkit documents for its .cnn files: chromosome,
        start, end, gene ('-'), depth (the mean depth), log2 (log2 of the depth; -20 for a depth of 0), plus reads."""
        with open(path, "w", newline="") as fp:
            fp.write("chromosome\tstart\tend\tgene\tdepth\tlog2\treads\n")
            for c in self.chroms:
                (starts, ends), depth, reads = self.bins(c), self.mean_depth(c), self.reads(c)
                log2 = np.full(len(depth), -20.0)
                np.log2(depth, out=log2, where=depth > 0)
                fp.write("".join("%s\t%d\t%d\t-\t%r\t%r\t%d\n" % (c, a, b, d, l, r)
                                 for a, b, d, l, r in zip(starts.tolist(), ends.tolist(), depth.tolist(), log2.tolist(), reads.tolist())))
        return path

    @classmethod
    def read(cls, path: str, bin_size: Optional[int] = None) -> "BinnedDepth":
        """The table ``write`` wrote, back as a ``BinnedDepth``: contigs in the file's order (a contig without bins is not in
        the file), a contig's length = the end of its last bin, ``bases`` = depth * the bin's length, rounded (exact below
        2^52).  ``bin_size``: taken from the first bin that is not its contig's last - or, where every contig has one bin, the
        longest bin - unless given.  What the file does not say (min_mapq, exclude_flags, count_deletions) is the defaults'.
        ValueError: other columns, bins that are not ``write``'s."""
        chroms, rows = [], {}
        with open(path) as fp:
            head = fp.readline().rstrip("\n").split("\t")
            if head[:5] != ["chromosome", "start", "end", "gene", "depth"]:
                raise ValueError("%s: not a binned-depth table (columns %r)" % (path, head))
            reads_at = head.index("reads") if "reads" in head else -1
            for line in fp:
                s = line.rstrip("\n").split("\t")
                if len(s) < 5:
                    continue
                if s[0] not in rows:
                    chroms.append(s[0])
                    rows[s[0]] = []
                rows[s[0]].append((int(s[1]), int(s[2]), float(s[4]), int(s[reads_at]) if reads_at >= 0 else 0))
        if bin_size is None:
            inner = [r[1] - r[0] for c in chroms for r in rows[c][:-1]]
            bin_size = inner[0] if inner else max([r[1] - r[0] for c in chroms for r in rows[c]], default=1)
        bin_size = int(bin_size)
        if bin_size < 1:
            raise ValueError("bin_size must be at least 1, got %r" % (bin_size,))
        lengths, bases, reads = [], [], []
        for c in chroms:
            length = rows[c][-1][1]
            for k, (a, b, d, r) in enumerate(rows[c]):
                if a != k * bin_size or b != min(a + bin_size, length):
                    raise ValueError("%s: bin %s:%d-%d is not bin %d of bins of %d bases" % (path, c, a, b, k, bin_size))
                bases.append(int(round(d * (b - a))))
                reads.append(r)
            if len(rows[c]) != (length + bin_size - 1) // bin_size:
                raise ValueError("%s: contig %s does not end with its last bin" % (path, c))
            lengths.append(length)
        bin_off = np.concatenate([[0], np.cumsum([len(rows[c]) for c in chroms], dtype=np.int64)]).astype(np.int64)
        return cls(chroms, lengths, bin_size, 0, 0x704, True, bin_off, np.array(bases, dtype=np.int64), np.array(reads, dtype=np.int64))


def depth_parameters(bin_size, min_mapq, exclude_flags, count_deletions):
    """The parameters of a binned-depth request as ints, or ValueError: bin_size >= 1, min_mapq 0..255, exclude_flags 0..0xffff."""
    for name, v in (("bin_size", bin_size), ("min_mapq", min_mapq), ("exclude_flags", exclude_flags)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError("%s must be an integer, got %r" % (name, v))
    if not 1 <= bin_size <= _I32_MAX:
        raise ValueError("bin_size must be at least 1, got %r" % (bin_size,))
    if not 0 <= min_mapq <= 255:
        raise ValueError("min_mapq must be in 0..255, got %r" % (min_mapq,))
    if not 0 <= exclude_flags <= 0xffff:
        raise ValueError("exclude_flags must be in 0..0xffff, got %r" % (exclude_flags,))
    return int(bin_size), int(min_mapq), int(exclude_flags), 1 if count_deletions else 0


def binned_depth(path: str, bin_size: int = 1000, min_mapq: int = 0, exclude_flags: int = 0x704, count_deletions: bool = True,
                 device="cuda:0", rank: int = 0, world: int = 1, batch_bytes: int = 0, n_threads: Optional[int] = None, *,
                 record_filter=None) -> BinnedDepth:
    """Read depth per bin of ``bin_size`` bases along every contig (``BinnedDepth``), counted while the BAM is decoded: only the
    fixed fields and the CIGAR of a record are looked at, so a file without SEQ or QUAL serves as well.  A record takes part
    when it has a contig, a position and a CIGAR, ``flag & exclude_flags == 0`` and ``mapq >= min_mapq``; M / = / X ops (and D
    ops with ``count_deletions``) add their reference positions inside the contig to ``bases``, the record's start adds 1 to
    ``reads``.  The defaults are meant to be ``samtools bedcov``'s (what CNVkit's WGS coverage runs); parity with samtools or
    CNVkit is not pinned here, the rule is.  Bad parameters, or more than 2^28 bins, raise ValueError before
    anything is decoded.  GPU pipeline (k_bam_depth per batch) on a GPU ``device``, host pipeline with ``device="cpu"`` or
    ``CORAL_BAM_DECODE=cpu``; identical results.  With ``world`` > 1 the tables are those of the ``rank``-th byte range;
    ``merge_binned_depth`` adds them.  ``record_filter``: a ``RecordFilter``, applied in front of (and so together with)
    ``min_mapq`` / ``exclude_flags``."""
    params = depth_parameters(bin_size, min_mapq, exclude_flags, count_deletions)
    chroms, lengths = bam_reference_names(path), bam_reference_lengths(path)
    n_bins = sum((max(l, 0) + params[0] - 1) // params[0] for l in lengths)
    if n_bins > DEPTH_MAX_BINS:
        raise ValueError("bins of %d bases make %d bins of this header: a binned-depth request takes at most 2^28" % (params[0], n_bins))
    res = _decode(path, device, n_threads=n_threads, rank=rank, world=world, batch_bytes=batch_bytes, records=False, depth=params,
                  record_filter=record_filter)
    return BinnedDepth(chroms, lengths, *params, *res.depth)


def merge_binned_depth(parts: Sequence[BinnedDepth]) -> BinnedDepth:
    """The tables of byte ranges decoded by several ranks, added.  The parts must have the same header and parameters."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_binned_depth needs at least one part")
    first = parts[0]
    for p in parts[1:]:
        if p.params != first.params or p.chroms != first.chroms or p.lengths != first.lengths:
            raise ValueError("merge_binned_depth: the parts do not have the same header and parameters")
    return BinnedDepth(first.chroms, first.lengths, *first.params, first.bin_off, np.sum([p.all_bases for p in parts], axis=0),
                       np.sum([p.all_reads for p in parts], axis=0))


# ----------------------------------------------------------------------------------------------
# reads: the selected records as FASTQ text, written during the decode
# ----------------------------------------------------------------------------------------------
class Reads:
    """FASTQ text of the reads one decode selected (``extract_reads``): ``text`` uint8, the records `@name\\nSEQ\\n+\\nQUAL\\n` one
    after the other in file order, ``offsets`` int64 [n + 1] where each starts, ``n`` their number.  Iterating yields (name, seq,
    qual) as str."""

    def __init__(self, text=None, offsets=None):
        self.text = np.ascontiguousarray(text if text is not None else np.zeros(0, dtype=np.uint8), dtype=np.uint8)
        self.offsets = np.ascontiguousarray(offsets if offsets is not None else np.zeros(1, dtype=np.int64), dtype=np.int64)
        if len(self.offsets) < 1 or int(self.offsets[0]) != 0 or int(self.offsets[-1]) != len(self.text):
            raise ValueError("Reads: the offsets do not fit the text")
        self.n = len(self.offsets) - 1

    def __len__(self):
        return self.n

    def __iter__(self):
        raw, off = self.text.tobytes(), self.offsets.tolist()
        for a, b in zip(off, off[1:]):
            name, seq, _, qual = raw[a:b - 1].decode("latin-1").split("\n")      # (a name holds no line end: its bytes are printable)
            yield name[1:], seq, qual

    def names(self):
        raw, off = self.text.tobytes(), self.offsets.tolist()
        return [raw[a + 1:raw.index(b"\n", a)].decode("latin-1") for a in off[:-1]]

    def write(self, path: str) -> str:
        with open(path, "wb") as fp:
            fp.write(self.text.tobytes())
        return path


def merge_reads(parts: Sequence[Reads]) -> Reads:
    """The results of consecutive byte ranges (in rank order) as one: the texts concatenated."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_reads needs at least one part")
    base = np.concatenate([[0], np.cumsum([len(p.text) for p in parts])]).astype(np.int64)
    return Reads(np.concatenate([p.text for p in parts]),
                 np.concatenate([np.zeros(1, dtype=np.int64)] + [p.offsets[1:] + b for p, b in zip(parts, base)]))


def extract_reads(path: str, regions=None, names=None, exclude_flags: int = 0x900, device="cuda:0", n_threads: Optional[int] = None,
                  rank: int = 0, world: int = 1, batch_bytes: int = 0, *, index=None, record_filter=None, output: Optional[str] = None):
    """The reads of the BAM file as FASTQ (``Reads``), written while it is decoded - the only time SEQ and QUAL are at hand: what
    ``samtools view x.bam region... | samtools fastq`` or ``samtools view -N names.txt`` get from a second pass over the file.

    A record is written when it has SEQ, ``flag & exclude_flags == 0`` (default 0x900: one record per read - a hard-clipped
    supplementary holds only a part of it), with ``regions`` [(chrom, start, stop)] (they may overlap or touch and are merged):
    it is on a region's contig and ``[pos, end)`` meets the region (a record with flag 0x4: ``[pos, pos + 1)``), with ``names``
    (str or bytes): its read name is one of them.  Regions and names intersect; neither: every read.  An empty ``regions`` or
    ``names`` list selects nothing, and the file is not opened.  Text of a record: ``@name``, SEQ ("=ACMGRSVTWYHKDBN"), ``+``,
    QUAL (min(q, 93) + 33; '"' throughout when the record has no QUAL); a record with flag 0x10 is reverse-complemented back to
    the orientation it was sequenced in, its QUAL reversed.  The quality-1 default, the clamp at 93 and the 0x900 default are
    meant to be ``samtools fastq``'s; parity with samtools is not pinned here, the rule is.

    GPU pipeline (k_bam_reads_plan / k_bam_reads_emit per batch) on a GPU ``device``, host pipeline with ``device="cpu"`` or
    ``CORAL_BAM_DECODE=cpu``; identical bytes.  With regions, a BAI index (``index``: the rules of ``window_coverage``) restricts
    the decode to the BGZF blocks it names; with names only, or neither, the byte range (``rank`` of ``world``) is decoded and
    ``merge_reads`` joins the ranges.  ``record_filter``: a ``RecordFilter``, applied first.  The whole result lives in host
    memory: meant for the reads of an amplicon.  For every read of a 2 M-read file give ``output``: each batch's text is written
    to that file where it would be appended to the result (the CORAL_SINK_TEXT sink of coral_bamgpu_open_request; a GPU ``device``, the whole file:
    ``world`` 1), nothing is kept, and the call returns ``(records, bytes)``; the file's bytes are those of ``Reads.write``."""
    if output is None:
        got = _selected(1, path, regions, names, exclude_flags, device, n_threads, rank, world, batch_bytes, index, record_filter)
        return Reads(*got) if got is not None else Reads()
    if torch.device(device).type != "cuda":
        raise ValueError("extract_reads(output=...) writes during a GPU decode, got device %r; the host path is extract_reads(...).write(...)" % (device,))
    if (rank, world) != (0, 1):
        raise ValueError("extract_reads(output=...) writes one file: byte ranges (world > 1) do not go with it")
    regions, names = (None if x is None else list(x) for x in (regions, names))
    got = _selected(1, path, regions, names, exclude_flags, device, n_threads, 0, 1, batch_bytes, index, record_filter, sink=TextFile(output))
    if got is None:                                              # nothing was decoded: an empty file
        open(output, "wb").close()
        return 0, 0
    return int(got[0]), int(got[1])


def _selected(mode: int, path, regions, names, exclude_flags, device, n_threads, rank, world, batch_bytes, index, record_filter, order: int = 0,
              sink=None):
    """What ``extract_reads`` (mode 1), ``extract_records`` (mode 2) and ``view_bam`` (mode 2 with ``sink``, see _decode) share: the
    argument rules, the index use and the decode -> (bytes uint8, offsets int64 [n + 1]) of the reads request - with ``sink``
    its four counts -, or None for a selection that is empty before any record is decoded (an empty list: the file is not
    opened).  ``order`` 1 (mode 2 only): the records in coordinate order."""
    _exclude_flags_argument(exclude_flags)
    if names is not None:
        names = sorted(set(nm.encode("latin-1") if isinstance(nm, str) else bytes(nm) for nm in names))
        for nm in names:
            if not 1 <= len(nm) <= 254:
                raise ValueError("a read name has 1..254 bytes, got %r" % (nm,))
    if (regions is not None and len(list(regions)) == 0) or (names is not None and len(names) == 0):
        return None
    if n_threads is None:
        n_threads = default_threads()
    if regions is None:
        res = _decode(path, device, n_threads=n_threads, rank=rank, world=world, batch_bytes=batch_bytes, records=False,
                      record_filter=record_filter, reads=(exclude_flags, None, names, mode, order), sink=sink)
        return res.reads
    ref_names = bam_reference_names(path)
    _, segs = pileup_regions(list(regions), ref_names)
    if segs.shape[1] == 0:                                       # only empty regions
        return None
    idx, skipped = _index_choice(path, index, world, len(ref_names))
    res = _decode_regions(idx, skipped, segs.T.tolist(), n_threads, lambda spans: _decode(     # (the segments as they are: none joined)
        path, device, n_threads=n_threads, rank=rank, world=world, batch_bytes=batch_bytes, spans=spans, records=False, record_filter=record_filter,
        reads=(exclude_flags, segs, names, mode, order), sink=sink))
    return None if res is None else res.reads


# ----------------------------------------------------------------------------------------------
# records: the selected records' own bytes, and the BAM file around them
# ----------------------------------------------------------------------------------------------
def bam_header_bytes(path: str) -> bytes:
    """The inflated bytes of a BAM file in front of its first record, verbatim: magic, header text, contig names and lengths
    (read with gzip, as ``bam_reference_names`` reads them)."""
    with gzip.open(path, "rb") as fp:
        out = []

        def take(n):
            b = fp.read(n)
            if len(b) != n:
                raise _lib.CoralHipError("%s: truncated BAM header" % path)
            out.append(b)
            return b
        if take(4) != b"BAM\x01":
            raise _lib.CoralHipError("%s: not a BAM file" % path)
        take(struct.unpack("<i", take(4))[0])
        for _ in range(struct.unpack("<i", take(4))[0]):
            take(struct.unpack("<i", take(4))[0])
            take(4)
        return b"".join(out)


_RECORD_ORDERS = {"file": 0, "coordinate": 1}


def sorted_header_bytes(header: bytes) -> bytes:
    """The inflated BAM header ``header`` (``bam_header_bytes``) saying that the records are in coordinate order: the ``SO:``
    value of the text's ``@HD`` line becomes ``coordinate``, an ``@HD`` line without ``SO:`` gets ``\tSO:coordinate`` appended, a
    text without ``@HD`` (an empty one too) gets ``@HD\tVN:1.6\tSO:coordinate\n`` in front; ``l_text`` follows, and everything
    behind the text (the contigs) stays byte for byte."""
    header = bytes(header)
    if len(header) < 8 or header[:4] != b"BAM\x01":
        raise ValueError("sorted_header_bytes: not the inflated header of a BAM file")
    l_text = struct.unpack_from("<i", header, 4)[0]
    if l_text < 0 or 8 + l_text > len(header):
        raise ValueError("sorted_header_bytes: l_text reaches behind the header")
    text, rest = header[8:8 + l_text], header[8 + l_text:]
    if text[:3] == b"@HD" and text[3:4] in (b"\t", b"\n", b""):
        end = text.find(b"\n") if b"\n" in text else len(text)
        fields = text[:end].split(b"\t")
        if any(f.startswith(b"SO:") for f in fields[1:]):
            fields = fields[:1] + [b"SO:coordinate" if f.startswith(b"SO:") else f for f in fields[1:]]
        else:
            fields.append(b"SO:coordinate")
        text = b"\t".join(fields) + text[end:]
    else:
        text = b"@HD\tVN:1.6\tSO:coordinate\n" + text
    return header[:4] + struct.pack("<i", len(text)) + text + rest


class RecordBytes:
    """The records one decode selected (``extract_records``) as they stand in the source's inflated stream: ``data`` uint8, per
    record its block_size word and the block_size bytes behind it, in file order - or, with ``order`` "coordinate", sorted;
    ``offsets`` int64 [n + 1] where each starts; ``n`` their number; ``header`` the source's inflated bytes in front of its first
    record (None where the file was never opened: an empty ``regions`` or ``names`` list), for coordinate order rewritten by
    ``sorted_header_bytes``; ``order`` "file" or "coordinate"."""

    def __init__(self, data=None, offsets=None, header: Optional[bytes] = None, order: str = "file"):
        if order not in _RECORD_ORDERS:
            raise ValueError("order must be 'file' or 'coordinate', got %r" % (order,))
        self.order = order
        self.data = np.ascontiguousarray(data if data is not None else np.zeros(0, dtype=np.uint8), dtype=np.uint8)
        self.offsets = np.ascontiguousarray(offsets if offsets is not None else np.zeros(1, dtype=np.int64), dtype=np.int64)
        if len(self.offsets) < 1 or int(self.offsets[0]) != 0 or int(self.offsets[-1]) != len(self.data):
            raise ValueError("RecordBytes: the offsets do not fit the data")
        self.n = len(self.offsets) - 1
        self.header = None if header is None else bytes(header)

    def __len__(self):
        return self.n

    def names(self):
        raw = self.data.tobytes()
        return [raw[a + 36:a + 36 + raw[a + 12] - 1].decode("latin-1") for a in self.offsets[:-1].tolist()]

    def write(self, path: str, level: int = 1, index: bool = False, n_threads: Optional[int] = None, device="cpu",
              workspace_bytes: Optional[int] = None) -> str:
        """The header and the records as a BGZF / BAM file (coral_bgzf_write: blocks of at most 0xff00 bytes, the header in
        blocks of its own, the EOF block last; ``level`` 0..9; the bytes do not depend on ``n_threads``).  ``index``: also its
        BAI index beside it (``build_index`` of the file written, host pipeline; the records must be in coordinate order, as
        those of a sorted source are).

        With a GPU ``device`` the same blocks are deflated there (coral_bgzf_write_gpu: k_bgzf_deflate, k_bgzf_pack): the same
        cuts, so the same inflated bytes per block, other compressed bytes.  The GPU compressor has one setting: ``level`` must
        be 1.  ``workspace_bytes``: device memory for the call (default: what it asks for; less means smaller chunks, the same
        file)."""
        if self.header is None:
            raise ValueError("RecordBytes.write needs the source's header (bam_header_bytes)")
        if isinstance(level, bool) or not isinstance(level, numbers.Integral) or not 0 <= level <= 9:
            raise ValueError("level must be an integer in 0..9, got %r" % (level,))
        L = _lib.lib()
        head = np.frombuffer(self.header, dtype=np.uint8)
        parts = (C.c_void_p * 2)(head.ctypes.data, self.data.ctypes.data if len(self.data) else None)
        sizes = (C.c_int64 * 2)(len(head), len(self.data))
        if torch.device(device).type == "cuda":
            if level != 1:
                raise ValueError("the GPU compressor has one setting: level must be 1 with a GPU device, got %r" % (level,))
            _bgzf_write_gpu(path, parts, sizes, 2, device, workspace_bytes)
        else:
            rc = L.coral_bgzf_write(os.fsencode(path), parts, sizes, 2, int(level), n_threads or default_threads())
            if rc != 0:
                raise _lib.CoralHipError("coral_bgzf_write(%s) failed (%d): %s" % (path, rc, L.coral_bam_last_error().decode()))
        if index:
            build_index(path, device="cpu")
        return path


def _bgzf_write_gpu(path, parts, sizes, n_parts: int, device, workspace_bytes: Optional[int] = None) -> None:
    """coral_bgzf_write_gpu with its workspace as a torch uint8 tensor on ``device``, as the decode's is."""
    L = _lib.lib()
    dev = torch.device(device)
    torch.cuda.set_device(dev)
    ws_bytes = int(L.coral_bgzf_write_gpu_workspace_bytes()) if workspace_bytes is None else int(workspace_bytes)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    rc = L.coral_bgzf_write_gpu(os.fsencode(path), parts, sizes, n_parts, ws.data_ptr(), ws_bytes, stream.cuda_stream)
    stream.synchronize()                                  # (the call has waited already; `ws` is released behind it)
    if rc != 0:
        raise _lib.CoralHipError("coral_bgzf_write_gpu(%s) failed (%d): %s" % (path, rc, L.coral_bam_last_error().decode()))


_BGZF_SLOT = 65536


def bgzf_compress(data, device="cuda:0") -> bytes:
    """``data`` (bytes, or a uint8 array) as BGZF: one member per 0xff00 bytes, made on the GPU (coral_bgzf_deflate,
    coral_bgzf_pack: one wave per member, dynamic Huffman or stored, whichever is smaller), and the 28-byte EOF block.
    ``gzip.decompress`` of the result is ``data``; the bytes depend on ``data`` alone.  The thin public face of the kernel:
    everything stays in torch tensors on ``device``, 1 024 blocks at a time."""
    L = _lib.lib()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("bgzf_compress runs on a GPU device, got %r" % (device,))
    raw = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    out = []
    per_call = 1024
    for at in range(0, len(raw), per_call * 0xff00):
        piece = raw[at:at + per_call * 0xff00]
        n = (len(piece) + 0xff00 - 1) // 0xff00
        desc = np.zeros((n, 4), dtype=np.uint32)
        desc[:, 0] = np.arange(n, dtype=np.uint32) * 0xff00
        desc[:, 1] = np.minimum(0xff00, len(piece) - desc[:, 0].astype(np.int64))
        desc[:, 2] = np.arange(n, dtype=np.uint32) * _BGZF_SLOT
        t_in = torch.from_numpy(piece.copy()).to(dev)
        t_desc = torch.from_numpy(desc.view(np.int32)).to(dev)
        slots = torch.empty(n * _BGZF_SLOT, dtype=torch.uint8, device=dev)
        packed = torch.empty(n * _BGZF_SLOT, dtype=torch.uint8, device=dev)
        member = torch.empty(n, dtype=torch.int32, device=dev)
        off = torch.empty(n + 1, dtype=torch.int32, device=dev)
        scratch = torch.empty(int(L.coral_bgzf_deflate_scratch_bytes(n)), dtype=torch.uint8, device=dev)
        tmp = torch.empty(max(int(L.coral_bgzf_pack_scratch_bytes(n)), 1), dtype=torch.uint8, device=dev)
        rc = L.coral_bgzf_deflate(t_in.data_ptr(), t_desc.data_ptr(), n, slots.data_ptr(), member.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                  stream.cuda_stream)
        if rc == 0:
            rc = L.coral_bgzf_pack(slots.data_ptr(), member.data_ptr(), n, packed.data_ptr(), off.data_ptr(), tmp.data_ptr(), tmp.numel(), stream.cuda_stream)
        if rc != 0:
            raise _lib.CoralHipError("bgzf_compress failed (%d): %s" % (rc, L.coral_bam_last_error().decode()))
        total = int(off[n].item())
        out.append(packed[:total].cpu().numpy().tobytes())
    return b"".join(out) + _BGZF_EMPTY


def merge_record_bytes(parts: Sequence[RecordBytes]) -> RecordBytes:
    """The results of consecutive byte ranges (in rank order) as one: the bytes concatenated.  The parts are of one file: their
    headers must be equal."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_record_bytes needs at least one part")
    if any(p.header != parts[0].header for p in parts[1:]):
        raise ValueError("merge_record_bytes: the parts have different headers")
    if any(p.order != parts[0].order for p in parts[1:]):
        raise ValueError("merge_record_bytes: the parts have different orders")
    if parts[0].order != "file" and len(parts) > 1:
        raise ValueError("merge_record_bytes: sorted parts do not concatenate to a sorted whole (merge_sorted_record_bytes)")
    base = np.concatenate([[0], np.cumsum([len(p.data) for p in parts])]).astype(np.int64)
    return RecordBytes(np.concatenate([p.data for p in parts]),
                       np.concatenate([np.zeros(1, dtype=np.int64)] + [p.offsets[1:] + b for p, b in zip(parts, base)]), parts[0].header,
                       parts[0].order)


def merge_sorted_record_bytes(parts: Sequence[RecordBytes], n_threads: Optional[int] = None) -> RecordBytes:
    """The coordinate-ordered results of consecutive byte ranges (in rank order) as one sorted whole: the native stable k-way
    merge (coral_bam_records_merge) with the parts as runs, so records with equal keys stay in file order.  The parts are of
    one file: their headers must be equal."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_sorted_record_bytes needs at least one part")
    if any(p.order != "coordinate" for p in parts):
        raise ValueError("merge_sorted_record_bytes: every part must be in coordinate order")
    if any(p.header != parts[0].header for p in parts[1:]):
        raise ValueError("merge_sorted_record_bytes: the parts have different headers")
    L = _lib.lib()
    k = len(parts)
    data = (C.c_void_p * k)(*[p.data.ctypes.data if len(p.data) else None for p in parts])
    off = (C.c_void_p * k)(*[p.offsets.ctypes.data for p in parts])
    n = (C.c_int64 * k)(*[p.n for p in parts])
    out = np.zeros(sum(len(p.data) for p in parts), dtype=np.uint8)
    out_off = np.zeros(sum(p.n for p in parts) + 1, dtype=np.int64)
    rc = L.coral_bam_records_merge(k, data, off, n, out.ctypes.data if len(out) else None, out_off.ctypes.data, n_threads or default_threads())
    if rc != 0:
        raise _lib.CoralHipError("coral_bam_records_merge failed (%d): %s" % (rc, L.coral_bam_last_error().decode()))
    return RecordBytes(out, out_off, parts[0].header, "coordinate")


def extract_records(path: str, regions=None, names=None, exclude_flags: int = 0, device="cuda:0", n_threads: Optional[int] = None,
                    rank: int = 0, world: int = 1, batch_bytes: int = 0, *, index=None, record_filter=None, order: str = "file") -> RecordBytes:
    """The selected records of the BAM file as raw BAM record bytes (``RecordBytes``), copied out while it is decoded; with
    ``RecordBytes.write`` what ``samtools view -b x.bam region... > amp.bam && samtools index amp.bam`` gets from a second pass.

    The arguments, the index use and the empty-selection shortcuts are ``extract_reads``'s, and so is the rule but for one
    condition: a record is written when ``flag & exclude_flags == 0`` (default 0: nothing is left out), with ``regions``: it is
    on a region's contig and ``[pos, end)`` meets the region (flag 0x4: ``[pos, pos + 1)``), with ``names``: its read name is
    listed - SEQ is NOT required: a record without SEQ is still a record.  ``record_filter`` acts first.  Every written record
    is ``4 + block_size`` bytes, byte for byte the source's (a CIGAR in a CG:B,I tag stays there), in file order.

    GPU pipeline (k_bam_reads_plan / k_bam_reads_copy per batch) on a GPU ``device``, host pipeline with ``device="cpu"`` or
    ``CORAL_BAM_DECODE=cpu``; identical bytes.  ``merge_record_bytes`` joins byte ranges.  The whole result lives in host memory:
    meant for the records of an amplicon; ``view_bam`` streams the same selection of a whole 2 M-read file to disk.

    ``order="coordinate"``: the written records sorted during the same decode, ascending by ``(tid, pos, reverse strand)`` with
    ``tid = -1`` last and records of equal key in file order - what ``samtools sort`` does in a pass of its own.  On the GPU each
    batch is sorted on the device (k_bam_sort_keys, hipcub's radix sort, k_bam_sort_permute, k_bam_reads_copy_sorted) and the
    batches' runs are merged on the host; the host pipeline sorts what it wrote.  The result carries ``sorted_header_bytes`` of
    the source's header; ``merge_sorted_record_bytes`` joins byte ranges.  It lives in host memory, about twice its size while
    the runs are merged."""
    if order not in _RECORD_ORDERS:
        raise ValueError("order must be 'file' or 'coordinate', got %r" % (order,))
    regions, names = (None if x is None else list(x) for x in (regions, names))
    got = _selected(2, path, regions, names, exclude_flags, device, n_threads, rank, world, batch_bytes, index, record_filter,
                    _RECORD_ORDERS[order])
    if got is None and (regions == [] or names == []):
        return RecordBytes(order=order)                          # (the file was not opened: no header)
    header = bam_header_bytes(path)
    return RecordBytes(*(got if got is not None else (None, None)), header=sorted_header_bytes(header) if order == "coordinate" else header,
                       order=order)


ViewStats = collections.namedtuple("ViewStats", "records bytes file_bytes")


def view_bam(path: str, output: str, regions=None, names=None, exclude_flags: int = 0, *, record_filter=None, index: bool = False, bam_index=None,
             device="cuda:0", n_threads: Optional[int] = None, batch_bytes: int = 0, chunk_blocks: int = 0) -> ViewStats:
    """``samtools view -b`` of a file of any size: the selected records of ``path`` as the BAM file ``output``, written WHILE the
    file is decoded.  Each batch's records are copied out of the inflated batch and deflated where they are, in HBM
    (k_bam_reads_copy_shifted, k_bgzf_chunk_desc, k_bgzf_deflate, k_bgzf_pack; the CORAL_SINK_BAM sink of coral_bamgpu_open_request): uncompressed
    record bytes never cross PCIe, compressed ones once, and host memory is bounded by two pinned chunks whatever the output's
    size.  Returns ``ViewStats(records, bytes, file_bytes)``: records written, their inflated bytes, the size of ``output``.

    Selection (``regions``, ``names``, ``exclude_flags``), ``record_filter`` and the index use (``bam_index`` is
    ``extract_records``'s ``index``) are exactly ``extract_records``'s, and ``output`` is byte for byte
    ``extract_records(...).write(output, device=gpu)``: the source's header in blocks of its own, the records in file order cut
    at 0xff00 bytes, the EOF block; the bytes do not depend on ``batch_bytes``, on ``chunk_blocks`` (blocks per deflate launch:
    0 = 1 024, at most 16 384) or on the run.  An empty ``regions`` or ``names`` list writes header + EOF without a decode.
    ``index``: also ``output``'s BAI index beside it (``build_index`` of the file written, host pipeline, as
    ``RecordBytes.write``).  It needs a GPU ``device``: the host path is ``extract_records(...).write(...)``.  On an exception
    the partial output is removed.  Coordinate order is ``sort_bam`` and, streamed, ``sort_bam_stream``."""
    if torch.device(device).type != "cuda":
        raise ValueError("view_bam streams through a GPU device, got %r; the host path is extract_records(...).write(...)" % (device,))
    chunk_blocks = _size_argument("chunk_blocks", chunk_blocks, 16384, "1 024")
    batch_bytes = _size_argument("batch_bytes", batch_bytes, zero=None)
    regions, names = (None if x is None else list(x) for x in (regions, names))
    header = bam_header_bytes(path)
    with _output_guard(output):
        got = _selected(2, path, regions, names, exclude_flags, device, n_threads, 0, 1, batch_bytes, bam_index, record_filter,
                        sink=BamFile(output, header, chunk_blocks))
        if got is None:                                          # nothing was decoded: header + EOF, the same members
            head = np.frombuffer(header, dtype=np.uint8)
            _bgzf_write_gpu(output, (C.c_void_p * 1)(head.ctypes.data), (C.c_int64 * 1)(len(head)), 1, device)
            got = (0, 0, os.path.getsize(output), 0)
        if index:
            build_index(output, device="cpu")
    return ViewStats(int(got[0]), int(got[1]), int(got[2]))


def sort_bam(path: str, output: str, *, index: bool = True, level: int = 1, record_filter=None, exclude_flags: int = 0, device="cuda:0",
             n_threads: Optional[int] = None, batch_bytes: int = 0, write_device=None, stream: bool = False) -> str:
    """``path``'s records - those that pass ``record_filter`` and ``exclude_flags`` - in coordinate order as the BAM file
    ``output``, with its BAI index beside it (``index``): ``samtools view -b -q ... | samtools sort | samtools index`` from one
    decode (``extract_records(order="coordinate")`` and ``RecordBytes.write``).  Returns ``output``.  The result lives in host
    memory, about twice its size while the batches' runs are merged.  ``write_device``: where the output's BGZF blocks are
    deflated (``RecordBytes.write``'s ``device``; None: on the host, as before).

    ``stream=True``: ``sort_bam_stream`` - the runs are spilled to disk and merged on the GPU, in bounded host memory, for a file
    of any size; the same bytes as ``write_device=device``.  The GPU compressor has one setting (``level`` must be 1), and a GPU
    ``write_device`` other than ``device`` is refused."""
    if stream:
        if level != 1:
            raise ValueError("a streamed sort deflates on the GPU, which has one setting: level must be 1, got %r" % (level,))
        if write_device is not None and torch.device(write_device).type == "cuda" and torch.device(write_device) != torch.device(device):
            raise ValueError("a streamed sort deflates where it decodes: write_device %r is not device %r" % (write_device, device))
        sort_bam_stream(path, output, index=index, record_filter=record_filter, exclude_flags=exclude_flags, device=device, n_threads=n_threads,
                        batch_bytes=batch_bytes)
        return output
    rec = extract_records(path, None, None, exclude_flags, device=device, n_threads=n_threads, batch_bytes=batch_bytes, index=False,
                          record_filter=record_filter, order="coordinate")
    return rec.write(output, level=level, index=index, n_threads=n_threads, device="cpu" if write_device is None else write_device)


SortStats = collections.namedtuple("SortStats", "records bytes file_bytes runs spill_bytes")
LAST_SORT_STREAM = {}                                            # what the last sort_bam_stream did: coral_bamgpu_merge_stats and the two phases' seconds
_ERR_NAMES = {-1: "CORAL_ERR_ARG", -2: "CORAL_ERR_HIP", -3: "CORAL_ERR_CAPACITY", -4: "CORAL_ERR_FORMAT"}


def _size_argument(name: str, value, upper: Optional[int] = None, zero: Optional[str] = "the default") -> int:
    """``zero``: what 0 stands for in the message (None: the message does not say)."""
    if isinstance(value, bool) or not isinstance(value, numbers.Integral) or value < 0 or (upper is not None and value > upper):
        raise ValueError("%s must be an integer %s%s, got %r" % (name, ">= 0" if upper is None else "in 0..%d" % upper,
                                                                 "" if zero is None else " (0: %s)" % zero, value))
    return int(value)


def _exclude_flags_argument(exclude_flags) -> None:
    if isinstance(exclude_flags, bool) or not isinstance(exclude_flags, numbers.Integral) or not 0 <= exclude_flags <= 0xffff:
        raise ValueError("exclude_flags must be an integer in 0..0xffff, got %r" % (exclude_flags,))


@contextlib.contextmanager
def _output_guard(output):
    """Around the writing of the file ``output``: a partial output is removed on any exception, while a file that was there and
    that nothing has touched - an argument error came first - is left alone."""
    stat_of = lambda p: (lambda st: (st.st_ino, st.st_size, st.st_mtime_ns))(os.stat(p)) if os.path.exists(p) else None
    before = stat_of(output)
    try:
        yield
    except BaseException:
        if stat_of(output) not in (None, before):
            os.remove(output)
        raise


def sort_bam_stream(path: str, output: str, *, index: bool = True, record_filter=None, exclude_flags: int = 0, device="cuda:0",
                    n_threads: Optional[int] = None, batch_bytes: int = 0, chunk_blocks: int = 0, stage_bytes: int = 0, tmp_dir=None) -> SortStats:
    """``samtools view -b ... | samtools sort | samtools index`` of a file of any size: ``sort_bam``'s output, byte for byte that of
    ``extract_records(order="coordinate", ...).write(output, device=gpu)``, made in two phases in which uncompressed record
    bytes exist only in HBM.

    Phase 1, while the file is decoded (the CORAL_SINK_RUNS sink of coral_bamgpu_open_request): every batch is sorted on the device as for
    ``order="coordinate"``, and its sorted records are deflated where they are and appended to the spill file
    ``<tmp_dir or output's directory>/<output's name>.runs.tmp`` as one run of BGZF members.  Per written record 12 bytes come
    back to the host: its sort key and its length.  Phase 2 (coral_bamgpu_merge_runs): one stable radix sort of all keys on the
    device gives the final order; in steps of at most ``stage_bytes`` inflated source bytes (0: one batch's capacity) the runs'
    members are read, inflated on the device (k_bgzf_inflate, k_bgzf_crc), gathered in final order (k_bam_merge_copy) and
    deflated into ``output`` behind the sorted header (``sorted_header_bytes``), cut at 0xff00 bytes as every writer here cuts.
    Host memory is bounded by 16 bytes per written record and a few pinned buffers, whatever the output's size; device memory
    by the decode's workspace plus about 52 bytes per record and three times ``stage_bytes``; the spill file is about as large
    as the output.  Fewer than 2^31 records.  A record whose source blocks do not fit ``stage_bytes`` raises (CORAL_ERR_CAPACITY).

    ``batch_bytes`` and ``chunk_blocks`` are ``view_bam``'s; the output's bytes depend on none of the three sizes.  ``index``:
    also the BAI index beside ``output`` (``build_index`` of the file written, host pipeline).  The spill file is removed on
    success and on any exception; on an exception the partial output is removed too.  It needs a GPU ``device``: the host path
    is ``sort_bam``.  Returns ``SortStats(records, bytes, file_bytes, runs, spill_bytes)``."""
    if torch.device(device).type != "cuda":
        raise ValueError("sort_bam_stream streams through a GPU device, got %r; the host path is sort_bam" % (device,))
    chunk_blocks = _size_argument("chunk_blocks", chunk_blocks, 16384, "1 024")
    batch_bytes = _size_argument("batch_bytes", batch_bytes)
    stage_bytes = _size_argument("stage_bytes", stage_bytes, 0xf0000000, "one batch's capacity")
    _exclude_flags_argument(exclude_flags)
    if tmp_dir is not None and not os.path.isdir(tmp_dir):
        raise ValueError("tmp_dir %r is not a directory" % (tmp_dir,))
    record_filter = _as_filter(record_filter)
    spill = os.path.join(os.fspath(tmp_dir) if tmp_dir is not None else os.path.dirname(os.path.abspath(output)), os.path.basename(output) + ".runs.tmp")
    header = np.frombuffer(sorted_header_bytes(bam_header_bytes(path)), dtype=np.uint8)
    if n_threads is None:
        n_threads = default_threads()
    req = _lib.bam_request(keep=record_filter, reads=(exclude_flags, None, None, 2, 1))
    try:
        with _output_guard(output):
            with DecodeSession(path, req, device=device, n_threads=n_threads, batch_bytes=batch_bytes, sink=Runs(spill, chunk_blocks),
                               error_names=_ERR_NAMES) as s:
                L, t0 = s.L, time.perf_counter()
                s.start()
                s.run(keep=False)                                # (the decode's CIGAR ops: not kept)
                s.finish()
                t1 = time.perf_counter()
                counts = (C.c_int64 * 3)()
                _lib.check(L.coral_bamgpu_run_table(s.h, 0, None, counts), "coral_bamgpu_run_table")
                ws2_bytes = int(L.coral_bamgpu_merge_workspace_bytes(s.h, stage_bytes))
                if ws2_bytes < 0:
                    raise s.fail("coral_bamgpu_merge_workspace_bytes", ws2_bytes)
                rc = L.coral_bamgpu_merge_runs(s.h, os.fsencode(output), header.ctypes.data, len(header), s.workspace(ws2_bytes), ws2_bytes, stage_bytes, s.stream)
                if rc != 0:
                    raise s.fail("coral_bamgpu_merge_runs", rc)
                st, secs = (C.c_int64 * 8)(), (C.c_double * 8)()
                _lib.check(L.coral_bamgpu_merge_stats(s.h, st, secs), "coral_bamgpu_merge_stats")
                LAST_SORT_STREAM.clear()
                LAST_SORT_STREAM.update(batches=s.batches, runs=int(counts[0]), phase1_seconds=t1 - t0, phase2_seconds=float(secs[0]), order_seconds=float(secs[1]),
                                        read_seconds=float(secs[2]), inflate_wait_seconds=float(secs[3]), inflate_gpu_seconds=float(secs[4]),
                                        copy_gpu_seconds=float(secs[5]), sink_seconds=float(secs[6]), steps=int(st[0]), spill_members_inflated=int(st[1]),
                                        edge_members_inflated_twice=int(st[2]), members=int(st[6]), workspace_bytes=s.ws_bytes, merge_workspace_bytes=ws2_bytes)
                stats = SortStats(int(st[3]), int(st[4]), int(st[5]), int(counts[0]), int(st[7]))
            if index:                                            # (the handle is closed: the output is whole)
                build_index(output, device="cpu")
    finally:
        if os.path.exists(spill):
            os.remove(spill)
    return stats


# ----------------------------------------------------------------------------------------------
# import: a mapper's SAM text as a BAM file (coral_sam_core.h: htslib's sam_parse1 + bam_write1)
# ----------------------------------------------------------------------------------------------
ImportStats = collections.namedtuple("ImportStats", "lines records dropped text_bytes bytes file_bytes members batches seconds")
LAST_IMPORT = {}                                                 # what the last import_sam on a GPU did: coral_samgpu_import's seconds and fix-ups


class SamHeader(collections.namedtuple("SamHeader", "bam names name_off slots n_ref n_slots text_bytes n_lines")):
    """What coral_sam_header makes of a SAM text's leading ``@`` lines: ``bam`` the inflated BAM header (uint8), the contig table
    (``names`` back to back, ``name_off`` int64 [n_ref + 1], ``slots`` uint32 [n_slots]), and how many bytes and lines of the
    text the header is."""


def _sam_header(text) -> SamHeader:
    L = _lib.lib()
    buf = np.frombuffer(bytes(text), dtype=np.uint8)
    sizes = (C.c_int64 * 6)()
    rc = L.coral_sam_header(buf.ctypes.data if len(buf) else None, len(buf), sizes, None, None, None, None)
    if rc != 0:
        raise _sam_error("coral_sam_header", rc)
    bam, names = np.zeros(int(sizes[0]), dtype=np.uint8), np.zeros(int(sizes[2]) + 1, dtype=np.uint8)
    name_off, slots = np.zeros(int(sizes[1]) + 1, dtype=np.int64), np.zeros(int(sizes[3]) + 1, dtype=np.uint32)
    rc = L.coral_sam_header(buf.ctypes.data if len(buf) else None, len(buf), sizes, bam.ctypes.data, names.ctypes.data, name_off.ctypes.data, slots.ctypes.data)
    if rc != 0:
        raise _sam_error("coral_sam_header", rc)
    return SamHeader(bam, names, name_off, slots, int(sizes[1]), int(sizes[3]), int(sizes[4]), int(sizes[5]))


def _sam_error(what: str, rc: int) -> _lib.CoralHipError:
    """The library's refusal as an exception; ``code`` is the C return value (-4, CORAL_ERR_FORMAT, for a refused line)."""
    e = _lib.CoralHipError("%s failed (%d, %s): %s" % (what, rc, _ERR_NAMES.get(rc, "?"), _lib.lib().coral_bam_last_error().decode()))
    e.code = rc
    return e


def sam_header_bytes(text) -> bytes:
    """The inflated BAM header (magic, ``l_text``, the text verbatim without a NUL, ``n_ref``, the contigs of the ``@SQ`` lines in
    their order) of a SAM text: ``text`` is bytes or str, and only its leading ``@`` lines count.  No ``@PG`` line is added."""
    return _sam_header(text.encode() if isinstance(text, str) else text).bam.tobytes()


def _read_sam_head(fd: int):
    """Reads ``fd`` until the header's end is in sight -> (all bytes read, bytes of the header): the header ends in front of the
    first line that does not begin with ``@``, or with the text."""
    buf, at = bytearray(), 0                                     # at: the first line start not yet judged
    while True:
        while at < len(buf) and buf[at] == 0x40:
            nl = buf.find(b"\n", at)
            if nl < 0:
                break
            at = nl + 1
        if at < len(buf) and buf[at] != 0x40:
            return bytes(buf), at
        chunk = os.read(fd, 1 << 20)
        if not chunk:
            return bytes(buf), len(buf)
        buf += chunk


def sam_encode(text, header: SamHeader, record_filter=None, first_line: int = 1):
    """The host's rule book (coral_sam_encode): the whole record lines ``text`` (bytes) under ``header`` -> (record bytes uint8,
    lines, records written, records dropped).  One thread; a refused line raises with ``code`` -4 and the line's number, counted
    from ``first_line``."""
    L = _lib.lib()
    keep = np.array(tuple(_as_filter(record_filter) or RecordFilter()), dtype=np.int32)
    buf = np.frombuffer(bytes(text), dtype=np.uint8)
    n_lines = int((buf == 10).sum()) + 1
    out = np.empty(2 * len(buf) + 36 * n_lines + 64, dtype=np.uint8)
    counts = (C.c_int64 * 6)()
    rc = L.coral_sam_encode(buf.ctypes.data if len(buf) else None, len(buf), int(first_line), header.names.ctypes.data, header.name_off.ctypes.data,
                            header.slots.ctypes.data, header.n_ref, header.n_slots, keep.ctypes.data, out.ctypes.data, len(out), counts)
    if rc != 0:
        raise _sam_error("coral_sam_encode", rc)
    return out[:int(counts[3])], int(counts[0]), int(counts[1]), int(counts[2])


def import_sam(path, output: str, *, record_filter=None, device="cuda:0", batch_bytes: int = 0, chunk_blocks: int = 0, level: int = 1,
               write_device=None) -> ImportStats:
    """``samtools view -bS`` behind a long-read mapper: the SAM text ``path`` (``"-"``: standard input, so that the mapper pipes
    into it; a file descriptor is taken as it is) as the BAM file ``output``.  The rules are htslib's sam_parse1 + bam_write1 as
    coral_sam_core.h states them; a line they refuse raises ``CoralHipError`` with ``code`` -4 (CORAL_ERR_FORMAT) and the 1-based
    line number and the field in its text - of several bad lines the lowest one -, and ``output`` is removed.

    On a GPU ``device`` (coral_samgpu_import) a feeder thread reads the text into pinned buffers of ``batch_bytes`` (0: 128 MiB);
    per batch k_sam_lines, k_sam_size, a scan and k_sam_encode make the records in HBM, and the record sink of ``view_bam``
    deflates them where they are (``chunk_blocks`` blocks per launch, 0: 1 024): the text goes up once and only compressed bytes
    come back.  A line longer than ``batch_bytes`` raises with ``code`` -3 (CORAL_ERR_CAPACITY).  ``level`` and ``write_device``
    have no meaning there: the GPU compressor has one setting.

    ``device="cpu"``: the same rules on one host thread (coral_sam_header, coral_sam_encode) with the whole text and all records
    in host memory, written by ``coral_bgzf_write`` at ``level``, or deflated on the GPU ``write_device``.

    The file is laid out as every writer here lays out (header, records): each part cut at 0xff00 bytes, the header ending a
    block, the EOF block last, no ``@PG`` line added.  Its bytes depend on the text and the filter alone - not on
    ``batch_bytes``, ``chunk_blocks`` or the run; the GPU path's file is ``coral_bgzf_write_gpu``'s of the host path's two parts.
    ``record_filter``: lines it drops write nothing.  Mapper order cannot be indexed: ``sort_bam_stream`` is the next step.
    Returns ``ImportStats(lines, records, dropped, text_bytes, bytes, file_bytes, members, batches, seconds)``."""
    on_gpu = torch.device(device).type == "cuda"
    chunk_blocks = _size_argument("chunk_blocks", chunk_blocks, 16384, "1 024")
    batch_bytes = _size_argument("batch_bytes", batch_bytes, 1 << 30, "128 MiB")
    if isinstance(level, bool) or not isinstance(level, numbers.Integral) or not 0 <= level <= 9:
        raise ValueError("level must be an integer in 0..9, got %r" % (level,))
    keep = np.array(tuple(_as_filter(record_filter) or RecordFilter()), dtype=np.int32)
    L = _lib.lib()
    t0 = time.perf_counter()
    own = not isinstance(path, int)
    fd = (0 if path == "-" else os.open(path, os.O_RDONLY)) if own else path
    try:
        head, n_head = _read_sam_head(fd)
        H = _sam_header(head[:n_head])
        lead = head[n_head:]
        with _output_guard(output):
            if not on_gpu:
                pieces = [lead]
                while True:
                    chunk = os.read(fd, 1 << 24)
                    if not chunk:
                        break
                    pieces.append(chunk)
                text = b"".join(pieces)
                del pieces
                data, lines, written, dropped = sam_encode(text, H, record_filter, H.n_lines + 1)
                rb = RecordBytes(data, np.array([0, len(data)], dtype=np.int64), header=H.bam.tobytes())
                rb.write(output, level=level, device="cpu" if write_device is None else write_device)
                size = os.path.getsize(output)
                blocks = lambda n: (n + 0xfeff) // 0xff00
                return ImportStats(lines, written, dropped, len(text), len(data), size, blocks(len(H.bam)) + blocks(len(data)) + 1, 1, time.perf_counter() - t0)
            dev = torch.device(device)
            torch.cuda.set_device(dev)
            ws_bytes = int(L.coral_samgpu_workspace_bytes(batch_bytes, chunk_blocks, H.n_ref, H.n_slots, int(H.name_off[-1])))
            if ws_bytes < 0:
                raise _sam_error("coral_samgpu_workspace_bytes", ws_bytes)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream(dev)
            stream.synchronize()                                 # (DecodeSession's rule 1: the block may be a recycled one)
            lead_a = np.frombuffer(lead, dtype=np.uint8)
            stats, secs = (C.c_int64 * 9)(), (C.c_double * 4)()
            rc = L.coral_samgpu_import(fd, lead_a.ctypes.data if len(lead_a) else None, len(lead_a), H.n_lines + 1, os.fsencode(output), H.bam.ctypes.data, len(H.bam),
                                       H.names.ctypes.data, H.name_off.ctypes.data, H.slots.ctypes.data, H.n_ref, H.n_slots, keep.ctypes.data, batch_bytes,
                                       chunk_blocks, ws.data_ptr(), ws_bytes, stream.cuda_stream, stats, secs)
            stream.synchronize()                                 # (the call has waited already; `ws` is released behind it)
            if rc != 0:
                raise _sam_error("coral_samgpu_import(%s)" % (path,), rc)
            LAST_IMPORT.clear()
            LAST_IMPORT.update(seconds=float(secs[0]), feeder_wait_seconds=float(secs[1]), size_kernel_seconds=float(secs[2]), encode_kernel_seconds=float(secs[3]),
                               float_fixups=int(stats[8]), workspace_bytes=ws_bytes)
            return ImportStats(*(int(stats[k]) for k in range(8)), time.perf_counter() - t0)
    finally:
        if own and fd != 0:
            os.close(fd)


# ----------------------------------------------------------------------------------------------
# BAI index (SAMv1 §5.2): built during a decode, read, queried
# ----------------------------------------------------------------------------------------------
_PSEUDO_BIN = 37450
_NO_OFFSET = np.uint64(0xffffffffffffffff)


def _decode_spans(path, spans, device, n_threads, batch_bytes, record_filter=None) -> Records:
    """The records that start inside ``spans`` (uint64 [K][2] virtual offsets), on either pipeline (no span: on the host)."""
    return _decode(path, device if len(spans) else "cpu", n_threads=n_threads, batch_bytes=batch_bytes, spans=spans,
                   record_filter=record_filter).records


def _index_partial_from_handle(L, h) -> dict:
    sz = (C.c_int64 * 4)()
    _lib.check(L.coral_bam_index_sizes(h, sz), "coral_bam_index_sizes")
    n_heads, n_lin, n_ref, n_rec = (int(v) for v in sz)
    key, voff = np.empty(n_heads, dtype=np.int64), np.empty(n_heads, dtype=np.uint64)
    lin = np.empty(n_lin, dtype=np.uint64)
    mapped, unmapped = np.empty(n_ref, dtype=np.int64), np.empty(n_ref, dtype=np.int64)
    sc = (C.c_uint64 * 4)()
    _lib.check(L.coral_bam_index_fill(h, key.ctypes.data, voff.ctypes.data, lin.ctypes.data, mapped.ctypes.data, unmapped.ctypes.data, sc),
               "coral_bam_index_fill")
    return dict(head_key=key, head_voff=voff, lin=lin, n_mapped=mapped, n_unmapped=unmapped, n_records=n_rec, n_no_coor=int(sc[0]),
                end_voff=int(sc[1]), first_sort=int(sc[2]), last_sort=int(sc[3]))


def index_partial(path: str, device="cuda:0", rank: int = 0, world: int = 1, n_threads: Optional[int] = None, batch_bytes: int = 0) -> dict:
    """What the ``rank``-th of ``world`` byte ranges of the BAM contributes to its BAI index, from one decode with an index
    request (GPU: k_bam_index per batch; host: coral_bam_decode_request).  ``merge_index_partials`` puts
    consecutive ranges together, ``index_bytes`` writes the file's bytes."""
    return _decode(path, device, n_threads=n_threads, rank=rank, world=world, batch_bytes=batch_bytes, index=True, records=False).index


def merge_index_partials(parts: Sequence[dict]) -> dict:
    """The partial indexes of consecutive byte ranges (in rank order) as one: a run of equal (tid, bin) that goes on across a
    boundary is one run, a window takes the smallest offset, counts add up, and the file ends where the last range that holds a
    record ends.  Raises CoralHipError when the ranges are not in coordinate order among each other."""
    parts = list(parts)
    full = [p for p in parts if p["n_records"] > 0]
    for a, b in zip(full, full[1:]):
        if b["first_sort"] < a["last_sort"]:
            raise _lib.CoralHipError("the records are not in coordinate order: no index can be built")
    key = np.concatenate([p["head_key"] for p in parts])
    voff = np.concatenate([p["head_voff"] for p in parts])
    if len(key):
        new = np.concatenate([[True], key[1:] != key[:-1]])
        key, voff = key[new], voff[new]
    last = full[-1] if full else parts[0]
    return dict(head_key=key, head_voff=voff, lin=np.minimum.reduce([p["lin"] for p in parts]),
                n_mapped=np.sum([p["n_mapped"] for p in parts], axis=0), n_unmapped=np.sum([p["n_unmapped"] for p in parts], axis=0),
                n_records=sum(p["n_records"] for p in parts), n_no_coor=sum(p["n_no_coor"] for p in parts), end_voff=last["end_voff"],
                first_sort=(full[0] if full else parts[0])["first_sort"], last_sort=last["last_sort"])


def index_bytes(partial: dict, ref_lens: Sequence[int]) -> bytes:
    """The BAI file (SAMv1 §5.2) of a whole file's (merged) partial index: per contig its bins in ascending order, each with
    its chunks in file order, the pseudo-bin 37450 last (first and last offset of the contig, records with and without flag
    0x4), the linear index up to the last window a record overlaps (a window without records repeats the one in front, leading
    ones hold 0), and the number of records without coordinates."""
    key, beg = partial["head_key"], partial["head_voff"]
    end = np.concatenate([beg[1:], np.array([partial["end_voff"]], dtype=np.uint64)]) if len(beg) else beg
    placed = key >= 0
    key, beg, end = key[placed], beg[placed], end[placed]
    order = np.argsort(key, kind="stable")                       # by (tid, bin); a bin's chunks stay in file order
    key, beg, end = key[order], beg[order], end[order]
    tid_of = key >> 16
    lin_off = np.concatenate([[0], np.cumsum([(max(int(l), 0) >> 14) + 1 for l in ref_lens])]).astype(np.int64)
    out = [b"BAI\x01", struct.pack("<i", len(ref_lens))]
    for t in range(len(ref_lens)):
        a, b = np.searchsorted(tid_of, t), np.searchsorted(tid_of, t, side="right")
        if a == b:
            out.append(struct.pack("<ii", 0, 0))
            continue
        k, cb, ce = key[a:b] & 0xffff, beg[a:b], end[a:b]
        cut = np.concatenate([[0], np.nonzero(k[1:] != k[:-1])[0] + 1, [len(k)]])
        out.append(struct.pack("<i", len(cut)))                  # (the bins + the pseudo-bin)
        # all bins of the contig as 64-bit words at once: per bin one word (bin number | chunk count << 32), then its chunks
        n_bins, counts = len(cut) - 1, np.diff(cut)
        words = np.empty(n_bins + 2 * len(k), dtype="<u8")
        words[np.arange(n_bins) + 2 * cut[:-1]] = k[cut[:-1]].astype(np.uint64) | (counts.astype(np.uint64) << np.uint64(32))
        at = 2 * np.arange(len(k)) + np.repeat(np.arange(n_bins), counts) + 1
        words[at], words[at + 1] = cb, ce
        out.append(words.tobytes())
        out.append(struct.pack("<IiQQQQ", _PSEUDO_BIN, 2, int(cb.min()), int(ce.max()), int(partial["n_mapped"][t]), int(partial["n_unmapped"][t])))
        lin = partial["lin"][lin_off[t]:lin_off[t + 1]].copy()
        have = np.nonzero(lin != _NO_OFFSET)[0]
        n_intv = int(have[-1]) + 1 if len(have) else 0
        lin = lin[:n_intv]
        src = np.maximum.accumulate(np.where(lin != _NO_OFFSET, np.arange(n_intv), -1))      # the last window with a record at or in front
        filled = np.where(src >= 0, lin[np.maximum(src, 0)], np.uint64(0)).astype("<u8")
        out.append(struct.pack("<i", n_intv) + filled.tobytes())
    out.append(struct.pack("<Q", int(partial["n_no_coor"])))
    return b"".join(out)


def bam_reference_lengths(path: str):
    with gzip.open(path, "rb") as fp:
        fp.read(4)
        fp.read(struct.unpack("<i", fp.read(4))[0])
        lens = []
        for _ in range(struct.unpack("<i", fp.read(4))[0]):
            fp.read(struct.unpack("<i", fp.read(4))[0])
            lens.append(struct.unpack("<i", fp.read(4))[0])
        return lens


def build_index(path: str, index_path: Optional[str] = None, device="cuda:0", n_threads: Optional[int] = None, batch_bytes: int = 0,
                world: int = 1) -> str:
    """Write the BAI index of a coordinate-sorted BAM (default ``path + ".bai"``; to a temporary name first, then renamed) and
    return its path — what ``samtools index`` does, from one decode of the file: on the GPU pipeline when ``device`` is a GPU
    (k_bam_index beside the parse of every batch), on the host pipeline otherwise or with ``CORAL_BAM_DECODE=cpu``.  ``world`` >
    1 decodes that many byte ranges one after the other and merges their partial indexes (the bytes are the same).  A file that
    is not in coordinate order raises CoralHipError and leaves no index behind.  The bytes are a function of the BAM file alone
    (spec-conformant; not the sparser file htslib writes, which also folds small bins into their parents)."""
    bam_reference_names(path)                                    # (a clear error for something that is not a BAM file)
    parts = [index_partial(path, device, r, world, n_threads, batch_bytes) for r in range(world)]
    data = index_bytes(merge_index_partials(parts), bam_reference_lengths(path))
    index_path = index_path or path + ".bai"
    tmp = "%s.tmp%d" % (index_path, os.getpid())
    try:
        with open(tmp, "wb") as fp:
            fp.write(data)
        os.replace(tmp, index_path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return index_path


class BamIndex:
    """A BAI index in memory (``read_index``): per contig ``bins[tid]`` = {bin: uint64 [K][2] chunks (begin, end)} without the
    pseudo-bin, ``linear[tid]`` = uint64 [n_intv], ``meta[tid]`` = (first offset, last offset, mapped, unmapped) or None, and
    ``n_no_coor`` (None when the file ends without it)."""

    def __init__(self, bins, linear, meta, n_no_coor, path=None):
        self.bins, self.linear, self.meta, self.n_no_coor, self.path = bins, linear, meta, n_no_coor, path
        self.n_ref = len(bins)


def read_index(index_path: str) -> BamIndex:
    """Read any spec-conformant ``.bai`` (SAMv1 §5.2): chunks wherever the writer put them (htslib moves those of sparse bins
    into a parent bin and merges neighbours), the pseudo-bin and the trailing ``n_no_coor`` present or not, contigs without
    bins, a linear index shorter than the contig.  A truncated file or one that is not a BAI raises CoralHipError."""
    try:
        with open(index_path, "rb") as fp:
            raw = fp.read()
    except OSError as e:
        raise _lib.CoralHipError("cannot read the index %s: %s" % (index_path, e))
    bad = lambda why: _lib.CoralHipError("%s: %s" % (index_path, why))
    if raw[:4] != b"BAI\x01":
        raise bad("not a BAI index")
    o = [4]

    def take(fmt):
        n = struct.calcsize(fmt)
        if o[0] + n > len(raw):
            raise bad("truncated BAI index")
        v = struct.unpack_from(fmt, raw, o[0])
        o[0] += n
        return v

    def array(count, width):
        if count < 0 or o[0] + 8 * count * width > len(raw):
            raise bad("truncated BAI index")
        a = np.frombuffer(raw, dtype="<u8", count=count * width, offset=o[0]).astype(np.uint64)
        o[0] += 8 * count * width
        return a
    (n_ref,) = take("<i")
    if n_ref < 0:
        raise bad("not a BAI index")
    bins, linear, meta = [], [], []
    for _ in range(n_ref):
        (n_bin,) = take("<i")
        b, m = {}, None
        for _ in range(n_bin):
            bin_no, n_chunk = take("<Ii")
            ch = array(n_chunk, 2).reshape(-1, 2)
            if bin_no == _PSEUDO_BIN:
                if n_chunk == 2:
                    m = tuple(int(v) for v in ch.reshape(-1))
            elif bin_no > _PSEUDO_BIN:
                raise bad("bin number %d" % bin_no)
            else:
                b[int(bin_no)] = np.concatenate([b[int(bin_no)], ch]) if int(bin_no) in b else ch
        (n_intv,) = take("<i")
        bins.append(b)
        meta.append(m)
        linear.append(array(n_intv, 1))
    n_no_coor = None
    if o[0] + 8 <= len(raw):
        (n_no_coor,) = take("<Q")
    if o[0] != len(raw):
        raise bad("bytes behind the end of the BAI index")
    return BamIndex(bins, linear, meta, n_no_coor, index_path)


def _reg2bins(beg: int, end: int):
    """SAMv1 §5.3: the bins that may hold a record overlapping [beg, end)."""
    end -= 1
    out = [0]
    for shift, off in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out.extend(range(off + (beg >> shift), off + (end >> shift) + 1))
    return out


def region_spans(index: BamIndex, regions) -> np.ndarray:
    """The query of SAMv1 §5.3 for ALL ``regions`` [(tid, beg, end), ...] at once: the chunks of the bins ``reg2bins(beg, end)``
    of every region, without those that end at or in front of the linear index's offset for window ``beg >> 14``, merged over
    all regions into sorted, disjoint spans of virtual offsets uint64 [K][2] (spans that overlap, touch or share a BGZF block
    become one).  Decoding the records that start inside the spans reaches every record that overlaps a region, each once —
    two windows whose chunk lists name the same record must not make it count twice."""
    chunks = []
    for tid, beg, end in regions:
        tid, beg, end = int(tid), max(int(beg), 0), min(int(end), 1 << 29)
        if not 0 <= tid < index.n_ref:
            raise ValueError("region on contig %d: the index has %d contigs" % (tid, index.n_ref))
        if end <= beg:
            continue
        lin = index.linear[tid]
        min_off = int(lin[min(beg >> 14, len(lin) - 1)]) if len(lin) else 0
        b = index.bins[tid]
        for k in _reg2bins(beg, end) if ((end - beg) >> 14) + 6 < len(b) else [k for k in b if _bin_overlaps(k, beg, end)]:
            ch = b.get(k)
            if ch is not None:
                chunks.append(ch[ch[:, 1] > np.uint64(min_off)])
    if not chunks:
        return np.zeros((0, 2), dtype=np.uint64)
    ch = np.concatenate(chunks)
    ch = ch[ch[:, 1] > ch[:, 0]]
    ch = ch[np.argsort(ch[:, 0], kind="stable")]
    out = []
    for a, b in ch.tolist():
        if out and (a >> 16) <= (out[-1][1] >> 16):
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return np.array(out, dtype=np.uint64).reshape(-1, 2)


_BIN_LEVELS = ((0, 29), (1, 26), (9, 23), (73, 20), (585, 17), (4681, 14))


def _bin_overlaps(k: int, beg: int, end: int) -> bool:
    for first, shift in reversed(_BIN_LEVELS):
        if k >= first:
            lo = (k - first) << shift
            return lo < end and lo + (1 << shift) > beg
    return False


def _index_beside(path: str, must: bool = False):
    for cand in (path + ".bai", path[:-4] + ".bai" if path.endswith(".bam") else None):
        if cand and os.path.exists(cand):
            return cand
    if must:
        raise _lib.CoralHipError("%s has no index beside it (bam.build_index writes one)" % path)
    return None


def _usable_index(path: str, index, n_ref: int) -> BamIndex:
    idx = index if isinstance(index, BamIndex) else read_index(os.fspath(index))
    if idx.n_ref != n_ref:
        raise _lib.CoralHipError("the index %s has %d contigs, the BAM header %d" % (idx.path or "", idx.n_ref, n_ref))
    return idx


def _regions_as_tids(regions, ref_names):
    tid_of = {c: k for k, c in enumerate(ref_names)}
    out = []
    for r in regions:
        if len(r) != 3:
            raise ValueError("a region is (chrom, start, stop), got %r" % (r,))
        chrom, a, b = r
        if chrom not in tid_of:
            raise ValueError("unknown contig %r" % (chrom,))
        if int(a) < 0 or int(b) < int(a):
            raise ValueError("bad region %r: needs 0 <= start <= stop" % (r,))
        out.append((tid_of[chrom], int(a), int(b)))
    return out


def write_bam_native(rec: Records, path: str, seed: int = 0, level: int = 1, n_threads: Optional[int] = None) -> None:
    """Serialise ``rec`` as a coordinate-sorted BAM with the native multi-threaded writer (coral_bam_write): what benchmarks
    and the larger tests use — same content rules as ``write_bam`` (deterministic ACGT with N at the listed positions, QUAL
    absent, NM / SA / CG tags), different (hash-made) bases."""
    L = _lib.lib()
    g = lambda x, dt: np.ascontiguousarray(x.cpu().numpy(), dtype=dt)
    i32 = lambda k: g(getattr(rec, k), np.int32)
    cols = [i32(k) for k in ("tid", "pos", "flag", "mapq", "qlen", "has_seq", "nm", "name_id", "n_cigar")]
    cigar_off, cigar = g(rec.cigar_off, np.int64), g(rec.cigar, np.int32).view(np.uint32)
    sa_off, sa, sa_nm = g(rec.sa_off, np.int64), g(rec.sa, np.int32), g(rec.sa_nm, np.int32)
    na_rec, na_pos = g(rec.nonacgt_rec, np.int64), g(rec.nonacgt_pos, np.int32)
    names = [s.encode() for s in rec.materialise_names()]
    name_arr = (C.c_char_p * max(len(names), 1))(*names)
    refs = [c.encode() for c in rec.header_chroms]
    ref_arr = (C.c_char_p * max(len(refs), 1))(*refs)
    ref_lens = np.ascontiguousarray(rec.header_lens, dtype=np.int32)
    ptr = lambda a: a.ctypes.data
    rc = L.coral_bam_write(path.encode(), rec.n, *[ptr(c) for c in cols], ptr(cigar_off), ptr(cigar), ptr(sa_off), ptr(sa), ptr(sa_nm),
                           len(na_rec), ptr(na_rec), ptr(na_pos), name_arr, len(refs), ref_arr, ptr(ref_lens), seed, level,
                           n_threads or default_threads())
    if rc != 0:
        raise _lib.CoralHipError("coral_bam_write(%s) failed (%d): %s" % (path, rc, L.coral_bam_last_error().decode()))


# ----------------------------------------------------------------------------------------------
# pure-Python writer (tests / tools)
# ----------------------------------------------------------------------------------------------
_SEQ_CODE = {65: 1, 67: 2, 71: 4, 84: 8, 78: 15}     # A C G T N


def _reg2bin(beg: int, end: int) -> int:
    end -= 1
    for shift, off in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return off + (beg >> shift)
    return 0


_BGZF_EMPTY = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")      # 28 bytes; at the end: the EOF marker


def _bgzf_blocks(data: bytes, level: int = 1, block_size: int = 0xff00, empty_block_every: int = 0):
    """BGZF blocks of ``data`` (``block_size`` payload bytes each, at most 0xff00) + the EOF marker.  ``empty_block_every`` = k:
    an empty block (the 28 bytes of the EOF marker, legal anywhere in a BGZF stream) after every k-th data block."""
    assert 0 < block_size <= 0xff00
    for n, i in enumerate(range(0, len(data), block_size)):
        chunk = data[i:i + block_size]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        comp = co.compress(chunk) + co.flush()
        bsize = len(comp) + 25
        yield (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize) + comp +
               struct.pack("<II", zlib.crc32(chunk) & 0xffffffff, len(chunk)))
        if empty_block_every and (n + 1) % empty_block_every == 0:
            yield _BGZF_EMPTY
    yield _BGZF_EMPTY      # BGZF EOF marker


_NM_PACK = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


def write_bam(rec: Records, path: str, seed: int = 0, long_cigar_as_cg: bool = True, fast_seq: bool = False, *, aux=None,
              nm_type="i", with_qual=False, block_size: int = 0xff00, empty_block_every: int = 0,
              header_comment: str = "", qual=None) -> None:
    """Serialise ``rec`` as a coordinate-sorted BAM (SEQ = deterministic ACGT with N at the listed non-ACGT
    positions, QUAL absent, tags NM:i and SA:Z; CIGARs with more than 65535 ops go to the CG:B,I tag).

    Options for files shaped like what aligners and htslib really write (tests of the decoders):
      ``aux(i)``        -> (raw tag bytes in FRONT of NM, raw tag bytes BEHIND the last tag) of record i: any SAM aux tags;
      ``nm_type``       one of c C s S i I (htslib stores integers in the smallest type that fits), None (no NM tag), or a
                        callable i -> one of these;
      ``with_qual``     real QUAL bytes (a hash of the position, 0..60) instead of 0xff; a callable i -> bool decides per record;
      ``qual``          a callable i -> the record's QUAL bytes (any values 0..255, exactly l_seq of them), or None for what
                        ``with_qual`` says;
      ``block_size``    payload bytes per BGZF block (small: header, records and tags straddle blocks);
      ``empty_block_every``  an empty BGZF block after every k-th block;
      ``header_comment``     extra @CO text (a long header spans several BGZF blocks)."""
    g = lambda x: x.cpu().numpy()
    tid, pos, flag, mapq, qlen, has_seq, nm, name_id, n_cigar = (g(getattr(rec, k)) for k in
                                                                ("tid", "pos", "flag", "mapq", "qlen", "has_seq", "nm", "name_id", "n_cigar"))
    cigar_off, cigar = g(rec.cigar_off), g(rec.cigar).view(np.uint32)
    sa_off, sa, sa_nm = g(rec.sa_off), g(rec.sa), g(rec.sa_nm)
    names = rec.materialise_names()
    na = {}
    for r, p in zip(g(rec.nonacgt_rec), g(rec.nonacgt_pos)):
        na.setdefault(int(r), []).append(int(p))
    out = bytearray()
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (c, l) for c, l in zip(rec.header_chroms, rec.header_lens))
    if header_comment:
        text += "".join("@CO\t%s\n" % line for line in header_comment.split("\n"))
    out += b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(rec.header_chroms))
    for c, l in zip(rec.header_chroms, rec.header_lens):
        out += struct.pack("<i", len(c) + 1) + c.encode() + b"\0" + struct.pack("<i", l)
    rng = np.random.default_rng(seed)
    lut = np.zeros(256, dtype=np.uint8)
    for k, v in _SEQ_CODE.items():
        lut[k] = v
    ref_adv = np.array([1, 0, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0])
    qry_adv = np.array([1, 1, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0])
    for i in range(rec.n):
        ops = cigar[cigar_off[i]: cigar_off[i] + n_cigar[i]]
        l_seq = int(qlen[i]) if has_seq[i] else 0
        seq_bytes = b""
        if l_seq:
            if fast_seq:            # decode benchmarks: any ACGT content will do
                s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, l_seq, dtype=np.uint8)]
            else:
                k = torch.arange(l_seq, dtype=torch.int64) + i * (1 << 22)
                s = np.frombuffer(b"ACGT", dtype=np.uint8)[(hash_u32(seed, S_SEQ, k) & 3).numpy()].copy()
            if i in na:     # reference position -> query offset through the CIGAR
                op, ln = ops & 15, (ops >> 4).astype(np.int64)
                r0 = int(pos[i]) + np.cumsum(ref_adv[op] * ln) - ref_adv[op] * ln
                q0 = np.cumsum(qry_adv[op] * ln) - qry_adv[op] * ln
                for p in na[i]:
                    j = np.nonzero((ref_adv[op] * qry_adv[op] == 1) & (r0 <= p) & (p < r0 + ln))[0][0]
                    s[q0[j] + (p - r0[j])] = 78
            code = lut[s]
            if l_seq & 1:
                code = np.append(code, 0)
            seq_bytes = ((code[0::2] << 4) | code[1::2]).astype(np.uint8).tobytes()
        front, behind = aux(i) if aux is not None else (b"", b"")
        ty = nm_type(i) if callable(nm_type) else nm_type
        tags = front + (b"NM" + ty.encode() + struct.pack(_NM_PACK[ty], int(nm[i])) if ty is not None else b"")
        if i in getattr(rec, "sa_text", {}):            # tests: verbatim SA text (odd CIGAR shapes)
            tags += b"SAZ" + rec.sa_text[i].encode() + b"\0"
        elif sa_off[i + 1] > sa_off[i]:
            ents = [sa_entry_string(sa[j], int(sa_nm[j]), rec.header_chroms) for j in range(sa_off[i], sa_off[i + 1])]
            tags += b"SAZ" + (";".join(ents) + ";").encode() + b"\0"
        rlen = int((ref_adv[ops & 15] * (ops >> 4)).sum()) if not (flag[i] & 4) else 0
        cig_field = ops
        if long_cigar_as_cg and len(ops) > 65535:
            tags += b"CGBI" + struct.pack("<I", len(ops)) + ops.astype("<u4").tobytes()
            cig_field = np.array([(l_seq << 4) | 4, (rlen << 4) | 3], dtype=np.uint32)
        name = names[name_id[i]].encode() + b"\0"
        body = struct.pack("<iiBBHHHiiii", int(tid[i]), int(pos[i]), len(name), int(mapq[i]),
                           _reg2bin(int(pos[i]), int(pos[i]) + max(1, rlen)), len(cig_field), int(flag[i]), l_seq, -1, -1, 0)
        given = qual(i) if qual is not None and l_seq else None
        if given is not None:
            qual_bytes = bytes(given)
            if len(qual_bytes) != l_seq:
                raise ValueError("write_bam: qual(%d) gave %d bytes for a record of %d bases" % (i, len(qual_bytes), l_seq))
        elif l_seq and (with_qual(i) if callable(with_qual) else with_qual):
            qual_bytes = ((hash_u32(seed, S_SEQ, torch.arange(l_seq, dtype=torch.int64) + (i + 7) * (1 << 22)) % 61).numpy()
                          .astype(np.uint8).tobytes())
        else:
            qual_bytes = b"\xff" * l_seq
        body += name + cig_field.astype("<u4").tobytes() + seq_bytes + qual_bytes + tags + behind
        out += struct.pack("<i", len(body)) + body
    with open(path, "wb") as fp:
        for blk in _bgzf_blocks(bytes(out), block_size=block_size, empty_block_every=empty_block_every):
            fp.write(blk)


# ----------------------------------------------------------------------------------------------
# copy number from the binned depth: coral_amd/cnv.py, at hand here beside binned_depth
# ----------------------------------------------------------------------------------------------
from .cnv import CopyNumberSegments, call_copy_number, find_seeds, segment_depth, write_seeds      # noqa: E402,F401
