"""The repetitive k-mers of a reference genome (the `kmers` mode): the list the mapper takes with ``-W``, made from the FASTA file by
this project alone.

The reference gets it from lines 29-30 of scripts/align_nanopore_reads.sh (``meryl count k=15 output merylDB ref.fa`` and ``meryl
print greater-than distinct=0.9998 merylDB > repetitive_k15.txt``).  Here ``count_kmers`` counts every k-mer into one
direct-addressed table of 4^k uint32 counters - 4 GiB at k = 15 - on the GPU (coral_kmer.hip) or on the host (``device="cpu"``,
coral_kmer_host.h), and ``KmerCounts.write`` prints the k-mers above the ``distinct=`` threshold.  The rule is coral_kmer_core.h's,
stated in DESIGN.md §4.  Meryl was not available to compare with: its rounding of ``distinct=``, its choice between a k-mer and its
reverse complement and its print order are not pinned; the file's meaning, a set of repetitive k-mers with counts, does not
depend on them.
"""
from __future__ import annotations

import ctypes as C
import numbers
import re
import time

import numpy as np

from . import _lib, fasta_stream

LAST_COUNT = {}                      # seconds of the last count_kmers / select / write, by stage
_FIRST_SELECT = 1 << 16              # rows the first coral_kmer_select makes room for
_LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
_DECIMAL = re.compile(r"^(\d+)(?:\.(\d*))?$|^\.(\d+)$")


def parse_distinct(distinct):
    """``distinct`` as the exact fraction P / 10^d -> (P, d).  Decimal text; a float goes through ``repr``.  ``ValueError`` when it
    is not decimal or lies outside [0, 1]."""
    if isinstance(distinct, bool) or not isinstance(distinct, (str, numbers.Real)):
        raise ValueError("distinct must be decimal text or a number, got %r" % (distinct,))
    text = distinct if isinstance(distinct, str) else repr(distinct)
    m = _DECIMAL.match(text.strip())
    if not m:
        raise ValueError("distinct must be a decimal in [0, 1] such as '0.9998', got %r" % (distinct,))
    whole, frac = (m.group(1), m.group(2) or "") if m.group(1) is not None else ("0", m.group(3))
    P, d = int(whole + frac), len(frac)
    if P > 10 ** d:
        raise ValueError("distinct must lie in [0, 1], got %r" % (distinct,))
    return P, d


def threshold_of(values, numbers_, distinct="0.9998") -> int:
    """The threshold t of ``distinct`` = P / 10^d on a histogram (rising count values, numbers of distinct k-mers): with need =
    ceil(P * distinct k-mers / 10^d), the smallest count c >= 0 such that at least ``need`` distinct k-mers have a count <= c.
    Integers only."""
    P, d = parse_distinct(distinct)
    nums = [int(x) for x in numbers_]
    need = -((-P * sum(nums)) // 10 ** d)
    if need <= 0:
        return 0
    seen = 0
    for v, x in zip(values, nums):
        seen += x
        if seen >= need:
            return int(v)
    raise AssertionError("need exceeds the number of distinct k-mers")


def kmer_text(kmers: np.ndarray, k: int) -> np.ndarray:
    """uint64 k-mers -> their letters, uint8 [n][k] (first base in the top bits, A < C < G < T)."""
    shifts = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
    return _LETTERS[((np.asarray(kmers, dtype=np.uint64)[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.intp)]


def encode_kmer(seq, k: int) -> int:
    """A k-mer's letters (str or bytes, either case) -> its integer; ``ValueError`` for a wrong length or a letter outside ACGT."""
    text = seq.decode("ascii", "replace") if isinstance(seq, (bytes, bytearray)) else seq
    if not isinstance(text, str) or len(text) != k:
        raise ValueError("a k-mer of k = %d needs %d letters, got %r" % (k, k, seq))
    out = 0
    for ch in text.upper():
        code = "ACGT".find(ch)
        if code < 0:
            raise ValueError("a k-mer has the letters ACGT only, got %r" % (seq,))
        out = out << 2 | code
    return out


def reverse_complement(kmer: int, k: int) -> int:
    out = 0
    for _ in range(k):
        out = out << 2 | (3 - (kmer & 3))
        kmer >>= 2
    return out


def _check_arguments(k, chunk_bytes):
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= k <= 16:
        raise ValueError("k must be an integer in 1..16, got %r" % (k,))
    if isinstance(chunk_bytes, bool) or not isinstance(chunk_bytes, numbers.Integral) or chunk_bytes < 16:
        raise ValueError("chunk_bytes must be an integer of at least 16, got %r" % (chunk_bytes,))


def _check_selection(distinct, greater_than):
    if distinct is not None and greater_than is not None:
        raise ValueError("give distinct or greater_than, not both")
    if greater_than is not None and (isinstance(greater_than, bool) or not isinstance(greater_than, numbers.Integral) or greater_than < 0):
        raise ValueError("greater_than must be an integer of at least 0, got %r" % (greater_than,))
    if greater_than is None:
        parse_distinct("0.9998" if distinct is None else distinct)


class KmerCounts:
    """A finished count: ``k``, ``canonical``, ``n_sequences`` (header lines), ``n_bases`` (valid bases), ``total`` (k-mers counted),
    ``distinct`` (non-zero entries), ``max_count``.  The table stays where it was counted - device memory for a GPU count - until
    the object goes (or ``close()``)."""

    def __init__(self, handle, k, canonical, device, stats, keep):
        self._handle, self._keep, self._device = handle, keep, device
        self.k, self.canonical = int(k), bool(canonical)
        self.n_sequences, self.n_bases, self.total, self.distinct, self._hist_rows, self.max_count = (int(x) for x in stats[:6])
        self._hist = None

    def close(self):
        if self._handle is not None:
            _lib.lib().coral_kmer_close(self._handle)
            self._handle, self._keep = None, None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise _lib.CoralHipError("%s failed (%d): %s" % (what, rc, _lib.lib().coral_bam_last_error().decode()))

    def histogram(self):
        """The exact histogram: two int64 arrays, the rising count values and the numbers of distinct k-mers with them."""
        if self._hist is None:
            values, nums = np.zeros(self._hist_rows, dtype=np.int64), np.zeros(self._hist_rows, dtype=np.int64)
            self._check(_lib.lib().coral_kmer_histogram(self._handle, self._hist_rows, values.ctypes.data, nums.ctypes.data), "coral_kmer_histogram")
            self._hist = (values, nums)
        return self._hist[0].copy(), self._hist[1].copy()

    def threshold(self, distinct="0.9998") -> int:
        """The count t of ``distinct``: the k-mers with a count above t are the repetitive ones (``threshold_of``)."""
        values, nums = self.histogram()
        return threshold_of(values.tolist(), nums.tolist(), distinct)

    def select(self, greater_than: int):
        """The k-mers with a count above ``greater_than``: (uint64 k-mers, rising; uint32 counts)."""
        if isinstance(greater_than, bool) or not isinstance(greater_than, numbers.Integral) or greater_than < 0:
            raise ValueError("greater_than must be an integer of at least 0, got %r" % (greater_than,))
        L = _lib.lib()
        t0 = time.perf_counter()
        cap, n = _FIRST_SELECT, C.c_int64(0)
        for _attempt in range(2):
            if self._device is None:
                kmers, counts = np.empty(cap, dtype=np.uint64), np.empty(cap, dtype=np.uint32)
                rc = L.coral_kmer_select(self._handle, int(greater_than), cap, kmers.ctypes.data, counts.ctypes.data, C.byref(n))
            else:
                import torch
                kd, cd = torch.empty(cap, dtype=torch.int64, device=self._device), torch.empty(cap, dtype=torch.int32, device=self._device)
                torch.cuda.current_stream(self._device).synchronize()
                rc = L.coral_kmer_select(self._handle, int(greater_than), cap, kd.data_ptr(), cd.data_ptr(), C.byref(n))
                if rc == 0:
                    kmers, counts = kd[:n.value].cpu().numpy().view(np.uint64), cd[:n.value].cpu().numpy().view(np.uint32)
            if rc == -3 and n.value > cap:                       # CORAL_ERR_CAPACITY: n rows suffice
                cap = n.value
                continue
            break
        self._check(rc, "coral_kmer_select")
        LAST_COUNT["select"] = time.perf_counter() - t0
        return kmers[:n.value].copy(), counts[:n.value].copy()

    def counts(self, seqs) -> np.ndarray:
        """The counts of k-mers given as letters, uint32; under the canonical form when the count is canonical."""
        idx = []
        for s in seqs:
            v = encode_kmer(s, self.k)
            idx.append(min(v, reverse_complement(v, self.k)) if self.canonical else v)
        idx = np.array(idx, dtype=np.uint64)
        out = np.zeros(len(idx), dtype=np.uint32)
        if len(idx) == 0:
            return out
        L = _lib.lib()
        if self._device is None:
            self._check(L.coral_kmer_lookup(self._handle, idx.ctypes.data, len(idx), out.ctypes.data), "coral_kmer_lookup")
            return out
        import torch
        di = torch.from_numpy(idx.view(np.int64)).to(self._device)
        do = torch.empty(len(idx), dtype=torch.int32, device=self._device)
        torch.cuda.current_stream(self._device).synchronize()
        self._check(L.coral_kmer_lookup(self._handle, di.data_ptr(), len(idx), do.data_ptr()), "coral_kmer_lookup")
        return do.cpu().numpy().view(np.uint32)

    def count(self, seq) -> int:
        return int(self.counts([seq])[0])

    def table(self) -> np.ndarray:
        """The whole table on the host, uint32 [4^k] (a copy; for small k)."""
        if self._device is None:
            return self._keep[0].copy()
        return self._keep[0].cpu().numpy().view(np.uint32)

    def write(self, path, distinct=None, greater_than=None, both_strands: bool = False) -> int:
        """Writes one line ``KMER<tab>COUNT`` per k-mer with a count above the threshold of ``distinct`` (default "0.9998") or above
        ``greater_than``, in rising order of the k-mer's integer (with A < C < G < T: lexicographic); returns the number of lines.
        ``both_strands``: each k-mer that is not its own reverse complement is followed by that, with the same count - for a consumer
        that does not canonicalise what it reads."""
        _check_selection(distinct, greater_than)
        t = int(greater_than) if greater_than is not None else self.threshold("0.9998" if distinct is None else distinct)
        kmers, counts = self.select(t)
        t0 = time.perf_counter()
        k = self.k
        text = kmer_text(kmers, k)
        fwd = np.ascontiguousarray(text).view("S%d" % k).ravel().tolist() if len(kmers) else []
        cnt = counts.tolist()
        if both_strands and len(kmers):
            codes = ((kmers[:, None] >> (2 * (k - 1 - np.arange(k))).astype(np.uint64)[None, :]) & np.uint64(3)).astype(np.intp)
            rev = np.ascontiguousarray(_LETTERS[3 - codes[:, ::-1]]).view("S%d" % k).ravel().tolist()
            lines = [b"%s\t%d\n" % (a, c) if a == b else b"%s\t%d\n%s\t%d\n" % (a, c, b, c) for a, b, c in zip(fwd, rev, cnt)]
            n_lines = len(fwd) + sum(a != b for a, b in zip(fwd, rev))
        else:
            lines = [b"%s\t%d\n" % (a, c) for a, c in zip(fwd, cnt)]
            n_lines = len(fwd)
        with open(path, "wb") as fp:
            fp.write(b"".join(lines))
        LAST_COUNT["write"] = time.perf_counter() - t0
        return n_lines

    def write_histogram(self, path) -> int:
        """``count<tab>kmers`` lines, rising (what `meryl histogram` is used for); returns the number of lines."""
        values, nums = self.histogram()
        with open(path, "w", newline="") as fp:
            fp.write("".join("%d\t%d\n" % (v, x) for v, x in zip(values.tolist(), nums.tolist())))
        return len(values)


def count_kmers(fasta, k: int = 15, canonical: bool = True, device="cuda:0", chunk_bytes: int = 64 << 20, _bases_before: int = 0) -> KmerCounts:
    """Counts every k-mer of the FASTA ``fasta`` - a path (one ending in .gz is read through Python's ``gzip`` on the host, which is
    slow and not the hot path) or an open binary file - into a table of 4^k uint32 counters -> ``KmerCounts``.

    A k-mer is a window of ``k`` bases (ACGT, either case) without a break; a header line, N, IUPAC codes and any other byte are
    breaks; '\\n' and '\\r' are skipped.  ``canonical``: a window counts under the smaller of itself and its reverse complement (as
    ``meryl count``); else under itself.  The file is read in pieces of ``chunk_bytes``; the result does not depend on them.  On
    a GPU ``device`` the pieces go through two pinned buffers, so that reading, the upload and the kernels (k_kmer_* of
    coral_kmer.hip) overlap; ``device="cpu"`` is the host backend, one thread.  Both give the same table.  A stream of 2^32 bases
    or more is refused (``CoralHipError``): no counter can wrap.  ``ValueError`` before any work: ``k`` outside 1..16,
    ``chunk_bytes`` below 16."""
    _check_arguments(k, chunk_bytes)
    import torch
    L = _lib.lib()
    on_gpu = torch.device(device).type == "cuda"
    entries = 1 << (2 * k)
    staging = min(int(chunk_bytes), 1 << 30)
    handle = C.c_void_p()
    LAST_COUNT.clear()
    t_all = time.perf_counter()
    if on_gpu:
        dev = torch.device(device)
        table = torch.zeros(entries, dtype=torch.int32, device=dev)
        ws, stream = fasta_stream.gpu_side(dev, int(L.coral_kmer_workspace_bytes(k, staging)), "coral_kmer_workspace_bytes")
        keep = (table, ws)
        rc = L.coral_kmer_open(k, int(bool(canonical)), dev.index or 0, table.data_ptr(), staging, ws.data_ptr(), ws.numel(), stream.cuda_stream, int(_bases_before),
                               C.byref(handle))
    else:
        dev = None
        table = np.zeros(entries, dtype=np.uint32)
        keep = (table,)
        rc = L.coral_kmer_open(k, int(bool(canonical)), -1, table.ctypes.data, 0, None, 0, None, int(_bases_before), C.byref(handle))
    fasta_stream.check(rc, "coral_kmer_open")
    LAST_COUNT["zero_table"] = time.perf_counter() - t_all
    stats, secs = (C.c_int64 * 8)(), (C.c_double * 4)()
    try:
        read_s, feed_s = fasta_stream.feed_all(L.coral_kmer_feed, handle, fasta, chunk_bytes)
        t0 = time.perf_counter()
        fasta_stream.check(L.coral_kmer_finish(handle, stats, secs), "coral_kmer_finish")
        finish_s = time.perf_counter() - t0
    except BaseException:
        L.coral_kmer_close(handle)
        raise
    LAST_COUNT.update(read=read_s, feed=feed_s, finish_wait=finish_s, upload=float(secs[0]), classify_compact=float(secs[1]), count=float(secs[2]),
                      statistics=float(secs[3]), wall=time.perf_counter() - t_all)
    return KmerCounts(handle, k, canonical, dev, stats, keep)


def repetitive_kmers(fasta, output, k: int = 15, distinct=None, greater_than=None, canonical: bool = True, both_strands: bool = False, device="cuda:0",
                     chunk_bytes: int = 64 << 20) -> KmerCounts:
    """``count_kmers`` of ``fasta``, then ``write`` to ``output``: lines 29-30 of the reference's scripts/align_nanopore_reads.sh in
    one call.  The arguments are theirs; the errors of both come before any work.  Returns the ``KmerCounts`` (``lines_written``
    and ``threshold_used`` set)."""
    _check_arguments(k, chunk_bytes)
    _check_selection(distinct, greater_than)
    kc = count_kmers(fasta, k, canonical, device, chunk_bytes)
    kc.threshold_used = int(greater_than) if greater_than is not None else kc.threshold("0.9998" if distinct is None else distinct)
    kc.lines_written = kc.write(output, greater_than=kc.threshold_used, both_strands=both_strands)
    return kc
