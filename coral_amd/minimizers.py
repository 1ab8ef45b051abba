"""The minimizer sketch of a reference genome and its seed index (the `sketch` mode): the first stage of the mapper, made from the
FASTA file and the repetitive k-mers of the `kmers` mode by this project alone.

The reference maps its reads with ``winnowmap -W repetitive_k15.txt -ax map-ont ref.fa reads.fq`` (scripts/align_nanopore_reads.sh,
line 34).  The first thing every minimizer mapper does is the sketch: it picks the window minimizers of the reference, down-weights
the repetitive k-mers and keeps the result as a table sorted by hash, in which the reads' minimizers are looked up.  Here
``sketch_reference`` streams the FASTA through the GPU (coral_sketch.hip) or the host (``device="cpu"``, coral_sketch_host.h) and
returns a ``MinimizerIndex``; ``sketch_sequences`` sketches a batch of reads under the same rule through the same kernel, and
``MinimizerIndex.anchors`` expands their minimizers into anchors.  Chaining and base-level alignment are not here.  The rule is
coral_sketch_core.h's, stated in DESIGN.md §4.  Neither winnowmap nor minimap2 was available to compare with: winnowmap's
floating-point weighting (here a repetitive k-mer simply loses to every other one) and its handling of windows at ambiguous bases
(here an N keeps its place in the window with the key +infinity) are not pinned.
"""
from __future__ import annotations

import ctypes as C
import io
import numbers
import os
import time

import numpy as np

from . import _lib, fasta_stream
from .kmers import encode_kmer, reverse_complement

LAST_SKETCH = {}                     # seconds of the last sketch_reference, by stage
FORMAT_VERSION = 1
_UNKNOWN_SIZE_CAPACITY = 1 << 24     # entries the first attempt makes room for when the stream's size is not known
_M32 = np.uint64(0xFFFFFFFF)


def _check_arguments(k, w, chunk_bytes=16):
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= k <= 16:
        raise ValueError("k must be an integer in 1..16, got %r" % (k,))
    if isinstance(w, bool) or not isinstance(w, numbers.Integral) or not 1 <= w <= 256:
        raise ValueError("w must be an integer in 1..256, got %r" % (w,))
    if isinstance(chunk_bytes, bool) or not isinstance(chunk_bytes, numbers.Integral) or chunk_bytes < 16:
        raise ValueError("chunk_bytes must be an integer of at least 16, got %r" % (chunk_bytes,))


def hash64(x: int, k: int) -> int:
    """The rule's hash of a k-mer's integer (coral_sketch_core.h's hash64), in Python integers."""
    mask = (1 << (2 * k)) - 1
    x = (~x + (x << 21)) & mask
    x ^= x >> 24
    x = (x + (x << 3) + (x << 8)) & mask
    x ^= x >> 14
    x = (x + (x << 2) + (x << 4)) & mask
    x ^= x >> 28
    x = (x + (x << 31)) & mask
    return x


def weights_bitmap(weights, k: int):
    """The repetitive k-mers as the rule's bitmap: uint32 words, bit (canon & 31) of word canon >> 5 -> array, or None for None.
    ``weights``: a path to a `kmers` output file (``KMER<tab>COUNT`` lines), an iterable of k-mer strings or integers, or a bitmap
    that this function made.  Each k-mer is canonicalised.  ``ValueError``: a k-mer whose length is not ``k``."""
    if weights is None:
        return None
    words = max(1, (1 << (2 * k)) // 32)
    if isinstance(weights, np.ndarray) and weights.dtype == np.uint32:
        if len(weights) != words:
            raise ValueError("a weights bitmap of k = %d has %d words, got %d" % (k, words, len(weights)))
        return np.ascontiguousarray(weights)
    if isinstance(weights, (str, bytes, os.PathLike)):
        items = []
        with open(weights, "rb") as fp:
            for line in fp:
                line = line.strip()
                if line:
                    items.append(line.split(b"\t")[0].split(b" ")[0])
    else:
        items = list(weights)
    canon = np.empty(len(items), dtype=np.uint64)
    for i, item in enumerate(items):
        if isinstance(item, numbers.Integral) and not isinstance(item, bool):
            v = int(item)
            if not 0 <= v < 1 << (2 * k):
                raise ValueError("a k-mer of k = %d is an integer below 4^k, got %r" % (k, item))
        else:
            v = encode_kmer(item, k)
        canon[i] = min(v, reverse_complement(v, k))
    bitmap = np.zeros(words, dtype=np.uint32)
    np.bitwise_or.at(bitmap, (canon >> np.uint64(5)).astype(np.intp), (np.uint32(1) << (canon & np.uint64(31)).astype(np.uint32)))
    return bitmap


def _first_capacity(size, w):
    if size is None:
        return _UNKNOWN_SIZE_CAPACITY
    return size * 3 // (w + 1) + 4096                            # (random sequence selects 2 / (w + 1) of its positions)


def _sketch(source, k, w, bitmap, device, chunk_bytes, capacity=None):
    """One session over ``source`` -> (keys, values: torch int64 on the device, or numpy uint64; n; contig names; lengths; timings).
    A capacity that proves too small is replaced by what the session asked for and the stream is started over."""
    import torch
    L = _lib.lib()
    on_gpu = torch.device(device).type == "cuda"
    staging = min(int(chunk_bytes), 1 << 30)
    size, rewind = fasta_stream.stream_size(source)
    if size is not None:
        staging = max(16, min(staging, size))                    # (a small file needs no large pinned buffers)
    capacity = int(capacity) if capacity is not None else _first_capacity(size, w)
    t_all = time.perf_counter()
    dev = torch.device(device) if on_gpu else None
    dbitmap = None
    if bitmap is not None:
        dbitmap = torch.from_numpy(bitmap.view(np.int32)).to(dev) if on_gpu else bitmap
    for attempt in range(2):
        handle, t_open = C.c_void_p(), time.perf_counter()
        if on_gpu:
            keys, values = torch.empty(capacity, dtype=torch.int64, device=dev), torch.empty(capacity, dtype=torch.int64, device=dev)
            ws, stream = fasta_stream.gpu_side(dev, int(L.coral_sketch_workspace_bytes(staging)), "coral_sketch_workspace_bytes")
            rc = L.coral_sketch_open(k, w, dev.index or 0, dbitmap.data_ptr() if dbitmap is not None else None, keys.data_ptr(), values.data_ptr(), capacity, staging, ws.data_ptr(),
                                     ws.numel(), stream.cuda_stream, C.byref(handle))
        else:
            keys, values = np.empty(capacity, dtype=np.uint64), np.empty(capacity, dtype=np.uint64)
            rc = L.coral_sketch_open(k, w, -1, dbitmap.ctypes.data if dbitmap is not None else None, keys.ctypes.data, values.ctypes.data, capacity, 0, None, 0, None, C.byref(handle))
        fasta_stream.check(rc, "coral_sketch_open")
        open_s = time.perf_counter() - t_open                   # (the arrays, the workspace and the session's pinned buffers)
        stats, secs = (C.c_int64 * 8)(), (C.c_double * 4)()
        try:
            read_s, feed_s = fasta_stream.feed_all(L.coral_sketch_feed, handle, source, chunk_bytes)
            t0 = time.perf_counter()
            rc = L.coral_sketch_finish(handle, stats, secs)
            finish_s = time.perf_counter() - t0
            n_contigs, positions, n, names_bytes = int(stats[0]), int(stats[1]), int(stats[2]), int(stats[6])
            if rc == -3 and n > capacity and attempt == 0:       # CORAL_ERR_CAPACITY: n entries suffice
                if rewind is None:
                    raise _lib.CoralHipError("the stream has %d minimizers, more than the %d there was room for, and cannot be started over" % (n, capacity))
                capacity = n
                rewind()
                continue
            fasta_stream.check(rc, "coral_sketch_finish")
            lengths, name_off, blob = np.zeros(n_contigs, dtype=np.int64), np.zeros(n_contigs + 1, dtype=np.int64), np.zeros(max(names_bytes, 1), dtype=np.uint8)
            fasta_stream.check(L.coral_sketch_contigs(handle, n_contigs, lengths.ctypes.data, names_bytes, blob.ctypes.data, name_off.ctypes.data), "coral_sketch_contigs")
        finally:
            L.coral_sketch_close(handle)
        break
    text = blob.tobytes()
    names = [text[name_off[c]:name_off[c + 1]].decode("utf-8", "surrogateescape") for c in range(n_contigs)]
    timings = dict(open=open_s, read=read_s, feed=feed_s, finish_wait=finish_s, upload=float(secs[0]), symbols=float(secs[1]), sketch=float(secs[2]), last_tile=float(secs[3]),
                   attempts=attempt + 1, session=time.perf_counter() - t_all)
    return keys[:n], values[:n], n, names, lengths, positions, timings


def _split_values(values: np.ndarray):
    v = np.asarray(values, dtype=np.uint64)
    return (v >> np.uint64(32)).astype(np.int64), ((v & _M32) >> np.uint64(1)).astype(np.int64), (v & np.uint64(1)).astype(np.uint8)


class MinimizerIndex:
    """A reference's minimizers sorted by key: ``k``, ``w``, ``weighted`` (a weights list was given), ``contig_names`` and
    ``contig_lengths`` in file order, ``n`` entries.  The two arrays stay where they were made - device memory for a GPU sketch -
    until the object goes (or ``close()``)."""

    def __init__(self, k, w, weighted, contig_names, contig_lengths, keys, values, device):
        self.k, self.w, self.weighted = int(k), int(w), bool(weighted)
        self.contig_names, self.contig_lengths = list(contig_names), [int(l) for l in contig_lengths]
        self._keys, self._values, self._device = keys, values, device
        self.n = int(len(keys))

    def close(self):
        self._keys, self._values = None, None

    def _host(self):
        if self._keys is None:
            raise ValueError("the index is closed")
        if self._device is None:
            return self._keys, self._values
        return self._keys.cpu().numpy().view(np.uint64), self._values.cpu().numpy().view(np.uint64)

    def arrays(self):
        """(keys uint64, contigs int64, positions int64, strands uint8), sorted by key; ties in (contig, position) order."""
        keys, values = self._host()
        return (keys.copy(),) + _split_values(values)

    def _up(self, a, dtype):
        import torch
        a = np.ascontiguousarray(a, dtype=dtype)
        signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint8): np.uint8}[np.dtype(dtype)]
        return torch.from_numpy(a.view(signed)).to(self._device)

    def lookup(self, keys):
        """The entries of every key: (first, count), int64; ``first`` is the insertion point of a key without entries."""
        if self._keys is None:
            raise ValueError("the index is closed")
        q = np.ascontiguousarray(keys, dtype=np.uint64)
        L = _lib.lib()
        if self._device is None:
            first, count = np.zeros(len(q), dtype=np.int64), np.zeros(len(q), dtype=np.int64)
            fasta_stream.check(L.coral_sketch_lookup(-1, self._keys.ctypes.data, self.n, q.ctypes.data, len(q), first.ctypes.data, count.ctypes.data, None), "coral_sketch_lookup")
            return first, count
        import torch
        dq = self._up(q, np.uint64)
        first, count = torch.empty(len(q), dtype=torch.int64, device=self._device), torch.empty(len(q), dtype=torch.int64, device=self._device)
        stream = torch.cuda.current_stream(self._device)
        fasta_stream.check(L.coral_sketch_lookup(self._device.index or 0, self._keys.data_ptr(), self.n, dq.data_ptr(), len(q), first.data_ptr(), count.data_ptr(), stream.cuda_stream),
                           "coral_sketch_lookup")
        return first.cpu().numpy(), count.cpu().numpy()

    def anchors(self, queries, max_occ: int = 200):
        """Expands query minimizers - ``queries`` = (query, pos, strand, key) arrays, what ``sketch_sequences`` returns - into
        anchors -> (query, qpos, contig, rpos, strand) arrays: one anchor per index entry of every key that has at most ``max_occ``
        entries, ``strand`` = the query's strand ^ the entry's; query order, then index order.  ``max_occ = 200`` is an untuned
        default parameter, not a measured optimum."""
        if self._keys is None:
            raise ValueError("the index is closed")
        if isinstance(max_occ, bool) or not isinstance(max_occ, numbers.Integral) or max_occ < 0:
            raise ValueError("max_occ must be an integer of at least 0, got %r" % (max_occ,))
        query, qpos, qstrand, qkey = queries
        query, qpos = np.ascontiguousarray(query, dtype=np.uint32), np.ascontiguousarray(qpos, dtype=np.uint32)
        qstrand, qkey = np.ascontiguousarray(qstrand, dtype=np.uint8), np.ascontiguousarray(qkey, dtype=np.uint64)
        nq = len(qkey)
        if not len(query) == len(qpos) == len(qstrand) == nq:
            raise ValueError("the four query arrays differ in length")
        L = _lib.lib()
        n, cap = C.c_int64(0), 0
        if self._device is None:
            for _attempt in range(2):
                aq, ar = np.empty(cap, dtype=np.uint64), np.empty(cap, dtype=np.uint64)
                rc = L.coral_sketch_anchors(-1, self._keys.ctypes.data, self._values.ctypes.data, self.n, query.ctypes.data, qpos.ctypes.data, qstrand.ctypes.data, qkey.ctypes.data, nq,
                                            int(max_occ), cap, aq.ctypes.data, ar.ctypes.data, None, 0, None, C.byref(n))
                if rc == -3 and n.value > cap:                   # CORAL_ERR_CAPACITY: n anchors
                    cap = n.value
                    continue
                break
            fasta_stream.check(rc, "coral_sketch_anchors")
        else:
            import torch
            dev = self._device
            dq, dp, ds, dk = self._up(query, np.uint32), self._up(qpos, np.uint32), self._up(qstrand, np.uint8), self._up(qkey, np.uint64)
            ws = torch.empty(max(int(L.coral_sketch_anchors_workspace_bytes(nq)), 256), dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream(dev)
            for _attempt in range(2):
                taq, tar = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
                stream.synchronize()
                rc = L.coral_sketch_anchors(dev.index or 0, self._keys.data_ptr(), self._values.data_ptr(), self.n, dq.data_ptr(), dp.data_ptr(), ds.data_ptr(), dk.data_ptr(), nq,
                                            int(max_occ), cap, taq.data_ptr(), tar.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream, C.byref(n))
                if rc == -3 and n.value > cap:
                    cap = n.value
                    continue
                break
            fasta_stream.check(rc, "coral_sketch_anchors")
            aq, ar = taq.cpu().numpy().view(np.uint64), tar.cpu().numpy().view(np.uint64)
        aq, ar = aq[:n.value], ar[:n.value]
        contig, rpos, strand = _split_values(ar)
        return (aq >> np.uint64(32)).astype(np.int64), (aq & _M32).astype(np.int64), contig, rpos, strand

    def save(self, path) -> str:
        """An uncompressed .npz: ``meta`` (int64: format version, k, w, weighted), ``names`` (the contig names' bytes) with
        ``name_off``, ``lengths``, ``keys`` and ``values`` (contig << 32 | pos << 1 | strand)."""
        keys, values = self._host()
        blobs = [c.encode("utf-8", "surrogateescape") for c in self.contig_names]
        name_off = np.concatenate([[0], np.cumsum([len(b) for b in blobs], dtype=np.int64)]).astype(np.int64)
        with open(path, "wb") as fp:
            np.savez(fp, meta=np.array([FORMAT_VERSION, self.k, self.w, int(self.weighted)], dtype=np.int64), names=np.frombuffer(b"".join(blobs), dtype=np.uint8),
                     name_off=name_off, lengths=np.array(self.contig_lengths, dtype=np.int64), keys=keys, values=values)
        return path

    @classmethod
    def load(cls, path, device="cpu") -> "MinimizerIndex":
        """An index that ``save`` wrote, with its arrays on ``device``.  ``ValueError``: another format version."""
        import torch
        with np.load(path) as z:
            meta = z["meta"]
            if int(meta[0]) != FORMAT_VERSION:
                raise ValueError("%s: format version %d, this code reads %d" % (path, int(meta[0]), FORMAT_VERSION))
            text, name_off = z["names"].tobytes(), z["name_off"]
            names = [text[name_off[c]:name_off[c + 1]].decode("utf-8", "surrogateescape") for c in range(len(name_off) - 1)]
            keys, values, lengths = np.ascontiguousarray(z["keys"], dtype=np.uint64), np.ascontiguousarray(z["values"], dtype=np.uint64), z["lengths"].tolist()
        if torch.device(device).type == "cuda":
            dev = torch.device(device)
            return cls(meta[1], meta[2], meta[3], names, lengths, torch.from_numpy(keys.view(np.int64)).to(dev), torch.from_numpy(values.view(np.int64)).to(dev), dev)
        return cls(meta[1], meta[2], meta[3], names, lengths, keys, values, None)


def sketch_reference(fasta, k: int = 15, w: int = 50, weights=None, device="cuda:0", chunk_bytes: int = 64 << 20, _capacity=None) -> MinimizerIndex:
    """Sketches the FASTA ``fasta`` - a path (one ending in .gz is read through Python's ``gzip`` on the host) or an open binary
    file - and sorts the minimizers by key -> ``MinimizerIndex``.

    The k-mer at a position is valid when its ``k`` bytes are bases (ACGT, either case) and it differs from its reverse
    complement; its key is the hash of the smaller of the two, with one bit on top for a k-mer of ``weights`` (None, a `kmers`
    output file, or k-mer strings / integers), so that a repetitive k-mer is chosen only where a whole window is repetitive.  A
    position is a minimizer when its key is the smallest of some window of ``w`` consecutive positions of its contig (of all of
    them in a shorter contig); ties all count; N and other codes keep their place.  The defaults are the mapper's ``map-ont``
    values.  The file is read in pieces of ``chunk_bytes``; the result does not depend on them.  On a GPU ``device`` the pieces go
    through two pinned buffers, so that reading, the upload and the kernels (k_sketch_* of coral_sketch.hip) overlap, and the
    pairs are sorted by one radix sort; ``device="cpu"`` is the host backend, one thread.  Both give the same arrays.  The
    output is sized from the file's size; when the file has more minimizers (a homopolymer selects every position), the sketch
    is repeated once with what it asked for - a stream that cannot be started over raises ``CoralHipError`` instead.
    ``CoralHipError`` too: a sequence byte in front of the first header, a header without a name, a contig of 2^31 positions or
    more.  ``ValueError`` before any work: ``k`` outside 1..16, ``w`` outside 1..256, ``chunk_bytes`` below 16, a listed k-mer
    whose length is not ``k``."""
    _check_arguments(k, w, chunk_bytes)
    bitmap = weights_bitmap(weights, k)
    import torch
    L = _lib.lib()
    LAST_SKETCH.clear()
    t_all = time.perf_counter()
    keys, values, n, names, lengths, positions, timings = _sketch(fasta, int(k), int(w), bitmap, device, chunk_bytes, _capacity)
    t0 = time.perf_counter()
    if torch.device(device).type == "cuda":
        dev = torch.device(device)
        ws = torch.empty(max(int(L.coral_sketch_sort_workspace_bytes(n)), 256), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        stream.synchronize()
        fasta_stream.check(L.coral_sketch_sort(dev.index or 0, keys.data_ptr(), values.data_ptr(), n, int(k), ws.data_ptr(), ws.numel(), stream.cuda_stream), "coral_sketch_sort")
        keys, values = keys.clone(), values.clone()              # (the arrays sized for the capacity go)
    else:
        dev = None
        keys, values = np.ascontiguousarray(keys), np.ascontiguousarray(values)
        fasta_stream.check(L.coral_sketch_sort(-1, keys.ctypes.data, values.ctypes.data, n, int(k), None, 0, None), "coral_sketch_sort")
    LAST_SKETCH.update(timings, sort=time.perf_counter() - t0, wall=time.perf_counter() - t_all)
    out = MinimizerIndex(k, w, bitmap is not None, names, lengths.tolist(), keys, values, dev)
    out.positions = positions
    return out


def sketch_sequences(seqs, k: int = 15, w: int = 50, weights=None, device="cuda:0"):
    """Sketches a batch of byte strings under the rule of ``sketch_reference`` and through the same session, each string one contig
    -> (query uint32, pos uint32, strand uint8, key uint64) in (query, pos) order: the input of ``MinimizerIndex.anchors``.
    ``ValueError``: a string that holds '>', '\\n' or '\\r'."""
    _check_arguments(k, w)
    bitmap = weights_bitmap(weights, k)
    parts = []
    for i, s in enumerate(seqs):
        s = s.encode("ascii") if isinstance(s, str) else bytes(s)
        if b">" in s or b"\n" in s or b"\r" in s:
            raise ValueError("sequence %d holds '>', '\\n' or '\\r'" % i)
        parts.append(b">%d\n%s\n" % (i, s))
    text = b"".join(parts)
    if not text:
        return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint64)
    keys, values, _n, _names, _lengths, _positions, _t = _sketch(io.BytesIO(text), int(k), int(w), bitmap, device, max(16, min(len(text), 64 << 20)))
    if not isinstance(keys, np.ndarray):
        keys, values = keys.cpu().numpy().view(np.uint64), values.cpu().numpy().view(np.uint64)
    query, pos, strand = _split_values(values)
    return query.astype(np.uint32), pos.astype(np.uint32), strand, keys.copy()


def write_index(fasta, output, k: int = 15, w: int = 50, weights=None, device="cuda:0", chunk_bytes: int = 64 << 20) -> MinimizerIndex:
    """``sketch_reference`` of ``fasta``, then ``save`` to ``output``: the `sketch` mode in one call."""
    idx = sketch_reference(fasta, k, w, weights, device, chunk_bytes)
    t0 = time.perf_counter()
    idx.save(output)
    LAST_SKETCH["write"] = time.perf_counter() - t0
    return idx
