"""The composition of a reference genome per bin (the `composition` mode): how many G/C, A/T and soft-masked bases each bin of
the binned depth holds, counted from the FASTA file the mapper was given.

The reference gets these columns from the table that scripts/call_cnvs.sh:12-17 hands to CNVkit (``cnvkit.py batch --seq-method
wgs --reference hg38full_ref_5k.cnn``: ``gc`` and ``rmask`` per bin).  Here ``reference_composition`` streams the FASTA through
the GPU (coral_comp.hip) or the host (``device="cpu"``, coral_comp_host.h) and returns a ``Composition``; both give the same
integers.  The rule is coral_comp_core.h's, stated in DESIGN.md §4.  CNVkit was not available to compare with: its ``reference``
command is not pinned.
"""
from __future__ import annotations

import ctypes as C
import numbers
import time

import numpy as np

from . import _lib, fasta_stream

LAST_COMPOSITION = {}                # seconds of the last reference_composition, by stage
MAX_BINS = 1 << 28
MAX_BIN_SIZE = (1 << 31) - 1
COLUMNS = ("chromosome", "start", "end", "gene", "gc", "rmask", "gc_bases", "at_bases", "masked_bases")


def _check_arguments(bin_size, chunk_bytes):
    if isinstance(bin_size, bool) or not isinstance(bin_size, numbers.Integral) or not 1 <= bin_size <= MAX_BIN_SIZE:
        raise ValueError("bin_size must be an integer in 1 .. 2^31 - 1, got %r" % (bin_size,))
    if isinstance(chunk_bytes, bool) or not isinstance(chunk_bytes, numbers.Integral) or chunk_bytes < 16:
        raise ValueError("chunk_bytes must be an integer of at least 16, got %r" % (chunk_bytes,))


class Composition:
    """The finished count: ``chroms`` / ``lengths`` in file order, ``bin_size``, ``bin_off`` (contig c has the bins bin_off[c] ..
    bin_off[c + 1], ceil(length / bin_size) of them: the bins of ``bam.BinnedDepth``) and the uint32 tables ``gc`` (G C g c),
    ``at`` (A T a t) and ``masked`` (a..z) per bin.  A bin's uncalled positions are its length - gc - at."""

    def __init__(self, chroms, lengths, bin_size, gc, at, masked):
        self.chroms, self.lengths, self.bin_size = list(chroms), [int(l) for l in lengths], int(bin_size)
        if len(set(self.chroms)) != len(self.chroms):
            seen = set()
            twice = next(c for c in self.chroms if c in seen or seen.add(c))
            raise ValueError("the contig name %r stands in the FASTA more than once" % (twice,))
        self.bin_off = np.concatenate([[0], np.cumsum([(l + self.bin_size - 1) // self.bin_size for l in self.lengths], dtype=np.int64)]).astype(np.int64)
        self.gc, self.at, self.masked = (np.ascontiguousarray(x, dtype=np.uint32) for x in (gc, at, masked))
        if not len(self.gc) == len(self.at) == len(self.masked) == self.bin_off[-1] or len(self.chroms) != len(self.lengths):
            raise ValueError("Composition: the tables do not fit the contigs and the bin size")
        self._tid = {c: k for k, c in enumerate(self.chroms)}
        self.positions = int(sum(self.lengths))

    @property
    def n_bins(self) -> int:
        return int(self.bin_off[-1])

    def bin_lengths(self) -> np.ndarray:
        """The positions of every bin, int64: ``bin_size`` but for a contig's last bin."""
        out = np.full(self.n_bins, self.bin_size, dtype=np.int64)
        for c, length in enumerate(self.lengths):
            if length % self.bin_size:
                out[self.bin_off[c + 1] - 1] = length % self.bin_size
        return out

    def gc_fraction(self) -> np.ndarray:
        """gc / (gc + at) per bin as float64; nan where no base was called."""
        called = self.gc.astype(np.float64) + self.at.astype(np.float64)
        out = np.full(self.n_bins, np.nan)
        np.divide(self.gc.astype(np.float64), called, out=out, where=called > 0)
        return out

    def masked_fraction(self) -> np.ndarray:
        """masked / the bin's length per bin as float64 (CNVkit's rmask)."""
        return self.masked.astype(np.float64) / self.bin_lengths().astype(np.float64)

    def genome_gc(self) -> float:
        called = int(self.gc.sum(dtype=np.int64)) + int(self.at.sum(dtype=np.int64))
        return int(self.gc.sum(dtype=np.int64)) / called if called else float("nan")

    def write(self, path) -> str:
        """Tab-separated: a line ``#bin_size<tab>N`` and a line ``#contig<tab>name<tab>length`` per contig in file order, the column
        names, then one row per bin: chromosome, start, end, gene ('-'), gc and rmask (the two fractions, as CNVkit's reference table
        names them; gc is 'nan' where nothing was called), and the three counters, which ``read`` takes."""
        gcf, mf, lens = self.gc_fraction(), self.masked_fraction(), self.bin_lengths()
        with open(path, "w", newline="") as fp:
            fp.write("#bin_size\t%d\n" % self.bin_size)
            fp.write("".join("#contig\t%s\t%d\n" % (c, l) for c, l in zip(self.chroms, self.lengths)))
            fp.write("\t".join(COLUMNS) + "\n")
            for c, name in enumerate(self.chroms):
                lo, hi = int(self.bin_off[c]), int(self.bin_off[c + 1])
                starts = np.arange(hi - lo, dtype=np.int64) * self.bin_size
                fp.write("".join("%s\t%d\t%d\t-\t%r\t%r\t%d\t%d\t%d\n" % (name, a, a + n, g, m, x, y, z)
                                 for a, n, g, m, x, y, z in zip(starts.tolist(), lens[lo:hi].tolist(), gcf[lo:hi].tolist(), mf[lo:hi].tolist(), self.gc[lo:hi].tolist(),
                                                                self.at[lo:hi].tolist(), self.masked[lo:hi].tolist())))
        return path

    @classmethod
    def read(cls, path) -> "Composition":
        """A table that ``write`` made; the integer columns come back exactly.  ``ValueError`` for other columns, a missing
        ``#bin_size`` line or rows that are not the contigs' bins in order."""
        chroms, lengths, rows, bin_size, head = [], [], [], None, None
        with open(path, "r", newline="") as fp:
            for line in fp:
                f = line.rstrip("\n").split("\t")
                if head is None and f[0] == "#bin_size" and len(f) == 2:
                    bin_size = int(f[1])
                elif head is None and f[0] == "#contig" and len(f) == 3:
                    chroms.append(f[1])
                    lengths.append(int(f[2]))
                elif head is None:
                    head = tuple(f)
                    if head != COLUMNS:
                        raise ValueError("%s: the columns are not %s" % (path, " ".join(COLUMNS)))
                elif len(f) != len(COLUMNS):
                    raise ValueError("%s: a row with %d columns" % (path, len(f)))
                else:
                    rows.append((f[0], int(f[1]), int(f[2]), int(f[6]), int(f[7]), int(f[8])))
        if bin_size is None or head is None:
            raise ValueError("%s: no #bin_size line or no column names" % (path,))
        out = cls(chroms, lengths, bin_size, [r[3] for r in rows], [r[4] for r in rows], [r[5] for r in rows])
        lens, k = out.bin_lengths().tolist(), 0
        for c, name in enumerate(out.chroms):
            for b in range(int(out.bin_off[c + 1] - out.bin_off[c])):
                if rows[k][:3] != (name, b * bin_size, b * bin_size + lens[k]):
                    raise ValueError("%s: row %d is not bin %d of %s" % (path, k, b, name))
                k += 1
        return out

    def for_depth(self, depth):
        """(gc, at, masked) laid out along the contigs of ``depth`` (a ``bam.BinnedDepth``), matched by name; contigs of the
        FASTA that the depth lacks are dropped.  ``ValueError``: another bin size, a contig of the depth that the FASTA lacks, a
        contig of another length."""
        if int(depth.bin_size) != self.bin_size:
            raise ValueError("the composition has bins of %d positions, the depth of %d" % (self.bin_size, depth.bin_size))
        parts = []
        for name, length in zip(depth.chroms, depth.lengths):
            if name not in self._tid:
                raise ValueError("the contig %r of the depth is not in the FASTA" % (name,))
            c = self._tid[name]
            if self.lengths[c] != int(length):
                raise ValueError("the contig %r has %d positions in the FASTA and %d in the depth" % (name, self.lengths[c], length))
            parts.append(slice(int(self.bin_off[c]), int(self.bin_off[c + 1])))
        pick = lambda x: np.concatenate([x[p] for p in parts]) if parts else x[:0].copy()
        return pick(self.gc), pick(self.at), pick(self.masked)


def reference_composition(fasta, bin_size: int = 1000, device="cuda:0", chunk_bytes: int = 64 << 20, _capacity=None) -> Composition:
    """Counts G/C, A/T and soft-masked positions per bin of ``bin_size`` along every contig of the FASTA ``fasta`` - a path (one
    ending in .gz is read through Python's ``gzip`` on the host) or an open binary file -> ``Composition``.

    Every byte of a sequence line but '\\n' and '\\r' is a position (``samtools faidx`` coordinates: N and IUPAC codes too); a
    contig's name is its header line up to the first blank.  The file is read in pieces of ``chunk_bytes``; the result does not
    depend on them.  On a GPU ``device`` the pieces go through two pinned buffers, so that reading, the upload and the kernels
    (k_comp_* of coral_comp.hip) overlap; ``device="cpu"`` is the host backend, one thread.  The tables are sized from the
    file's size; when the file needs more bins (many short contigs, a .gz), the count is repeated once with what it asked for.
    ``CoralHipError``: a sequence byte in front of the first header, a header without a name, more than 2^28 bins.
    ``ValueError`` before any work: ``bin_size`` outside 1 .. 2^31 - 1, ``chunk_bytes`` below 16; afterwards: a name that stands
    twice."""
    _check_arguments(bin_size, chunk_bytes)
    import torch
    L = _lib.lib()
    on_gpu = torch.device(device).type == "cuda"
    staging = min(int(chunk_bytes), 1 << 30)
    size, rewind = fasta_stream.stream_size(fasta)
    if size is not None:
        staging = max(16, min(staging, size))                    # (a small file needs no large pinned buffers)
    capacity = int(_capacity) if _capacity is not None else min(MAX_BINS, (size if size is not None else 1 << 30) // int(bin_size) + 4096)
    LAST_COMPOSITION.clear()
    t_all = time.perf_counter()
    for attempt in range(2):
        handle = C.c_void_p()
        if on_gpu:
            dev = torch.device(device)
            tables = torch.zeros((3, capacity), dtype=torch.int32, device=dev)
            ws, stream = fasta_stream.gpu_side(dev, int(L.coral_comp_workspace_bytes(staging)), "coral_comp_workspace_bytes")
            rc = L.coral_comp_open(int(bin_size), dev.index or 0, tables[0].data_ptr(), tables[1].data_ptr(), tables[2].data_ptr(), capacity, staging, ws.data_ptr(), ws.numel(),
                                   stream.cuda_stream, C.byref(handle))
        else:
            tables = np.zeros((3, capacity), dtype=np.uint32)
            rc = L.coral_comp_open(int(bin_size), -1, tables[0].ctypes.data, tables[1].ctypes.data, tables[2].ctypes.data, capacity, 0, None, 0, None, C.byref(handle))
        fasta_stream.check(rc, "coral_comp_open")
        stats, secs = (C.c_int64 * 8)(), (C.c_double * 4)()
        try:
            read_s, feed_s = fasta_stream.feed_all(L.coral_comp_feed, handle, fasta, chunk_bytes)
            t0 = time.perf_counter()
            rc = L.coral_comp_finish(handle, stats, secs)
            finish_s = time.perf_counter() - t0
            n_contigs, positions, bins, names_bytes = int(stats[0]), int(stats[1]), int(stats[2]), int(stats[6])
            if rc == -3 and attempt == 0 and capacity < bins <= MAX_BINS and rewind is not None:      # CORAL_ERR_CAPACITY: `bins` suffice
                capacity = bins
                rewind()
                continue
            fasta_stream.check(rc, "coral_comp_finish")
            lengths, name_off, blob = np.zeros(n_contigs, dtype=np.int64), np.zeros(n_contigs + 1, dtype=np.int64), np.zeros(max(names_bytes, 1), dtype=np.uint8)
            fasta_stream.check(L.coral_comp_contigs(handle, n_contigs, lengths.ctypes.data, names_bytes, blob.ctypes.data, name_off.ctypes.data), "coral_comp_contigs")
        finally:
            L.coral_comp_close(handle)
        break
    t0 = time.perf_counter()
    host = tables[:, :bins].cpu().numpy().view(np.uint32) if on_gpu else tables[:, :bins]
    text = blob.tobytes()
    chroms = [text[name_off[c]:name_off[c + 1]].decode("utf-8", "surrogateescape") for c in range(n_contigs)]
    LAST_COMPOSITION.update(read=read_s, feed=feed_s, finish_wait=finish_s, upload=float(secs[0]), ordinals=float(secs[1]), count=float(secs[2]),
                            download=time.perf_counter() - t0, attempts=attempt + 1, wall=time.perf_counter() - t_all)
    out = Composition(chroms, lengths.tolist(), bin_size, host[0], host[1], host[2])
    out.totals = dict(contigs=n_contigs, positions=positions, bins=bins, gc=int(stats[3]), at=int(stats[4]), masked=int(stats[5]))
    return out
