"""Coverage track of the ``plot`` mode on the MI355X path.

The reference draws, for every amplified interval of a ``*_graph.txt``, one grey rectangle per window of 150 / 1 000 /
10 000 bp whose height is ``sum(count_coverage(chrom, w, w + window)) / window``
(/root/reference/src/plot_amplicons.py:376-411) — thousands of pysam calls that each walk the CIGARs of the overlapping
reads.  Here all windows of a plot are ONE ``coral_segment_coverage`` launch over the HBM-resident records (the kernel of
the graph build's A2 / A10 steps: per-record sums from the fused CIGAR scan, CIGAR re-walk only for records straddling a
window border).  Only the numbers are produced; drawing stays with the reference's matplotlib code.

For a base-quality threshold above 0 (the reference's ``--min_mapq``, which pysam applies per base) the resident records are
not enough — they hold no QUAL — so ``coverage_track_bam`` / ``CoverageTable`` count the windows while the BAM file is
decoded (``bam.window_coverage``).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import kernels


def parse_graph_intervals(graph_fn: str) -> Dict[str, List[List[int]]]:
    """Amplified intervals of a breakpoint-graph file: consecutive sequence edges merged (plot:108-121, :167-184)."""
    by_chr: Dict[str, list] = {}
    with open(graph_fn) as fp:
        for line in fp:
            s = line.strip().split("\t")
            if s[0] == "sequence":
                chrom = s[1].split(":")[0]
                by_chr.setdefault(chrom, []).append((int(s[1].split(":")[1][:-1]), int(s[2].split(":")[1][:-1])))
    out: Dict[str, List[List[int]]] = {}
    for chrom, edges in by_chr.items():
        lstart, lend = -2, -2
        out[chrom] = []
        for start, end in edges:
            if start != lend + 1:
                if lstart >= 0:
                    out[chrom].append([lstart, lend])
                lstart, lend = start, end
            else:
                lend = end
        out[chrom].append([lstart, lend])
    return out


def sort_chrom_names(chromlist):
    """bu:419-427."""
    def sort_key(x):
        val = x[3:] if x.startswith("chr") else x
        return int(val) if val.isnumeric() else ord(val)
    return sorted(chromlist, key=sort_key)


def track_windows(intervals: Dict[str, Sequence[Sequence[int]]], plot_bounds: Optional[Tuple[str, int, int]] = None):
    """(chrom, start, stop) of every rectangle, in drawing order (plot:376-411), as arrays per run of equal window size."""
    out = []
    for chrom in sort_chrom_names(intervals.keys()):
        for a, b in intervals[chrom]:
            if plot_bounds:
                if chrom != plot_bounds[0] or not (b >= plot_bounds[1] and a <= plot_bounds[2]):
                    continue
            window = 150
            length = (plot_bounds[2] - plot_bounds[1]) if plot_bounds else (b - a)
            if length >= 1000000:
                window = 10000
            elif length >= 100000:
                window = 1000
            starts = np.arange(a, b, window, dtype=np.int64)
            tail = b - ((b - a + 1) % window)
            if tail < b:
                starts = np.concatenate([starts, [tail]])
            out.append((chrom, window, starts))
    return out


def coverage_track(dr, intervals, plot_bounds=None, scan=None):
    """[(chrom, start, stop, bases)] for every window of the plot; height of the rectangle = bases / (stop - start).

    ``dr``: DeviceRecords; ``scan``: a previous ``kernels.cigar_scan(dr)`` result to reuse (else it is run once)."""
    runs = track_windows(intervals, plot_bounds)
    if not runs:
        return []
    tid_of = {c: k for k, c in enumerate(dr.header_chroms)}
    segs = np.concatenate([np.stack([np.full(len(st), tid_of[c], dtype=np.int64), st, st + w], axis=1) for c, w, st in runs])
    if scan is None:
        scan = kernels.cigar_scan(dr)
    _, n_bases = kernels.segment_coverage(dr, scan, segs)
    out, k = [], 0
    for c, w, st in runs:
        for s in st.tolist():
            out.append((c, s, s + w, int(n_bases[k])))
            k += 1
    return out


def plot_windows(intervals, plot_bounds=None):
    """(chrom, start, stop) of every rectangle of the coverage track, in drawing order."""
    return [(c, s, s + w) for c, w, st in track_windows(intervals, plot_bounds) for s in st.tolist()]


def coverage_track_bam(bam_path, intervals, plot_bounds=None, quality_threshold=0, read_callback="nofilter", device="cuda:0", index=None, *,
                       record_filter=None):
    """``coverage_track`` straight from a BAM file, for any base-quality threshold (what the reference passes as ``min_mapq``,
    plot:935) and either read callback: [(chrom, start, stop, bases)], counted while the file is decoded
    (``bam.window_coverage``).  At threshold 0 with 'nofilter' it equals ``coverage_track`` on the file's records.  ``index``: as
    in ``bam.window_coverage`` — with a BAI index beside the file only the plot's regions are decoded.  ``record_filter``: a
    ``bam.RecordFilter`` - only the records it keeps are counted."""
    from . import bam
    windows = plot_windows(intervals, plot_bounds)
    if not windows:
        return []
    counts = bam.window_coverage(bam_path, windows, quality_threshold, read_callback, device=device, index=index, record_filter=record_filter)
    return [(c, s, e, int(n)) for (c, s, e), n in zip(windows, counts)]


def parse_region(region: Optional[str]):
    """'chr:start-end' -> (chr, start, end) plot bounds, None -> None."""
    if not region:
        return None
    chrom, span = region.split(":")
    a, b = span.split("-")
    return chrom, int(a), int(b)


class CoverageTable:
    """A stand-in for the pysam handle the reference's plot code draws the coverage track from (``graph_vis.lr_bamfh``,
    plot:399-409): every window of one plot is counted in ONE decode of the BAM file, and ``count_coverage`` answers those
    windows from the table.  Only what was precomputed can be answered: another window, threshold or read callback raises
    KeyError."""

    def __init__(self, windows, counts, quality_threshold=0, read_callback="nofilter"):
        from . import bam
        self.quality_threshold = bam.quality_threshold_value(quality_threshold)
        self.read_callback = read_callback
        self._counts = {(c, int(s), int(e)): int(n) for (c, s, e), n in zip(windows, counts)}

    @classmethod
    def from_bam(cls, bam_path, graph_fn, region=None, min_mapq=0, read_callback="nofilter", device="cuda:0", index=None, *, record_filter=None):
        """The windows of the plot of ``graph_fn`` (optionally restricted to ``region`` 'chr:start-end'), counted with
        ``quality_threshold=min_mapq`` as the reference does (plot:935)."""
        track = coverage_track_bam(bam_path, parse_graph_intervals(graph_fn), parse_region(region), min_mapq, read_callback, device, index,
                                   record_filter=record_filter)
        return cls([(c, s, e) for c, s, e, _ in track], [n for _, _, _, n in track], min_mapq, read_callback)

    def __len__(self):
        return len(self._counts)

    def count_coverage(self, contig=None, start=None, stop=None, region=None, quality_threshold=15, read_callback="all",
                       reference=None, end=None):
        """pysam's signature; answers ([bases], [0], [0], [0]) — the reference only ever sums the four arrays."""
        from . import bam
        contig = reference if contig is None else contig
        stop = end if stop is None else stop
        if region is not None or contig is None or start is None or stop is None:
            raise KeyError("CoverageTable answers (contig, start, stop) windows only")
        if bam.quality_threshold_value(quality_threshold) != self.quality_threshold or read_callback != self.read_callback:
            raise KeyError("CoverageTable was built for quality_threshold=%d, read_callback=%r"
                           % (self.quality_threshold, self.read_callback))
        return ([self._counts[(contig, int(start), int(stop))]], [0], [0], [0])

    def close(self):
        self._counts = {}
