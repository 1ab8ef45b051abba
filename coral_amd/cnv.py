"""Copy number from binned depth (the `cnv` mode): the two files `reconstruct` starts from - `--cn_seg`, a CNVkit-style .cns of
segmented copy number, and `--cnv_seed`, the seed intervals - made from a sorted BAM by this project alone.

The reference gets them from scripts/call_cnvs.sh (`cnvkit.py batch --seq-method wgs`: CNVkit plus R's DNAcopy) and then its
`seed` mode (src/cnv_seed.py).  Here ``segment_depth`` segments a ``bam.BinnedDepth`` with a deterministic Haar-wavelet segmenter
after HaarSeg (Ben-Yaacov & Eldar 2008; what CNVkit offers as ``-m haar``, not CBS) - the rule is coral_cn_core.h's, stated in
DESIGN.md §4, and parity with CNVkit is not claimed -, and ``find_seeds`` is the reference's ``run_seeding``.
"""
from __future__ import annotations

import ctypes as C
import numbers
import os
import re
from typing import Sequence

import numpy as np

from . import _lib

_AUTOSOME = re.compile(r"^(chr)?([1-9]|1[0-9]|2[0-2])$")
LAST_SEGMENT = {}                    # seconds of the last GPU segment_depth, by stage (coral_cn_segment_gpu)
_STAGES = ("upload", "signal", "noise", "levels", "cuts_host", "unify_rows", "gc")


class CopyNumberSegments:
    """The rows of a segmentation, one per segment in contig and position order: ``chrom`` (list of str), ``start`` / ``end``
    int64 (the first kept bin's start, the last one's end), ``probes`` int64 (kept bins), ``log2`` float64 (the mean log2 ratio
    against the centre: ``sum_s / (probes * 65536)`` of the integers both backends compute) and ``depth`` float64 (mean depth,
    ``sum_bases / (probes * bin_size)``).  ``counts``: rows, kept bins, centre, reference centre, breakpoints, uncalled (the
    candidates lost to the called-base mask).  ``gc_bias``: None without a composition, else a dict of ``strata`` (G),
    ``stratum_bins`` (int64 [G + 1]: the centring contigs' kept bins per GC stratum) and ``bias`` (float64 [G + 1]: what was
    subtracted from the signal per stratum, in log2 units; ``bias_q16`` holds the integers)."""

    def __init__(self, chroms, bin_size, contig, start, end, probes, sum_s, sum_bases, counts=None, gc_bias=None):
        self.chroms, self.bin_size = list(chroms), int(bin_size)
        self.contig = np.ascontiguousarray(contig, dtype=np.int32)
        self.start, self.end, self.probes, self.sum_s, self.sum_bases = (np.ascontiguousarray(a, dtype=np.int64) for a in (start, end, probes, sum_s, sum_bases))
        self.counts = dict(counts or {})
        self.gc_bias = gc_bias

    def __len__(self) -> int:
        return len(self.contig)

    @property
    def chrom(self):
        return [self.chroms[c] for c in self.contig.tolist()]

    @property
    def log2(self) -> np.ndarray:
        return self.sum_s.astype(np.float64) / (self.probes.astype(np.float64) * 65536.0)

    @property
    def depth(self) -> np.ndarray:
        return self.sum_bases.astype(np.float64) / (self.probes.astype(np.float64) * float(self.bin_size))

    def cn(self) -> np.ndarray:
        """Absolute copy number under a diploid centre: 2 * 2**log2 (how the reference reads a .cns)."""
        return 2.0 * np.exp2(self.log2)

    def rows(self):
        return list(zip(self.chrom, self.start.tolist(), self.end.tolist(), self.log2.tolist(), self.depth.tolist(), self.probes.tolist()))

    def write(self, path: str) -> str:
        """CNVkit's .cns columns, tab-separated: chromosome, start, end, gene ('-'), log2, depth, probes, weight (= probes)."""
        with open(path, "w", newline="") as fp:
            fp.write("chromosome\tstart\tend\tgene\tlog2\tdepth\tprobes\tweight\n")
            fp.write("".join("%s\t%d\t%d\t-\t%r\t%r\t%d\t%d\n" % (c, a, b, l, d, p, p) for c, a, b, l, d, p in self.rows()))
        return path


def default_centre_contigs(chroms: Sequence[str]):
    """The contigs named chr1..chr22 or 1..22; every contig when there is none of them."""
    auto = [c for c in chroms if _AUTOSOME.match(c)]
    return auto if auto else list(chroms)


def _check_gc_arguments(gc_strata, gc_min_bins, min_called):
    """-> min_called in permille.  ``ValueError``: gc_strata outside 1..1000, gc_min_bins below 1, min_called outside [0, 1]."""
    if isinstance(gc_strata, bool) or not isinstance(gc_strata, numbers.Integral) or not 1 <= gc_strata <= 1000:
        raise ValueError("gc_strata must be an integer in 1..1000, got %r" % (gc_strata,))
    if isinstance(gc_min_bins, bool) or not isinstance(gc_min_bins, numbers.Integral) or gc_min_bins < 1:
        raise ValueError("gc_min_bins must be an integer of at least 1, got %r" % (gc_min_bins,))
    if isinstance(min_called, bool) or not isinstance(min_called, numbers.Real) or not 0.0 <= min_called <= 1.0:
        raise ValueError("min_called must lie in [0, 1], got %r" % (min_called,))
    return int(round(float(min_called) * 1000))


def _check_arguments(depth, reference, levels, fdr_q, centre_contigs):
    if isinstance(levels, bool) or not isinstance(levels, numbers.Integral) or not 1 <= levels <= 20:
        raise ValueError("levels must be an integer in 1..20, got %r" % (levels,))
    if isinstance(fdr_q, bool) or not isinstance(fdr_q, numbers.Real) or not 0.0 < fdr_q < 1.0:
        raise ValueError("fdr_q must lie in (0, 1), got %r" % (fdr_q,))
    if reference is not None and (reference.chroms != depth.chroms or reference.lengths != depth.lengths or reference.bin_size != depth.bin_size):
        raise ValueError("the reference table has other bins: contigs, lengths and bin_size must equal the sample's")
    if centre_contigs is None:
        centre_contigs = default_centre_contigs(depth.chroms)
    unknown = [c for c in centre_contigs if c not in set(depth.chroms)]
    if unknown:
        raise ValueError("centre_contigs: unknown contig %r" % (unknown[0],))
    wanted = set(centre_contigs)
    return np.array([c in wanted for c in depth.chroms], dtype=np.uint8)


def segment_depth(depth, reference=None, levels: int = 5, fdr_q: float = 1e-4, centre_contigs=None, device="cuda:0", composition=None, gc_strata: int = 100,
                  gc_min_bins: int = 256, min_called: float = 0.5) -> CopyNumberSegments:
    """Segments the binned depth ``depth`` (a ``bam.BinnedDepth``) into runs of equal copy number -> ``CopyNumberSegments``.

    Bins of the full size with depth are candidates; the centre is the lower median of their ``bases`` over ``centre_contigs``
    (default: chr1..chr22 / 1..22, or all contigs without any of those); candidates below 1/32 of the centre are masked.  With
    ``reference`` - a ``BinnedDepth`` of a normal sample with the same bins - its log2 ratio against its own centre is
    subtracted and its empty or low bins are masked too.  Each contig's kept bins are one sequence: Haar details at ``levels``
    dyadic scales, local peaks, a Benjamini-Hochberg cut at ``fdr_q`` per contig and level against a MAD noise estimate, and
    the levels' breakpoints unified fine to coarse.  The rule is integer arithmetic except for the cut (coral_cn_core.h), so the
    GPU ``device`` (coral_cn_segment_gpu: kernels k_cn_*, k_haar_*) and ``device="cpu"`` (coral_cn_segment_host) give the same
    rows.  With ``composition`` - a ``composition.Composition`` of the reference genome at the depth's bin size - bins with fewer
    called (A C G T) bases than ``min_called`` of the bin are masked as well, and the GC bias is taken out of the signal in
    front of the details: a kept bin's stratum is its GC fraction in ``gc_strata`` steps, a stratum's bias is the lower median
    of the signal over the centring contigs' kept bins of the nearest strata that together hold ``gc_min_bins`` bins, and every
    kept bin's signal has its stratum's bias subtracted (``CopyNumberSegments.gc_bias``).  ``ValueError`` before any work:
    ``levels`` outside 1..20, ``fdr_q`` not in (0, 1), a reference with other bins, an unknown centring contig, ``gc_strata``
    outside 1..1000, ``gc_min_bins`` below 1, ``min_called`` outside [0, 1], a composition that does not fit the depth's
    contigs and bin size (``Composition.for_depth``)."""
    import torch
    centre = _check_arguments(depth, reference, levels, fdr_q, centre_contigs)
    permille = _check_gc_arguments(gc_strata, gc_min_bins, min_called)
    gc = at = None
    if composition is not None:
        gc, at, _masked = composition.for_depth(depth)
        gc, at = np.ascontiguousarray(gc, dtype=np.uint32), np.ascontiguousarray(at, dtype=np.uint32)
    G = int(gc_strata)
    bias, stratum_bins = np.zeros(G + 1, dtype=np.int64), np.zeros(G + 1, dtype=np.int64)
    gc_args = [None, None, 0, 0, 0, None, None] if gc is None else [gc.ctypes.data, at.ctypes.data, G, int(gc_min_bins), permille, bias.ctypes.data, stratum_bins.ctypes.data]
    L = _lib.lib()
    n_contigs, n_bins = len(depth.chroms), depth.n_bins
    lengths = np.array(depth.lengths, dtype=np.int64)
    ref = None if reference is None else reference.all_bases
    on_gpu = torch.device(device).type == "cuda"
    cap = min(n_bins, max(4096, 2 * n_contigs))
    for _attempt in range(2):
        rows = [np.empty(cap, dtype=np.int32)] + [np.empty(cap, dtype=np.int64) for _ in range(5)]
        counts = (C.c_int64 * 8)()
        common = [n_contigs, depth.bin_off.ctypes.data, lengths.ctypes.data, depth.bin_size, depth.all_bases.ctypes.data, None if ref is None else ref.ctypes.data,
                  centre.ctypes.data, int(levels), float(fdr_q), cap] + [a.ctypes.data for a in rows] + [counts]
        if on_gpu:
            dev = torch.device(device)
            torch.cuda.set_device(dev)
            ws_bytes = int(L.coral_cn_workspace_gc_bytes(n_bins, n_contigs, int(levels), int(ref is not None), cap, int(gc is not None), G))
            if ws_bytes < 0:
                raise _lib.CoralHipError("coral_cn_workspace_gc_bytes failed (%d)" % ws_bytes)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream(dev)
            stream.synchronize()                                 # (the block may be a recycled one)
            secs = (C.c_double * 7)()
            rc = L.coral_cn_segment_gc_gpu(dev.index or 0, *common, ws.data_ptr(), ws_bytes, stream.cuda_stream, secs, *gc_args)
            stream.synchronize()
            del ws
            LAST_SEGMENT.clear()
            LAST_SEGMENT.update(zip(_STAGES, (float(s) for s in secs)), workspace_bytes=ws_bytes)
        else:
            rc = L.coral_cn_segment_gc_host(*common, *gc_args)
        if rc == -3 and cap < n_bins:                            # CORAL_ERR_CAPACITY: counts[0] rows suffice
            cap = min(n_bins, max(int(counts[0]), cap + 1))
            continue
        break
    if rc != 0:
        raise _lib.CoralHipError("coral_cn_segment_%s failed (%d): %s" % ("gpu" if on_gpu else "host", rc, L.coral_bam_last_error().decode()))
    n = int(counts[0])
    names = ("rows", "kept", "centre", "ref_centre", "breakpoints", "uncalled")
    gc_bias = None if gc is None else dict(strata=G, stratum_bins=stratum_bins, bias_q16=bias, bias=bias.astype(np.float64) / 65536.0)
    return CopyNumberSegments(depth.chroms, depth.bin_size, *(a[:n].copy() for a in rows), counts={k: int(counts[i]) for i, k in enumerate(names)}, gc_bias=gc_bias)


def call_copy_number(bam_path: str, bin_size: int = 1000, min_mapq: int = 0, exclude_flags: int = 0x704, count_deletions: bool = True, *, reference=None,
                     levels: int = 5, fdr_q: float = 1e-4, centre_contigs=None, record_filter=None, device="cuda:0", composition=None, gc_strata: int = 100,
                     gc_min_bins: int = 256, min_called: float = 0.5) -> CopyNumberSegments:
    """``bam.binned_depth`` of ``bam_path`` (one decode), then ``segment_depth``; the arguments are theirs."""
    from . import bam
    if isinstance(levels, bool) or not isinstance(levels, numbers.Integral) or not 1 <= levels <= 20:
        raise ValueError("levels must be an integer in 1..20, got %r" % (levels,))
    if isinstance(fdr_q, bool) or not isinstance(fdr_q, numbers.Real) or not 0.0 < fdr_q < 1.0:
        raise ValueError("fdr_q must lie in (0, 1), got %r" % (fdr_q,))
    _check_gc_arguments(gc_strata, gc_min_bins, min_called)
    depth = bam.binned_depth(bam_path, bin_size, min_mapq, exclude_flags, count_deletions, device=device, record_filter=record_filter)
    return segment_depth(depth, reference, levels, fdr_q, centre_contigs, device=device, composition=composition, gc_strata=gc_strata, gc_min_bins=gc_min_bins,
                         min_called=min_called)


# ----------------------------------------------------------------------------------------------
# seeds: the reference's run_seeding (src/cnv_seed.py:42-128)
# ----------------------------------------------------------------------------------------------
GAIN = 6.0
CNSIZE_MIN = 99999
CNSIZE_MAX = 5000001                 # not a parameter in the reference either
CNGAP_MAX = 300001


def read_chrom_sizes(source) -> dict:
    """Contig lengths as a dict: a dict as it is, a BAM file's header (a name ending in .bam), or a two-column text file."""
    if isinstance(source, dict):
        return {str(k): int(v) for k, v in source.items()}
    path = os.fspath(source)
    if path.endswith(".bam"):
        from . import bam
        return dict(zip(bam.bam_reference_names(path), bam.bam_reference_lengths(path)))
    sizes = {}
    with open(path) as fp:
        for line in fp:
            s = line.split()
            if len(s) >= 2 and not line.startswith("#"):
                sizes[s[0]] = int(s[1])
    return sizes


def read_centromeres(path, chrom_sizes: dict) -> dict:
    """The arm table of cnv_seed.py:31-40 from a file in the format of the reference's annotations/GRCh38_centromere.bed
    (chrom, start, end, band, 'acen'; the p row of a contig in front of its q row): contig -> [[p row's start, q row's end], [the
    p arm's segments, the q arm's], [p arm length, q arm length]].  Rows of contigs with names longer than 5 characters are
    left out, as there."""
    arms = {}
    with open(path) as fp:
        for line in fp:
            s = line.strip().split()
            if len(s) < 4 or len(s[0]) > 5:
                continue
            if "p" in s[3]:
                arms[s[0]] = [[int(s[1])], [[], []], [int(s[1])]]
            if "q" in s[3]:
                if s[0] not in arms or len(arms[s[0]][0]) != 1:
                    raise ValueError("centromeres: the q row of %s does not follow its p row" % s[0])
                if s[0] not in chrom_sizes:
                    raise ValueError("centromeres: no length for contig %s" % s[0])
                arms[s[0]][0].append(int(s[2]))
                arms[s[0]][2].append(chrom_sizes[s[0]] - int(s[2]))
    half = [c for c, a in arms.items() if len(a[0]) != 2]
    if half:
        raise ValueError("centromeres: contig %s has no q row" % half[0])
    return arms


def _arm_cn(segs, arm_len: int) -> float:
    """cnv_seed.py:75-91: 2.0 unless the arm's segments cover half of it; then the CN at which the segments, taken by rising CN,
    reach 49 % of the covered length."""
    total = sum(e - s for _c, s, e, _cn in segs)
    ccn = 2.0
    if total >= 0.5 * arm_len:
        acc = 0
        for seg in sorted(segs, key=lambda seg: seg[3]):
            ccn = seg[3]
            acc += seg[2] - seg[1]
            if acc >= 0.49 * total:
                break
    return ccn


def find_seeds(cn_seg_path, centromeres, chrom_sizes, gain: float = GAIN, min_seed_size: int = CNSIZE_MIN, max_seg_gap: int = CNGAP_MAX):
    """The reference's ``run_seeding``: the seed intervals [(chrom, start, end)] of a segmented copy-number file, ``end`` being the
    last segment's end - 1 as the reference writes it.  ``cn_seg_path``: a .cns (CN = 2 * 2**log2 of column 5) or a .bed (CN in
    column 4), sorted by contig and position.  Segments of CN >= ``gain`` that lie on one side of the centromere are chained
    while the gap to the chain's last segment is at most ``max_seg_gap``; a chain longer than 5 000 001 bases in sum needs 1.2 *
    ``gain``; the cutoff rises by (the arm's CN - 2) - the arm's CN being taken at 49 % of its covered length when at least half
    the arm is covered; what is left of a chain is merged across gaps of at most ``max_seg_gap`` and written when its summed
    length reaches ``min_seed_size``.  ``centromeres``: a file like the reference's annotations/GRCh38_centromere.bed (the user's
    to pass; none is shipped); ``chrom_sizes``: a dict, a .bam (its header) or a two-column file.

    Not the reference's: a chain that is neither left nor right of the centromere raises ``ValueError`` naming it (``os.abort()``
    there); segments on contigs the centromere file does not list are skipped (``KeyError`` there); a file without any segment of
    CN >= ``gain`` gives no seeds (``IndexError`` there); another extension than .cns / .bed raises ``ValueError``."""
    path = os.fspath(cn_seg_path)
    if not path.endswith((".cns", ".bed")):
        raise ValueError("%s: the copy-number file must be a .cns or a .bed" % path)
    is_cns = path.endswith(".cns")
    arms = read_centromeres(centromeres, read_chrom_sizes(chrom_sizes))
    chains, cur = [], []
    with open(path) as fp:
        for line in fp:
            s = line.strip().split()
            if not s or s[0] == "chromosome" or s[0] not in arms:
                continue
            start, end = int(s[1]), int(s[2])
            cn = 2 * (2 ** float(s[4])) if is_cns else float(s[3])
            p_start, q_end = arms[s[0]][0]
            seg = (s[0], start, end, cn)
            if cn >= gain and (end <= p_start or start >= q_end):
                if cur and s[0] == cur[-1][0] and start - cur[-1][2] <= max_seg_gap:
                    cur.append(seg)
                else:
                    if cur:
                        chains.append(cur)
                    cur = [seg]
            if end <= p_start:
                arms[s[0]][1][0].append(seg)
            if start >= q_end:
                arms[s[0]][1][1].append(seg)
    chains.append(cur)
    arm_cn = {c: (_arm_cn(a[1][0], a[2][0]), _arm_cn(a[1][1], a[2][1])) for c, a in arms.items()}
    seeds = []
    for chain in chains:
        if not chain:
            continue
        chrom = chain[-1][0]
        cutoff = gain
        if sum(e - s for _c, s, e, _cn in chain) > CNSIZE_MAX:
            cutoff = 1.2 * gain
        if chain[-1][2] <= arms[chrom][0][0]:
            cutoff = cutoff + arm_cn[chrom][0] - 2.0
        elif chain[0][1] >= arms[chrom][0][1]:
            cutoff = cutoff + arm_cn[chrom][1] - 2.0
        else:
            raise ValueError("seed %s:%d-%d is neither left nor right of the centromere" % (chrom, chain[0][1], chain[-1][2]))
        chain = [seg for seg in chain if not seg[3] < cutoff]
        if not chain:
            continue
        last, total = [], 0
        for seg in chain:
            if last and seg[1] - last[2] <= max_seg_gap:
                total += seg[2] - seg[1]
                last[2] = seg[2]
            elif not last:
                last = list(seg)
                total += seg[2] - seg[1]
            elif total >= min_seed_size:
                seeds.append((last[0], last[1], last[2] - 1))
                total = 0
                last = list(seg)
        if total >= min_seed_size:
            seeds.append((last[0], last[1], last[2] - 1))
    return seeds


def write_seeds(seeds, path: str) -> str:
    """The seed bed as the reference writes it: chrom, start, end, tab-separated."""
    with open(path, "w", newline="") as fp:
        fp.write("".join("%s\t%d\t%d\n" % (c, a, b) for c, a, b in seeds))
    return path
