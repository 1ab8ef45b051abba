"""The copy-number segmenter's shared case table and its rule restated in plain Python (big ints, math.erfc), for
tests/test_cnv_core.py (host backend and stand-alone program against the restatement) and tests/test_cnv_gpu.py (device against
host).  The restatement follows include/coral_hip.h's statement of the rule, not the C++: mirror padding by index, sums by
slicing, medians by sorting.

Every case is asserted to keep a margin at the one floating-point step: no p_i lies within relative 1e-6 of its line q * i / M,
so that a last-bit difference between math.erfc and std::erfc cannot flip a cut."""
import math
import struct

import numpy as np

MASK64 = (1 << 64) - 1
NO_CUT = (1 << 63) - 1
MARGIN = 1e-6


class Case:
    def __init__(self, chroms, lengths, bin_size, bases, ref=None, centre_contigs=None, levels=5, q=1e-4):
        self.chroms, self.lengths, self.bin_size = list(chroms), [int(l) for l in lengths], int(bin_size)
        self.bases = np.asarray(bases, dtype=np.int64)
        self.ref = None if ref is None else np.asarray(ref, dtype=np.int64)
        self.centre_contigs, self.levels, self.q = centre_contigs, levels, q
        self.bin_off = np.concatenate([[0], np.cumsum([(max(l, 0) + bin_size - 1) // bin_size for l in self.lengths])]).astype(np.int64)
        assert len(self.bases) == self.bin_off[-1] and (self.ref is None or len(self.ref) == len(self.bases))

    def centre_flags(self):
        names = self.centre_contigs
        if names is None:
            auto = [c for c in self.chroms if (c[3:] if c.startswith("chr") else c) in [str(k) for k in range(1, 23)]]
            names = auto if auto else self.chroms
        return [int(c in names) for c in self.chroms]

    def depth(self, bam, which="bases"):
        """The case as a bam.BinnedDepth (``which`` = "ref": the reference table)."""
        a = self.bases if which == "bases" else self.ref
        return bam.BinnedDepth(self.chroms, self.lengths, self.bin_size, 0, 0x704, True, self.bin_off, a, np.zeros(len(a), dtype=np.int64))

    def pack(self):
        """The case for tests/native/cnv_host.cpp."""
        nc = len(self.chroms)
        out = struct.pack("<iqiid", nc, self.bin_size, self.levels, int(self.ref is not None), self.q)
        out += self.bin_off.astype("<i8").tobytes() + np.array(self.lengths, dtype="<i8").tobytes() + bytes(self.centre_flags())
        out += self.bases.astype("<i8").tobytes() + (b"" if self.ref is None else self.ref.astype("<i8").tobytes())
        return out


def noisy(rng, n, level, steps=()):
    """n bins of Poisson depth around ``level``, multiplied by f over [a, b) for each (a, b, f) of ``steps``."""
    mean = np.full(n, float(level))
    for a, b, f in steps:
        mean[a:b] *= f
    return rng.poisson(mean).astype(np.int64)


def cases():
    rng = np.random.RandomState(20240611)
    T = {}
    T["one_step"] = Case(["chr1"], [600 * 100], 100, noisy(rng, 600, 3000, [(200, 260, 3.0)]))
    T["short_last_bin_and_tiny_contigs"] = Case(["chr1", "chr2", "chr3", "chr4", "chrX", "chrM"], [40050, 100, 250, 300, 0, 99], 100,
                                                np.concatenate([noisy(rng, 401, 5000, [(100, 140, 0.5)]), [4800], [5100, 5300, 70], [4000, 9000, 4100], [60]]))
    b = noisy(rng, 500, 2000, [(50, 90, 4.0), (300, 302, 8.0), (420, 500, 0.25)])
    b[[0, 17, 18, 19, 250, 499]] = 0
    b[[5, 120, 121]] = [40, 61, 62]                      # under and at the floor of 1/32 of the centre
    T["masked_bins"] = Case(["1"], [500 * 1000], 1000, b)
    T["boundary_step"] = Case(["chr1", "chr2"], [300 * 50, 280 * 50], 50, np.concatenate([noisy(rng, 300, 1000), noisy(rng, 280, 8000)]))
    T["centre_on_chr2"] = Case(["chr1", "chr2"], [300 * 50, 280 * 50], 50, T["boundary_step"].bases, centre_contigs=["chr2"])
    T["no_autosome_names"] = Case(["ctgA", "ctgB"], [256 * 10, 100 * 10], 10, np.concatenate([noisy(rng, 256, 900, [(128, 160, 2.0)]), noisy(rng, 100, 1800)]))
    flat = np.full(400, 1000, dtype=np.int64)
    flat[100:150] = 2000
    T["sigma_zero"] = Case(["chr1"], [400 * 100], 100, flat)
    T["levels_1"] = Case(["chr1"], [600 * 100], 100, T["one_step"].bases, levels=1)
    T["levels_9_skips_the_large_ones"] = Case(["chr1", "chr2"], [100 * 100, 20 * 100], 100, np.concatenate([noisy(rng, 100, 4000, [(30, 60, 2.0)]), noisy(rng, 20, 4000, [(8, 12, 3.0)])]),
                                              levels=9)
    ref = noisy(rng, 600, 2500, [(400, 480, 0.5)])
    ref[[10, 11, 599]] = [0, 0, 3]
    T["reference"] = Case(["chr1"], [600 * 100], 100, T["one_step"].bases, ref=ref)
    T["loose_q"] = Case(["chr1", "chr2"], [800 * 100, 300 * 100], 100,
                        np.concatenate([noisy(rng, 800, 400, [(100, 104, 1.6), (300, 420, 1.3), (600, 603, 2.5), (700, 760, 0.7)]), noisy(rng, 300, 400, [(150, 151, 3.0)])]), q=0.05)
    T["nothing_kept"] = Case(["chr1", "chr2"], [1000, 950], 100, np.zeros(20, dtype=np.int64))
    T["one_kept_bin"] = Case(["chr1"], [350], 100, [0, 70, 0, 12])
    return T


# ---- the rule, restated -------------------------------------------------------------------------------------------------------
def log2_q16(x):
    e = x.bit_length() - 1
    m = x << (63 - e)
    bits = 0
    for _ in range(16):
        p = m * m
        hi, lo = p >> 64, p & MASK64
        if hi >= 1 << 63:
            bits, m = (bits << 1) | 1, hi
        else:
            bits, m = bits << 1, ((hi << 1) | (lo >> 63)) & MASK64
    return (e << 16) | bits


def lower_median(values):
    return sorted(values)[(len(values) - 1) // 2]


def fdr_cut(mags_desc, h, sigma, q, margins=None):
    M = len(mags_desc)
    if M == 0:
        return NO_CUT
    if sigma == 0:
        return 1
    denom = math.sqrt(2.0 * h) * sigma * math.sqrt(2.0)
    best = None
    for i, m in enumerate(mags_desc, 1):
        p, line = math.erfc(m / denom), q * i / M
        if margins is not None:
            margins.append(abs(p - line) / line)
        if p <= line:
            best = m
    return NO_CUT if best is None else best


def details(x, h):
    """c_h[0..n] of the mirror-padded x, c_h[0] = c_h[n] = 0."""
    n = len(x)
    pad = lambda j: x[-j - 1] if j < 0 else x[2 * n - 1 - j] if j >= n else x[j]
    c = [0] * (n + 1)
    for k in range(1, n):
        c[k] = sum(pad(j) for j in range(k, k + h)) - sum(pad(j) for j in range(k - h, k))
    return c


def peaks(c):
    """{k: |c[k]|} of the peaks of c[0..n]."""
    out = {}
    for k in range(1, len(c) - 1):
        if (c[k] > 0 and c[k] > c[k - 1] and c[k] >= c[k + 1]) or (c[k] < 0 and c[k] < c[k - 1] and c[k] <= c[k + 1]):
            out[k] = abs(c[k])
    return out


def restate(case, margins=None):
    """-> (rows [(contig, start, end, probes, sum_s, sum_bases)], counts {kept, centre, ref_centre, breakpoints})."""
    bases = [int(v) for v in case.bases]
    ref = None if case.ref is None else [int(v) for v in case.ref]
    flags = case.centre_flags()
    size = case.bin_size
    contig_bins = [range(int(case.bin_off[c]), int(case.bin_off[c + 1])) for c in range(len(case.chroms))]
    cand = set()
    for c, bins in enumerate(contig_bins):
        for b in bins:
            k = b - bins.start
            if (k + 1) * size <= case.lengths[c] and bases[b] > 0 and (ref is None or ref[b] > 0):
                cand.add(b)
    mid = [b for c, bins in enumerate(contig_bins) if flags[c] for b in bins if b in cand]
    counts = {"kept": 0, "centre": 0, "ref_centre": 0, "breakpoints": 0}
    if not mid:
        return [], counts
    C = counts["centre"] = lower_median([bases[b] for b in mid])
    Cr = counts["ref_centre"] = lower_median([ref[b] for b in mid]) if ref is not None else 0
    rows = []
    for c, bins in enumerate(contig_bins):
        kept = [b for b in bins if b in cand and bases[b] * 32 >= C and (ref is None or ref[b] * 32 >= Cr)]
        n = len(kept)
        if n == 0:
            continue
        counts["kept"] += n
        x = [log2_q16(bases[b]) - log2_q16(C) - ((log2_q16(ref[b]) - log2_q16(Cr)) if ref is not None else 0) for b in kept]
        found = set()
        if n >= 2:
            d = lower_median([abs(x[k] - x[k - 1]) for k in range(1, n)])
            sigma = 1.4826 * d / math.sqrt(2.0)
            for l in range(1, case.levels + 1):
                h = 1 << l
                if h > n:
                    continue
                pk = peaks(details(x, h))
                cut = fdr_cut(sorted(pk.values(), reverse=True), h, sigma, case.q, margins)
                before = set(found)
                for k, m in pk.items():
                    if m >= cut and not any(abs(k - b) <= 1 << (l - 1) for b in before):
                        found.add(k)
        counts["breakpoints"] += len(found)
        edges = [0] + sorted(found) + [n]
        for a, b in zip(edges[:-1], edges[1:]):
            first, last = kept[a] - bins.start, kept[b - 1] - bins.start
            rows.append((c, first * size, min((last + 1) * size, case.lengths[c]), b - a, sum(x[a:b]), sum(bases[j] for j in kept[a:b])))
    return rows, counts


def rows_of(seg):
    """A cnv.CopyNumberSegments as the restatement's rows."""
    return list(zip(seg.contig.tolist(), seg.start.tolist(), seg.end.tolist(), seg.probes.tolist(), seg.sum_s.tolist(), seg.sum_bases.tolist()))
