"""coral_cigar_scan, coral_segment_coverage and coral_point_cover at the sizes where their launch geometry changes, compared
exactly with the oracle (oracle.hostrecords.HostRecords) or, above a few thousand records, with a flat numpy restatement of
include/coral_hip.h that a CPU test of this module pins against the oracle.

Thresholds crossed (every case asserts, from its own inputs, that it crosses its threshold):
  scan      groups from the work cursor (n_groups > 2 * waves), a full 64-row park buffer, the RING = 4 / 8 / 12 instantiations
  coverage  n_seg > 2048 (global atomics instead of LDS bins), 65-ary segment search (n_seg around 64, 65, 65 * 65), more than
            8192 straddlers (a wave's second straddler comes from prefetched fields), more than 524 288 records (second round
            of the classify loop), records over more than 4 segments (the walk restarts), CIGARs of several 64-quad chunks
  points    more than 256 distinct points (second job of a workgroup), more than 8192 records in a window (second slice round),
            the max_span window's edge, max_span <= 0, 65-ary record search (n_rec around 64, 65, 65 * 65)

Shown to bite on three single-line mutants of coral_kernels.hip, one per kernel, each of which only changes a value or removes
work (no index range, load or store gets wider); tests/test_gpu_kernels.py passes on all three:
  scan    `g_next = dyn_base + ticket + 1`: group dyn_base is never processed.  g is still tested against n_groups before use
          and request_group clamps its loads, so only the skipped group's summary rows stay unwritten.  Fails
          test_cigar_scan_variant[6-1-1] and [12-1-1], test_cigar_scan_default_settings_cursor (cursor word one short) and,
          through the unwritten rows, test_segment_coverage_second_classify_round.
  walk    `p_next` not refreshed in k_seg_walk's prefetch branch: a wave's later straddlers are placed at its first one's start.
          The stale value only enters the segment search, whose result the walk tests against n_seg and seg_start < end before
          every use, and the record-relative segment bounds; the CIGAR is read through the correct offset and op count.  Fails
          test_segment_coverage_more_straddlers_than_waves.
  points  `p - max_span + 2` for the window's first position: the window [lo, hi) only loses records at its front (max_span > 0
          keeps first_pos <= p + 1, so lo <= hi).  Fails test_point_cover_max_span_window and every size of
          test_point_cover_search_boundaries.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from coral_amd import synth
from tests import _scan_variant_worker as svw
from tests.bamfile import D, EQ, H, I, M, N, P, S, X          # BAM op codes
from tests.test_gpu_kernels import _adversarial_records, _odd_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

COV_LDS_SEGS = 2048             # coral_segment_coverage: segment tables up to this size are summed in LDS
WALK_BLOCKS, WALK_WAVES = 2048, 4       # k_seg_walk: at most 2048 workgroups of 4 waves
CLASSIFY_ROUND = 2048 * 256     # k_seg_classify: records per round of its grid-stride loop
POINT_JOBS, POINT_SLICES = 8192, 32     # k_point_cover: workgroups per launch, workgroups per point
SLICE_ROUND = 32 * 256          # k_point_cover: records of a window per round of the slice loop


# ---------------------------------------------------------------------------------------------------------------------------------
# 0. the flat restatement (include/coral_hip.h: record layout, coral_cigar_scan, coral_segment_coverage, coral_point_cover)
# ---------------------------------------------------------------------------------------------------------------------------------
def _table(ops):
    t = np.zeros(16, dtype=np.int64)
    t[list(ops)] = 1
    return t


_REF, _ALN, _QRY = _table([M, D, N, EQ, X]), _table([M, EQ, X]), _table([M, I, S, H, EQ, X])


class _Flat:
    """Everything the three entry points promise, from per-op arrays of ALL records at once (no loop over records)."""

    def __init__(self, rec):
        g = lambda t: t.cpu().numpy()
        n = self.n = int(rec.n)
        self.tid, self.pos, self.end = (g(v).astype(np.int64) for v in (rec.tid, rec.pos, rec.end))
        n_cigar = g(rec.n_cigar).astype(np.int64)
        self.with_seq = (g(rec.has_seq) != 0) & (n_cigar > 0)
        off, cigar = g(rec.cigar_off).astype(np.int64), g(rec.cigar).view(np.uint32)
        owner = np.repeat(np.arange(n, dtype=np.int64), n_cigar)
        first = np.cumsum(n_cigar) - n_cigar                           # a record's first op in the list of all real ops
        w = cigar[off[owner] + np.arange(len(owner), dtype=np.int64) - first[owner]].astype(np.int64)
        op, ln = w & 15, w >> 4
        adv = _REF[op] * ln
        before = np.cumsum(adv) - adv                                  # reference advance of all ops in front of this one
        base = np.zeros(n, dtype=np.int64)
        base[n_cigar > 0] = before[first[n_cigar > 0]]
        start = self.pos[owner] + before - base[owner]
        aln = _ALN[op] != 0
        self.b_rec, self.b_start, self.b_end = owner[aln], start[aln], start[aln] + ln[aln]
        self.mbases, self.qinfer = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        np.add.at(self.mbases, self.b_rec, ln[aln])
        np.add.at(self.qinfer, owner, _QRY[op] * ln)
        self.blk_first, self.blk_last = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
        if len(self.b_rec):
            u, i0 = np.unique(self.b_rec, return_index=True)           # b_rec ascends: the first block of every record
            self.blk_first[u] = self.b_start[i0]
            self.blk_last[u] = self.b_end[np.append(i0[1:], len(self.b_rec)) - 1]
        na_rec = g(rec.nonacgt_rec).astype(np.int64)
        self.na_tid, self.na_pos = self.tid[na_rec], g(rec.nonacgt_pos).astype(np.int64)

    def summary(self):
        return np.stack([self.mbases, self.qinfer, self.blk_first, self.blk_last], axis=1)

    def coverage(self, segs, correct=True):
        """(n_reads, n_bases) of half-open segments; ``correct``: aligned non-ACGT bases taken out, as kernels.segment_coverage does."""
        n_reads, n_bases = np.zeros(len(segs), dtype=np.int64), np.zeros(len(segs), dtype=np.int64)
        counted = self.qinfer > 0
        use = self.with_seq[self.b_rec]
        bs, be, bt = self.b_start[use], self.b_end[use], self.tid[self.b_rec[use]]
        for j, (t, s, e) in enumerate(segs):
            n_reads[j] = np.count_nonzero((self.tid == t) & (self.pos < e) & (self.end > s) & counted)
            ov = np.minimum(be, np.int64(e)) - np.maximum(bs, np.int64(s))
            n_bases[j] = ov[(bt == t) & (ov > 0)].sum()
            if correct:
                n_bases[j] -= np.count_nonzero((self.na_tid == t) & (self.na_pos >= s) & (self.na_pos < e))
        return n_reads, n_bases

    def cover(self, t, p):
        if t < 0 or p < 0:
            return np.zeros(0, dtype=np.int64)
        return np.nonzero((self.tid == t) & (self.pos <= p) & (p < self.end))[0]

    def classes(self, segs):
        """Per record: number of overlapped segments, and whether one segment holds the whole record."""
        n_ov, inside = np.zeros(self.n, dtype=np.int64), np.zeros(self.n, dtype=bool)
        for t, s, e in segs:
            ov = (self.tid == t) & (self.pos < e) & (self.end > s)
            n_ov += ov
            inside |= ov & (s <= self.pos) & (self.end <= e)
        return n_ov, inside

    def straddlers(self, segs):
        """Records whose CIGAR coral_segment_coverage has to walk: SEQ, ops, a segment overlapped and none that holds them."""
        n_ov, inside = self.classes(segs)
        return (n_ov > 0) & ~inside & self.with_seq


def _host_coverage(host, segs, correct=True):
    """The same from the oracle, as tests/test_gpu_kernels.py asks it."""
    if not correct:
        keep = host.nonacgt_rec, host.nonacgt_pos
        host.nonacgt_rec, host.nonacgt_pos = keep[0][:0], keep[1][:0]
    qi = [host.infer_read_length(i) or 0 for i in range(host.n)]
    n_reads = np.array([sum(1 for i in host.region(host.chroms[t], s, e) if qi[i]) for t, s, e in segs], dtype=np.int64)
    n_bases = np.array([host.count_coverage_sum(host.chroms[t], s, e) for t, s, e in segs], dtype=np.int64)
    if not correct:
        host.nonacgt_rec, host.nonacgt_pos = keep
    return n_reads, n_bases


def _host_cover(host, t, p):
    if t < 0 or p < 0:
        return np.zeros(0, dtype=np.int64)
    return host.region(host.chroms[t], p, p + 1)


def _host_summary(host):
    out = np.full((host.n, 4), -1, dtype=np.int64)
    for i in range(host.n):
        bl = host.blocks(i)
        out[i, 0], out[i, 1] = sum(e - s for s, e in bl), host.infer_read_length(i) or 0
        if bl:
            out[i, 2], out[i, 3] = bl[0][0], bl[-1][1]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# records straight from numpy arrays (the per-dict builder of synth is a Python loop per op)
# ---------------------------------------------------------------------------------------------------------------------------------
class _Src:
    """Per-record arrays of a data set in file order; ``words`` are the real CIGAR ops of all records, one after the other."""

    def __init__(self, tid, pos, n_ops, words, has_seq, na_rec=(), na_pos=()):
        self.tid, self.pos, self.n_ops = (np.asarray(v, dtype=np.int64) for v in (tid, pos, n_ops))
        self.words, self.has_seq = np.asarray(words, dtype=np.int64), np.asarray(has_seq, dtype=np.int64)
        self.na_rec, self.na_pos = np.asarray(na_rec, dtype=np.int64), np.asarray(na_pos, dtype=np.int64)
        assert len(self.words) == self.n_ops.sum()

    def take(self, a, b):
        """Records a .. b - 1 as a data set of their own."""
        first = np.concatenate([[0], np.cumsum(self.n_ops)])
        sel = (self.na_rec >= a) & (self.na_rec < b)
        return _Src(self.tid[a:b], self.pos[a:b], self.n_ops[a:b], self.words[first[a]:first[b]], self.has_seq[a:b],
                    self.na_rec[sel] - a, self.na_pos[sel])

    def records(self):
        n = len(self.tid)
        owner = np.repeat(np.arange(n), self.n_ops)
        first = np.cumsum(self.n_ops) - self.n_ops
        off = np.concatenate([[0], np.cumsum((self.n_ops + 3) // 4 * 4)])
        cigar = np.full(int(off[-1]), synth.OP_PAD, dtype=np.int64)
        cigar[off[owner] + np.arange(len(owner)) - first[owner]] = self.words
        ref_len, q_len = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        np.add.at(ref_len, owner, _REF[self.words & 15] * (self.words >> 4))
        np.add.at(q_len, owner, _table([M, I, S, EQ, X])[self.words & 15] * (self.words >> 4))
        t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
        t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))
        z = np.zeros(n, dtype=np.int64)
        return synth.Records(n=n, tid=t32(self.tid), pos=t32(self.pos), end=t32(self.pos + np.maximum(ref_len, 1)), flag=t32(z),
                             mapq=t32(z + 60), qlen=t32(q_len), has_seq=t32(self.has_seq), nm=t32(z), name_id=t32(np.arange(n)),
                             n_cigar=t32(self.n_ops), cigar_off=t64(off), cigar=torch.from_numpy(cigar.astype(np.uint32).view(np.int32)),
                             sa_off=t64(np.zeros(n + 1)), sa=torch.zeros((0, 8), dtype=torch.int32), sa_nm=t32(np.zeros(0)),
                             nonacgt_rec=t64(self.na_rec), nonacgt_pos=t32(self.na_pos), n_names=n, name_gid=t64(np.arange(n)))


CROSS_X, CROSS_Z = 50_000, 50_900
CROSS_TAIL = 12              # contigs 1 .. 12: a short run of crossing records each, so that neighbours in the straddler list differ in contig
CROSS_SEGS = [(0, CROSS_X - 2000, CROSS_X), (0, CROSS_X, CROSS_X + 850), (0, CROSS_Z, CROSS_Z + 600)] + \
    [sg for t in range(1, CROSS_TAIL + 1) for sg in ((t, CROSS_X - 2000, CROSS_X), (t, CROSS_X, CROSS_X + 850))]


def _crossing_src(n=20_000, seed=41, per_tail=40):
    """Sections 2d / 3c: n records that all cross position CROSS_X of contig 0, about a third of them reaching past CROSS_Z: 1 .. 3
    ops, every tenth 5, 7 or 9 (two or three quads); then ``per_tail`` one-op records across CROSS_X on each of the contigs 1 ..
    CROSS_TAIL.  Neighbours in the file differ in contig, start, end, op count and CIGAR offset."""
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(CROSS_X - 1500, CROSS_X, n))
    far = rng.random(n) < 1 / 3
    L = CROSS_X - pos + np.where(far, rng.integers(901, 1500, n), rng.integers(2, 800, n))           # reference span >= 3
    n_ops = rng.integers(1, 4, n)
    a = 1 + (rng.random(n) * (L - 2)).astype(np.int64)                                                # 1 .. L - 2
    mid = np.array([D, N, I])[rng.integers(0, 3, n)]
    b = np.where(mid == I, 2, 1 + (rng.random(n) * (L - a - 1)).astype(np.int64))                     # D / N: 1 .. L - a - 1
    c = np.where(mid == I, L - a, L - a - b)
    W = np.zeros((n, 9), dtype=np.int64)
    one, two, three = n_ops == 1, n_ops == 2, n_ops == 3
    W[one, 0] = L[one] << 4 | M
    W[two, 0], W[two, 1] = a[two] << 4 | M, (L - a)[two] << 4 | X
    W[three, 0], W[three, 1], W[three, 2] = a[three] << 4 | EQ, b[three] << 4 | mid[three], c[three] << 4 | M
    for i in np.nonzero((rng.random(n) < 0.1) & (L >= 10))[0]:          # k aligned pieces that add up to L, one inserted base between them
        k = int(rng.choice([3, 4, 5]))
        pieces = np.diff(np.concatenate([[0], np.sort(rng.choice(np.arange(1, L[i]), k - 1, replace=False)), [L[i]]]))
        W[i, 0:2 * k:2] = pieces << 4 | np.array([M, EQ, X, M, EQ])[:k]
        W[i, 1:2 * k - 1:2] = 1 << 4 | I
        n_ops[i] = 2 * k - 1
    has_seq = (rng.random(n) >= 0.013).astype(np.int64)
    na = np.nonzero(one & (n_ops == 1) & (has_seq == 1))[0]
    na = na[(na >= 9000) & (na < 11000)][:40]                         # non-ACGT bases on both sides of the shared boundary
    words = W[np.arange(9)[None, :] < n_ops[:, None]]
    m = CROSS_TAIL * per_tail
    t_tid = np.repeat(np.arange(1, CROSS_TAIL + 1), per_tail)
    t_pos = np.sort(rng.integers(CROSS_X - 300, CROSS_X, (CROSS_TAIL, per_tail)), axis=1).reshape(-1)
    t_len = CROSS_X - t_pos + rng.integers(2, 800, m)
    return _Src(np.concatenate([np.zeros(n, dtype=np.int64), t_tid]), np.concatenate([pos, t_pos]), np.concatenate([n_ops, np.ones(m, dtype=np.int64)]),
                np.concatenate([words, t_len << 4 | M]), np.concatenate([has_seq, np.ones(m, dtype=np.int64)]),
                np.repeat(na, 2), np.stack([np.full(len(na), CROSS_X - 1), np.full(len(na), CROSS_X)], axis=1).reshape(-1))


FLAT_N = CLASSIFY_ROUND + 64 * 3 + 17


def _flat_src(seed=43):
    """Section 2e: FLAT_N records of one M op of 1 .. 50 bases, positions ascending over contigs 0 and 1, and about 100 segments,
    some of which cut through records of the classify loop's second round."""
    rng = np.random.default_rng(seed)
    n, n0 = FLAT_N, 300_000
    pos = 1000 + np.concatenate([np.cumsum(rng.integers(0, 4, n0)), np.cumsum(rng.integers(0, 4, n - n0))])
    tid = np.concatenate([np.zeros(n0, dtype=np.int64), np.ones(n - n0, dtype=np.int64)])
    ln = rng.integers(1, 51, n)
    src = _Src(tid, pos, np.ones(n), ln << 4 | M, (rng.random(n) >= 0.02).astype(np.int64))
    segs = []
    for t, a, b in ((0, 0, n0), (1, n0, n)):
        cuts = set(rng.integers(pos[a] - 20, pos[b - 1] + 60, 48).tolist()) | {int(pos[a]) - 50, int(pos[b - 1]) + 80}
        if t == 1:
            cuts |= {int(pos[k] + 1 + (ln[k] > 2)) for k in (n - 150, n - 60, n - 5, CLASSIFY_ROUND + 1)}
        cuts = sorted(cuts)
        segs += [(t, s, e - (3 if k % 4 == 2 and e - s > 3 else 0)) for k, (s, e) in enumerate(zip(cuts[:-1], cuts[1:]))]
    return src, segs


@pytest.fixture(scope="module")
def crossing():
    src = _crossing_src()
    rec = src.records()
    return src, rec, _Flat(rec)


@pytest.fixture(scope="module")
def flat_case():
    src, segs = _flat_src()
    rec = src.records()
    return src, rec, _Flat(rec), segs


def _sample_points(flat, step):
    pts = []
    for i in range(0, flat.n, step):
        t, p, e = int(flat.tid[i]), int(flat.pos[i]), int(flat.end[i])
        pts += [(t, p - 1), (t, p), (t, e - 1), (t, e)]
    return pts


def _tiling(flat, rng, n_cuts):
    segs = []
    for t in np.unique(flat.tid[flat.tid >= 0]):
        lo, hi = int(flat.pos[flat.tid == t].min()), int(flat.end[flat.tid == t].max())
        cuts = np.unique(np.concatenate([[lo - 10, hi + 10], rng.integers(lo, hi + 1, n_cuts)]))
        segs += [(int(t), int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])] + [(int(t), lo + 1, hi - 1)]
    return segs


def test_flat_reference_equals_oracle(crossing, flat_case):
    """No GPU: the restatement this module checks its large cases against gives what HostRecords gives - summaries, n_reads and
    n_bases in front of and behind the non-ACGT correction, cover lists - on the odd and the adversarial records of
    tests/test_gpu_kernels.py and on 2000 consecutive records of each large case with that case's own segments and points."""
    from oracle.hostrecords import REF_ADV, HostRecords
    rng = np.random.default_rng(2)
    cases = [("odd", _odd_records(), None, None), ("adversarial", _adversarial_records(), None, None)]
    src, _, _ = crossing
    cases.append(("crossing", src.take(9000, 11000).records(), CROSS_SEGS,
                  [(0, CROSS_X - 1), (0, CROSS_X), (0, CROSS_X + 1), (0, CROSS_Z)]))
    src, _, _, segs = flat_case
    cases.append(("flat", src.take(FLAT_N - 2000, FLAT_N).records(), segs, None))
    n_corrected = 0
    for name, rec, segs, pts in cases:
        host, flat = HostRecords(rec), _Flat(rec)
        assert np.array_equal(flat.summary(), _host_summary(host)), name
        ref_len = [int((REF_ADV[host.ops(i)[0]] * host.ops(i)[1]).sum()) for i in range(host.n)]
        assert np.array_equal(flat.end, host.pos + np.maximum(ref_len, 1)), name          # bam_endpos, also of the numpy-built records
        segs = (segs or []) + _tiling(flat, rng, 9)
        for correct in (False, True):
            want, got = _host_coverage(host, segs, correct), flat.coverage(segs, correct)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, correct)
        n_corrected += int((flat.coverage(segs, False)[1] != flat.coverage(segs, True)[1]).sum())
        assert flat.coverage(segs)[1].sum() > 0 and flat.coverage(segs)[0].sum() > 0, name
        pts = (pts or []) + _sample_points(flat, max(1, flat.n // 150)) + [(0, -1), (-1, 5)]
        n_cov = 0
        for t, p in pts:
            assert np.array_equal(flat.cover(t, p), _host_cover(host, t, p)), (name, t, p)
            n_cov += len(flat.cover(t, p))
        assert n_cov > len(pts) // 4, name
    assert n_corrected >= 3          # the correction was there to be compared (odd: two bases; crossing: both sides of X)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. coral_cigar_scan: the tuning overrides, one child process each
# ---------------------------------------------------------------------------------------------------------------------------------
_FATAL = (124, 137, 134, 139)          # time limit, kill, abort, segmentation fault: nothing more is started on the GPU
_child_died = []


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def scan_expectation():
    """(n_rec, summary [n_rec][4], gap rows (record, op index, previous block end, next block start) in the reference's order) of
    the worker's records, from the oracle."""
    from oracle.hostrecords import IS_ALN, HostRecords
    n_rec = 8 * _cus() + 1000
    host = HostRecords(synth.records_from_alignments(svw.variant_alignments(n_rec, 7)))
    gaps = []
    for i in range(host.n):
        bl = host.blocks(i)
        at = np.nonzero(IS_ALN[host.ops(i)[0]])[0]
        if host.mapq[i] >= svw.MIN_MAPQ:
            gaps += [(i, int(at[k + 1]), bl[k][1], bl[k + 1][0]) for k in range(len(bl) - 1) if bl[k + 1][0] - bl[k][1] > svw.MIN_GAP]
    n_ops = host.n_cigar
    assert (n_ops[:3] == 0).all() and (n_ops[-4:] == 0).all() and (n_ops == 0).sum() > 20
    assert {256 * k + d for k in range(1, 14) for d in (-1, 0, 1)} <= set(n_ops.tolist())
    assert len(gaps) > 1000 and (host.mapq < svw.MIN_MAPQ).sum() > n_rec // 8
    return n_rec, _host_summary(host), gaps


@gpu
@pytest.mark.parametrize("ring,group,wg_per_cu", [(6, 1, 1), (12, 1, 1), (8, 7, 1), (4, 64, None)])
def test_cigar_scan_variant(ring, group, wg_per_cu, scan_expectation, tmp_path):
    """One launch in a fresh process with CORAL_SCAN_RING / _GROUP / _WG_PER_CU set, against the oracle: the four summary columns,
    every gap row in the reference's order, and the work cursor: every loop iteration of a wave takes one ticket and processes one
    group, and a ticket that is dropped names a group beyond the last one, so the cursor ends at the number of groups if and
    only if every group was handed out exactly once."""
    assert not _child_died, "an earlier scan child ended with %s: no further child is started" % _child_died
    n_rec, summary, gaps = scan_expectation
    n_groups = (n_rec + group - 1) // group
    if group == 1:
        # one workgroup per CU at most: at most 4 * CUs waves, whose two static groups each do not cover the file
        assert wg_per_cu == 1 and n_groups > 2 * 4 * _cus()
    if group == 64:
        assert n_rec // 64 >= 40         # full groups: the 64-row park buffer fills exactly
    env = dict(os.environ, CORAL_SCAN_RING=str(ring), CORAL_SCAN_GROUP=str(group))
    env.pop("CORAL_SCAN_WG_PER_CU", None)
    if wg_per_cu is not None:
        env["CORAL_SCAN_WG_PER_CU"] = str(wg_per_cu)
    out = str(tmp_path / "scan.npz")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tests", "_scan_variant_worker.py"), str(n_rec), "7", out],
                       env=env, cwd=ROOT, capture_output=True, text=True)
    if r.returncode in _FATAL or r.returncode < 0:
        _child_died.append(r.returncode)
    assert r.returncode == 0, "exit %s\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    got = np.load(out)
    assert got["summary"].shape == summary.shape
    bad = np.nonzero((got["summary"] != summary).any(axis=1))[0]
    assert len(bad) == 0, (bad[:8], got["summary"][bad[:4]], summary[bad[:4]])
    rows = got["gaps"].astype(np.int64)
    rows = rows[np.lexsort((rows[:, 1], rows[:, 0]))]
    assert int(got["counters"][0]) == len(gaps)
    assert [tuple(x) for x in rows.tolist()] == gaps
    assert int(got["counters"][1]) == n_groups


@gpu
def test_cigar_scan_default_settings_cursor(flat_case):
    """Default settings, more than 524 288 one-quad records: groups of 24 records, about 21 900 of them - more than two per wave
    for any occupancy up to 10 workgroups per CU, so most groups come from the cursor.  Parity with the flat reference."""
    import ctypes as C
    from coral_amd import _lib
    from coral_amd.records import DeviceRecords
    _, rec, flat, _ = flat_case
    dr = DeviceRecords(rec, "cuda:0")
    summary = torch.empty((dr.n, 4), dtype=torch.int32, device=dr.device)
    gaps = torch.empty((64, 4), dtype=torch.int32, device=dr.device)
    cnt = torch.zeros(2, dtype=torch.int32, device=dr.device)
    rs = dr.c_struct()
    _lib.check(_lib.lib().coral_cigar_scan(C.byref(rs), 600, 20, summary.data_ptr(), gaps.data_ptr(), cnt.data_ptr(), 64, dr.stream()),
               "coral_cigar_scan")
    counters = cnt.cpu().numpy().view(np.uint32)
    n_groups = (dr.n + 23) // 24
    print("default scan: %d records, %d groups of 24, cursor word %d, %d CUs" % (dr.n, n_groups, int(counters[1]), _cus()))
    assert n_groups > 2 * 4 * 10 * _cus(), "%d CUs: the cursor is certain to be used only above %d records" % (_cus(), 24 * 80 * _cus())
    got = summary.cpu().numpy()
    bad = np.nonzero((got != flat.summary()).any(axis=1))[0]
    assert len(bad) == 0, (bad[:8], got[bad[:4]], flat.summary()[bad[:4]])
    assert int(counters[0]) == 0
    assert int(counters[1]) == n_groups


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. coral_segment_coverage
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_coverage(rec, segs, want, what):
    from coral_amd import kernels
    from coral_amd.records import DeviceRecords
    sg = np.asarray(segs, dtype=np.int64).reshape(len(segs), 3)
    batches = kernels._disjoint_batches(sg)
    assert len(batches) == 1 and np.array_equal(batches[0], np.arange(len(segs))), "the table must reach the kernel as it is"
    dr = DeviceRecords(rec, "cuda:0")
    n_reads, n_bases = kernels.segment_coverage(dr, kernels.cigar_scan(dr), segs)
    for name, g, w in (("n_reads", n_reads, want[0]), ("n_bases", n_bases, want[1])):
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, (what, name, bad[:8], [segs[j] for j in bad[:4]], g[bad[:8]], w[bad[:8]])


def _seg_table(n_seg, rng):
    """n_seg sorted, disjoint segments over contigs 0 and 2: irregular lengths, gaps between some, shared boundaries between
    others, a few empty ones."""
    segs = []
    for t, k in ((0, (n_seg + 1) // 2), (2, n_seg // 2)):
        cur = 500
        for i in range(k):
            s = cur + int(rng.choice([0, 0, 0, 1, 7, 30]))
            lone = 0 < i < k - 1 and segs[-1][2] > segs[-1][1]          # never the first or last of a contig, never two in a row
            e = s + (0 if rng.random() < 0.06 and lone else int(rng.integers(1, 40)))
            segs.append((t, s, e))
            cur = e
    return segs


def _probe_targets(n, rng, extra=60):
    """Indices 0 .. n - 1 a 65-ary search over n entries has to tell apart: both ends, every probe of the first step and its two
    neighbours, and some at random (second-step probes)."""
    if n <= 64:
        return list(range(n))
    t = {0, 1, n - 2, n - 1} | {int(v) for v in rng.integers(0, n, extra)}
    for lane in range(64):
        idx = (n * (lane + 1)) // 65
        t |= {idx - 1, idx, idx + 1}
    return sorted(v for v in t if 0 <= v < n)


def _records_around_segments(segs, targets, rng):
    """For every target segment: a record inside it, one that starts in it and reaches into the next one or two (or beyond the
    contig's last segment), one that starts in the gap in front of it and reaches into it, and one that stays in that gap."""
    alns = []

    def add(t, pos, length, k):
        if length >= 3 and k % 2:
            a = int(rng.integers(1, length - 1))
            mid = [(D, 1), (N, 1), (I, 2), (P, 1)][k % 4]
            cigar = [(M, a), mid, (EQ, length - a - (1 if mid[0] in (D, N) else 0))]
        else:
            cigar = [(M, length)]
        alns.append(dict(tid=t, pos=pos, cigar=cigar, has_seq=0 if k % 7 == 3 else 1, nonacgt=[pos] if k % 11 == 5 else []))
    for k, j in enumerate(targets):
        t, s, e = segs[j]
        prev_end = segs[j - 1][2] if j > 0 and segs[j - 1][0] == t else s - 40
        if e > s:
            p = int(rng.integers(s, e))
            add(t, p, int(rng.integers(1, e - p + 1)), k)
        nxt = [sg for sg in segs[j + 1:j + 3] if sg[0] == t]
        p = max(s, e - 3) if e > s else max(prev_end, s - 1)
        reach = (nxt[k % len(nxt)][1] + 1) if nxt else e + 5
        if reach > p:
            add(t, p, reach - p, k + 1)
        if s > prev_end:
            add(t, s - 1, 2, k)                                       # from the gap into the segment
            add(t, max(prev_end, s - 3), s - max(prev_end, s - 3), k)             # ends where the segment starts
    alns.sort(key=lambda a: (a["tid"], a["pos"]))
    return synth.records_from_alignments(alns)


@gpu
@pytest.mark.parametrize("n_seg", [1, 2, 63, 64, 65, 66, 129, 130, 2047, 2048, 2049, 4224, 4225, 4226])
def test_segment_coverage_table_sizes(n_seg):
    """The segment search of both kernels around 64, 65 and 65 * 65 entries, and the LDS / global-atomic switch at 2048: records
    whose first overlapped segment is the first, the last and every first-step probe of the 65-ary search and its neighbours."""
    from oracle.hostrecords import HostRecords
    rng = np.random.default_rng(n_seg)
    segs = _seg_table(n_seg, rng)
    rec = _records_around_segments(segs, _probe_targets(n_seg, np.random.default_rng(100 + n_seg)), rng)
    flat = _Flat(rec)
    n_ov, inside = flat.classes(segs)
    assert (inside & flat.with_seq).sum() > 0 and flat.straddlers(segs).sum() > 0 and (n_ov == 0).sum() > 0
    n_real, _ = flat.classes([sg for sg in segs if sg[2] > sg[1]])          # (an empty segment on a shared boundary is overlapped as well)
    assert n_real.max() <= 3 and n_ov.max() <= 4 and (n_seg < 4 or n_real.max() == 3)
    assert (n_seg > COV_LDS_SEGS) == (n_seg in (2049, 4224, 4225, 4226))
    assert n_seg < 30 or any(s == e for _, s, e in segs)
    # the first overlapped segment of the records, from the table's order (ends ascend with the starts in a disjoint table)
    seg_key = np.array([(t << 32) | e for t, _, e in segs], dtype=np.int64)
    first = set(np.searchsorted(seg_key, (flat.tid << 32) | flat.pos, side="right")[n_ov > 0].tolist())
    targets = _probe_targets(n_seg, np.random.default_rng(100 + n_seg))
    assert {0, n_seg - 1} <= first and len(first & set(targets)) >= 0.9 * len(targets)
    _check_coverage(rec, segs, _host_coverage(HostRecords(rec), segs), n_seg)


def _mixed_cigar(rng, n_ops):
    """n_ops ops of every kind, zero-length ones among them; ends ... aligned op, D, S: the record's end lies behind its last
    aligned base."""
    if n_ops == 3:
        return [(M, 400), (EQ, 300), (D, 50)]
    ops = [(S, 3)]
    while len(ops) < n_ops - 3:
        kind = rng.random()
        if kind < 0.5:
            ops.append((int(rng.choice([M, EQ, X])), int(rng.integers(1, 10))))
        elif kind < 0.7:
            ops.append((int(rng.choice([D, N])), int(rng.integers(1, 10))))
        elif kind < 0.9:
            ops.append((int(rng.choice([I, S, P])), int(rng.integers(1, 5))))
        else:
            ops.append((int(rng.choice([M, D, I, EQ, N])), 0))
    return ops + [(M, 7), (D, 9), (S, 5)]


def _many_segment_case(filler):
    """Section 2b: one record each over 1, 2, 4, 5, 8, 9 and 70 segments for CIGARs of 3, 255, 256, 257 and 1000 ops; segment
    boundaries on op boundaries, one base behind them and inside the trailing deletion; next to every record a SEQ-less one over
    its first boundary and one without ops.  ``filler``: that many more segments on a contig without records."""
    rng = np.random.default_rng(77)
    alns, segs, base = [], [], 1000
    for n_ops in (3, 255, 256, 257, 1000):
        for n_over in (1, 2, 4, 5, 8, 9, 70):
            ops = _mixed_cigar(rng, n_ops)
            assert len(ops) == n_ops
            ends = np.cumsum([ln if op in (M, D, N, EQ, X) else 0 for op, ln in ops])
            L = int(ends[-1])
            trailing = L - 4                                                        # inside the trailing deletion
            cand = sorted({int(v) for v in np.concatenate([ends, ends + 1]) if 0 < v < L and v != trailing})
            need = n_over - 1
            cuts = set([trailing] if need else [])
            cuts |= set(rng.choice(cand, min(len(cand), need - len(cuts)), replace=False).tolist()) if need > len(cuts) else set()
            while len(cuts) < need:
                cuts.add(int(rng.integers(1, L)))
            cuts = sorted(cuts)
            bounds = [1 if n_over == 1 else -5] + cuts + [L + 7]
            for k, (s, e) in enumerate(zip(bounds[:-1], bounds[1:])):
                segs.append((0, base + s, base + e - (1 if k % 3 == 1 and e - s >= 3 else 0)))
            c = cuts[0] if cuts else 1
            alns.append(dict(tid=0, pos=base, cigar=ops, nonacgt=[base + c - 1, base + c]))
            alns.append(dict(tid=0, pos=base + max(c - 2, 0), cigar=[(M, 6)], has_seq=0))
            alns.append(dict(tid=0, pos=base + max(c - 1, 0), cigar=[], flag=4, has_seq=1, qlen=30))
            base += L + 200
    alns.sort(key=lambda a: (a["tid"], a["pos"]))
    segs += [(5, 100 + 10 * k, 100 + 10 * k + 10 - k % 2) for k in range(filler)]
    return synth.records_from_alignments(alns), segs


@gpu
@pytest.mark.parametrize("filler", [0, 2100])
def test_segment_coverage_many_segments_per_record(filler):
    """The walk of a straddler: restarts from the top of the CIGAR after every four segments (5, 8, 9, 70), CIGARs of one chunk
    less one op, exactly one chunk, one op more, and of four chunks, the early exit once the walk's last segment is passed - with
    the LDS bins and, with 2100 more segments in the table, with global atomics."""
    from oracle.hostrecords import HostRecords
    rec, segs = _many_segment_case(filler)
    flat = _Flat(rec)
    n_ov, _ = flat.classes(segs)
    assert {1, 2, 4, 5, 8, 9, 70} <= set(n_ov[flat.straddlers(segs)].tolist())
    assert (len(segs) > COV_LDS_SEGS) == (filler > 0)
    assert sorted(set(int(v) for v in np.asarray(rec.n_cigar) if v > 1)) == [3, 255, 256, 257, 1000]
    _check_coverage(rec, segs, _host_coverage(HostRecords(rec), segs), filler)


@gpu
def test_segment_coverage_segments_that_cannot_match():
    """Segments on contigs without records, in front of and behind all records of a contig, and unplaced records (tid -1) at the
    end of the file."""
    from oracle.hostrecords import HostRecords
    rng = np.random.default_rng(9)
    alns = [dict(tid=t, pos=5000 + 13 * k, cigar=[(M, int(rng.integers(5, 60)))]) for t in (1, 3) for k in range(30)]
    alns += [dict(tid=-1, pos=-1, cigar=[], flag=4, has_seq=1, qlen=50) for _ in range(3)]
    rec = synth.records_from_alignments(alns)
    none = [(0, 0, 100), (0, 5000, 5400), (1, 10, 4000), (1, 4000, 5000), (1, 900_000, 900_100), (2, 5000, 6000), (3, 0, 4999),
            (3, 6000, 6001), (4, 5000, 5500), (24, 0, 1 << 30)]
    some = sorted(none + [(1, 5000, 5100), (1, 5100, 5101), (1, 5200, 6000), (3, 5003, 5300), (3, 5300, 5999)])
    host = HostRecords(rec)
    want = _host_coverage(host, none)
    assert want[0].sum() == 0 and want[1].sum() == 0
    _check_coverage(rec, none, want, "none")
    want = _host_coverage(host, some)
    assert (want[0] > 0).sum() >= 4 and want[1].sum() > 0
    _check_coverage(rec, some, want, "some")


@gpu
def test_segment_coverage_more_straddlers_than_waves(crossing):
    """20 000 records across one shared boundary: more straddlers than the walk has waves (2048 workgroups of 4), so a wave walks
    several records and takes every one after its first from the fields it requested a record earlier."""
    _, rec, flat = crossing
    strad = flat.straddlers(CROSS_SEGS)
    n_strad = int(strad.sum())
    per_block = -(-n_strad // WALK_BLOCKS)
    assert n_strad > WALK_BLOCKS * WALK_WAVES and per_block > WALK_WAVES and n_strad % per_block != 0
    n_ov, _ = flat.classes(CROSS_SEGS)
    assert (n_ov >= 2).all() and flat.n // 4 < (n_ov == 3).sum() < flat.n // 2 and len(CROSS_SEGS) <= COV_LDS_SEGS
    # none of the six prefetched fields can be stale unnoticed: neighbours in the list differ in start, end, quads and contig
    assert len(np.unique(flat.pos[strad])) > 1000 and len(np.unique(flat.end[strad])) > 1000
    n_cigar = rec.n_cigar.numpy()
    assert (n_cigar[strad] > 4).sum() > 1000 and (n_cigar[strad] > 8).sum() > 300
    assert len(np.unique(flat.tid[strad])) == CROSS_TAIL + 1
    _check_coverage(rec, CROSS_SEGS, flat.coverage(CROSS_SEGS), "crossing")


@gpu
def test_segment_coverage_second_classify_round(flat_case):
    """More records than one round of the classify loop (2048 workgroups of 256 threads): records inside a segment and
    straddlers whose ordinal lies in the second round."""
    _, rec, flat, segs = flat_case
    assert flat.n > CLASSIFY_ROUND and 80 <= len(segs) <= COV_LDS_SEGS
    n_ov, inside = flat.classes(segs)
    second = np.arange(flat.n) >= CLASSIFY_ROUND
    assert (flat.straddlers(segs) & second).sum() >= 3 and (inside & flat.with_seq & second).sum() >= 50
    assert (flat.straddlers(segs) & ~second).sum() > 500
    _check_coverage(rec, segs, flat.coverage(segs), "flat")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. coral_point_cover
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_points(dr, pts, want_of, pair_cap=0):
    from coral_amd import kernels
    got = kernels.point_cover(dr, pts, pair_cap=pair_cap)
    assert len(got) == len(pts)
    for (t, p), g in zip(pts, got):
        assert np.array_equal(g, want_of(t, p)), (t, p, g[:8], want_of(t, p)[:8])


@gpu
@pytest.mark.parametrize("n_rec", [1, 2, 63, 64, 65, 66, 129, 130, 4224, 4225, 4226])
def test_point_cover_search_boundaries(n_rec):
    """The record search around 64, 65 and 65 * 65 records (unplaced records at the end of the file included in the count): points
    at pos - 1, pos, end - 1 and end of every record, in front of and behind all records of a contig, on contigs without records,
    points with a negative coordinate among them; from 129 records on a workgroup also serves more than one point."""
    from coral_amd.records import DeviceRecords
    from oracle.hostrecords import HostRecords
    rng = np.random.default_rng(300 + n_rec)
    n_un = min(3, n_rec - 1)
    n_pl = n_rec - n_un
    alns = []
    for t, k, p in ((0, (n_pl + 1) // 2, 0), (3, n_pl // 2, 7)):
        for _ in range(k):
            alns.append(dict(tid=t, pos=p, cigar=[(M, int(rng.integers(1, 31)))]))
            p += int(rng.integers(1, 6))
    alns += [dict(tid=-1, pos=-1, cigar=[], flag=4, has_seq=1, qlen=50) for _ in range(n_un)]
    rec = synth.records_from_alignments(alns)
    host = HostRecords(rec)
    assert host.n == n_rec and (host.tid[n_pl:] == -1).all()
    pts = [(0, 0), (0, int(host.end[:n_pl].max()) + 50), (3, 100_000), (1, 0), (1, 10), (2, 100), (24, 5), (4, 0)]
    for i in range(n_pl):
        t, p, e = int(host.tid[i]), int(host.pos[i]), int(host.end[i])
        pts += [(t, p - 1), (t, p), (t, e - 1), (t, e)]
        if i % 5 == 0:
            pts.append([(t, -3), (-1, p), (-1, -1), (t, -(1 << 31))][(i // 5) % 4])
    distinct = len({tp for tp in pts if tp[0] >= 0 and tp[1] >= 0})
    assert n_rec < 4224 or distinct > POINT_JOBS // POINT_SLICES, distinct          # three of the sizes: workgroups take a second job
    assert (0, -1) in pts
    order = rng.permutation(len(pts))
    _check_points(DeviceRecords(rec, "cuda:0"), [pts[k] for k in order], lambda t, p: _host_cover(host, t, p))


def _point_cover_raw(dr, uniq, max_span):
    """coral_point_cover itself on sorted distinct points with the given max_span: the record ordinals per point, ascending."""
    import ctypes as C
    from coral_amd import _lib
    uniq = np.asarray(uniq, dtype=np.int64)
    assert (np.diff((uniq[:, 0] << 32) | uniq[:, 1]) > 0).all()
    t = torch.tensor(uniq[:, 0], dtype=torch.int32, device=dr.device)
    p = torch.tensor(uniq[:, 1], dtype=torch.int32, device=dr.device)
    cap = len(uniq) * dr.n
    pairs = torch.empty(cap, dtype=torch.int64, device=dr.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=dr.device)
    rs = dr.c_struct()
    _lib.check(_lib.lib().coral_point_cover(C.byref(rs), len(uniq), t.data_ptr(), p.data_ptr(), max_span, pairs.data_ptr(),
                                            cnt.data_ptr(), cap, dr.stream()), "coral_point_cover")
    k = int(cnt.item()) & 0xFFFFFFFF
    assert k <= cap
    keys = np.sort(pairs[:k].cpu().numpy())
    return [(keys[keys >> 32 == j] & 0xFFFFFFFF) for j in range(len(uniq))]


@gpu
def test_point_cover_max_span_window():
    """The window [p - max_span + 1, p] of record starts: the file's longest record covers a point with its last base, so it is
    the window's first record; the same points with max_span unknown (0, -1) and one too large."""
    from coral_amd.records import DeviceRecords
    from oracle.hostrecords import HostRecords
    rng = np.random.default_rng(12)
    alns = [dict(tid=0, pos=100 + 20 * k, cigar=[(M, int(rng.integers(1, 300)))]) for k in range(40)]
    alns += [dict(tid=0, pos=1000, cigar=[(M, 40)]), dict(tid=0, pos=1000, cigar=[(M, 5000)]), dict(tid=0, pos=1000, cigar=[(M, 3)])]
    inner = np.sort(rng.integers(1001, 6000, 200))
    alns += [dict(tid=0, pos=int(p), cigar=[(M, int(rng.integers(1, 300)))]) for p in inner]
    alns += [dict(tid=0, pos=6000 + 50 * k, cigar=[(EQ, 299)]) for k in range(20)]
    alns += [dict(tid=1, pos=10, cigar=[(M, 4999)])]
    rec = synth.records_from_alignments(alns)
    host, dr = HostRecords(rec), DeviceRecords(rec, "cuda:0")
    longest = 41
    assert dr.max_span == 5000 == int(host.end[longest] - host.pos[longest]) and (np.delete(host.end - host.pos, longest) < 5000).all()
    pts = [(0, 999), (0, 1000), (0, 1001), (0, 5998), (0, 5999), (0, 6000), (0, 6001), (1, 10), (1, 5008), (1, 5009)]
    want = [_host_cover(host, t, p) for t, p in pts]
    assert longest in want[4] and longest not in want[5] and len(want[4]) > 1 and want[4][0] == longest
    _check_points(dr, pts, lambda t, p: _host_cover(host, t, p))
    for max_span in (5000, 5001, 0, -1):
        got = _point_cover_raw(dr, pts, max_span)
        for k in range(len(pts)):
            assert np.array_equal(got[k], want[k]), (max_span, pts[k], got[k], want[k])


@gpu
def test_point_cover_window_wider_than_a_slice_round(crossing):
    """More than 32 * 256 records in the window of one point: every workgroup of the point goes through its slice loop more than
    once; pair_cap = 128, so the launch is repeated with room for all pairs."""
    from coral_amd.records import DeviceRecords
    _, rec, flat = crossing
    pts = [(0, CROSS_X - 1), (0, CROSS_X), (0, CROSS_X + 1), (0, CROSS_Z)]
    n_cov = [len(flat.cover(t, p)) for t, p in pts]
    assert min(n_cov[:3]) > 2 * SLICE_ROUND and n_cov[3] > 4000 and n_cov[3] < n_cov[0]
    dr = DeviceRecords(rec, "cuda:0")
    lo = np.searchsorted(flat.pos, CROSS_Z - dr.max_span + 1)
    assert np.searchsorted(flat.pos, CROSS_Z, side="right") - lo > SLICE_ROUND            # the window itself, not only its hits
    _check_points(dr, pts, flat.cover, pair_cap=128)
