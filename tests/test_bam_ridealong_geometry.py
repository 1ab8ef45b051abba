"""The kernels that ride along the GPU BAM decoder (read QC, FASTQ text, record copy / sorted copy / shifted copy, coordinate sort,
binned depth, window coverage, pileup, the BAI index) at the record counts where their launch geometry changes: every one is a
grid-stride loop over work items with a fixed grid cap, and the other BAM test modules stay below a thousand work items per batch.
One file of 36 946 records (short ones of 1 .. 80 bases and five reads of 40 000 bases, 4.2 MB inflated) and a shuffled twin of
it, each decoded as ONE batch; every result is compared exactly - every record, bin, position and byte - with tests/bamfile.py and
the restatements the other BAM test modules own (imported from them, not copied).  Nothing expected has passed through either
decoder.  Every test runs on the host pipeline too (not marked gpu): that pins the fixture and the restatements at this size, so
that a GPU failure points at the kernels.

Thresholds crossed (test_fixture_crosses_every_threshold asserts each of them from the parsed file, the item counts with the
kernels' plan rules as their comments state them):
  k_bam_qc              2 048 workgroups of one wave, an item = 16 384 QUAL bytes: 34 700 items; items 2 047 and 2 048 lie in one read
  k_bam_reads_emit      2 048 x 16 384 bases: 34 772 items, items 2 047 and 2 048 in one read; with exclude_flags = 0 and with regions
                        more than 2 048 items as well
  k_bam_reads_copy      2 048 x 32 768 record bytes: 36 951 items, items 2 047 and 2 048 in one 60 kB record; with regions more than
  (_sorted, _shifted)   2 048; the sorted copy sees the twin's 37 310 records, the shifted copy (view_bam) the same selections
  k_bam_depth           8 192 workgroups, one record each: 36 946 records, four and a half rounds
  k_bam_pileup          8 192 x 16 384 query bases: more than 32 768 items, items 8 191 and 8 192 in one read
  k_bam_cov_count       8 192 workgroups x 4 waves = 32 768: 34 689 items at threshold 0 with 'all' - items 8 191 | 8 192 in one
                        read, 32 767 | 32 768 in another -, more than 32 768 at thresholds 0 and 20 with both callbacks
  item_record           runs of records without a work item in front of the first item, behind the last, of 70 and of 2 100
                        records (QC, FASTQ, coverage with 'all'), of 2 300 where regions leave a stretch of the contig out
                        (pileup, FASTQ and record copy with regions)
  hipcub radix sort     37 310 keys in one batch, three tie groups of 120 records spread over the whole file, a reverse-strand
                        record in front of a forward one at one position, unplaced records among the first ten
  hipcub scan           every request's n_rec + 1 counts, several requests taking the parse's scratch arrays in turn
Every GPU decode asserts LAST_DECODE["batches"] == 1: the caps are per batch.

The records request does not go with an index request (coral_bam_common.h refuses the pair), so "everything at once" is two
decodes: QC + pileup + depth + index with the records, and QC + pileup + depth + a records request.

Shown to bite on single-line mutants of coral_amd/csrc/coral_bamgpu_*.h (eight builds), each built in a scratch copy of the tree; each one only
removes work or changes a value (no index range, load or store gets wider).  For every mutant the request's own GPU test
module(s) were run, then this module (-m gpu):
  k_bam_qc          `w < total` -> `w < min(total, (long long)gridDim.x)`: what lies behind the first round is dropped.
                    tests/test_read_qc.py passes; fails test_read_qc[gpu] and test_everything_at_once[gpu].
  k_bam_reads_emit, _copy, _copy_sorted, _copy_shifted   the same change in each (one build): the tail of the output stays as the
                    buffer had it.  tests/test_extract_reads.py, test_extract_records.py, test_view_stream.py and
                    test_sort_records.py pass (62 GPU tests); fails all of test_fastq_text[gpu-*] (emit), test_record_bytes[gpu-*]
                    (copy), test_streamed_view[*] (shifted), test_coordinate_order[gpu] (sorted) and test_everything_at_once[gpu].
  k_bam_depth       `i += gridDim.x` -> `i += 2 * gridDim.x`: every other round is skipped.  tests/test_binned_depth.py passes;
                    fails all six test_binned_depth[gpu-*] and test_everything_at_once[gpu].
  k_bam_cov_count   `w < total` -> `w < min(total, n_waves)`.  tests/test_window_coverage.py passes; fails all four
                    test_window_coverage[gpu-*].  (Leaving out the `flush()` that ends the item loop's body is not a geometry
                    mutant in this kernel: the counts and the current segment are variables of one item, so it loses every item's
                    last segment at any size.  All 7 GPU tests of tests/test_window_coverage.py fail on it, and the four here.)
  k_bam_pileup      the stride-bound change.  tests/test_pileup.py passes; fails both test_pileup[gpu-*] and
                    test_everything_at_once[gpu].
  item_record       `b = n_rec` -> `b = min(n_rec, 8192ll)`: an item behind record 8 191 is given to that record, where its slice is
                    empty.  The seven GPU modules of the requests above pass (98 tests); fails 16 of this module's 24 GPU tests:
                    everything but the depth, the index and the plain decode, which do not search.
  k_bam_sort_keys   the strand bit left out of the key.  This one the existing module already catches: 8 GPU tests of
                    tests/test_sort_records.py fail, whose file plants the same reverse-in-front-of-forward pair; here
                    test_coordinate_order[gpu] fails at `fwd_second`, and only there: the tie groups stay in file order.

Measured: the module-scoped fixture (both files built, written and read back) takes 1.6 s of CPU; the whole module takes 20 s on
the host pipeline alone and 10 s for its 24 GPU tests on an MI355X, the slowest test 0.9 s.
"""
import gzip
import os
import random
import struct

import numpy as np
import pytest
import torch  # noqa: F401

from coral_amd import _lib, bam
from tests.bamfile import D, EQ, I, M, N, X, oracle_coverage, pairs, read_bam, restate_read_qc
from tests.decode_support import DEVICE, PIPELINES, _pipeline_by_device, assert_qc_equals_restatement, assert_same_qc  # noqa: F401
from tests.test_bam_index import restated_index
from tests.test_binned_depth import Restatement as DepthRestatement
from tests.test_extract_reads import assert_reads, end_of, want_reads, write_raw, written as fastq_written
from tests.test_extract_records import assert_records, want_records, written as record_written
from tests.test_pileup import counted_bases, restated_table
from tests.test_sort_records import reg2bin, sort_key, want_sorted

# ---- the launch geometry (coral_amd/csrc/coral_bamgpu_*.h) ------------------------------------------------------------------------
SLICE = 16384                   # QC_SLICE, READS_SLICE, COV_SLICE: QUAL bytes / bases / query bases per work item
COPY_SLICE = 32768              # READS_COPY_SLICE: record bytes per work item
CAP_WAVES = 2048                # k_bam_qc, k_bam_reads_emit, k_bam_reads_copy*: workgroups of one wave
CAP_DEPTH = CAP_PILEUP = 8192   # k_bam_depth, k_bam_pileup: workgroups of one wave
CAP_COUNT = 8192 * 4            # k_bam_cov_count: workgroups of four waves

# ---- the file ---------------------------------------------------------------------------------------------------------------------
REFS = [("bulk", 400_000), ("side", 50_000), ("empty", 10_000), ("tail", 20_000)]
LONG = 40_000                   # bases of a long read: three items of 16 384 bases, two of 32 768 record bytes
N_BULK = 34_400                 # ordinary records on `bulk`: l_seq cycles through 1 .. 80, a third on the reverse strand
FRONT_RUN, SHORT_RUN, MIDDLE_RUN, HOLE_READS, END_RUN = 12, 70, 2100, 200, 8
HOLE_AT = 12_000                # ordinary records in front of the middle run
PLANTED_RECORDS, PLANTED_QC, PLANTED_FASTQ, PLANTED_COPY, PLANTED_COV = 36_946, 34_700, 34_772, 36_951, 34_689


def header_bytes():
    text = ("@HD\tVN:1.6\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in REFS)).encode()
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(REFS))
    for name, ln in REFS:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    return out


_J = np.arange(LONG + 4096, dtype=np.int64)
# SEQ codes: A / C / G / T, an N at every 13th base, an `=` now and then; QUAL 0 .. 44, on both sides of the threshold 20
_CODES = np.where(_J % 13 == 5, 15, np.where(_J % 101 == 7, 0, 1 << ((_J * 7 + _J // 5) % 4))).astype(np.uint8)
_QUAL = ((_J * 5 + _J // 7) % 45).astype(np.uint8)


def record(tid, pos, flag, name, l_seq, mapq=30, cigar=None, qual=True, k=0):
    """One record's bytes, block_size word first, in the style of test_sort_records.raw_record: by default a single M op of l_seq
    bases (of 30 for a record without SEQ) when it is placed and mapped, no tag; qual False: QUAL absent (0xff throughout)."""
    if cigar is None:
        cigar = [(M, l_seq or 30)] if tid >= 0 and not flag & 4 else []
    at = (k * 37) % 4000
    codes = _CODES[at:at + l_seq + (l_seq & 1)]
    q = _QUAL[at:at + l_seq].tobytes() if qual else b"\xff" * l_seq
    rlen = sum(n for op, n in cigar if op in (M, D, N, EQ, X))
    name_b = name.encode() + b"\0"
    bin_ = reg2bin(pos, pos + max(rlen, 1)) if tid >= 0 else 4680
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name_b), mapq, bin_, len(cigar), flag, l_seq, -1, -1, 0) + name_b
    body += struct.pack("<%dI" % len(cigar), *[(n << 4) | op for op, n in cigar]) + ((codes[0::2] << 4) | codes[1::2]).astype(np.uint8).tobytes() + q
    return struct.pack("<i", len(body)) + body


# records that get no work item under one rule or another: (flag, has SEQ, has QUAL)
ZERO_KINDS = [(0x100, True, True), (0, False, True), (0x800, True, True), (0, True, False), (4, True, True), (0x400, True, True)]
# ... and under every rule that looks at the flag or at SEQ (QC, FASTQ with its default 0x900, coverage with 'all')
ZERO_EVERYWHERE = [(0x100, True, True), (0x900, True, True), (0x500, True, True), (0x100, True, False), (0, False, True), (0x104, False, True)]
LONG_CIGARS = {"long_copy": [(M, LONG)], "long_fastq": [(M, 15_000), (I, 10), (D, 20), (M, LONG - 15_010)], "long_qc": [(M, LONG)],
               "long_cov8k": [(M, 9_000), (D, 5), (M, 7_383), (I, 2), (M, 2), (N, 40), (M, LONG - 16_387)], "long_cov32k": [(M, LONG)]}


def build_sorted():
    """[record bytes] in coordinate order, and (HOLE_LO, HOLE_HI): the stretch of `bulk` that the region requests leave out.
    The builder counts the work items of the four primary rules as it goes, only to know where a long read belongs; the fixture
    counts them again from the parsed file and asserts."""
    recs, cnt, hole = [], dict(qc=0, fastq=0, copy=0, cov=0), [None, None]
    shift = [0]

    def add(tid, flag, l_seq, qual=True, name=None, cigar=None, pos=None):
        k = len(recs)
        if pos is None:
            pos = 300 + 3 * k + shift[0] if tid >= 0 else -1
        b = record(tid, pos, flag, name or "r%d" % k, l_seq, mapq=k % 61, cigar=cigar, qual=qual, k=k)
        recs.append(b)
        read = l_seq > 0 and not flag & 0x900
        items = -(-l_seq // SLICE)
        cnt["qc"] += items if read and qual else 0
        cnt["fastq"] += items if read else 0
        cnt["copy"] += -(-len(b) // COPY_SLICE)
        cnt["cov"] += items if tid == 0 and l_seq > 0 and not flag & 0x704 else 0
        return pos

    def zero(kinds, n, tid=0):
        for j in range(n):
            flag, seq, qual = kinds[j % len(kinds)]
            add(tid, flag if tid >= 0 else flag | 4, 1 + (7 * j) % 80 if seq else 0, qual)

    # a long read goes in as soon as the items in front of it put 2 047 | 2 048 (8 191 | 8 192, 32 767 | 32 768) inside it
    wanted = [("long_copy", "copy", CAP_WAVES - 1, CAP_WAVES - 1), ("long_fastq", "fastq", CAP_WAVES - 2, CAP_WAVES - 1),
              ("long_qc", "qc", CAP_WAVES - 2, CAP_WAVES - 1), ("long_cov8k", "cov", CAP_PILEUP - 2, CAP_PILEUP - 1),
              ("long_cov32k", "cov", CAP_COUNT - 2, CAP_COUNT - 1)]

    def ordinary(n):
        for _ in range(n):
            for w in list(wanted):
                name, rule, lo, hi = w
                if name == "long_cov32k" and "long_cov8k" in [x[0] for x in wanted]:
                    continue
                assert cnt[rule] <= hi, (name, cnt)
                if cnt[rule] >= lo:
                    add(0, 0, LONG, name=name, cigar=LONG_CIGARS[name])
                    wanted.remove(w)
            k = len(recs)
            add(0, 0x10 if k % 3 == 1 else 0, 1 + k % 80)

    zero(ZERO_KINDS, FRONT_RUN)
    ordinary(50)
    zero(ZERO_EVERYWHERE, SHORT_RUN)                                    # a run of more than 64
    ordinary(20)
    for j in range(SHORT_RUN):                                          # QUAL absent: 70 more without a QC item
        add(0, 0, 1 + (11 * j) % 80, qual=False)
    ordinary(HOLE_AT - 70)
    shift[0] += 100                                                     # (whatever lies in front ends in front of the hole)
    hole[0] = 300 + 3 * len(recs) + shift[0]
    zero(ZERO_EVERYWHERE, MIDDLE_RUN)                                   # a run of more than 2 048
    for j in range(HOLE_READS):                                         # ordinary reads that only the region requests leave out
        last = add(0, 0x10 if j % 3 == 1 else 0, 1 + j % 80)
    hole[1] = last + 1 + (HOLE_READS - 1) % 80                          # the last one ends exactly where the hole ends
    shift[0] += 100
    ordinary(N_BULK - HOLE_AT)
    assert not wanted, wanted
    for j in range(SHORT_RUN):                                          # off every requested segment
        add(1, 0x10 if j % 2 else 0, 20 + j % 50, pos=100 + 3 * j)
    for j in range(5):
        add(3, 0, 33 + j, pos=40 + 10 * j)
    for j in range(6):                                                  # without coordinates, with SEQ and QUAL: reads all the same
        add(-1, 4, 40 + j)
    zero(ZERO_EVERYWHERE, END_RUN, tid=-1)
    return recs, tuple(hole)


def build_twin(recs):
    """The same records shuffled, and on top: three tie groups of 120 records with one key each under distinct names, spread over
    the whole file; a reverse-strand record in front of a forward one at one position; unplaced records among the first ten."""
    recs = list(recs)
    random.Random(20250131).shuffle(recs)
    n = len(recs)
    ties = {"tieA": (0, 41_234, 0), "tieB": (0, 90_001, 0x10), "tieC": (1, 77, 0)}
    for g, (name, (tid, pos, flag)) in enumerate(sorted(ties.items())):
        for j in range(120):
            recs.insert((j * n) // 120 + 7 * g + 11, record(tid, pos, flag, "%s_%03d" % (name, j), 10 + (j + g) % 60, k=j))
    recs.insert(100, record(0, 77_778, 0x10, "rev_first", 25))
    recs.insert(n - 50, record(0, 77_778, 0, "fwd_second", 26))
    recs.insert(2, record(-1, -1, 4, "u_early_a", 40))
    recs.insert(6, record(-1, -1, 4, "u_early_b", 0))
    return recs, ties


# ---- the kernels' plan rules, restated from their comments, on the parsed records ---------------------------------------------------
def _slices(n, slice_):
    return -(-int(n) // slice_)


def items_qc(parsed):
    """k_bam_qc_plan: qc_is_read && QUAL present"""
    return np.array([_slices(r["l_seq"], SLICE) if r["flag"] & 0x900 == 0 and r["l_seq"] > 0 and r["qual"][0] != 0xFF else 0 for r in parsed.recs])


def items_fastq(parsed, regions=None, exclude_flags=0x900):
    """k_bam_reads_plan, FASTQ: reads_takes_part and the regions"""
    return np.array([_slices(r["l_seq"], SLICE) if fastq_written(r, parsed.refs, regions, None, exclude_flags) else 0 for r in parsed.recs])


def items_copy(parsed, regions=None, exclude_flags=0):
    """k_bam_reads_plan, records: SEQ is not required, the items are slices of the record's own bytes"""
    return np.array([_slices(r["size"], COPY_SLICE) if record_written(r, parsed.refs, regions, None, exclude_flags) else 0 for r in parsed.recs])


def items_cov(parsed, windows, threshold, read_callback):
    """k_bam_cov_plan: on a contig, SEQ, a CIGAR, not filtered, QUAL present at a threshold above 0, a segment met (an unmapped
    record with a CIGAR is walked whatever bam_endpos says).  The segments are the windows cut up: a record meets one of them
    when it meets a window."""
    out = []
    for r in parsed.recs:
        ok = r["tid"] >= 0 and r["l_seq"] > 0 and len(r["ops"]) > 0 and not (read_callback == "all" and r["flag"] & 0x704)
        ok = ok and (threshold == 0 or r["qual"][0] != 0xFF)
        if ok:
            end = 1 << 40 if r["flag"] & 4 else end_of(r)
            ok = any(parsed.refs[r["tid"]] == c and a < b and a < end and b > r["pos"] for c, a, b in windows)
        out.append(_slices(r["l_seq"], SLICE) if ok else 0)
    return np.array(out)


def straddles(items, k, w):
    """Record k owns the work items w - 1 and w."""
    off = np.concatenate([[0], np.cumsum(items)])
    return bool(off[k] <= w - 1 and w < off[k + 1])


def zero_runs(items):
    """(records without a work item in front of the first item, behind the last, the lengths of all such runs in descending order)"""
    runs, n = [], 0
    for v in list(items) + [1]:
        if v:
            runs.append(n)
            n = 0
        else:
            n += 1
    return runs[0], runs[-1], sorted(runs, reverse=True)


# ---- the requests -------------------------------------------------------------------------------------------------------------------
def requests_of(hole):
    lo, hi = hole
    narrow = [("bulk", 1_000 + 2_900 * j, 1_000 + 2_900 * j + 1 + 17 * (j % 5)) for j in range(36)]
    return dict(
        read_regions=[("bulk", 500, lo), ("bulk", hi, 300_000), ("tail", 0, 20_000)],
        pile_regions=[("bulk", 0, lo), ("bulk", hi, 150_000)],
        # one window over the bulk, narrow ones, one that only a long read reaches, one on the contig without records
        windows=[("bulk", 0, 150_000)] + narrow + [("bulk", 115_000, 138_000), ("empty", 0, 10_000)])


COVERAGE_RULES = [(0, "all"), (0, "nofilter"), (20, "all"), (20, "nofilter")]
DEPTH_RULES = [(b, cd) for b in (1, 7, 1000) for cd in (True, False)]


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    d = tmp_path_factory.mktemp("ridealong_geometry")
    header = header_bytes()
    blobs, hole = build_sorted()
    twin_blobs, ties = build_twin(blobs)
    out = dict(dir=d, header=header, hole=hole, ties=ties, memo={}, **requests_of(hole))
    for key, recs in (("sorted", blobs), ("twin", twin_blobs)):
        raw = header + b"".join(recs)
        path = str(d / (key + ".bam"))
        write_raw(raw, path)
        parsed = read_bam(path)
        assert len(parsed.recs) == len(recs) and parsed.n_bytes == len(raw) and [(c, l) for c, l in zip(parsed.refs, parsed.lens)] == REFS
        out[key] = dict(path=path, raw=raw, parsed=parsed, header=header)          # (the `case` of want_records / want_sorted)
    return out


def memo(big, key, make):
    """An expectation computed once for the host and the GPU test that share it, and never changed."""
    if key not in big["memo"]:
        big["memo"][key] = make()
    return big["memo"][key]


def one_batch(pipe):
    if pipe == "gpu":
        assert bam.LAST_DECODE.get("where") == "gpu" and bam.LAST_DECODE["batches"] == 1, bam.LAST_DECODE


def by_name(parsed):
    return {r["name"]: k for k, r in enumerate(parsed.recs)}


# ---- 1. the fixture crosses what it is meant to cross ------------------------------------------------------------------------------
def test_fixture_crosses_every_threshold(big):
    parsed, twin = big["sorted"]["parsed"], big["twin"]["parsed"]
    R, at = parsed.recs, by_name(parsed)
    lo, hi = big["hole"]
    assert len(R) == PLANTED_RECORDS > CAP_DEPTH and parsed.n_bytes < 8 << 20           # one default batch (64 MiB) by far
    keys = [(r["tid"] & 0xFFFFFFFF, r["pos"]) for r in R]
    assert keys == sorted(keys) and R[-1]["tid"] == -1                                  # coordinate order, unplaced last
    bulk = [r for r in R if r["name"].startswith("r") and r["tid"] == 0 and r["flag"] & ~0x10 == 0 and r["l_seq"] and r["qual"][0] != 0xFF]
    assert len(bulk) >= 34_000 and {r["l_seq"] for r in bulk} == set(range(1, 81)) and {r["start"] % 16 for r in bulk} == set(range(16))
    assert 0.3 < sum(1 for r in bulk if r["flag"] & 0x10) / len(bulk) < 0.37
    kinds = {(r["flag"] & 0xD04, r["l_seq"] > 0, r["l_seq"] == 0 or r["qual"][0] != 0xFF) for r in R}
    assert {(f, s, q) for f, s, q in ZERO_KINDS} <= kinds
    longs = [r for r in R if r["l_seq"] == LONG]
    assert sorted(r["name"] for r in longs) == sorted(LONG_CIGARS) and all(_slices(r["size"], COPY_SLICE) == 2 for r in longs)
    assert sum(len(r["ops"]) > 1 for r in longs) == 2

    # the work items of the primary rules, and the long read that lies across each round's end
    qc, fastq, copy = items_qc(parsed), items_fastq(parsed), items_copy(parsed)
    cov = items_cov(parsed, big["windows"], 0, "all")
    pile = items_cov(parsed, big["pile_regions"], 0, "all")
    assert (int(qc.sum()), int(fastq.sum()), int(copy.sum()), int(cov.sum())) == (PLANTED_QC, PLANTED_FASTQ, PLANTED_COPY, PLANTED_COV)
    assert min(PLANTED_QC, PLANTED_FASTQ, PLANTED_COPY) > CAP_WAVES and PLANTED_COV > CAP_COUNT and int(pile.sum()) > CAP_COUNT > CAP_PILEUP
    assert straddles(qc, at["long_qc"], CAP_WAVES) and straddles(fastq, at["long_fastq"], CAP_WAVES) and straddles(copy, at["long_copy"], CAP_WAVES)
    assert straddles(cov, at["long_cov8k"], CAP_PILEUP) and straddles(pile, at["long_cov8k"], CAP_PILEUP) and straddles(cov, at["long_cov32k"], CAP_COUNT)
    # ... the other requests of this module cross the same caps, wherever their rounds end
    for thr, cb in COVERAGE_RULES:
        assert items_cov(parsed, big["windows"], thr, cb).sum() > CAP_COUNT, (thr, cb)
    assert items_cov(parsed, big["pile_regions"], 20, "nofilter").sum() > CAP_PILEUP
    assert items_fastq(parsed, exclude_flags=0).sum() > fastq.sum()
    fastq_reg, copy_reg = items_fastq(parsed, big["read_regions"]), items_copy(parsed, big["read_regions"])
    assert fastq_reg.sum() > CAP_WAVES and copy_reg.sum() > CAP_WAVES and np.count_nonzero(fastq_reg) > CAP_WAVES

    # runs of records without work items: in front, at the end, one of more than 64, one of more than 2 048
    for name, items in (("qc", qc), ("fastq", fastq), ("cov", cov), ("pile", pile), ("fastq_reg", fastq_reg), ("copy_reg", copy_reg)):
        head, tail, runs = zero_runs(items)
        assert head >= 2 and tail >= END_RUN and runs[0] > CAP_WAVES and runs[1] > 64, (name, head, tail, runs[:4])
    assert zero_runs(copy) == (0, 0, [0] * (len(R) + 1))                                # (the whole-file copy leaves no record out)
    in_hole = [r for r in R if r["tid"] == 0 and r["pos"] >= lo and end_of(r) <= hi]
    assert len(in_hole) == MIDDLE_RUN + HOLE_READS and max(end_of(r) for r in in_hole) == hi and cov[at[in_hole[-1]["name"]]] == 1
    # the window that only a long read reaches
    c, a, b = big["windows"][-2]
    assert [r["name"] for r in R if r["tid"] == 0 and r["pos"] < b and end_of(r) > a] == ["long_cov32k"]
    assert not any(r["tid"] == 2 for r in R)

    # the twin: the same records and the planted ones, not in order; ties, reverse in front of forward, unplaced first
    T, tw = twin.recs, by_name(twin)
    assert len(T) == len(R) + 3 * 120 + 4 > CAP_WAVES and sorted(r["name"] for r in T if r["name"] in at) == sorted(at)
    tkeys = [sort_key(r) for r in T]
    assert tkeys != sorted(tkeys)
    for name, (tid, pos, flag) in big["ties"].items():
        group = [k for k, r in enumerate(T) if (r["tid"], r["pos"], r["flag"] & 0x10) == (tid, pos, flag)]
        assert len(group) == 120 and [T[k]["name"] for k in group] == ["%s_%03d" % (name, j) for j in range(120)]
        assert group[0] < len(T) // 100 * 2 and group[-1] > len(T) // 100 * 97 and max(np.diff(group)) < len(T) // 100
    rev, fwd = T[tw["rev_first"]], T[tw["fwd_second"]]
    assert (rev["tid"], rev["pos"]) == (fwd["tid"], fwd["pos"]) and rev["flag"] & 0x10 and not fwd["flag"] & 0x10 and rev["start"] < fwd["start"]
    assert sum(1 for r in T[:10] if r["tid"] == -1) >= 2


@pytest.mark.gpu
def test_a_plain_gpu_decode_is_one_batch(big):
    for key in ("sorted", "twin"):
        rec = bam.load_bam(big[key]["path"], device="cuda:0", n_threads=2)
        assert rec.n == len(big[key]["parsed"].recs) and bam.LAST_DECODE["where"] == "gpu" and bam.LAST_DECODE["batches"] == 1


# ---- 2. one test per kernel: host pipeline (pins fixture and restatement at this size) and GPU -----------------------------------------
@pytest.mark.parametrize("pipe", PIPELINES)
def test_read_qc(big, pipe):
    """k_bam_qc: every workgroup serves about 17 items and adds its LDS table once"""
    want = memo(big, "qc", lambda: restate_read_qc(big["sorted"]["parsed"].recs))
    got = bam.read_qc(big["sorted"]["path"], device=DEVICE[pipe], n_threads=2)
    one_batch(pipe)
    assert_qc_equals_restatement(got, want, pipe)
    assert (want["qual_sum"] == -1).sum() >= SHORT_RUN and (want["qual_sum"] == 0).sum() >= 1 and int(want["hist"].sum()) > 1_000_000


FASTQ_SELECTIONS = {"whole file": dict(), "regions": dict(regions="read_regions"), "no flag excluded": dict(exclude_flags=0)}


@pytest.mark.parametrize("what", list(FASTQ_SELECTIONS))
@pytest.mark.parametrize("pipe", PIPELINES)
def test_fastq_text(big, pipe, what):
    """k_bam_reads_emit"""
    kw = dict(FASTQ_SELECTIONS[what])
    regions = big[kw.pop("regions")] if "regions" in kw else None
    want = memo(big, ("fastq", what), lambda: want_reads(big["sorted"]["parsed"], regions, None, kw.get("exclude_flags", 0x900)))
    got = bam.extract_reads(big["sorted"]["path"], regions, device=DEVICE[pipe], n_threads=2, index=False, **kw)
    one_batch(pipe)
    assert len(want[1]) > CAP_WAVES
    assert_reads(got, want, what)
    assert got.offsets.tolist() == np.concatenate([[0], np.cumsum([len(t) for t in want[1]])]).tolist()


@pytest.mark.parametrize("what", ["whole file", "regions"])
@pytest.mark.parametrize("pipe", PIPELINES)
def test_record_bytes(big, pipe, what):
    """k_bam_reads_copy"""
    case = big["sorted"]
    regions = big["read_regions"] if what == "regions" else None
    want = memo(big, ("records", what), lambda: want_records(case, regions))
    got = bam.extract_records(case["path"], regions, device=DEVICE[pipe], n_threads=2, index=False)
    one_batch(pipe)
    assert CAP_WAVES < len(want[1]) and (what == "regions") == (len(want[1]) < len(case["parsed"].recs))
    assert_records(got, want, what)
    assert got.header == case["header"] and got.order == "file"
    if what == "whole file":
        assert got.data.tobytes() == case["raw"][len(case["header"]):]


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["whole file", "regions"])
def test_streamed_view(big, what, tmp_path):
    """k_bam_reads_copy_shifted: the batch's records land behind the bytes carried for the output's first block"""
    case = big["sorted"]
    regions = big["read_regions"] if what == "regions" else None
    names, blobs = memo(big, ("records", what), lambda: want_records(case, regions))
    out = str(tmp_path / "view.bam")
    st = bam.view_bam(case["path"], out, regions, device="cuda:0", n_threads=2, bam_index=False)
    one_batch("gpu")
    with open(out, "rb") as fp:
        raw = fp.read()
    payload = b"".join(blobs)
    assert gzip.decompress(raw) == case["header"] + payload
    assert st == bam.ViewStats(len(blobs), len(payload), len(raw)) and len(blobs) > CAP_WAVES


def check_order(big, names):
    """What the contract of `sort` says about the twin, on the names as they came out."""
    where = {n: k for k, n in enumerate(names)}
    for g in big["ties"]:
        got = [n for n in names if n.startswith(g + "_")]
        assert got == ["%s_%03d" % (g, j) for j in range(120)], g                     # equal keys: file order
        assert where[got[-1]] - where[got[0]] == 119, g                               # ... and nothing in between
    assert where["fwd_second"] + 1 == where["rev_first"]                               # forward before reverse at one position
    T = big["twin"]["parsed"].recs
    unplaced = [r["name"] for r in T if r["tid"] == -1]
    assert names[-len(unplaced):] == unplaced and names[-len(unplaced)] == "u_early_a"      # unplaced last, in file order


@pytest.mark.parametrize("pipe", PIPELINES)
def test_coordinate_order(big, pipe, tmp_path):
    """k_bam_sort_keys, hipcub's radix sort over 37 000 keys, k_bam_sort_permute, k_bam_reads_copy_sorted: one batch, so the device
    sort alone decides the order and the host merge sees one run."""
    case = big["twin"]
    want = memo(big, "sorted", lambda: want_sorted(case))
    check_order(big, want[0])                                                          # (the restatement itself keeps the contract)
    got = bam.extract_records(case["path"], device=DEVICE[pipe], n_threads=2, index=False, order="coordinate")
    one_batch(pipe)
    assert_records(got, want, pipe)
    check_order(big, got.names())
    assert got.order == "coordinate" and got.header == bam.sorted_header_bytes(case["header"]) and got.n == len(case["parsed"].recs) > CAP_WAVES
    out = str(tmp_path / "sorted.bam")
    assert bam.sort_bam(case["path"], out, index=False, device=DEVICE[pipe], n_threads=2) == out
    one_batch(pipe)
    with gzip.open(out, "rb") as fp:
        assert fp.read() == bam.sorted_header_bytes(case["header"]) + b"".join(want[1])


@pytest.mark.parametrize("bin_size,count_deletions", DEPTH_RULES)
@pytest.mark.parametrize("pipe", PIPELINES)
def test_binned_depth(big, pipe, bin_size, count_deletions):
    """k_bam_depth: 8 192 workgroups, four and a half rounds"""
    want = memo(big, "depth", lambda: DepthRestatement(big["sorted"]["path"]))
    for exclude in (0x704, 0):
        off, bases, reads = want.tables(bin_size, 0, exclude, count_deletions)
        got = bam.binned_depth(big["sorted"]["path"], bin_size, 0, exclude, count_deletions, device=DEVICE[pipe], n_threads=2)
        one_batch(pipe)
        assert got.all_bases.dtype == np.int64 and np.array_equal(got.bin_off, off) and got.n_bins == off[-1]
        assert np.array_equal(got.all_reads, reads) and np.array_equal(got.all_bases, bases)
        assert reads.sum() > 4 * CAP_DEPTH and bases.sum() > 1_000_000


@pytest.mark.parametrize("thr,cb", COVERAGE_RULES)
@pytest.mark.parametrize("pipe", PIPELINES)
def test_window_coverage(big, pipe, thr, cb):
    """k_bam_cov_count: 32 768 waves, every one with a second item"""
    parsed = big["sorted"]["parsed"]
    want = memo(big, ("cov", thr, cb), lambda: oracle_coverage((parsed.refs, parsed.recs), big["windows"], thr, cb))
    got = bam.window_coverage(big["sorted"]["path"], big["windows"], thr, cb, device=DEVICE[pipe], n_threads=2, index=False)
    one_batch(pipe)
    assert got.dtype == np.int64 and got.tolist() == want.tolist()
    assert want[0] > 500_000 and (want[1:-2] > 0).sum() >= 30 and 0 < want[-2] <= 23_000 and want[-1] == 0


def pile_segments(big):
    tid = {c: k for k, (c, _) in enumerate(REFS)}
    return [(tid[c], a, b) for c, a, b in big["pile_regions"]]


def pile_bases(big, thr, cb):
    parsed = big["sorted"]["parsed"]
    return memo(big, ("bases", thr, cb), lambda: counted_bases((parsed.refs, [dict(r, ops=pairs(r["ops"])) for r in parsed.recs]), thr, cb))


@pytest.mark.parametrize("thr,cb", [(0, "all"), (20, "nofilter")])
@pytest.mark.parametrize("pipe", PIPELINES)
def test_pileup(big, pipe, thr, cb):
    """k_bam_pileup: 8 192 workgroups, more than four rounds; the whole table, not its sums"""
    want = restated_table(pile_bases(big, thr, cb), pile_segments(big))
    got = bam.pileup(big["sorted"]["path"], big["pile_regions"], thr, cb, device=DEVICE[pipe], n_threads=2, index=False)
    one_batch(pipe)
    assert got.regions == big["pile_regions"] and got.table.dtype == np.uint32 and got.table.shape == want.shape
    lo, hi = big["hole"]
    assert np.array_equal(got.table, want) and want.sum() > 500_000 and want[lo + 115_000 - hi:lo + 138_000 - hi].sum() > 0


@pytest.mark.parametrize("pipe", PIPELINES)
def test_index(big, pipe, tmp_path):
    """k_bam_index over 36 000 records of one batch; the twin is refused"""
    want = memo(big, "bai", lambda: restated_index(big["sorted"]["path"]))
    out = bam.build_index(big["sorted"]["path"], str(tmp_path / "sorted.bai"), device=DEVICE[pipe], n_threads=2)
    one_batch(pipe)
    with open(out, "rb") as fp:
        assert fp.read() == want
    with pytest.raises(_lib.CoralHipError, match="coordinate order"):
        bam.build_index(big["twin"]["path"], str(tmp_path / "twin.bai"), device=DEVICE[pipe], n_threads=2)
    assert os.listdir(str(tmp_path)) == ["sorted.bai"]


@pytest.mark.parametrize("pipe", PIPELINES)
def test_everything_at_once(big, pipe):
    """The ride-alongs take the parse's scratch arrays in turn (Scratch::take); at 36 000 records each of them fills those arrays
    well past one scan tile.  A records request does not go with an index request: two decodes."""
    case = big["sorted"]
    parsed, path = case["parsed"], case["path"]
    segs = np.array(pile_segments(big), dtype=np.int32).reshape(-1, 3).T.copy()
    common = dict(n_threads=2, qc=True, coverage=(segs, 0, 1), per_base=True, depth=(7, 0, 0x704, 1))
    with_index = bam._decode(path, DEVICE[pipe], index=True, **common)
    one_batch(pipe)
    with_records = bam._decode(path, DEVICE[pipe], records=False, reads=(0, None, None, 2), **common)
    one_batch(pipe)
    alone = dict(qc=bam._decode(path, DEVICE[pipe], n_threads=2, qc=True, records=False).qc,
                 pile=bam._decode(path, DEVICE[pipe], n_threads=2, coverage=(segs, 0, 1), per_base=True, records=False),
                 depth=bam._decode(path, DEVICE[pipe], n_threads=2, depth=(7, 0, 0x704, 1), records=False).depth)
    table = restated_table(pile_bases(big, 0, "all"), pile_segments(big))
    off, bases, reads = memo(big, "depth", lambda: DepthRestatement(path)).tables(7, 0, 0x704, True)
    qc = memo(big, "qc", lambda: restate_read_qc(parsed.recs))
    n_pos = np.concatenate([[0], np.cumsum([b - a for _, a, b in pile_segments(big)])])
    for name, res in (("with index", with_index), ("with records", with_records)):
        assert_qc_equals_restatement(res.qc, qc, name)
        assert_same_qc(res.qc, alone["qc"], name)
        assert np.array_equal(res.pileup, table) and np.array_equal(res.pileup, alone["pile"].pileup), name
        assert res.counts.tolist() == [int(table[a:b].sum()) for a, b in zip(n_pos, n_pos[1:])] == alone["pile"].counts.tolist(), name
        for got, want, sep in zip(res.depth, (off, bases, reads), alone["depth"]):
            assert np.array_equal(got, want) and np.array_equal(got, sep), name
    assert with_index.records.n == len(parsed.recs) and with_records.records is None and with_index.reads is None
    got = bam.index_bytes(bam.merge_index_partials([with_index.index]), parsed.lens)
    assert got == memo(big, "bai", lambda: restated_index(path))
    text, offsets = with_records.reads
    assert text.tobytes() == case["raw"][len(case["header"]):] and offsets.tolist() == [r["start"] - len(case["header"]) for r in parsed.recs] + [len(text)]
