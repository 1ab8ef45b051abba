"""Bases per position (A / C / G / T) counted during the BAM decode (bam.pileup, the `pileup` mode): both pipelines against an
INDEPENDENT restatement of the counting rule in this module.  The BAM is read with gzip + struct and the CG tag resolved by
tests/bamfile.py, the CIGAR walked in plain Python and [positions][4] built per segment.  (pysam's own count_coverage cannot be
run here: parity with it is not pinned; what is pinned is the rule.)"""
import array
import ctypes as C
import gzip
import struct

import numpy as np
import pytest

from coral_amd import _lib, bam, synth
from coral_amd import CoRAL
from tests.bamfile import D, EQ, H, I, M, N, S, X, many_ops, pairs, read_bam as _read_bam
from tests.decode_support import CORAL_ERR_ARG, CORAL_OK, DEVICE, PIPELINES, _pipeline_by_device, gpu_decode, gpu_open_only  # noqa: F401

THRESHOLDS = (0, 1, 15, 255)
CALLBACKS = ("nofilter", "all")
CB_CODE = {"nofilter": 0, "all": 1}
COLUMN = {1: 0, 2: 1, 4: 2, 8: 3}
EDGE_QUAL = bytes([0, 14, 15, 254])


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def read_bam(path):
    """(ref names, [record dicts]): the records of tests/bamfile.py with the CIGAR as (op, len) pairs."""
    parsed = _read_bam(path)
    return parsed.refs, [dict(r, ops=pairs(r["ops"])) for r in parsed.recs]


def counted_bases(parsed, threshold, read_callback):
    """tid -> (reference positions, columns) of every base the rule counts, whatever the segments: the record has SEQ (and, with
    'all', none of the flags 0x704), the base is an aligned base of an M / = / X op, its code is 1, 2, 4 or 8, and the threshold is
    0 or the record has QUAL (first byte not 0xff) with QUAL >= threshold there."""
    _, recs = parsed
    out = {}
    for r in recs:
        l_seq = len(r["codes"])
        if r["tid"] < 0 or l_seq == 0 or (read_callback == "all" and r["flag"] & 0x704):
            continue
        if threshold > 0 and r["qual"][0] == 0xFF:
            continue
        q, ref = 0, r["pos"]
        for op, ln in r["ops"]:                           # the CIGAR walk
            if op in (M, EQ, X) and ln and q < l_seq:
                n = min(ln, l_seq - q)
                codes = r["codes"][q:q + n]
                ok = (codes == 1) | (codes == 2) | (codes == 4) | (codes == 8)
                if threshold > 0:
                    ok &= r["qual"][q:q + n] >= threshold
                at = np.nonzero(ok)[0]
                if len(at):
                    out.setdefault(r["tid"], []).append((ref + at, np.array([COLUMN[c] for c in codes[at].tolist()])))
            q += ln if op in (M, I, S, EQ, X) else 0
            ref += ln if op in (M, D, N, EQ, X) else 0
    return {t: (np.concatenate([a for a, _ in v]), np.concatenate([b for _, b in v])) for t, v in out.items()}


def restated_table(bases, segments):
    """int64 [positions of the segments (tid, lo, hi), in their order][4]"""
    rows = []
    for t, lo, hi in segments:
        tab = np.zeros((hi - lo, 4), dtype=np.int64)
        if t in bases:
            pos, col = bases[t]
            inside = (pos >= lo) & (pos < hi)
            np.add.at(tab, (pos[inside] - lo, col[inside]), 1)
        rows.append(tab)
    return np.concatenate(rows) if rows else np.zeros((0, 4), dtype=np.int64)


# ---- test data -----------------------------------------------------------------------------------------------------------------
HOT_POS, HOT_LEN, HOT_DEPTH = 500_000, 200, 2000


def odd_records():
    big = [(M, 3), (I, 1), (D, 2)] * 22000 + [(M, 5)]            # 66001 ops -> CG tag
    alns = [
        dict(tid=2, pos=1000, cigar=[(M, 300)], name="c3a"),
        dict(tid=2, pos=1100, cigar=[(S, 7), (M, 150), (D, 40), (M, 100)], name="c3b"),
        dict(tid=5, pos=2000, cigar=[(M, 100)], name="noregion"),
        dict(tid=7, pos=150_000, cigar=[(S, 5), (M, 50), (D, 70), (M, 20), (I, 3), (M, 10)], name="edgeq", nonacgt=[150_001, 150_021, 150_140]),
        dict(tid=7, pos=150_010, cigar=[(H, 9), (EQ, 10), (X, 2), (N, 90), (M, 30), (H, 7)], name="b", flag=0x10),
        dict(tid=7, pos=150_020, cigar=[(M, 60)], flag=4, name="unmapped"),
        dict(tid=7, pos=150_030, cigar=[(M, 200)], has_seq=0, name="noseq"),
        dict(tid=7, pos=150_040, cigar=[(M, 120)], flag=0x100, name="secondary"),
        dict(tid=7, pos=150_050, cigar=[(M, 80), (I, 4), (M, 40)], flag=0x400, name="duplicate", nonacgt=[150_060]),
        dict(tid=7, pos=150_060, cigar=[(S, 3), (M, 90)], flag=0x200, name="qcfail"),
        dict(tid=7, pos=150_065, cigar=[(M, 100)], name="noqual"),
        dict(tid=7, pos=150_066, cigar=[(M, 100)], name="recode"),
        dict(tid=7, pos=150_070, cigar=big, name="longcigar"),
        dict(tid=7, pos=150_080, cigar=many_ops(64), name="ops64"),
        dict(tid=7, pos=150_081, cigar=many_ops(65), name="ops65"),
        dict(tid=7, pos=150_082, cigar=many_ops(129), name="ops129"),
        dict(tid=7, pos=150_090, cigar=[(M, 100)], flag=0x800, name="supplementary"),
        dict(tid=7, pos=200_000, cigar=[(M, 16383)], name="r16383"),
        dict(tid=7, pos=200_001, cigar=[(M, 16384)], name="r16384"),
        dict(tid=7, pos=200_002, cigar=[(S, 1), (M, 16384)], name="r16385"),
        dict(tid=7, pos=200_003, cigar=[(M, 16384), (I, 3), (M, 23613)], name="r40000"),      # a slice edge at an op boundary, one inside an op
    ]
    alns += [dict(tid=7, pos=HOT_POS, cigar=[(M, HOT_LEN)], name="hot%d" % k) for k in range(HOT_DEPTH)]
    alns += [dict(tid=24, pos=16000, cigar=[(M, 500)], name="mito")]
    return synth.records_from_alignments(alns)


# segments as the C ABI takes them (tid, lo, hi), sorted and disjoint: the shapes of the kernel's inner loop
SEGMENTS = [
    (2, 1050, 1120),
    (7, 0, 100),                       # no record reaches it
    (7, 150_020, 150_045),             # starts and ends inside an M op; "edgeq" starts at an odd query index, "b" ...
    (7, 150_045, 150_048),             # ... touches the one in front
    (7, 150_060, 150_130),             # begins inside the D gap of "edgeq" and the N gap of "b"
    (7, 150_130, 150_130),             # empty
    (7, 150_131, 150_200),             # "noqual" starts at an even query index here, "recode" at an odd one
    (7, 150_200, 150_500),             # touching
    (7, 200_000, 200_010),
    (7, 216_380, 216_395),             # the ends of the 16383 / 16384 / 16385-base reads, the first slice edge of the 40000-base one
    (7, 232_760, 232_775),             # its second slice edge, inside an op
    (7, 239_990, 240_010),             # its end
    (7, HOT_POS - 50, HOT_POS + HOT_LEN + 50),
    (24, 15_900, 16_600),
]
# the same ground as regions of the Python interface: unsorted, overlapping, touching, empty - merged by bam.pileup
REGIONS = [("chr8", 150_020, 150_045), ("chrM", 15_900, 16_600), ("chr8", 150_040, 150_130), ("chr8", 150_130, 150_500), ("chr8", 7, 7),
           ("chr8", 0, 100), ("chr8", 216_380, 216_395), ("chr3", 1050, 1120), ("chr8", 232_760, 232_775),
           ("chr8", HOT_POS - 50, HOT_POS + HOT_LEN + 50), ("chr8", 200_000, 200_010), ("chr8", 239_990, 240_010)]
MERGED = [("chr3", 1050, 1120), ("chr8", 0, 100), ("chr8", 150_020, 150_500), ("chr8", 200_000, 200_010), ("chr8", 216_380, 216_395),
          ("chr8", 232_760, 232_775), ("chr8", 239_990, 240_010), ("chr8", HOT_POS - 50, HOT_POS + HOT_LEN + 50), ("chrM", 15_900, 16_600)]


def rewrite_codes(raw, name, changes):
    """The uncompressed BAM stream with SEQ nibbles of the record called `name` set: changes = {query index: code}."""
    raw = bytearray(raw)
    o = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, o)[0]
    o += 4
    for _ in range(n_ref):
        o += 8 + struct.unpack_from("<i", raw, o)[0]
    while o < len(raw):
        bs, l_name, n_cig = struct.unpack_from("<i", raw, o)[0], raw[o + 12], struct.unpack_from("<H", raw, o + 16)[0]
        if bytes(raw[o + 36:o + 36 + l_name - 1]) == name.encode():
            seq = o + 36 + l_name + 4 * n_cig
            for qi, code in changes.items():
                b = raw[seq + qi // 2]
                raw[seq + qi // 2] = (b & 0xF0) | code if qi & 1 else (b & 0x0F) | (code << 4)
            return bytes(raw)
        o += 4 + bs
    raise AssertionError("no record called " + name)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("pileup")
    rec = synth.merge_sorted(synth.generate(synth.scaled_config("tiny", 300), "cpu"), odd_records())
    names = rec.materialise_names()
    name_of = lambda i: names[int(rec.name_id[i])]
    qlen = rec.qlen.numpy()

    def qual(i):
        nm, n = name_of(i), int(qlen[i])
        if nm in ("edgeq", "r16384"):
            return (EDGE_QUAL * (n // 4 + 1))[:n]
        if nm == "recode":                                   # 255 behind the first byte is a quality, not "no QUAL"
            return (EDGE_QUAL * 20)[:80] + b"\xff" + (EDGE_QUAL * 5)[:n - 81]
        if nm.startswith("hot"):
            return ((np.arange(n) * 3 + i) % 31).astype(np.uint8).tobytes()
        return None
    plain = str(d / "plain.bam")
    bam.write_bam(rec, plain, seed=9, fast_seq=True, qual=qual, with_qual=lambda i: name_of(i) != "noqual" and i % 3 != 1)
    raw = gzip.open(plain, "rb").read()
    raw = rewrite_codes(raw, "recode", {64: 3, 65: 15, 66: 3, 67: 15, 70: 0, 71: 5})       # (what write_bam cannot express)
    path, small = str(d / "mixed.bam"), str(d / "mixed_small_blocks.bam")
    for name, kw in ((path, {}), (small, dict(block_size=1500, empty_block_every=5))):
        with open(name, "wb") as fp:
            for blk in bam._bgzf_blocks(raw, **kw):
                fp.write(blk)
    parsed = read_bam(path)
    assert len(parsed[1]) == rec.n
    bases = {(thr, cb): counted_bases(parsed, thr, cb) for thr in THRESHOLDS for cb in CALLBACKS}
    return dict(rec=rec, path=path, small=small, parsed=parsed, bases=bases, dir=d)


def segment_array(segments=SEGMENTS):
    return np.array(segments, dtype=np.int32).reshape(-1, 3).T.copy()


def merged_as_tids(case):
    refs = case["parsed"][0]
    return [(refs.index(c), a, b) for c, a, b in MERGED]


# ---- the restatement itself sees what was planted ------------------------------------------------------------------------------
def test_restatement_reads_the_planted_records(case):
    refs, recs = case["parsed"]
    by_name = {r["name"]: r for r in recs}
    assert [len(by_name[k]["codes"]) for k in ("r16383", "r16384", "r16385", "r40000")] == [16383, 16384, 16385, 40000]
    assert [len(by_name[k]["ops"]) for k in ("ops64", "ops65", "ops129", "longcigar")] == [64, 65, 129, 66001]
    assert {op for op, _ in by_name["ops129"]["ops"]} == set(range(9)) and any(ln == 0 for _, ln in by_name["ops129"]["ops"])
    assert by_name["recode"]["codes"][64:68].tolist() == [3, 15, 3, 15] and by_name["recode"]["codes"][70:72].tolist() == [0, 5]
    assert (by_name["edgeq"]["codes"] == 15).sum() == 3 and by_name["noqual"]["qual"][0] == 0xFF and len(by_name["noseq"]["codes"]) == 0
    assert set(by_name["edgeq"]["qual"].tolist()) == {0, 14, 15, 254}
    assert {by_name[k]["flag"] for k in ("unmapped", "secondary", "qcfail", "duplicate", "supplementary")} == {0x4, 0x100, 0x200, 0x400, 0x800}
    assert sum(r["name"].startswith("hot") for r in recs) == HOT_DEPTH
    assert refs[2] == "chr3" and refs[5] == "chr6" and refs[7] == "chr8" and refs[24] == "chrM"
    base = restated_table(case["bases"][(0, "nofilter")], SEGMENTS)
    assert base.shape == (sum(hi - lo for _, lo, hi in SEGMENTS), 4) and (base.sum(axis=0) > 0).all()
    hot = restated_table(case["bases"][(0, "nofilter")], [(7, HOT_POS, HOT_POS + HOT_LEN)])
    assert (hot.sum(axis=1) >= HOT_DEPTH).all() and (hot > 300).all()          # differing SEQ seeds: every base at every position
    # every threshold and the callback bite on this file
    sums = [restated_table(case["bases"][(thr, "nofilter")], SEGMENTS).sum() for thr in THRESHOLDS]
    assert sums[0] > sums[1] > sums[2] > sums[3] > 0
    assert restated_table(case["bases"][(0, "all")], SEGMENTS).sum() < sums[0]


# ---- the table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cb", CALLBACKS)
@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("pipe", PIPELINES)
def test_table_equals_restatement(case, pipe, thr, cb):
    """The segments of the C ABI as they are (touching, empty, inside a gap, both nibbles), and the regions of bam.pileup."""
    bases = case["bases"][(thr, cb)]
    got = bam._decode(case["path"], DEVICE[pipe], n_threads=3, coverage=(segment_array(), thr, CB_CODE[cb]), per_base=True, records=False)
    want = restated_table(bases, SEGMENTS)
    assert got.pileup.dtype == np.uint32 and got.pileup.shape == want.shape
    assert np.array_equal(got.pileup, want)
    # coral_bam_coverage_result under per_base: the table's sums per segment
    off = np.concatenate([[0], np.cumsum([hi - lo for _, lo, hi in SEGMENTS])])
    assert got.counts.dtype == np.int64 and got.counts.tolist() == [int(want[a:b].sum()) for a, b in zip(off, off[1:])]
    p = bam.pileup(case["path"], REGIONS, thr, cb, device=DEVICE[pipe], index=False)
    assert p.regions == MERGED and np.array_equal(p.table, restated_table(bases, merged_as_tids(case)))
    assert p.quality_threshold == thr and p.read_callback == cb


@pytest.mark.parametrize("cb", CALLBACKS)
@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("pipe", PIPELINES)
def test_counts_equal_restatement_sums(case, pipe, thr, cb):
    """The counting request on its own (no table): one walk serves both results, so the counters face the same shapes as the table."""
    got = bam._decode(case["path"], DEVICE[pipe], coverage=(segment_array(), thr, CB_CODE[cb]), records=False)
    want = restated_table(case["bases"][(thr, cb)], SEGMENTS)
    off = np.concatenate([[0], np.cumsum([hi - lo for _, lo, hi in SEGMENTS])])
    assert got.pileup is None and got.counts.dtype == np.int64
    # (no case is empty: test_restatement_reads_the_planted_records asserts counted bases at every threshold, 255 included)
    assert got.counts.tolist() == [int(want[a:b].sum()) for a, b in zip(off, off[1:])] and want.sum() > 0


@pytest.mark.parametrize("pipe", PIPELINES)
def test_depth_equals_window_coverage(case, pipe):
    windows = [("chr8", 150_020, 150_045), ("chr8", 150_100, 150_101), ("chr8", 150_021, 150_400), ("chr8", HOT_POS + 3, HOT_POS + 150),
               ("chr8", 216_381, 216_394), ("chrM", 16_000, 16_001), ("chr3", 1050, 1120), ("chr8", 10, 90), ("chr8", 150_300, 150_300)]
    for thr, cb in ((0, "nofilter"), (15, "all")):
        p = bam.pileup(case["path"], REGIONS, thr, cb, device=DEVICE[pipe], index=False)
        cov = bam.window_coverage(case["path"], windows, thr, cb, device=DEVICE[pipe], index=False)
        assert cov.sum() > HOT_DEPTH and [int(p.depth(*w).sum()) for w in windows] == cov.tolist()
        c = p.counts(*windows[0])
        assert c.dtype == np.int64 and c.shape == (4, 25) and np.array_equal(c.sum(axis=0), p.depth(*windows[0]))


@pytest.mark.parametrize("pipe", PIPELINES)
def test_byte_ranges_add_up(case, pipe):
    whole = bam.pileup(case["small"], REGIONS, 15, "all", device=DEVICE[pipe], index=False)
    assert np.array_equal(whole.table, restated_table(case["bases"][(15, "all")], merged_as_tids(case)))
    parts = [bam.pileup(case["small"], REGIONS, 15, "all", device=DEVICE[pipe], rank=r, world=3, batch_bytes=1 << 17, index=False) for r in range(3)]
    assert sum(int(p.table.sum()) > 0 for p in parts) >= 2
    merged = bam.merge_pileups(parts)
    assert merged.regions == whole.regions and np.array_equal(merged.table, whole.table)
    other = bam.pileup(case["small"], REGIONS[:3], 15, "all", device="cpu", index=False)
    with pytest.raises(ValueError):
        bam.merge_pileups([parts[0], other])


@pytest.mark.parametrize("pipe", PIPELINES)
def test_index_restricts_the_decode(case, pipe):
    regions = [("chrM", 15_900, 16_600), ("chr8", HOT_POS - 50, HOT_POS + 20), ("chr3", 1050, 1120)]
    whole = bam.pileup(case["small"], regions, 1, "nofilter", device=DEVICE[pipe], index=False)
    all_blocks = bam.LAST_DECODE["blocks"]
    assert bam.LAST_DECODE["index"] is None
    index = bam.build_index(case["small"], str(case["dir"] / ("%s.bai" % pipe)), device=DEVICE[pipe])
    for how in (index, bam.read_index(index)):
        got = bam.pileup(case["small"], regions, 1, "nofilter", device=DEVICE[pipe], index=how)
        assert np.array_equal(got.table, whole.table) and whole.table.sum() > 0
        assert 0 < bam.LAST_DECODE["blocks"] < all_blocks and bam.LAST_DECODE["index"] is not None and bam.LAST_DECODE["spans"] >= 2
    with pytest.raises(ValueError):
        bam.pileup(case["small"], regions, 1, "nofilter", device=DEVICE[pipe], index=index, world=2)
    with pytest.raises(_lib.CoralHipError):
        bam.pileup(case["small"], regions, device=DEVICE[pipe], index=str(case["dir"] / "missing.bai"))


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1 << 16, 40000])
def test_gpu_equals_host_over_several_batches(case, batch):
    """Small batches: records straddle them (the 66 001-op record alone is ~380 kB, the 40 000-base read 60 kB)."""
    segs = segment_array()
    host = bam._decode(case["small"], "cpu", coverage=(segs, 15, 0), per_base=True, records=False)
    got = bam._decode(case["small"], "cuda:0", batch_bytes=batch, coverage=(segs, 15, 0), per_base=True, records=False)
    assert bam.LAST_DECODE["where"] == "gpu" and bam.LAST_DECODE["batches"] >= 3
    assert np.array_equal(got.pileup, host.pileup) and np.array_equal(got.counts, host.counts)
    assert np.array_equal(got.pileup, restated_table(case["bases"][(15, "nofilter")], SEGMENTS))


@pytest.mark.parametrize("pipe", PIPELINES)
def test_every_request_in_one_decode(case, pipe):
    segs = segment_array()
    decode = lambda **kw: bam._decode(case["path"], DEVICE[pipe], n_threads=2, **kw)
    alone = decode(coverage=(segs, 15, 1), per_base=True, records=False)
    alone_cov = decode(coverage=(segs, 15, 1), records=False).counts
    alone_idx, alone_qc = decode(index=True, records=False).index, decode(qc=True, records=False).qc
    got = decode(coverage=(segs, 15, 1), per_base=True, index=True, qc=True)
    assert alone.pileup.sum() > 0 and np.array_equal(got.pileup, alone.pileup)
    assert np.array_equal(got.counts, alone.counts) and np.array_equal(got.counts, alone_cov)      # one result, not two rules
    assert set(got.index) == set(alone_idx) and all(np.array_equal(got.index[k], v) for k, v in alone_idx.items())
    for k in ("length", "qual_sum", "mapq", "flag", "base_quality_hist"):
        assert np.array_equal(getattr(got.qc, k), getattr(alone_qc, k)), k
    assert got.qc.counters == alone_qc.counters and got.records.n == case["rec"].n
    assert alone.records is None and alone.index is None and alone.qc is None and decode(records=False).pileup is None


@pytest.mark.gpu
def test_gpu_workspace_grows_by_the_table(case):
    segs = segment_array()
    n_seg, n_pos = segs.shape[1], int((segs[2].astype(np.int64) - segs[1]).sum())
    up256 = lambda n: (n + 255) & ~255
    bam.decode_bam_gpu(case["path"], "cuda:0")
    plain = bam.LAST_DECODE["workspace_bytes"]
    bam._decode(case["path"], "cuda:0", coverage=(segs, 15, 0), records=False)
    coverage = bam.LAST_DECODE["workspace_bytes"]
    assert coverage == plain + up256(3 * n_seg * 4) + up256(n_seg * 8)
    bam._decode(case["path"], "cuda:0", coverage=(segs, 15, 0), per_base=True, records=False)
    assert bam.LAST_DECODE["workspace_bytes"] == coverage + up256((n_seg + 1) * 8) + up256(n_pos * 4 * 4)
    bam._decode(case["path"], "cuda:0", index=True, qc=True, records=False)          # unchanged without the request
    other = bam.LAST_DECODE["workspace_bytes"]
    bam.decode_bam_gpu(case["path"], "cuda:0")
    assert bam.LAST_DECODE["workspace_bytes"] == plain < other


# ---- argument rules, equal on both pipelines -----------------------------------------------------------------------------------
def bad_requests():
    """name -> (arguments of _lib.bam_request, a word of the message)"""
    return {
        "per_base without segments": (dict(per_base=True), "per_base needs segments"),
        "per_base on spans without segments": (dict(per_base=True, spans=[[0, 1 << 16]]), "per_base needs segments"),
        "more than 2^28 positions": (dict(per_base=True, coverage=(segment_array([(0, 0, 1 << 27), (0, 1 << 27, 1 << 28), (1, 5, 6)]), 0, 0)), "2^28 positions"),
    }


def test_host_refuses_bad_requests(case):
    L = _lib.lib()
    for name, (kw, word) in bad_requests().items():
        req, h = _lib.bam_request(**kw), C.c_void_p()
        assert L.coral_bam_decode_request(case["path"].encode(), 1, C.byref(req), C.byref(h)) == CORAL_ERR_ARG and h.value is None, name
        assert word in L.coral_bam_last_error().decode(), name
    # exactly 2^28 positions are a legal request (not decoded here: the table would be 4 GiB), a wrong n_pos is refused
    segs = segment_array()
    n_pos = int((segs[2].astype(np.int64) - segs[1]).sum())
    req, h = _lib.bam_request(coverage=(segs, 0, 0), per_base=True), C.c_void_p()
    assert L.coral_bam_decode_request(case["path"].encode(), 2, C.byref(req), C.byref(h)) == CORAL_OK
    try:
        table = np.zeros((n_pos + 1, 4), dtype=np.uint32)
        for wrong in (n_pos - 1, n_pos + 1, 0, -1):
            assert L.coral_bam_pileup_result(h, wrong, table.ctypes.data) == CORAL_ERR_ARG
            assert "pileup request of this size" in L.coral_bam_last_error().decode() or wrong < 0
        assert L.coral_bam_pileup_result(h, n_pos, table.ctypes.data) == CORAL_OK and table[:n_pos].sum() > 0 and table[n_pos].sum() == 0
    finally:
        L.coral_bam_decode_close(h)
    req, h = _lib.bam_request(coverage=(segs, 0, 0)), C.c_void_p()                 # a handle without the request holds no table
    assert L.coral_bam_decode_request(case["path"].encode(), 2, C.byref(req), C.byref(h)) == CORAL_OK
    try:
        assert L.coral_bam_pileup_result(h, n_pos, table.ctypes.data) == CORAL_ERR_ARG
    finally:
        L.coral_bam_decode_close(h)


@pytest.mark.gpu
def test_gpu_refuses_the_same_requests(case):
    L = _lib.lib()
    for name, (kw, word) in bad_requests().items():
        rc, h, ws_bytes, message = gpu_open_only(case["path"], **kw)
        assert rc == CORAL_ERR_ARG and h is None and ws_bytes == 0, name
        assert word in message, name
    # a wrong n_pos, on the handle of a GPU decode
    segs = segment_array()
    n_pos = int((segs[2].astype(np.int64) - segs[1]).sum())
    with gpu_decode(case["path"], coverage=(segs, 0, 0), per_base=True) as d:
        table = np.zeros((n_pos + 1, 4), dtype=np.uint32)
        for wrong in (n_pos - 1, n_pos + 1, 0):
            assert L.coral_bam_pileup_result(d.dh, wrong, table.ctypes.data) == CORAL_ERR_ARG
        assert L.coral_bam_pileup_result(d.dh, n_pos, table.ctypes.data) == CORAL_OK
        assert np.array_equal(table[:n_pos], restated_table(case["bases"][(0, "nofilter")], SEGMENTS))


@pytest.mark.parametrize("regions,thr,cb", [
    ([("chrNope", 0, 10)], 0, "nofilter"),
    ([("chr8", -1, 10)], 0, "nofilter"),
    ([("chr8", 10, 9)], 0, "nofilter"),
    ([("chr8", 0, 10, 11)], 0, "nofilter"),
    ([("chr8", 0, 10)], 20.5, "nofilter"),
    ([("chr8", 0, 10)], 256, "nofilter"),
    ([("chr8", 0, 10)], 0, "none"),
    ([("chr1", 0, 1 << 28), ("chr2", 0, 1)], 0, "nofilter"),
])
def test_bad_arguments_raise_value_error(case, regions, thr, cb):
    with pytest.raises(ValueError):
        bam.pileup(case["path"], regions, thr, cb, device="cpu")


# ---- the stand-in for lr_bamfh -------------------------------------------------------------------------------------------------
def test_count_coverage_has_pysams_shape(case):
    p = bam.pileup(case["path"], REGIONS, 15, "all", device="cpu")
    want = restated_table(case["bases"][(15, "all")], [(7, 150_030, 150_210)])
    got = p.count_coverage("chr8", 150_030, 150_210)                       # pysam's defaults: threshold 15, callback 'all'
    assert isinstance(got, tuple) and len(got) == 4
    assert all(isinstance(a, array.array) and a.typecode == "L" and len(a) == 180 for a in got)
    assert [a.tolist() for a in got] == want.T.tolist() and want.sum() > 0
    assert [a.tolist() for a in p.count_coverage(None, region="chr8:150031-150210")] == want.T.tolist()      # 1-based, inclusive
    assert [len(a) for a in p.count_coverage("chr8", 150_100, 150_100)] == [0, 0, 0, 0]
    for outside in (("chr8", 150_019, 150_030), ("chr8", 150_400, 150_501), ("chr8", 100, 150_030), ("chr6", 2000, 2010), ("chr8", 150_040, 150_030)):
        with pytest.raises(KeyError):
            p.count_coverage(*outside)
        with pytest.raises(KeyError):
            p.counts(*outside)
    with pytest.raises(ValueError):
        p.count_coverage("chr8", 150_030, 150_210, quality_threshold=14)
    with pytest.raises(ValueError):
        p.count_coverage("chr8", 150_030, 150_210, read_callback="nofilter")
    one_shot = bam.count_coverage(case["path"], "chr8", 150_030, 150_210, device="cpu")
    assert [a.tolist() for a in one_shot] == want.T.tolist() and one_shot[0].typecode == "L"
    p.close()
    with pytest.raises(KeyError):
        p.count_coverage("chr8", 150_030, 150_210)


# ---- the command line ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", PIPELINES)
def test_cli_writes_the_restated_table(case, pipe, tmp_path):
    table = restated_table(case["bases"][(15, "all")], merged_as_tids(case))
    lines, at = ["chrom\tpos\tA\tC\tG\tT\n"], 0
    for chrom, a, b in MERGED:
        for x in range(a, b):
            if table[at].sum() > 0:
                lines.append("%s\t%d\t%d\t%d\t%d\t%d\n" % ((chrom, x) + tuple(table[at].tolist())))
            at += 1
    assert len(lines) > 500
    out = str(tmp_path / "regions.tsv")
    argv = ["pileup", "--lr_bam", case["path"], "--min_base_quality", "15", "--read_callback", "all", "--device", DEVICE[pipe]]
    CoRAL.main(argv + ["--output", out] + [a for c, s, e in REGIONS for a in ("--region", "%s:%d-%d" % (c, s, e))])
    assert open(out).readlines() == lines
    bed = str(tmp_path / "regions.bed")
    with open(bed, "w") as fp:
        fp.write("".join("%s\t%d\t%d\tname\n" % r for r in REGIONS))
    out = str(tmp_path / "bed.tsv")
    CoRAL.main(argv + ["--output", out, "--bed", bed])
    assert open(out).readlines() == lines
