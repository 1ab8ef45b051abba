"""Window coverage with a base-quality threshold, counted during the BAM decode (bam.window_coverage, the coverage track of
`plot` at any --min_mapq): both pipelines against an INDEPENDENT restatement of pysam count_coverage in this module (the BAM
is read with gzip + struct, CIGAR / SEQ / QUAL walked per record), and against the plot goldens at threshold 0."""
import gzip
import json
import os
import struct

import numpy as np
import pytest

from coral_amd import bam, plot_coverage, synth

M, I, D, N, S, H, P, EQ, X = range(9)
THRESHOLDS = (0, 1, 7, 20, 30, 61, 255)
CALLBACKS = ("nofilter", "all")


# ---- the oracle: pysam AlignmentFile.count_coverage, summed over the four bases -------------------------------------------
def read_bam(path):
    """[(ref names), [record dicts]] straight from the bytes: tid, pos, flag, ops (the CG:B,I CIGAR for the placeholder),
    SEQ codes, QUAL."""
    raw = gzip.open(path, "rb").read()
    assert raw[:4] == b"BAM\x01"
    o = 8 + struct.unpack_from("<i", raw, 4)[0]
    refs = []
    n_ref = struct.unpack_from("<i", raw, o)[0]
    o += 4
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", raw, o)[0]
        refs.append(raw[o + 4:o + 4 + ln - 1].decode())
        o += 8 + ln
    recs = []
    while o < len(raw):
        bs, tid, pos, l_name, _mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", raw, o)
        p = o + 36 + l_name
        ops = np.frombuffer(raw, dtype="<u4", count=n_cig, offset=p).copy()
        p += 4 * n_cig
        packed = np.frombuffer(raw, dtype=np.uint8, count=(l_seq + 1) // 2, offset=p)
        codes = np.empty(2 * len(packed), dtype=np.uint8)
        codes[0::2], codes[1::2] = packed >> 4, packed & 15
        p += (l_seq + 1) // 2
        qual = np.frombuffer(raw, dtype=np.uint8, count=l_seq, offset=p)
        p += l_seq
        end = o + 4 + bs
        while p < end:                                    # tags: only CG:B,I matters here
            key, ty = raw[p:p + 2], chr(raw[p + 2])
            p += 3
            if ty in "AcC":
                p += 1
            elif ty in "sS":
                p += 2
            elif ty in "iIf":
                p += 4
            elif ty in "ZH":
                p = raw.index(b"\0", p) + 1
            else:
                sub, cnt = chr(raw[p]), struct.unpack_from("<I", raw, p + 1)[0]
                size = {"c": 1, "C": 1, "s": 2, "S": 2}.get(sub, 4)
                if key == b"CG" and sub == "I" and len(ops) == 2 and ops[0] & 15 == S and ops[0] >> 4 == l_seq and ops[1] & 15 == N:
                    ops = np.frombuffer(raw, dtype="<u4", count=cnt, offset=p + 5).copy()
                p += 5 + size * cnt
        recs.append(dict(tid=tid, pos=pos, flag=flag, ops=ops, codes=codes[:l_seq], qual=qual))
        o = end
    return refs, recs


def oracle_coverage(parsed, windows, threshold, read_callback):
    """For every window: #(read, qpos, refpos) with the read on the contig (and, with 'all', none of the flags 0x704), SEQ
    present, (qpos, refpos) an aligned pair of an M / = / X op inside the window, SEQ code A/C/G/T, and threshold 0 or QUAL
    present (first byte not 0xff) and QUAL[qpos] >= threshold."""
    refs, recs = parsed
    hits = {}
    for r in recs:
        if r["tid"] < 0 or len(r["codes"]) == 0 or (read_callback == "all" and r["flag"] & 0x704):
            continue
        if threshold > 0 and r["qual"][0] == 0xFF:
            continue
        q, ref, qs, rs = 0, r["pos"], [], []
        for w in r["ops"]:
            op, ln = int(w & 15), int(w >> 4)
            if op in (M, EQ, X):
                qs.append(np.arange(q, q + ln))
                rs.append(np.arange(ref, ref + ln))
            q += ln if op in (M, I, S, EQ, X) else 0
            ref += ln if op in (M, D, N, EQ, X) else 0
        if not qs:
            continue
        qp, rp = np.concatenate(qs), np.concatenate(rs)
        keep = qp < len(r["codes"])
        qp, rp = qp[keep], rp[keep]
        c = r["codes"][qp]
        ok = (c == 1) | (c == 2) | (c == 4) | (c == 8)
        if threshold > 0:
            ok &= r["qual"][qp] >= threshold
        hits.setdefault(r["tid"], []).append(rp[ok])
    hits = {t: np.sort(np.concatenate(v)) for t, v in hits.items()}
    out = []
    for chrom, a, b in windows:
        h = hits.get(refs.index(chrom), np.zeros(0, dtype=np.int64))
        out.append(int(np.searchsorted(h, b) - np.searchsorted(h, a)))
    return np.array(out, dtype=np.int64)


# ---- test data ---------------------------------------------------------------------------------------------------------------
def odd_records():
    """Hand-written records: the flags the 'all' callback drops, no SEQ, N bases, an unmapped read with a CIGAR, a CIGAR of
    more than 65 535 ops (CG tag), soft / hard clips, =, X, D, N."""
    big = [(M, 3), (I, 1), (D, 2)] * 22000 + [(M, 5)]            # 66001 ops -> CG tag
    return synth.records_from_alignments([
        dict(tid=7, pos=150_000, cigar=[(S, 5), (M, 50), (D, 70), (M, 20), (I, 3), (M, 10)], name="a", nonacgt=[150_001, 150_140]),
        dict(tid=7, pos=150_010, cigar=[(H, 9), (EQ, 10), (X, 2), (N, 90), (M, 30), (H, 7)], name="b", flag=0x10),
        dict(tid=7, pos=150_020, cigar=[(M, 60)], flag=4, name="c"),
        dict(tid=7, pos=150_030, cigar=[(M, 200)], has_seq=0, flag=256, name="a"),
        dict(tid=7, pos=150_040, cigar=[(M, 120)], flag=256, name="d"),
        dict(tid=7, pos=150_050, cigar=[(M, 80), (I, 4), (M, 40)], flag=0x400, name="e", nonacgt=[150_060]),
        dict(tid=7, pos=150_060, cigar=[(S, 3), (M, 90)], flag=0x200, name="f"),
        dict(tid=7, pos=150_070, cigar=big, name="long"),
        dict(tid=7, pos=400_000, cigar=[(M, 500)], flag=0x800, name="g"),
        dict(tid=24, pos=16000, cigar=[(M, 500)], name="mito"),
    ])


def make_records(n=700):
    return synth.merge_sorted(synth.generate(synth.scaled_config("tiny", n), "cpu"), odd_records())


def make_windows(rec, seed=3):
    """Random windows where the reads are (overlapping ones included), the plot's own window shape, windows at both ends of
    chr8 and chrM, a window on a contig without reads, empty windows."""
    rng = np.random.default_rng(seed)
    tid, pos, end = (getattr(rec, k).numpy() for k in ("tid", "pos", "end"))
    chroms, lens = rec.header_chroms, rec.header_lens
    out = []
    for k in rng.choice(rec.n, 60):
        a = int(pos[k]) + int(rng.integers(-300, 300))
        out.append((chroms[tid[k]], max(a, 0), max(a, 0) + int(rng.choice([1, 37, 150, 1000, 25_000]))))
    out += [("chr8", 150_000 + 150 * k, 150_000 + 150 * (k + 1)) for k in range(8)]
    out += [("chr8", 150_000, 151_000), ("chr8", 150_100, 150_250), ("chr8", 150_100, 150_250)]     # overlapping, repeated
    out += [("chr8", 0, 1000), ("chr8", lens[7] - 1000, lens[7]), ("chrM", 0, 10), ("chrM", lens[24] - 5, lens[24])]
    out += [("chr3", 1000, 500_000), ("chr8", 150_090, 150_090), ("chrM", 16_100, 16_100)]
    assert chroms[7] == "chr8" and chroms[24] == "chrM"
    return out


def with_qual(i):
    return i % 3 != 1                 # QUAL on two records in three, absent (0xff) on the rest


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("wcov")
    rec = make_records()
    path = str(d / "mixed.bam")
    bam.write_bam(rec, path, seed=9, with_qual=with_qual)
    small = str(d / "mixed_small_blocks.bam")
    bam.write_bam(rec, small, seed=9, with_qual=with_qual, block_size=1500, empty_block_every=5)
    parsed = read_bam(path)
    assert len(parsed[1]) == rec.n
    return dict(rec=rec, path=path, small=small, parsed=parsed, windows=make_windows(rec))


def host(path, windows, thr, cb, **kw):
    old = os.environ.get("CORAL_BAM_DECODE")
    os.environ["CORAL_BAM_DECODE"] = "cpu"
    try:
        return bam.window_coverage(path, windows, thr, cb, device="cpu", **kw)
    finally:
        if old is None:
            del os.environ["CORAL_BAM_DECODE"]
        else:
            os.environ["CORAL_BAM_DECODE"] = old


# ---- the oracle itself sees what was planted -----------------------------------------------------------------------------------
def test_oracle_reads_the_planted_records(case):
    refs, recs = case["parsed"]
    long_ = [r for r in recs if len(r["ops"]) > 65535]
    assert len(long_) == 1 and len(long_[0]["ops"]) == 66001
    assert sum(r["qual"][0] == 0xFF for r in recs if len(r["qual"])) > 100
    assert sum(r["qual"][0] != 0xFF for r in recs if len(r["qual"])) > 200
    assert {0x4, 0x100, 0x200, 0x400} <= {r["flag"] & f for r in recs for f in (0x4, 0x100, 0x200, 0x400)}
    assert any(((r["codes"] == 15).any()) for r in recs)
    w = case["windows"]
    base = oracle_coverage(case["parsed"], w, 0, "nofilter")
    assert (base > 0).sum() > 40
    # the threshold and the callback both bite on this file
    assert (oracle_coverage(case["parsed"], w, 20, "nofilter") < base).sum() > 20
    assert (oracle_coverage(case["parsed"], w, 0, "all") < base).sum() > 3
    assert oracle_coverage(case["parsed"], w, 61, "nofilter").sum() == 0       # QUAL is 0..60 on this file


# ---- host pipeline -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cb", CALLBACKS)
@pytest.mark.parametrize("thr", THRESHOLDS)
def test_host_pipeline_matches_oracle(case, thr, cb):
    got = host(case["path"], case["windows"], thr, cb, n_threads=3)
    assert got.dtype == np.int64 and len(got) == len(case["windows"])
    assert np.array_equal(got, oracle_coverage(case["parsed"], case["windows"], thr, cb))


@pytest.mark.parametrize("thr,cb", [(0, "nofilter"), (20, "all"), (7, "nofilter")])
def test_host_pipeline_records_straddle_blocks_and_ranges(case, thr, cb):
    want = oracle_coverage(case["parsed"], case["windows"], thr, cb)
    assert np.array_equal(host(case["small"], case["windows"], thr, cb, n_threads=2), want)
    for world in (2, 3):
        parts = [host(case["small"], case["windows"], thr, cb, n_threads=2, rank=r, world=world) for r in range(world)]
        assert all(p.sum() < want.sum() for p in parts if want.sum())
        assert np.array_equal(np.sum(parts, axis=0), want), world


def test_float_threshold_and_empty_request(case):
    w = case["windows"]
    assert np.array_equal(host(case["path"], w, 20.0, "nofilter"), host(case["path"], w, 20, "nofilter"))
    assert np.array_equal(host(case["path"], w, np.int64(7), "all"), oracle_coverage(case["parsed"], w, 7, "all"))
    empty = host(case["path"], [], 20, "all")
    assert empty.dtype == np.int64 and empty.shape == (0,)


@pytest.mark.parametrize("windows,thr,cb", [
    ([("chrNope", 0, 10)], 0, "nofilter"),
    ([("chr8", -1, 10)], 0, "nofilter"),
    ([("chr8", 10, 9)], 0, "nofilter"),
    ([("chr8", 0, 10)], 20.5, "nofilter"),
    ([("chr8", 0, 10)], -1, "nofilter"),
    ([("chr8", 0, 10)], 256, "nofilter"),
    ([("chr8", 0, 10)], "20", "nofilter"),
    ([("chr8", 0, 10)], 0, "none"),
])
def test_bad_requests_raise_value_error(case, windows, thr, cb):
    with pytest.raises(ValueError):
        host(case["path"], windows, thr, cb)


def test_segments_cover_exactly_the_windows():
    refs = ["c0", "c1"]
    w = [("c1", 5, 20), ("c0", 0, 10), ("c1", 10, 30), ("c1", 40, 40), ("c1", 50, 60)]
    segs, first, last = bam.coverage_segments(w, refs)
    assert segs.T.tolist() == [[0, 0, 10], [1, 5, 10], [1, 10, 20], [1, 20, 30], [1, 50, 60]]
    assert [list(range(a, b)) for a, b in zip(first, last)] == [[1, 2], [0], [2, 3], [], [4]]


# ---- the plot's coverage track -------------------------------------------------------------------------------------------------
def _plot_case(golden_dir, name, tmp_path):
    with open(os.path.join(golden_dir, "plotcov_%s.json" % name)) as fp:
        gold = json.load(fp)
    _, rec = synth.dataset(gold["config"], "cpu")
    with open(os.path.join(golden_dir, "e2e_%s.json" % gold["config"])) as fp:
        text = json.load(fp)["files"][gold["graph_file"]]
    graph = str(tmp_path / "g_graph.txt")
    with open(graph, "w") as fp:
        fp.write(text)
    want = [(c, a + k * w, a + k * w + w, tot) for c, a, w, totals in gold["tracks"] for k, tot in enumerate(totals)]
    return gold, rec, graph, want


@pytest.mark.parametrize("name", ["tiny", "tiny_region", "tiny_edge_region", "ultra"])
def test_coverage_track_bam_equals_plot_goldens(name, golden_dir, tmp_path, monkeypatch):
    monkeypatch.setenv("CORAL_BAM_DECODE", "cpu")
    gold, rec, graph, want = _plot_case(golden_dir, name, tmp_path)
    path = str(tmp_path / "r.bam")
    bam.write_bam_native(rec, path, seed=4, n_threads=4)
    bounds = plot_coverage.parse_region(gold["region"])
    got = plot_coverage.coverage_track_bam(path, plot_coverage.parse_graph_intervals(graph), bounds, device="cpu")
    assert got == want


def test_coverage_table_answers_the_plot_windows(golden_dir, tmp_path, monkeypatch):
    monkeypatch.setenv("CORAL_BAM_DECODE", "cpu")
    gold, rec, graph, want = _plot_case(golden_dir, "tiny_region", tmp_path)
    path = str(tmp_path / "q.bam")
    bam.write_bam(rec, path, seed=2, with_qual=with_qual, fast_seq=True)
    table = plot_coverage.CoverageTable.from_bam(path, graph, gold["region"], min_mapq=20.0, device="cpu")
    windows = [(c, a, b) for c, a, b, _ in want]
    assert len(table) == len(set(windows))
    exp = oracle_coverage(read_bam(path), windows, 20, "nofilter")
    got = []
    for c, a, b in windows:                  # the reference's call (plot:399-400), summed as it sums them
        arrs = table.count_coverage(c, a, b, quality_threshold=20.0, read_callback="nofilter")
        assert arrs[1:] == ([0], [0], [0])
        got.append(sum(sum(nc) for nc in arrs))
    assert got == exp.tolist() and 0 < sum(got) < sum(t for *_, t in want)
    with pytest.raises(KeyError):
        table.count_coverage(windows[0][0], windows[0][1] + 1, windows[0][2] + 1, quality_threshold=20, read_callback="nofilter")
    with pytest.raises(KeyError):
        table.count_coverage(*windows[0], quality_threshold=15, read_callback="nofilter")
    with pytest.raises(KeyError):
        table.count_coverage(*windows[0], quality_threshold=20)          # pysam's default callback is 'all'
    table.close()
    with pytest.raises(KeyError):
        table.count_coverage(*windows[0], quality_threshold=20, read_callback="nofilter")


# ---- GPU pipeline --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_pipeline_matches_host_and_oracle(case):
    w = case["windows"]
    for thr in THRESHOLDS:
        for cb in CALLBACKS:
            want = oracle_coverage(case["parsed"], w, thr, cb)
            assert np.array_equal(host(case["path"], w, thr, cb, n_threads=2), want)
            assert np.array_equal(bam.window_coverage(case["path"], w, thr, cb, device="cuda:0"), want), (thr, cb)


@pytest.mark.gpu
@pytest.mark.parametrize("thr,cb", [(0, "nofilter"), (20, "all"), (7, "nofilter")])
def test_gpu_pipeline_small_batches_and_ranges(case, thr, cb):
    w = case["windows"]
    want = oracle_coverage(case["parsed"], w, thr, cb)
    for batch in (1 << 16, 40000):            # records straddle batches (the 66 001-op record is ~380 kB)
        assert np.array_equal(bam.window_coverage(case["small"], w, thr, cb, device="cuda:0", batch_bytes=batch), want), batch
    for world in (2, 3):
        parts = [bam.window_coverage(case["small"], w, thr, cb, device="cuda:0", rank=r, world=world, batch_bytes=1 << 17)
                 for r in range(world)]
        assert np.array_equal(np.sum(parts, axis=0), want), world


@pytest.mark.gpu
def test_gpu_pipeline_megabase_read(tmp_path):
    """A 1 Mb read (many work items of one record) and a 1 Mb read whose CIGAR lives in the CG tag, among short ones."""
    ops = [(M, 7000), (I, 3), (D, 5)] * 142 + [(M, 6000)]
    cg = [(M, 12), (D, 1), (M, 3), (I, 1)] * 66000 + [(M, 10)]
    alns = [dict(tid=7, pos=100_000 + 50 * k, cigar=[(S, 20), (M, 900)], name="s%d" % k) for k in range(20)]
    alns += [dict(tid=7, pos=102_000, cigar=[(S, 100)] + ops, name="big1"), dict(tid=7, pos=103_000, cigar=cg, name="big2")]
    alns += [dict(tid=7, pos=200_000 + 50 * k, cigar=[(M, 700)], name="t%d" % k) for k in range(20)]
    rec = synth.records_from_alignments(sorted(alns, key=lambda a: a["pos"]))
    assert int(rec.qlen.max()) >= 1_000_000
    path = str(tmp_path / "mb.bam")
    bam.write_bam(rec, path, seed=1, with_qual=lambda i: i % 5 != 3, fast_seq=True)
    parsed = read_bam(path)
    w = [("chr8", 90_000, 2_000_000), ("chr8", 500_000, 500_150), ("chr8", 1_000_000, 1_010_000), ("chr8", 101_900, 102_150)]
    w += [("chr8", 102_000 + 7 * k * 1000, 102_000 + 7 * k * 1000 + 150) for k in range(140)]
    base = oracle_coverage(parsed, w, 0, "nofilter")
    assert base[0] > 2_000_000
    for thr, cb in ((0, "nofilter"), (30, "all")):
        want = oracle_coverage(parsed, w, thr, cb)
        assert want[0] > base[0] // 3
        assert np.array_equal(host(path, w, thr, cb), want)
        assert np.array_equal(bam.window_coverage(path, w, thr, cb, device="cuda:0"), want), (thr, cb)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny_region", "ultra"])
def test_gpu_track_equals_resident_records_track(name, golden_dir, tmp_path):
    """At threshold 0 the decode-time track equals plot_coverage.coverage_track on the same records resident on the device."""
    from coral_amd.records import DeviceRecords
    gold, rec, graph, want = _plot_case(golden_dir, name, tmp_path)
    path = str(tmp_path / "r.bam")
    bam.write_bam_native(rec, path, seed=4, n_threads=4)
    iv, bounds = plot_coverage.parse_graph_intervals(graph), plot_coverage.parse_region(gold["region"])
    resident = plot_coverage.coverage_track(DeviceRecords(bam.load_bam(path, "cuda:0"), "cuda:0"), iv, bounds)
    got = plot_coverage.coverage_track_bam(path, iv, bounds, device="cuda:0")
    assert got == resident == want
