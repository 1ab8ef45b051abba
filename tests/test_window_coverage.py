"""Window coverage with a base-quality threshold, counted during the BAM decode (bam.window_coverage, the coverage track of
`plot` at any --min_mapq): both pipelines against an INDEPENDENT restatement of pysam count_coverage (oracle_coverage, which
tests/test_bam_index.py checks against as well and which therefore lives next to the reader in tests/bamfile.py: the BAM is
read there with gzip + struct, CIGAR / SEQ / QUAL walked per record), and against the plot goldens at threshold 0."""
import numpy as np
import pytest

from coral_amd import bam, plot_coverage, synth
from tests.bamfile import D, I, M, S, oracle_coverage, read_bam as _read_bam
from tests.decode_support import (coverage_odd_records as odd_records, coverage_windows as make_windows, host_window_coverage as host,
                                  plot_case as _plot_case, with_qual)

THRESHOLDS = (0, 1, 7, 20, 30, 61, 255)
CALLBACKS = ("nofilter", "all")


def read_bam(path):
    """(ref names, [record dicts]) as oracle_coverage takes them"""
    parsed = _read_bam(path)
    return parsed.refs, parsed.recs


def make_records(n=700):
    return synth.merge_sorted(synth.generate(synth.scaled_config("tiny", n), "cpu"), odd_records())


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
