"""The device queries of a graph build as one native call each (coral_segment_coverage_host, coral_hash_rows_host,
coral_point_cover_host, coral_sa_table_async) against the same wrappers of coral_amd.kernels on the torch-side path
(CORAL_DEVICE_QUERIES=legacy): array for array equal, on the shapes where batching, capacities, the arena's reuse and the
counts that stay on the device could go wrong; and whole builds under both settings, graph file for graph file."""
import glob
import os

import numpy as np
import pytest
import torch

from coral_amd import synth
from tests.bamfile import D, EQ, I, M, S
from tests.product_check import device_sa_table as _sa_table
from tests.test_gpu_kernel_geometry import _crossing_src, _probe_targets, _records_around_segments, _seg_table
from tests.test_gpu_kernels import _Rows

pytestmark = pytest.mark.gpu


def _both(monkeypatch, run):
    """run() on the native path and on the legacy path; the native one first, as a build would meet it."""
    from coral_amd import kernels
    monkeypatch.delenv("CORAL_DEVICE_QUERIES", raising=False)
    native = run()
    monkeypatch.setenv("CORAL_DEVICE_QUERIES", "legacy")
    legacy = run()
    monkeypatch.delenv("CORAL_DEVICE_QUERIES", raising=False)
    assert kernels._native_queries(type("_Dr", (), {"device": torch.device("cuda:0"), "world": 1})())
    return native, legacy


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (what, got.dtype, want.dtype, got.shape, want.shape)


def _mixed_records(n, seed=5):
    """n records on contigs 0 and 2 (none on contig 1), positions below 6000, one to five ops, some without SEQ, some non-ACGT."""
    rng = np.random.default_rng(seed)
    alns = []
    for k in range(n):
        a, b, c = (int(v) for v in rng.integers(5, 400, 3))
        cigar = [[(M, a)], [(S, 7), (M, a), (D, b), (EQ, c)], [(M, a), (I, 3), (M, b), (D, 9), (M, c)]][k % 3]
        pos = int(rng.integers(0, 5000))
        alns.append(dict(tid=0 if k % 4 else 2, pos=pos, cigar=cigar, has_seq=0 if k % 13 == 5 else 1, nonacgt=[pos + 1] if k % 17 == 3 else []))
    alns.sort(key=lambda x: (x["tid"], x["pos"]))
    return synth.records_from_alignments(alns)


@pytest.fixture(scope="module")
def mixed():
    from coral_amd import kernels
    from coral_amd.records import DeviceRecords
    dr = DeviceRecords(_mixed_records(300), "cuda:0")
    return dr, kernels.cigar_scan(dr)


# ---- segment coverage ----------------------------------------------------------------------------------------------------------
NESTED = [(0, 100, 5000), (0, 200, 4000), (0, 300, 3000), (0, 350, 360), (2, 0, 6000), (2, 10, 20)]
COVERAGE_CASES = {
    "none": [],
    "one": [(0, 1000, 2500)],
    "nested": NESTED,
    "duplicates": [(0, 500, 900), (0, 500, 900), (2, 40, 4000), (0, 500, 900), (2, 40, 4000)],
    "unsorted": [(2, 3000, 3500), (0, 4000, 4100), (0, 10, 700), (2, 5, 900), (0, 700, 4000)],
    "no_records": [(1, 0, 5000), (0, 0, 6000), (1, 100, 200), (3, 0, 10)],
}


def _coverage(dr, scan, segs):
    from coral_amd import kernels
    return kernels.segment_coverage(dr, scan, segs)


@pytest.mark.parametrize("case", sorted(COVERAGE_CASES))
def test_coverage_equals_legacy(case, mixed, monkeypatch):
    from coral_amd import kernels
    dr, scan = mixed
    segs = COVERAGE_CASES[case]
    if case == "nested":
        assert len(kernels._disjoint_batches(np.asarray(segs, dtype=np.int64))) >= 3
    native, legacy = _both(monkeypatch, lambda: _coverage(dr, scan, segs))
    _same(native[0], legacy[0], "n_reads")
    _same(native[1], legacy[1], "n_bases")
    if case not in ("none",):
        assert native[0].sum() > 0 and native[1].sum() > 0


@pytest.mark.parametrize("n_seg", [2048, 2049])
def test_coverage_lds_switch(n_seg, monkeypatch):
    """Both sides of the LDS / global-atomic switch of the kernels: the table alone (one batch of n_seg segments), then with a
    shifted copy of every segment added (several batches)."""
    from coral_amd import kernels
    from coral_amd.records import DeviceRecords
    rng = np.random.default_rng(n_seg)
    segs = _seg_table(n_seg, rng)
    rec = _records_around_segments(segs, _probe_targets(n_seg, np.random.default_rng(100 + n_seg)), rng)
    dr = DeviceRecords(rec, "cuda:0")
    scan = kernels.cigar_scan(dr)
    both = segs + [(t, s + 1, e + 2) for t, s, e in segs]
    assert len(kernels._disjoint_batches(np.asarray(segs, dtype=np.int64))) == 1          # n_seg segments reach the kernels as one table
    assert len(kernels._disjoint_batches(np.asarray(both, dtype=np.int64))) >= 2
    for table in (segs, both):
        native, legacy = _both(monkeypatch, lambda: _coverage(dr, scan, table))
        _same(native[0], legacy[0], "n_reads")
        _same(native[1], legacy[1], "n_bases")
        assert native[1].sum() > 0


@pytest.mark.parametrize("n", [1, 300])
def test_coverage_record_counts(n, monkeypatch):
    from coral_amd import kernels
    from coral_amd.records import DeviceRecords
    dr = DeviceRecords(_mixed_records(n, seed=9), "cuda:0")
    scan = kernels.cigar_scan(dr)
    segs = NESTED + [(0, 0, 1 << 30), (2, 0, 1 << 30)]
    native, legacy = _both(monkeypatch, lambda: _coverage(dr, scan, segs))
    _same(native[0], legacy[0], "n_reads")
    _same(native[1], legacy[1], "n_bases")
    assert native[0].max() >= 1


def test_coverage_small_call_after_large_call(mixed, monkeypatch):
    """Many segments, then one: sums or counters left in the arena by the first call would show in the second."""
    dr, scan = mixed
    many = [(t, s, s + 37) for t in (0, 2) for s in range(0, 5200, 13)]
    want_many = _both(monkeypatch, lambda: _coverage(dr, scan, many))[1]
    want_one = _both(monkeypatch, lambda: _coverage(dr, scan, [(0, 1000, 2500)]))[1]
    monkeypatch.delenv("CORAL_DEVICE_QUERIES", raising=False)
    for _ in range(2):
        got = _coverage(dr, scan, many)
        _same(got[0], want_many[0], "n_reads, many")
        _same(got[1], want_many[1], "n_bases, many")
        got = _coverage(dr, scan, [(0, 1000, 2500)])
        _same(got[0], want_one[0], "n_reads, one")
        _same(got[1], want_one[1], "n_bases, one")


# ---- hash rows -----------------------------------------------------------------------------------------------------------------
# contig 0: [100, 200) #4, [200, 300) #5 adjacent, gap, [400, 500) #6; contig 1: flagged, no segment; contig 2: [0, 50) #0, [60, 61) #1
SEG = np.array([[0, 100, 200, 4], [0, 200, 300, 5], [0, 400, 500, 6], [2, 0, 50, 0], [2, 60, 61, 1]], dtype=np.int32).T
HAS = np.array([1, 0, 1, 0], dtype=np.int32)
EDGES = [99, 100, 199, 200, 299, 300, 399, 400, 499, 500]


def _edge_rows():
    tid, ra, rb = [], [], []
    for a in EDGES:
        for b in EDGES:
            tid.append(0); ra.append(a); rb.append(b)
    for a, b in [(0, 0), (49, 50), (59, 60), (60, 61), (10, 5)]:
        tid.append(2); ra.append(a); rb.append(b)
    for t in (1, 3):                                        # a contig without segments, a contig absent from the table
        tid.append(t); ra.append(150); rb.append(250)
    return tid, ra, rb


HASH_CASES = {
    "no_rows": (([], [], []), SEG, HAS),
    "one_row": (([0], [150], [250]), SEG, HAS),
    "edges": (_edge_rows(), SEG, HAS),
    "absent_contig": (([3, 1, 3], [5, 6, 7], [1, 9, 7]), SEG, HAS),
    "one_segment": (_edge_rows(), SEG[:, 1:2], np.array([1, 0, 0, 0], dtype=np.int32)),
}


@pytest.mark.parametrize("case", sorted(HASH_CASES))
def test_hash_rows_equals_legacy(case, monkeypatch):
    from coral_amd import kernels
    from coral_amd.records import DeviceRecords
    (tid, ra, rb), seg, has = HASH_CASES[case]
    dr = DeviceRecords(synth.records_from_alignments([]), "cuda:0")
    T = _Rows(tid, ra, rb)
    native, legacy = _both(monkeypatch, lambda: kernels.hash_rows(dr, T, seg, has))
    for what, g, w in zip(("cni0", "cni1", "e_key", "e_row"), native, legacy):
        _same(g, w, what)
    if case in ("edges", "one_segment"):
        assert len(native[2]) > 10 and (native[0] == -3).sum() >= 2 and (native[0] == -1).sum() > 0
    if case == "absent_contig":
        assert (native[0] == -3).all() and len(native[2]) == 0


def test_hash_rows_small_call_after_large_call(monkeypatch):
    """300 k rows, then the hand-made table: entries or counts left in the arena would show; the first result stays intact
    while the second is made (its arrays are the caller's, not the arena's)."""
    from coral_amd import kernels
    from coral_amd.records import DeviceRecords
    dr = DeviceRecords(synth.records_from_alignments([]), "cuda:0")
    rng = np.random.default_rng(11)
    n = 300_000
    big = _Rows(rng.integers(0, 3, n), rng.integers(0, 600, n), rng.integers(0, 600, n))
    small = _Rows(*_edge_rows())
    want_big = kernels._hash_rows_local(dr, big, SEG, HAS)
    want_small = kernels._hash_rows_local(dr, small, SEG, HAS)
    got_big = kernels.hash_rows(dr, big, SEG, HAS)
    got_small = kernels.hash_rows(dr, small, SEG, HAS)
    for what, g, w in zip(("cni0", "cni1", "e_key", "e_row"), got_big + got_small, want_big + want_small):
        _same(g, w, what)
    assert len(got_big[2]) > n // 6                  # (a third of the rows is on contig 0, where half the positions lie in a segment)


# ---- point cover ---------------------------------------------------------------------------------------------------------------
def _cover(dr, pts, pair_cap=0):
    from coral_amd import kernels
    c = kernels.point_cover(dr, pts, pair_cap=pair_cap)
    return np.array(c.rec, copy=True), np.array(c.begin, copy=True), np.array(c.end, copy=True), [g.tolist() for g in c]


POINT_CASES = {
    "duplicates": [(0, 1200), (2, 800), (0, 1200), (0, 1200), (2, 800)],
    "negative": [(0, -5), (0, 1200), (2, -1), (0, 0)],
    "uncovered": [(1, 500), (0, 1 << 29), (3, 7), (0, 2500)],
    "overlapping_windows": [(0, 2000), (0, 2003), (0, 2300), (2, 2000), (2, 2001)],
}


@pytest.mark.parametrize("pair_cap", [0, 1])
@pytest.mark.parametrize("case", sorted(POINT_CASES))
def test_point_cover_equals_legacy(case, pair_cap, mixed, monkeypatch):
    """pair_cap 1: the first launch overflows and the wrapper launches again with room for every pair."""
    dr, _ = mixed
    pts = POINT_CASES[case]
    native, legacy = _both(monkeypatch, lambda: _cover(dr, pts, pair_cap))
    for what, g, w in zip(("rec", "begin", "end"), native, legacy):
        _same(g, w, what)
    assert native[3] == legacy[3] and len(native[3]) == len(pts)
    assert any(native[3]) and (case not in ("negative", "uncovered") or not all(native[3]))


def test_point_cover_small_call_after_large_call(mixed, monkeypatch):
    from coral_amd.records import DeviceRecords
    big = DeviceRecords(_crossing_src(n=3000, per_tail=5).records(), "cuda:0")
    large = [(0, p) for p in range(49_000, 51_000, 50)]
    want_large = _both(monkeypatch, lambda: _cover(big, large))[1]
    want_small = _both(monkeypatch, lambda: _cover(mixed[0], POINT_CASES["duplicates"]))[1]
    assert len(want_large[0]) > 20_000
    monkeypatch.delenv("CORAL_DEVICE_QUERIES", raising=False)
    for _ in range(2):
        for dr, pts, want in ((big, large, want_large), (mixed[0], POINT_CASES["duplicates"], want_small)):
            got = _cover(dr, pts)
            for what, g, w in zip(("rec", "begin", "end"), got, want):
                _same(g, w, what)


# ---- SA table ------------------------------------------------------------------------------------------------------------------
def _plain(k, name=None):
    return dict(tid=0, pos=100 + k, cigar=[(M, 50)], name=name or "plain%d" % k)


def _sa_cases():
    n = 90
    many = [(0, 1000 + 700 * k, k % 2, 100 * k if k else 0, 100, 0, 100 * (n - k), 60, 1) for k in range(1, n + 1)]
    ok = (1, 900, 1, 30, 10, 0, 0, 60, 1)
    return {
        "no_sa": [_plain(k) for k in range(5)],
        "one_sa": [dict(tid=0, pos=5, cigar=[(M, 30), (S, 10)], name="r", sa=[ok]), _plain(1)],
        "ninety": [dict(tid=0, pos=10, cigar=[(M, 100), (S, 100 * n)], name="long", sa=many), _plain(20, "y")],
        "mixed": [
            dict(tid=0, pos=5, cigar=[(M, 30), (S, 10)], name="a", sa=[ok, (2, 40, 0, 0, 25, -3, 15, 20, 2)]),
            dict(tid=0, pos=9, cigar=[(S, 30), (M, 10)], name="no_primary", flag=2048, sa=[(0, 6, 0, 0, 30, 0, 10, 60, 0)]),
            dict(tid=0, pos=12, cigar=[(M, 30), (S, 10)], name="dup", sa=[ok, ok, (0, 700, 0, 12, 20, 4, 4, 9, 3), ok]),
            dict(tid=0, pos=14, cigar=[(M, 40)], name="no_s", sa=[(0, 300, 0, 0, 40, 0, 0, 60, 0), ok]),
            dict(tid=1, pos=3, cigar=[(S, 30), (M, 10)], name="dup", flag=2048, sa=[ok, (0, 13, 0, 0, 30, 0, 10, 60, 0)]),
            dict(tid=1, pos=8, cigar=[(S, 20), (M, 20)], name="no_m", sa=[(0, 300, 0, 20, 0, 0, 20, 60, 0)]),
            dict(tid=1, pos=9, cigar=[(S, 10), (M, 30)], name="b", sa=[(0, 2000, 1, 10, 20, 5, 5, 60, 4), (3, 77, 0, 35, 5, 0, 0, 3, 0)]),
            dict(tid=-1, pos=-1, cigar=[], flag=4, name="unplaced", sa=[ok]),
        ],
        "few_reads_many_names": [_plain(k) for k in range(40)] + [dict(tid=0, pos=500, cigar=[(M, 30), (S, 10)], name="r", sa=[ok])] +
                                [dict(tid=1, pos=k, cigar=[(M, 20)], name="tail%d" % k) for k in range(300)],
    }


@pytest.mark.parametrize("case", ["no_sa", "one_sa", "ninety", "mixed", "few_reads_many_names"])
def test_sa_table_equals_legacy(case, monkeypatch):
    rec = synth.records_from_alignments(_sa_cases()[case])
    native, legacy = _both(monkeypatch, lambda: _sa_table(rec))
    for key in ("cols", "name", "failed", "read_length", "pairs", "rows"):
        _same(native[key], legacy[key], key)
    if len(legacy["name"]):                                  # (without a read the legacy path leaves the one offset unset)
        _same(native["off"], legacy["off"], "off")
    n_reads = {"no_sa": 0, "one_sa": 1, "ninety": 1, "mixed": 5, "few_reads_many_names": 1}[case]
    assert len(native["name"]) == n_reads and native["cols"].shape[0] == 8
    if case == "ninety":
        assert native["cols"].shape[1] == 90 and (native["pairs"][:, 5] & 1).sum() == 89 + 88
    if case == "mixed":
        from coral_amd import kernels
        from coral_amd.records import DeviceRecords
        cols, *_, st = kernels.sa_table(DeviceRecords(rec, "cuda:0"))          # nothing made beforehand
        _same(np.array(cols, copy=True), legacy["cols"], "cols, without sa_table_early")
        st.close()
        assert native["failed"].sum() == 2 and native["cols"].shape[1] == 2 + 3 + 2          # reads a, dup (de-duplicated), b


def test_sa_table_errors_equal_legacy(monkeypatch):
    """The two error shapes raise what they raised: KeyError for an SA CIGAR outside the nine shapes, ZeroDivisionError for a
    zero-length query interval.  A table that holds both raises what its first offending read raises: the reference walks the
    reads in dict order and stops there, and in [bad, zero] the read with the unknown shape comes first - KeyError, on both
    drivers (tests/test_sa_table_reference.py has the other orders)."""
    bad = dict(tid=0, pos=10, cigar=[(S, 5), (M, 50)], name="x", sa=[(0, 500, 0, -2, 40, 0, 0, 60, 1)])
    zero = dict(tid=0, pos=11, cigar=[(S, 5), (M, 50)], name="z", sa=[(0, 500, 0, 54, 1, 0, 0, 60, 1)])
    for alns, exc in (([bad, _plain(20)], KeyError), ([zero, _plain(20)], ZeroDivisionError), ([bad, zero, _plain(20)], KeyError)):
        rec = synth.records_from_alignments(alns)
        for mode in (None, "legacy"):
            if mode:
                monkeypatch.setenv("CORAL_DEVICE_QUERIES", mode)
            else:
                monkeypatch.delenv("CORAL_DEVICE_QUERIES", raising=False)
            with pytest.raises(exc):
                _sa_table(rec)


# ---- whole builds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tiny", "small", "cfg3_2amp"])
def test_build_writes_the_same_graph_files(case, tmp_path, monkeypatch):
    from coral_amd import infer_breakpoint_graph as ibg
    from coral_amd.records import DeviceRecords
    cfg, rec = synth.dataset(case, "cpu")
    cn, seeds = str(tmp_path / "cn.bed"), str(tmp_path / "seeds.bed")
    synth.write_cn_bed(cfg, cn)
    synth.write_seed_bed(cfg, seeds)
    files = {}
    for mode in ("native", "legacy"):
        monkeypatch.setenv("CORAL_DEVICE_QUERIES", mode)
        ibg.build_graph_from_records(DeviceRecords(rec, "cuda:0"), seeds, cn, str(tmp_path / mode))
        files[mode] = {os.path.basename(p)[len(mode):]: open(p, "rb").read() for p in sorted(glob.glob(str(tmp_path / (mode + "*_graph.txt"))))}
    assert len(files["native"]) >= (2 if case == "cfg3_2amp" else 1) and files["native"] == files["legacy"]


def test_arena_release_and_reuse(mixed, monkeypatch):
    """coral_query_arena_release frees the arenas; the next query allocates again and gives the same result."""
    from coral_amd import _lib
    dr, scan = mixed
    monkeypatch.delenv("CORAL_DEVICE_QUERIES", raising=False)
    first = _coverage(dr, scan, NESTED)
    assert _lib.lib().coral_query_arena_release() == 0
    again = _coverage(dr, scan, NESTED)
    _same(again[0], first[0], "n_reads")
    _same(again[1], first[1], "n_bases")
