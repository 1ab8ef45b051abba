"""The interval search with its handle made early and its threads kept (CPU, with the oracle-backed kernel stand-ins): whole
builds with the early handle (default) and with ``CORAL_SEARCH_EARLY=0`` (the handle made in front of the search, no early
prefetch) give the same intervals, breakpoints, statistics, component ids, connections and graphs — on the ``hash_rows`` branch
of hash_alignment_to_seg, on its overlapping-CN-segments branch and without ``launch_record_kernels`` — the search threads of
the process are reused from build to build, a build that fails in fetch() leaves no thread and no handle behind, and the grid
of tests/test_search_bfs.py holds when an early handle exists.  ``CORAL_SEARCH_MIN_READS=0``: the threaded search, which the
data sets of the tests are too small for by default."""
import copy
import json
import os

import pytest

from tests.canon import canon, graph_snapshot
from tests.product_check import install_cpu_kernel_fakes, load_case
from tests.test_search_bfs import DEFAULTS, GRID, _search

CASES = ["small", "ultra", "cfg3_2amp"]


def _threads():
    """Threads of the process.  (A joined thread leaves /proc/self/task a moment after join() returns — a Python thread even
    after its last bytecode: the count is read 2 ms apart until two readings agree.)"""
    import time
    n = len(os.listdir("/proc/self/task"))
    for _ in range(50):
        time.sleep(0.002)
        m = len(os.listdir("/proc/self/task"))
        if m == n:
            break
        n = m
    return n


def _files(cfg, tmp_path, overlapping=False):
    from coral_amd import synth
    cn, seeds = str(tmp_path / "cn.bed"), str(tmp_path / "seeds.bed")
    synth.write_cn_bed(cfg, cn)
    synth.write_seed_bed(cfg, seeds)
    if overlapping:
        # two segments that overlap each other, where no read lies and with a CN far from the median (read_cns never picks
        # them): hash_alignment_to_seg takes its general branch, every read still has at most one segment per end
        with open(cn, "a") as fp:
            fp.write("%s\t300000000\t300000100\t50.0\n%s\t300000050\t300000150\t50.0\n" % (synth.CHROMS[-1], synth.CHROMS[-1]))
    return cn, seeds


def _snapshot(b):
    return dict(intervals=canon(b.amplicon_intervals), bps=canon(b.new_bp_list), stats=canon(b.new_bp_stats), ccids=canon(b.new_bp_ccids),
                conn=canon(b.amplicon_interval_connections), ccid2id=canon(b.ccid2id), graphs=[graph_snapshot(g) for g in b.lr_graph])


def _build(rec, seeds, cn, gold):
    from coral_amd import infer_breakpoint_graph as ibg
    from coral_amd.records import DeviceRecords
    b = ibg.build_graph_from_records(DeviceRecords(rec, "cpu"), seeds, cn, None, min_bp_support=gold["min_bp_support"])
    return b, _snapshot(b)


def _same(a, b, what):
    for k in a:
        assert json.dumps(a[k]) == json.dumps(b[k]), (what, k)


@pytest.mark.parametrize("overlapping", [False, True], ids=["hash_rows", "overlapping_segments"])
@pytest.mark.parametrize("case", CASES)
def test_early_handle_builds_equal_late_handle_builds(case, overlapping, golden_dir, tmp_path, monkeypatch):
    from coral_amd import kernels
    install_cpu_kernel_fakes(monkeypatch)
    monkeypatch.setenv("CORAL_SEARCH_MIN_READS", "0")
    gold, cfg, rec = load_case(golden_dir, case)
    cn, seeds = _files(cfg, tmp_path, overlapping)
    calls = []
    real = kernels.hash_rows
    monkeypatch.setattr(kernels, "hash_rows", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setenv("CORAL_SEARCH_EARLY", "0")
    late, want = _build(rec, seeds, cn, gold)
    late_st = late._search_ctx.stats()
    assert not late._search_ctx.early and late_st["queued_before_bfs"] == 0 and late_st["queued"] >= 1, late_st
    assert bool(calls) != overlapping, "hash_alignment_to_seg took the other branch"
    monkeypatch.delenv("CORAL_SEARCH_EARLY")
    b1, got = _build(rec, seeds, cn, gold)
    st = b1._search_ctx.stats()
    assert b1._search_ctx.early and st["attached"] == 1 and st["fill_ready_at_attach"] == 1, st
    assert st["queued_before_bfs"] >= 1 and st["workers"] >= 1, st          # the seeds' steps were on the workers before the search began
    # ... and they are the steps the search then asks for: had the early snap given other coordinates, the search would have
    # queued its own seeds on top (a step is queued once per distinct key)
    assert st["queued"] == late_st["queued"], (st, late_st)
    assert len(want["bps"]) > 0 and len(want["graphs"]) > 0
    _same(got, want, "early handle")
    if case != "small":                                   # (the rest once per branch: a build with the stand-in kernels takes seconds)
        return
    # three builds in one process: the threads of the first serve the others
    n1 = _threads()
    del late
    b2, got2 = _build(rec, seeds, cn, gold)
    b3, got3 = _build(rec, seeds, cn, gold)
    _same(got3, want, "third build")
    assert _threads() == n1, "builds 2 and 3 changed the number of threads"
    # without launch_record_kernels there is no early handle: the search makes its own, on the same threads
    monkeypatch.setenv("CORAL_NO_EARLY_LAUNCH", "1")
    b4, got4 = _build(rec, seeds, cn, gold)
    assert not b4._search_ctx.early
    _same(got4, want, "CORAL_NO_EARLY_LAUNCH=1")
    assert _threads() == n1


def test_build_that_fails_in_fetch_leaves_nothing_behind(golden_dir, tmp_path, monkeypatch):
    from coral_amd import chimeric, infer_breakpoint_graph as ibg
    install_cpu_kernel_fakes(monkeypatch)
    monkeypatch.setenv("CORAL_SEARCH_MIN_READS", "0")
    gold, cfg, rec = load_case(golden_dir, "small")
    cn, seeds = _files(cfg, tmp_path)
    _, want = _build(rec, seeds, cn, gold)                # (starts the threads of the process)
    n1 = _threads()
    made, closed = [], []
    real_init, real_close, real_table = chimeric.PairSearch.__init__, chimeric.PairSearch.close, ibg.build_chimeric_table

    def init(self, *a, **k):
        real_init(self, *a, **k)
        made.append(self)

    def close(self):
        if getattr(self, "_h", None):
            closed.append(self)
        real_close(self)

    def table(*a, **k):
        T = real_table(*a, **k)
        T.finish_nm_stats()
        T.n_mapq60_plain = 0                               # ibg:159: no plain MAPQ-60 record -> ZeroDivisionError in fetch()
        T.finish_nm_stats = lambda: None
        return T
    monkeypatch.setattr(chimeric.PairSearch, "__init__", init)
    monkeypatch.setattr(chimeric.PairSearch, "close", close)
    monkeypatch.setattr(chimeric.PairSearch, "__del__", close)
    monkeypatch.setattr(ibg, "build_chimeric_table", table)
    with pytest.raises(ZeroDivisionError):
        _build(rec, seeds, cn, gold)
    assert len(made) == 1 and made[0].early and closed == made, "the early handle of the failed build was not freed"
    assert _threads() == n1, "the failed build left a thread behind"
    monkeypatch.setattr(ibg, "build_chimeric_table", real_table)
    _, got = _build(rec, seeds, cn, gold)
    _same(got, want, "the build after the failed one")
    assert _threads() == n1
    # a build given up after launch_record_kernels: the handle goes with the object
    from coral_amd.records import DeviceRecords
    del made[:], closed[:]
    b = ibg.bam_to_breakpoint_nanopore(None, seeds, records=DeviceRecords(rec, "cpu"))
    b.launch_record_kernels()
    del b
    assert len(made) == 1 and closed == made
    assert _threads() == n1


@pytest.mark.parametrize("case", CASES)
def test_search_grid_with_an_early_handle(case, golden_dir, tmp_path, monkeypatch):
    """The object of tests/test_search_bfs.py, prepared with launch_record_kernels: its first search runs on the early handle
    (attached, parameters set, seeds prefetched by hash_alignment_to_seg); every later one of the grid closes the handle it
    finds — the early one first, with steps possibly still queued — and makes its own."""
    from coral_amd import infer_breakpoint_graph as ibg
    from coral_amd.records import DeviceRecords
    install_cpu_kernel_fakes(monkeypatch)
    monkeypatch.setenv("CORAL_SEARCH_MIN_READS", "0")
    monkeypatch.setenv("CORAL_SEARCH_THREADS", "3")
    gold, cfg, rec = load_case(golden_dir, case)
    cn, seeds_file = _files(cfg, tmp_path)
    b = ibg.bam_to_breakpoint_nanopore(None, seeds_file, records=DeviceRecords(rec, "cpu"))
    b.launch_record_kernels()
    b.read_cns(cn)
    b.fetch()
    b.hash_alignment_to_seg()
    S = b._search_ctx
    assert S is not None and S.early and S.stats()["queued"] >= 1
    seeds, cutoff0 = copy.deepcopy(b.amplicon_intervals), b.min_cluster_cutoff
    b.find_amplicon_intervals()                           # on the early handle
    assert b._search_ctx is S and S.stats()["queued_before_bfs"] >= 1
    first = dict(intervals=canon(b.amplicon_intervals), bps=canon(b.new_bp_list), stats=canon(b.new_bp_stats), ccids=canon(b.new_bp_ccids),
                 conn=canon(b.amplicon_interval_connections))
    n_bps = 0
    for extra in GRID:
        params = dict(DEFAULTS, min_cluster_cutoff=cutoff0)
        params.update(extra)
        try:
            want = _search(b, "python", params, seeds)
        except Exception as exc:          # noqa: BLE001 — the reference's own KeyError / IndexError cases
            with pytest.raises(type(exc)):
                _search(b, "native", params, seeds)
            continue
        got = _search(b, "native", params, seeds)
        for k in want:
            assert json.dumps(got[k]) == json.dumps(want[k]), (case, extra, k)
        if extra == {}:
            for k in first:
                assert json.dumps(first[k]) == json.dumps(want[k]), (case, "the early handle's search", k)
        n_bps += len(want["bps"])
    assert n_bps > 0
    # a parameter changed between hash_alignment_to_seg and the search: the early handle has the old one and is replaced
    b2 = ibg.bam_to_breakpoint_nanopore(None, seeds_file, records=DeviceRecords(rec, "cpu"))
    b2.launch_record_kernels()
    b2.read_cns(cn)
    b2.fetch()
    b2.hash_alignment_to_seg()
    early = b2._search_ctx
    b2.max_seq_len = 200000
    got = _search_keep(b2)
    want = _search(b, "python", dict(DEFAULTS, min_cluster_cutoff=cutoff0, max_seq_len=200000), seeds)
    assert b2._search_ctx is not early
    for k in got:
        assert json.dumps(got[k]) == json.dumps(want[k]), (case, "parameter changed after hash_alignment_to_seg", k)


def test_search_lifecycle_host_program(tmp_path):
    """tests/native/search_lifecycle_host.cpp (the C API alone: early + attach against create, shared threads, free with
    steps queued and in flight, 200 create / free cycles, shutdown) compiled as a plain program and run; its header names the
    two sanitizer builds, which are run by hand."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH: the handle lifecycle cannot be checked")
    exe = str(tmp_path / "search_lifecycle_host")
    srcs = [os.path.join(root, "tests", "native", "search_lifecycle_host.cpp")] + \
           [os.path.join(root, "coral_amd", "csrc", f) for f in ("coral_search.cpp", "coral_bpcall.cpp", "coral_host.cpp")]
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off"] + srcs + ["-o", exe], check=True, cwd=root)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "search_lifecycle_host: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _search_keep(b):
    b.find_amplicon_intervals()
    return dict(intervals=canon(b.amplicon_intervals), bps=canon(b.new_bp_list), stats=canon(b.new_bp_stats), ccids=canon(b.new_bp_ccids),
                conn=canon(b.amplicon_interval_connections))
