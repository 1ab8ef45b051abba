"""The interval search exploring ahead from finished steps (``CORAL_SEARCH_SPECULATE``, coral_amd/csrc/coral_search.cpp), on
the CPU: a speculative entry is a step computed before the search asks for it, keyed like every other step, so not a byte of
the search's result may depend on it.

1. tests/native/search_speculate_host.cpp — the C API alone on a table built so that one seed's step yields an interval whose
   step yields another: the search without threads, with threads and speculation off, and with speculation on
   give byte-identical arrays; the counters; a handle freed with guesses queued and in flight; a shutdown in the middle of a
   search; the tail jobs right after a search that left guesses behind.  Compiled as a plain program and run; its header names
   the two sanitizer builds, which are run by hand.
2. The four golden data sets of tests/test_search_bfs.py with the oracle-backed kernel stand-ins and the threaded search forced
   (``CORAL_SEARCH_MIN_READS=0``): the native search with speculation on against the one with it off and against
   the step-by-step Python search — intervals, breakpoints with their supports, statistics, component ids, connections and the
   log lines, order included — and the same number of steps queued by the caller."""
import copy
import json
import os
import shutil
import subprocess

import pytest

from tests.product_check import install_cpu_kernel_fakes
from tests.test_search_bfs import DEFAULTS, _prepared, _search

SPEC_KEYS = ("spec_queued", "spec_asked", "spec_ready_when_asked", "spec_unused")


def test_search_speculate_host_program(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH: the speculative search cannot be checked")
    exe = str(tmp_path / "search_speculate_host")
    srcs = [os.path.join(root, "tests", "native", "search_speculate_host.cpp")] + \
           [os.path.join(root, "coral_amd", "csrc", f) for f in ("coral_search.cpp", "coral_bpcall.cpp", "coral_host.cpp")]
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off"] + srcs + ["-o", exe], check=True, cwd=root)
    env = {k: v for k, v in os.environ.items() if not k.startswith("CORAL_SEARCH_")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "search_speculate_host: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("case", ["tiny_edge", "small", "ultra", "cfg3_2amp"])
def test_speculation_changes_nothing_on_the_golden_cases(case, golden_dir, tmp_path, monkeypatch):
    install_cpu_kernel_fakes(monkeypatch)
    monkeypatch.setenv("CORAL_SEARCH_MIN_READS", "0")
    monkeypatch.setenv("CORAL_SEARCH_THREADS", "3")
    monkeypatch.setenv("CORAL_SEARCH_PAR_MIN", "1")
    b = _prepared(case, golden_dir, tmp_path)
    seeds = copy.deepcopy(b.amplicon_intervals)
    n_spec = 0
    # the defaults, and a short max_seq_len (many runs, `outside` ends, many intervals one hop from another)
    for extra in (dict(), dict(max_seq_len=200000)):
        params = dict(DEFAULTS, min_cluster_cutoff=b.min_cluster_cutoff)
        params.update(extra)
        want = _search(b, "python", params, seeds)
        monkeypatch.setenv("CORAL_SEARCH_SPECULATE", "0")
        off = _search(b, "native", params, seeds)
        st_off = b._search_ctx.stats()
        assert st_off["workers"] >= 1 and st_off["queued"] >= 1, st_off
        assert all(st_off[k] == 0 for k in SPEC_KEYS), st_off
        for k in want:
            assert json.dumps(off[k]) == json.dumps(want[k]), (case, extra, k, "speculation off")
        for mode in ("1", None):                          # set, and the default
            if mode is None:
                monkeypatch.delenv("CORAL_SEARCH_SPECULATE")
            else:
                monkeypatch.setenv("CORAL_SEARCH_SPECULATE", mode)
            on = _search(b, "native", params, seeds)
            st = b._search_ctx.stats()
            for k in want:
                assert json.dumps(on[k]) == json.dumps(want[k]), (case, extra, k, "speculation on", mode)
            assert st["queued"] == st_off["queued"], (case, extra, mode, st, st_off)
            assert all(st[k] >= 0 for k in SPEC_KEYS), st
            assert st["spec_asked"] <= st["spec_queued"] and st["spec_ready_when_asked"] <= st["spec_asked"], st
            assert st["spec_unused"] == st["spec_queued"] - st["spec_asked"], st
            n_spec += st["spec_queued"]
    assert len(want["bps"]) > 0
    # (else "on" would equal "off" trivially: four searches with speculation on, each with finished seeds' steps to guess from)
    assert n_spec > 0, "no speculative entry was queued on this data set"
    print("%s: %d speculative entries over the runs" % (case, n_spec))
