"""The host side of the streamed coordinate sort that needs no GPU: the step planner of the merge (coral_amd/csrc/coral_merge_plan.h
through its C entry coral_merge_plan) against a restatement in Python, tests/native/merge_plan_host.cpp compiled and run as a plain
program, the new symbols of the library, the `sort --stream` parser and the Python argument rules of bam.sort_bam_stream /
bam.sort_bam(stream=True), each checked before any file is opened.

The plan's rule: a step [j0, j1) is the longest stretch of whole records, in final order, whose sources fit `stage_bytes`; every
run gives a contiguous range of its records, rounded outwards to its 0xff00-byte blocks (the last block of a run may be
shorter), staged run after run in run order; a run with nothing in the step gives nothing."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from coral_amd import CoRAL, _lib, bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 0xff00
CORAL_OK, CORAL_ERR_ARG, CORAL_ERR_CAPACITY = 0, -1, -3


class Capacity(Exception):
    pass


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def parts_of(runs, pos, lens, run_bytes, recs):
    """recs: (run, ordinal in the run) of a stretch of final positions -> [(run, first block, blocks, staging base)], bytes"""
    parts, base = [], 0
    for r in range(len(runs)):
        mine = [k for rr, k in recs if rr == r]
        if not mine:
            continue
        assert mine == list(range(mine[0], mine[-1] + 1))        # contiguous: the merge keeps a run's order
        b0, b1 = pos[r][mine[0]] // BLOCK, -(-(pos[r][mine[-1]] + lens[r][mine[-1]]) // BLOCK)
        parts.append((r, b0, b1 - b0, base))
        base += min(b1 * BLOCK, run_bytes[r]) - b0 * BLOCK
    return parts, base


def restate(lens, order, stage):
    """lens: per run the record lengths; order: (run, ordinal in the run) per final position -> [(j0, j1, parts)]"""
    pos = [np.concatenate([[0], np.cumsum(l)]).astype(np.int64).tolist() for l in lens]
    run_bytes = [p[-1] for p in pos]
    steps, j0 = [], 0
    while j0 < len(order):
        if parts_of(lens, pos, lens, run_bytes, order[j0:j0 + 1])[1] > stage:
            raise Capacity()
        j1 = j0 + 1
        while j1 < len(order) and parts_of(lens, pos, lens, run_bytes, order[j0:j1 + 1])[1] <= stage:
            j1 += 1
        steps.append((j0, j1, parts_of(lens, pos, lens, run_bytes, order[j0:j1])[0]))
        j0 = j1
    return steps


def smallest_stage(lens, order):
    pos = [np.concatenate([[0], np.cumsum(l)]).astype(np.int64).tolist() for l in lens]
    return max([parts_of(lens, pos, lens, [p[-1] for p in pos], [o])[1] for o in order] or [0])


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
def plan(lens, order, stage):
    """-> (rc, [(j0, j1, parts)])"""
    L = _lib.lib()
    first = np.concatenate([[0], np.cumsum([len(l) for l in lens])]).astype(np.int64)
    run_records = np.array([len(l) for l in lens] + [0], dtype=np.int64)
    flat = np.array([x for l in lens for x in l] + [0], dtype=np.uint32)
    perm = np.array([first[r] + k for r, k in order] + [0], dtype=np.uint32)
    counts = (C.c_int64 * 2)()
    args = (len(lens), run_records.ctypes.data, flat.ctypes.data, perm.ctypes.data, stage)
    rc = L.coral_merge_plan(*args, 0, 0, None, None, None, counts)
    if rc != CORAL_OK:
        return rc, None
    n_steps, n_parts = counts[0], counts[1]
    step_j, step_part, parts = np.full(n_steps + 1, -1, np.int64), np.full(n_steps + 1, -1, np.int64), np.full((n_parts + 1, 4), -1, np.int64)
    assert L.coral_merge_plan(*args, n_steps - 1, n_parts, step_j.ctypes.data, step_part.ctypes.data, parts.ctypes.data, counts) == CORAL_ERR_CAPACITY
    assert L.coral_merge_plan(*args, n_steps, n_parts, step_j.ctypes.data, step_part.ctypes.data, parts.ctypes.data, counts) == CORAL_OK
    assert (counts[0], counts[1]) == (n_steps, n_parts) and parts[n_parts].tolist() == [-1] * 4
    return rc, [(int(step_j[s]), int(step_j[s + 1]), [tuple(p) for p in parts[step_part[s]:step_part[s + 1]].tolist()]) for s in range(n_steps)]


def random_case(rnd, n_runs):
    """Runs of 0..50 records of 40..200 000 bytes and a final order that keeps every run's own order."""
    lens = [[rnd.choice((40, 41, BLOCK - 1, BLOCK, BLOCK + 1, rnd.randrange(40, 3000), rnd.randrange(40, 200_001))) for _ in range(rnd.randrange(0, 51))]
            for _ in range(n_runs)]
    left = [list(range(len(l))) for l in lens]
    order = []
    while any(left):
        r = rnd.choice([r for r in range(n_runs) if left[r]])
        for _ in range(rnd.randrange(1, 6)):                     # stretches of one run, as sorted input gives
            if left[r]:
                order.append((r, left[r].pop(0)))
    return lens, order


def test_the_plan_is_the_restatement():
    rnd = random.Random(20250611)
    seen = dict(skipped=0, shared=0, one_step=0, many=0)
    for trial in range(60):
        lens, order = random_case(rnd, rnd.choice((1, 2, 3, 5, 8)))
        if trial == 0:
            lens, order = [[100, 200], [], [300]], [(2, 0), (0, 0), (0, 1)]      # an empty run between two others
        low = smallest_stage(lens, order)
        for stage in sorted({low, low + 1, low + BLOCK, 3 * low + 7, 10 * low + 1, 1 << 40}):
            rc, got = plan(lens, order, stage)
            want = restate(lens, order, stage)
            assert rc == CORAL_OK and got == want, (trial, stage)
            # the properties themselves, on the library's answer: the steps tile [0, N); every step is greedy-maximal
            assert [s[0] for s in got] == [0] + [s[1] for s in got[:-1]] and (got[-1][1] if got else 0) == len(order)
            pos = [np.concatenate([[0], np.cumsum(l)]).astype(np.int64).tolist() for l in lens]
            rb = [p[-1] for p in pos]
            for j0, j1, parts in got:
                assert parts_of(lens, pos, lens, rb, order[j0:j1])[1] <= stage
                assert j1 == len(order) or parts_of(lens, pos, lens, rb, order[j0:j1 + 1])[1] > stage
                touched = {r for r, _ in order[j0:j1]}
                assert [p[0] for p in parts] == sorted(touched)
                seen["skipped"] += len(touched) < sum(1 for l in lens if l)
                for r, b0, nb, base in parts:                    # outward rounding: the blocks cover the records and no block more
                    ks = [k for rr, k in order[j0:j1] if rr == r]
                    assert b0 * BLOCK <= pos[r][ks[0]] < (b0 + 1) * BLOCK and (b0 + nb - 1) * BLOCK < pos[r][ks[-1]] + lens[r][ks[-1]] <= (b0 + nb) * BLOCK
            for a, b in zip(got, got[1:]):
                ends = {p[0]: p[1] + p[2] - 1 for p in a[2]}
                seen["shared"] += any(ends.get(p[0]) == p[1] for p in b[2])
            seen["one_step" if len(got) == 1 else "many"] += 1
        if low > 0:
            assert plan(lens, order, low - 1) == (CORAL_ERR_CAPACITY, None) and "stage_bytes" in _lib.lib().coral_bam_last_error().decode()
            with pytest.raises(Capacity):
                restate(lens, order, low - 1)
    assert all(v > 20 for v in seen.values()), seen


def test_nothing_to_plan_and_what_is_refused():
    assert plan([], [], 0) == (CORAL_OK, [])                      # zero runs
    assert plan([[], [], []], [], 5) == (CORAL_OK, [])            # zero records
    assert plan([[40]], [(0, 0)], 40) == (CORAL_OK, [(0, 1, [(0, 0, 1, 0)])])
    assert plan([[40]], [(0, 0)], 39)[0] == CORAL_ERR_CAPACITY
    # an order that does not keep a run's own order, or names a record twice, is no merge
    assert plan([[40, 50]], [(0, 1), (0, 0)], 1 << 20)[0] == CORAL_ERR_ARG and "order" in _lib.lib().coral_bam_last_error().decode()
    assert plan([[40, 50], [60]], [(0, 0), (0, 0), (1, 0)], 1 << 20)[0] == CORAL_ERR_ARG
    L = _lib.lib()
    counts = (C.c_int64 * 2)()
    assert L.coral_merge_plan(-1, None, None, None, 0, 0, 0, None, None, None, counts) == CORAL_ERR_ARG
    assert L.coral_merge_plan(0, None, None, None, 0, 0, 0, None, None, None, None) == CORAL_ERR_ARG
    assert L.coral_merge_plan(0, None, None, None, -1, 0, 0, None, None, None, counts) == CORAL_ERR_ARG


def test_native_program(tmp_path):
    """tests/native/merge_plan_host.cpp (the planner and the spill-run reader on a spill the program writes itself, truncated and
    corrupt ones included) compiled as a plain program and run; its header names the sanitizer build."""
    exe = str(tmp_path / "merge_plan_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", os.path.join(ROOT, "tests/native/merge_plan_host.cpp"), "-o", exe], check=True, cwd=ROOT)
    done = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert done.returncode == 0 and "merge_plan_host: ok" in done.stdout, (done.returncode, done.stdout, done.stderr)


def test_the_library_exports_the_new_calls():
    L = _lib.lib()
    for name in ("coral_bamgpu_open_request", "coral_bamgpu_run_table", "coral_bamgpu_merge_workspace_bytes", "coral_bamgpu_merge_runs",
                 "coral_bamgpu_merge_stats", "coral_merge_plan"):
        assert getattr(L, name).argtypes is not None, name
    with open(os.path.join(ROOT, "include", "coral_hip.h")) as fp:
        header = fp.read()
    for name in ("coral_bamgpu_open_request(", "CORAL_SINK_RUNS", "coral_bamgpu_run_table(", "coral_bamgpu_merge_workspace_bytes(", "coral_bamgpu_merge_runs(",
                 "coral_bamgpu_merge_stats(", "coral_merge_plan("):
        assert name in header, name
    # neither call needs a GPU to refuse a handle that is none
    assert L.coral_bamgpu_merge_workspace_bytes(None, 0) == CORAL_ERR_ARG and "coral_bamgpu_open_request (runs sink)" in L.coral_bam_last_error().decode()
    assert L.coral_bamgpu_merge_runs(None, b"x", None, 0, None, 0, 0, None) == CORAL_ERR_ARG
    assert L.coral_bamgpu_run_table(None, 0, None, (C.c_int64 * 3)()) == CORAL_ERR_ARG


def test_the_runs_sink_refuses_what_the_bam_sink_refuses(tmp_path):
    """(the runs sink of coral_bamgpu_open_request and its BAM sink)"""
    from tests.test_sort_records import raw_record
    from tests.test_extract_reads import write_raw
    header = b"BAM\x01" + (0).to_bytes(4, "little") + (1).to_bytes(4, "little") + (5).to_bytes(4, "little") + b"chr1\0" + (1000).to_bytes(4, "little")
    path, spill = str(tmp_path / "one.bam"), str(tmp_path / "one.runs.tmp")
    write_raw(header + raw_record(0, 5, 0, "r", 10), path)
    L = _lib.lib()

    def open_runs(req, spill_path=spill, chunk_blocks=0):
        h, ws = C.c_void_p(), C.c_int64(0)
        to = _lib.coral_bam_sink_t(_lib.SINK_RUNS, None if spill_path is None else os.fsencode(spill_path), None, 0, chunk_blocks)
        rc = L.coral_bamgpu_open_request(path.encode(), 1, 0, C.byref(req), to, C.byref(h), C.byref(ws))
        if h.value is not None:
            L.coral_bamgpu_close(h)
        return rc, L.coral_bam_last_error().decode()
    records = lambda **kw: _lib.bam_request(reads=(0, None, None, 2, 1), **kw)
    for req, kw, word in ((_lib.bam_request(reads=(0, None, None, 1)), {}, "want_reads"), (_lib.bam_request(), {}, "want_reads"),
                          (records(rank=1, world=2), {}, "world"), (records(), dict(spill_path=None), "spill path"),
                          (records(), dict(chunk_blocks=-1), "chunk_blocks"), (records(), dict(chunk_blocks=16385), "chunk_blocks"),
                          (records(), dict(spill_path=str(tmp_path / "no_such_dir" / "x.tmp")), "cannot create")):
        rc, msg = open_runs(req, **kw)
        assert rc == CORAL_ERR_ARG and word in msg, (word, rc, msg)
        assert not os.path.exists(spill)                         # nothing is created for a request that is refused


# ---- the command line and the Python argument rules -------------------------------------------------------------------------------
def test_sort_stream_parser():
    p = CoRAL.build_parser()
    a = p.parse_args(["sort", "--lr_bam", "x.bam", "--output", "o.bam"])
    assert a.stream is False and a.tmp_dir is None
    a = p.parse_args(["sort", "--lr_bam", "x.bam", "--output", "o.bam", "--stream", "--tmp_dir", "/scratch/here", "--index"])
    assert a.stream is True and a.tmp_dir == "/scratch/here" and a.index is True and a.level == 1
    with pytest.raises(ValueError, match="--level must be 1"):
        CoRAL.main(["sort", "--lr_bam", "no_such.bam", "--output", "o.bam", "--stream", "--level", "6"])
    with pytest.raises(ValueError, match="--stream"):
        CoRAL.main(["sort", "--lr_bam", "no_such.bam", "--output", "o.bam", "--tmp_dir", "."])


def test_python_argument_rules(tmp_path):
    missing, out = str(tmp_path / "no_such_file.bam"), str(tmp_path / "out.bam")      # (a rule that opened the file would not raise ValueError)
    with pytest.raises(ValueError, match="sort_bam"):
        bam.sort_bam_stream(missing, out, device="cpu")
    for kw in (dict(chunk_blocks=-1), dict(chunk_blocks=16385), dict(chunk_blocks=True), dict(chunk_blocks=1.5), dict(batch_bytes=-1), dict(batch_bytes="1"),
               dict(stage_bytes=-1), dict(stage_bytes=2.0), dict(stage_bytes=False), dict(stage_bytes=1 << 32), dict(exclude_flags=-1), dict(exclude_flags=0x10000),
               dict(tmp_dir=str(tmp_path / "no_such_dir")), dict(record_filter="x")):
        with pytest.raises((ValueError, TypeError)):
            bam.sort_bam_stream(missing, out, **kw)
    with pytest.raises(ValueError, match="level must be 1"):
        bam.sort_bam(missing, out, stream=True, level=6)
    with pytest.raises(ValueError, match="write_device"):
        bam.sort_bam(missing, out, stream=True, device="cuda:0", write_device="cuda:1")
    with pytest.raises(ValueError, match="sort_bam"):
        bam.sort_bam(missing, out, stream=True, device="cpu")
    assert not os.path.exists(out) and not os.path.exists(out + ".runs.tmp")
    assert bam.SortStats(1, 2, 3, 4, 5)._fields == ("records", "bytes", "file_bytes", "runs", "spill_bytes")
