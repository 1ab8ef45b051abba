"""The streamed coordinate sort (bam.sort_bam_stream, bam.sort_bam(stream=True), `sort --stream`; the CORAL_SINK_RUNS sink of coral_bamgpu_open_request,
coral_bamgpu_merge_runs): sorted runs spilled to disk while the file is decoded, merged on the GPU.

Every expected byte comes from tests/bamfile.parse, the selection rule restated in test_extract_records and Python's stable
`sorted` with the key restated in test_sort_records (want_sorted / sort_key); nothing expected has passed through either decoder.
The file is test_sort_records' shuffled one (build_stream): 140 records, 3.2 MB inflated, in source blocks of 1 500 bytes, three
to four runs at the smallest batch size.  The runs are restated from the run table's record counts alone: run r holds the next
n_r selected records of the file, sorted."""
import contextlib
import ctypes as C
import gzip
import os
import struct

import numpy as np
import pytest

from coral_amd import CoRAL, _lib, bam
from coral_amd.decode_session import Runs
from tests.bamfile import bgzf_blocks, parse, read_bam
from tests.decode_support import CORAL_ERR_ARG, CORAL_OK, _ok, assert_same_records, gpu_decode, gpu_open_only
from tests.test_extract_reads import write_raw
from tests.test_extract_records import EOF_BLOCK, SMALL_BATCH, SMALLEST, bytes_of, gunzip, selected
from tests.test_merge_plan import plan, smallest_stage
from tests.test_sort_records import FILTER, SELECTIONS, build_stream, passes, raw_record, sort_key, want_sorted

pytestmark = pytest.mark.gpu

BLOCK = 0xff00
GPU = "cuda:0"
CORAL_ERR_CAPACITY, CORAL_ERR_FORMAT = -3, -4
STREAMABLE = [k for k, kw in SELECTIONS.items() if set(kw) <= {"exclude_flags", "record_filter"}]      # (no regions, no names: sort_bam_stream takes neither)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("sort_stream")
    header, recs, _, _ = build_stream()
    raw = header + b"".join(recs)
    path = str(d / "shuffled.bam")
    write_raw(raw, path, block_size=1500, empty_block_every=5)
    parsed = read_bam(path)
    assert len(parsed.recs) == len(recs)
    c = dict(dir=d, raw=raw, path=path, parsed=parsed, header=header, sorted_header=bam.sorted_header_bytes(header))
    ref = str(d / "in_memory.bam")                               # the in-memory sort's file, made once
    bam.extract_records(path, device=GPU, n_threads=2, batch_bytes=SMALL_BATCH, index=False, order="coordinate").write(ref, device=GPU)
    with open(ref, "rb") as fp:
        c["in_memory"], c["in_memory_path"] = fp.read(), ref
    return c


def members_of(path):
    with open(path, "rb") as fp:
        raw = fp.read()
    return raw, [n for _, _, n in bgzf_blocks(raw)]


def assert_members(path, header_bytes, record_bytes):
    """The header in blocks of its own, the records cut at 0xff00 through their concatenation, the EOF block: every member full but
    the header's last, the records' last and the EOF block."""
    raw, sizes = members_of(path)
    cut = lambda n: [BLOCK] * (n // BLOCK) + ([n % BLOCK] if n % BLOCK else [])
    assert sizes == cut(header_bytes) + cut(record_bytes) + [0] and raw.endswith(EOF_BLOCK)
    return len(raw), len(sizes)


def file_order(case, exclude_flags=0, record_filter=None):
    kept = [r for r in case["parsed"].recs if passes(r, record_filter)]
    return selected(case, None, None, exclude_flags, recs=kept)


def restated_runs(case, counts, **sel):
    """counts: records per run (the run table) -> per run its records, sorted: the next n_r selected records of the file"""
    recs, runs, at = file_order(case, **sel), [], 0
    for n in counts:
        runs.append(sorted(recs[at:at + n], key=sort_key))
        at += n
    assert at == len(recs)
    return runs


def plan_inputs(runs):
    """restated runs -> (lens per run, final order as (run, ordinal in the run)): a stable sort of the run-major keys"""
    flat = [(sort_key(r), ri, k) for ri, run in enumerate(runs) for k, r in enumerate(run)]
    return [[r["size"] for r in run] for run in runs], [(ri, k) for _, ri, k in sorted(flat)]


# ---- the C ABI: phase 1 alone, and the merge on its handle ---------------------------------------------------------------------------
@contextlib.contextmanager
def runs_decode(path, spill, batch_bytes=SMALL_BATCH, chunk_blocks=0, exclude_flags=0, record_filter=None):
    """open_request with a runs sink, the batches and `finish`; yields the DecodeSession (L, h, stream, dev, dh) with the run table (rows of
    first record, records, inflated bytes, file offset) and counts (runs, records, spill bytes).  Closed on every way out."""
    with gpu_decode(path, 2, batch_bytes, Runs(spill, chunk_blocks), keep=record_filter, reads=(exclude_flags, None, None, 2)) as d:
        L, counts = d.L, (C.c_int64 * 3)()
        _ok(L, "run_table", L.coral_bamgpu_run_table(d.h, 0, None, counts))
        table = np.full((counts[0] + 1, 4), -1, dtype=np.int64)
        _ok(L, "run_table", L.coral_bamgpu_run_table(d.h, counts[0], table.ctypes.data, counts))
        assert table[-1].tolist() == [-1] * 4
        d.table, d.counts = table[:-1], [int(c) for c in counts]
        yield d


def merge_runs(d, out, header, stage_bytes=0):
    L = d.L
    need = int(L.coral_bamgpu_merge_workspace_bytes(d.h, stage_bytes))
    assert need > 0, L.coral_bam_last_error().decode()
    head = np.frombuffer(header, dtype=np.uint8)
    rc = L.coral_bamgpu_merge_runs(d.h, os.fsencode(out), head.ctypes.data, len(head), d.workspace(need), need, stage_bytes, d.stream)
    return rc, L.coral_bam_last_error().decode()


def run_counts(case, tmp_path, batch_bytes=SMALL_BATCH, **sel):
    with runs_decode(case["path"], str(tmp_path / "counts.runs.tmp"), batch_bytes, **sel) as d:
        return d.table[:, 1].tolist()


def stream_sort(case, out, **kw):
    kw.setdefault("batch_bytes", SMALL_BATCH)
    kw.setdefault("index", False)
    st = bam.sort_bam_stream(case["path"], out, device=GPU, n_threads=2, **kw)
    assert not os.path.exists(out + ".runs.tmp")                 # the spill file is gone
    return st


# ---- 1. content and member structure -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", STREAMABLE)
def test_content_and_members(case, what, tmp_path):
    kw = SELECTIONS[what]
    names, blobs = want_sorted(case, **kw)
    out = str(tmp_path / "out.bam")
    st = stream_sort(case, out, **kw)
    assert gunzip(out) == case["sorted_header"] + b"".join(blobs) and len(names) >= 8
    n_bytes = sum(len(b) for b in blobs)
    file_bytes, _ = assert_members(out, len(case["sorted_header"]), n_bytes)
    assert (st.records, st.bytes, st.file_bytes) == (len(blobs), n_bytes, file_bytes) and st.runs >= 3 and 0 < st.spill_bytes
    assert len(STREAMABLE) == 3


# ---- 2. byte identity with the in-memory sort, whatever the three sizes --------------------------------------------------------------
@pytest.mark.parametrize("chunk_blocks", [1, 3, 0])
@pytest.mark.parametrize("batch_bytes", [SMALL_BATCH, 0])
def test_byte_identity(case, batch_bytes, chunk_blocks, tmp_path):
    counts = run_counts(case, tmp_path, batch_bytes)
    assert (len(counts) >= 3) if batch_bytes else (len(counts) == 1)      # many runs, one run
    lens, order = plan_inputs(restated_runs(case, counts))
    low = smallest_stage(lens, order)
    total = sum(sum(l) for l in lens)
    about_three = max(low, total // 3 + BLOCK)
    assert plan(lens, order, low)[0] == CORAL_OK and plan(lens, order, low - 1)[0] == CORAL_ERR_CAPACITY and len(plan(lens, order, about_three)[1]) >= 2
    out = str(tmp_path / "out.bam")
    for stage_bytes in (low, about_three, 0):
        st = stream_sort(case, out, batch_bytes=batch_bytes, chunk_blocks=chunk_blocks, stage_bytes=stage_bytes)
        with open(out, "rb") as fp:
            assert fp.read() == case["in_memory"], (batch_bytes, chunk_blocks, stage_bytes)
        assert st.runs == len(counts) and bam.LAST_SORT_STREAM["steps"] == len(plan(lens, order, stage_bytes or 1 << 40)[1])
    os.remove(out)
    with pytest.raises(_lib.CoralHipError, match="CORAL_ERR_CAPACITY"):
        stream_sort(case, out, batch_bytes=batch_bytes, chunk_blocks=chunk_blocks, stage_bytes=low - 1)
    assert not os.path.exists(out) and not os.path.exists(out + ".runs.tmp")


# ---- 3. the merge's rules, with many runs ----------------------------------------------------------------------------------------------
def test_merge_rules(case, tmp_path):
    out = str(tmp_path / "out.bam")
    st = stream_sort(case, out)
    assert st.runs >= 3
    got = [r["name"] for r in read_bam(out).recs]
    by_name = {r["name"]: r for r in case["parsed"].recs}
    counts = run_counts(case, tmp_path)
    run_of = lambda name: next(i for i, run in enumerate(restated_runs(case, counts)) if any(r["name"] == name for r in run))
    at = got.index("tie_a")
    assert got[at:at + 3] == ["tie_a", "tie_b", "tie_c"] and len({run_of(n) for n in ("tie_a", "tie_b", "tie_c")}) >= 2      # file order across runs
    assert got.index("far_a") + 1 == got.index("far_b") and run_of("far_a") != run_of("far_b")
    assert got.index("fwd_second") < got.index("rev_first") and by_name["rev_first"]["start"] < by_name["fwd_second"]["start"]
    unplaced = [r for r in case["parsed"].recs if r["tid"] == -1]              # last, and in file order (one key: `sorted` keeps it)
    assert len(unplaced) >= 4 and got[-len(unplaced):] == [r["name"] for r in sorted(unplaced, key=sort_key)] and got[0] == "first_of_all"
    assert len({sort_key(r) for r in unplaced}) > 1 or got[-len(unplaced):] == [r["name"] for r in unplaced]
    # forward only: the third batch writes nothing - an empty run between two that write
    fwd = run_counts(case, tmp_path, exclude_flags=0x10)
    assert len(fwd) >= 4 and fwd[2] == 0 and fwd[1] > 0 and fwd[3] > 0
    st = stream_sort(case, out, exclude_flags=0x10)
    assert st.runs == len(fwd) and gunzip(out) == case["sorted_header"] + b"".join(want_sorted(case, exclude_flags=0x10)[1])


# ---- 4. the copy kernel's edges, on a file of its own ------------------------------------------------------------------------------------
def filler(target):
    """An unplaced record of exactly `target` bytes (37 + name + 1.5 l_seq)."""
    for name_len in (1, 2, 3, 4):
        for l_seq in range(0, target):
            size = 37 + name_len + (l_seq + 1) // 2 + l_seq
            if size == target:
                rec = raw_record(-1, -1, 4, "f" * name_len, l_seq)
                assert len(rec) == target
                return rec
            if size > target:
                break
    raise AssertionError(target)


def edge_records():
    recs = [raw_record(0, 0, 0, "a", 0)]                         # the smallest record, 38 bytes: the first of all, so the first of a step
    assert len(recs[0]) == SMALLEST
    recs.append(raw_record(0, 900, 0, "small_in_front", 100))
    recs.append(raw_record(0, 1000, 0, "long", 140_000))         # longer than three staging blocks, its source starts mid-block
    assert len(recs[-1]) > 3 * BLOCK
    for k in range(44):                                          # records of ~50 KB all over chr1 and chr2: 2.3 MB, three runs
        recs.append(raw_record(k % 2, (k * 7919) % 50_000, 0x10 if k % 3 == 0 else 0, "m%02d" % k, 33_000 + 17 * k))
    recs.append(raw_record(-1, -1, 4, "b", 0))
    recs.append(raw_record(1, 49_999, 0, "long_too", 131_073))
    recs.append(raw_record(-1, -1, 4, "c", 0))                   # the smallest record again: the last of all, so the last of a step
    return recs


@pytest.mark.parametrize("beyond", [-1, 0, 1])
def test_kernel_edges(case, beyond, tmp_path):
    recs = edge_records()
    base = sum(len(r) for r in recs)
    k = (base + 200) // BLOCK + 1
    recs.insert(20, filler(k * BLOCK + beyond - base))           # the records' bytes: exactly k blocks, and one byte either side
    total = sum(len(r) for r in recs)
    assert total == k * BLOCK + beyond
    path, out = str(tmp_path / "edges.bam"), str(tmp_path / "out.bam")
    raw = case["header"] + b"".join(recs)
    write_raw(raw, path, block_size=1500, empty_block_every=7)
    own = dict(parsed=parse(raw), raw=raw, path=path)
    counts = run_counts(own, tmp_path)
    runs = restated_runs(own, counts)
    lens, order = plan_inputs(runs)
    low = smallest_stage(lens, order)
    steps = plan(lens, order, low)[1]
    sizes = [[runs[ri][ki]["size"] for ri, ki in order[j0:j1]] for j0, j1, _ in steps]
    pos = {(ri, ki): sum(lens[ri][:ki]) for ri, ki in order}
    long_at = next((ri, ki) for ri, ki in order if runs[ri][ki]["name"] == "long")
    assert len(counts) >= 3 and pos[long_at] % BLOCK != 0
    assert any(len(parts) == 1 for _, _, parts in steps)                                    # a step in which all but one run contribute nothing
    assert any(s[0] == SMALLEST for s in sizes) and any(s[-1] == SMALLEST for s in sizes)  # the smallest record first and last of a step
    want = case["sorted_header"] + b"".join(want_sorted(own)[1])
    for stage_bytes in (low, 0):
        st = bam.sort_bam_stream(path, out, index=False, device=GPU, n_threads=2, batch_bytes=SMALL_BATCH, stage_bytes=stage_bytes)
        assert gunzip(out) == want and (st.records, st.bytes) == (len(recs), total)
        assert_members(out, len(case["sorted_header"]), total)
        if stage_bytes:                                          # step boundaries inside source blocks: those blocks are inflated again
            assert bam.LAST_SORT_STREAM["steps"] == len(steps) and bam.LAST_SORT_STREAM["edge_members_inflated_twice"] > 0


# ---- 5. empty and single -----------------------------------------------------------------------------------------------------------------
def test_nothing_one_record_and_a_sorted_source(case, tmp_path):
    out = str(tmp_path / "out.bam")
    st = stream_sort(case, out, record_filter=bam.RecordFilter(min_mapq=255))
    assert gunzip(out) == case["sorted_header"] and assert_members(out, len(case["sorted_header"]), 0)[0] == st.file_bytes
    assert (st.records, st.bytes, st.spill_bytes) == (0, 0, 0) and st.runs >= 3      # empty runs only
    empty, one = str(tmp_path / "header_only.bam"), str(tmp_path / "one.bam")
    write_raw(case["header"], empty)
    st = bam.sort_bam_stream(empty, out, index=False, device=GPU)
    assert gunzip(out) == case["sorted_header"] and st.records == 0 and st.runs <= 1
    record = raw_record(3, 77, 0x10, "only", 19)
    write_raw(case["header"] + record, one)
    st = bam.sort_bam_stream(one, out, index=False, device=GPU)
    assert gunzip(out) == case["sorted_header"] + record and (st.records, st.bytes, st.runs) == (1, len(record), 1)
    # a source already sorted: view_bam's records under the sorted header
    srt, viewed = str(tmp_path / "sorted.bam"), str(tmp_path / "viewed.bam")
    write_raw(case["header"] + b"".join(want_sorted(case)[1]), srt, block_size=1500, empty_block_every=5)
    bam.view_bam(srt, viewed, device=GPU, batch_bytes=SMALL_BATCH)
    bam.sort_bam_stream(srt, out, index=False, device=GPU, batch_bytes=SMALL_BATCH)
    assert gunzip(out) == case["sorted_header"] + gunzip(viewed)[len(case["header"]):]


# ---- 6. the spill file's contract, at the C ABI --------------------------------------------------------------------------------------------
def records_in(blob):
    out, at = [], 0
    while at < len(blob):
        n = 4 + struct.unpack_from("<i", blob, at)[0]
        out.append(blob[at:at + n])
        at += n
    assert at == len(blob)
    return out


@pytest.mark.parametrize("sel", [dict(), dict(exclude_flags=0x10, record_filter=FILTER)])
def test_spill_contract(case, sel, tmp_path):
    spill = str(tmp_path / "x.runs.tmp")
    with runs_decode(case["path"], spill, chunk_blocks=3, **sel) as d:
        with open(spill, "rb") as fp:
            raw = fp.read()
        data = gzip.decompress(raw) if raw else b""
        runs = restated_runs(case, d.table[:, 1].tolist(), **sel)
        assert d.counts == [len(runs), sum(len(r) for r in runs), len(raw)] and len(runs) >= 3
        blocks = list(bgzf_blocks(raw))
        at = first = 0
        for (f, n, nbytes, off), run in zip(d.table.tolist(), runs):
            got = records_in(data[at:at + nbytes])
            assert got == [bytes_of(case, r) for r in run] and f == first and n == len(run)      # ascending by key, stable
            mine = [b for b in blocks if at <= b[1] < at + nbytes]                            # whole members, all full but the last
            assert [b[2] for b in mine] == [BLOCK] * (nbytes // BLOCK) + ([nbytes % BLOCK] if nbytes % BLOCK else [])
            assert (mine[0][0] if mine else off) == off
            at, first = at + nbytes, first + n
        assert at == len(data) and len(blocks) == sum(-(-int(b) // BLOCK) for b in d.table[:, 2])
        assert sorted(records_in(data)) == sorted(bytes_of(case, r) for r in file_order(case, **sel))      # the selection as a multiset
        sz = (C.c_int64 * 2)()
        assert d.L.coral_bam_reads_sizes(d.dh, sz) == CORAL_OK and list(sz) == [d.counts[1], len(data)]
        assert d.L.coral_bam_reads_fill(d.dh, None, (C.c_int64 * (d.counts[1] + 1))()) == CORAL_ERR_ARG
        out = str(tmp_path / "out.bam")
        rc, msg = merge_runs(d, out, case["sorted_header"], stage_bytes=1000)      # too small for any record: refused, nothing created ...
        assert rc == CORAL_ERR_CAPACITY and "stage_bytes" in msg and not os.path.exists(out)
        rc, msg = merge_runs(d, out, case["sorted_header"])                        # ... and answered with a larger stage
        assert rc == CORAL_OK, msg
        assert gunzip(out) == case["sorted_header"] + b"".join(want_sorted(case, **sel)[1])


@pytest.mark.parametrize("damage", ["truncated", "flipped"])
def test_a_damaged_spill_is_refused(case, damage, tmp_path):
    spill, out = str(tmp_path / "x.runs.tmp"), str(tmp_path / "out.bam")
    with runs_decode(case["path"], spill) as d:
        with open(spill, "rb") as fp:
            raw = bytearray(fp.read())
        if damage == "truncated":
            raw = raw[:-9]
        else:                                                    # a byte inside the DEFLATE stream of the second run's first member
            raw[int(d.table[1][3]) + 18 + 40] ^= 0x55
        with open(spill, "wb") as fp:
            fp.write(raw)
        rc, msg = merge_runs(d, out, case["sorted_header"])
        assert rc == CORAL_ERR_FORMAT and "spill" in msg, (rc, msg)
        assert not os.path.exists(out)


# ---- 7. nothing else moved ---------------------------------------------------------------------------------------------------------------
def test_the_other_entry_points_carve_what_they_carved(case, tmp_path):
    L = _lib.lib()
    path = case["path"].encode()

    def sizes():
        got = {}
        head = C.cast(C.c_char_p(b"BAM\x01"), C.c_void_p)
        h, ws = C.c_void_p(), C.c_int64(0)
        got["plain"] = gpu_open_only(case["path"], reads=(0, None, None, 2))[2]
        for name, order, to in (("ordered", 1, None),
                                ("to_file", 0, _lib.coral_bam_sink_t(_lib.SINK_BAM, os.fsencode(str(tmp_path / "f.bam")), head, 4, 5)),
                                ("to_runs", 1, _lib.coral_bam_sink_t(_lib.SINK_RUNS, os.fsencode(str(tmp_path / "r.tmp")), None, 0, 5))):
            req = _lib.bam_request(reads=(0, None, None, 2, order))
            assert L.coral_bamgpu_open_request(path, 1, 0, C.byref(req), to, C.byref(h), C.byref(ws)) == CORAL_OK, L.coral_bam_last_error().decode()
            L.coral_bamgpu_close(h)
            got[name] = ws.value
        return got
    a = sizes()
    assert a["plain"] < a["ordered"] < a["to_runs"] and a["plain"] < a["to_file"]
    # a spill request is an ordered request with a sink: the sort arrays of the one, the sink's arrays of the other, nothing more
    assert a["to_runs"] - a["ordered"] == a["to_file"] - a["plain"]
    assert sizes() == a


# ---- 8. round trip ------------------------------------------------------------------------------------------------------------------------
def test_round_trip_and_command_line(case, tmp_path):
    out, cli = str(tmp_path / "out.bam"), str(tmp_path / "cli.bam")
    os.mkdir(str(tmp_path / "spills"))
    st = bam.sort_bam_stream(case["path"], out, device=GPU, n_threads=2, batch_bytes=SMALL_BATCH, tmp_dir=str(tmp_path / "spills"))
    assert os.path.exists(out + ".bai") and os.listdir(str(tmp_path / "spills")) == [] and st.records == len(case["parsed"].recs)
    bam.build_index(case["in_memory_path"], device="cpu")
    regions = [("chr8", 49_990, 60_010), ("chr3", 1000, 2000)]
    got = bam.load_bam(out, device=GPU, regions=regions)
    want = bam.load_bam(case["in_memory_path"], device=GPU, regions=regions)
    assert_same_records(got, want)
    assert got.n > 4
    assert CoRAL.main(["sort", "--lr_bam", case["path"], "--output", cli, "--stream", "--index", "--tmp_dir", str(tmp_path / "spills")]) == cli
    for suffix in ("", ".bai"):
        with open(out + suffix, "rb") as a, open(cli + suffix, "rb") as b:
            assert a.read() == b.read(), suffix
    assert bam.sort_bam(case["path"], cli, stream=True, index=False, batch_bytes=SMALL_BATCH, device=GPU, write_device=GPU) == cli
    with open(cli, "rb") as fp:
        assert fp.read() == case["in_memory"]
