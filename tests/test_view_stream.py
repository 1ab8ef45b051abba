"""bam.view_bam / the CORAL_SINK_BAM sink of coral_bamgpu_open_request: the selected records of a BAM file streamed to a BAM file while the decode
runs, each batch's records deflated on the device.  Expected bytes are restated from the parsed fixture (tests/bamfile.py, the
rule of tests/test_extract_records.py) and checked through gzip.decompress - which checks every member's CRC -, never taken from
the code under test; the byte-identity partner is extract_records(...).write(device=gpu), the in-memory path."""
import ctypes as C
import gzip
import os
import shutil
import struct

import numpy as np
import pytest
import torch  # noqa: F401

from coral_amd import CoRAL, _lib, bam, synth
from coral_amd.decode_session import BamFile, TextFile, open_handle
from tests.bamfile import bgzf_blocks, parse, read_bam
from tests.decode_support import CORAL_ERR_ARG, CORAL_OK, _ok, _pipeline_by_device, assert_same_records, gpu_decode_started  # noqa: F401
from tests.test_extract_reads import fastq_of, patch_codes, qual_of, write_raw
from tests.test_extract_records import EOF_BLOCK, REGIONS, SMALL_BATCH, SMALLEST, edge_record, more_alignments, want_records

BLOCK = 0xFF00
MIB = 1 << 20
GPU = "cuda:0"
# sizes of the records the carry corners are built from: alone or in pairs they total 0xff00 - 1, 0xff00, 0xff00 + 1, 2 * 0xff00
CORNER_SIZES = (BLOCK - 1, BLOCK, BLOCK + 1, BLOCK - SMALLEST)
WIDE = 3 * BLOCK + 16                                  # one record over four output blocks (1 mod 3: edge_record gives its 7-character
                                                       # name 7 bytes)
FILLER_SIZES = tuple(60_000 + 1_001 * k for k in range(16))
SMALL_SIZES = tuple(100 + 13 * k for k in range(6))


def stream_alignments():
    """more_alignments() with, on chr8 in front of its last record there, about 1.5 MiB more: the corner records, one wide
    record, fillers, and a small record behind every third filler - three batches of 1 MiB."""
    alns = more_alignments()
    at = [k for k, a in enumerate(alns) if a.get("name") == "chim" and a["tid"] == 7][0]
    sizes = list(CORNER_SIZES) + [WIDE]
    small = list(SMALL_SIZES)
    for k, size in enumerate(FILLER_SIZES):
        sizes.append(size)
        if k % 3 == 2 and small:
            sizes.append(small.pop(0))
    sizes += small
    extra = [edge_record(size, 100_000 + 10 * k) for k, size in enumerate(sizes)]
    return alns[:at] + extra + alns[at:]


def name_of_size(size):
    return edge_record(size, 0)["name"]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("view_stream")
    rec = synth.records_from_alignments(stream_alignments())
    names = rec.materialise_names()
    name_of = lambda i: names[int(rec.name_id[i])]
    l_seq = lambda i: int(rec.qlen[i]) if int(rec.has_seq[i]) else 0
    first = str(d / "first.bam")
    bam.write_bam(rec, first, seed=11, fast_seq=True, qual=lambda i: qual_of(name_of(i), l_seq(i)),
                  nm_type=lambda i: None if name_of(i) == "z" else "i")
    with gzip.open(first, "rb") as fp:
        raw = fp.read()
    raw = patch_codes(raw, parse(raw))
    path = str(d / "records.bam")
    write_raw(raw, path, block_size=1500, empty_block_every=5)
    parsed = read_bam(path)
    assert len(parsed.recs) == rec.n and parsed.n_bytes == len(raw)
    assert 2 * MIB + MIB // 4 < len(raw) < 3 * MIB               # three batches of 1 MiB, the last one not a sliver
    by_size = {}
    for r in parsed.recs:
        by_size.setdefault(r["size"], []).append(r["name"])
    for size in CORNER_SIZES + (WIDE,) + FILLER_SIZES + SMALL_SIZES:
        assert by_size[size].count(name_of_size(size)) == 1, size      # the sizes are met, by the records named after them
    assert by_size[SMALLEST] == ["z"]
    count = {}
    for r in parsed.recs:
        count[r["name"]] = count.get(r["name"], 0) + 1
    return dict(dir=d, raw=raw, path=path, parsed=parsed, header=raw[:parsed.recs[0]["start"]], count=count, memo={})


def view(case, out, *args, **kw):
    kw.setdefault("batch_bytes", SMALL_BATCH)
    kw.setdefault("bam_index", False)
    st = bam.view_bam(case["path"], str(out), *args, device=GPU, n_threads=2, **kw)
    return st, read_file(out)


def read_file(path):
    with open(str(path), "rb") as fp:
        return fp.read()


def members(raw):
    """[(file offset, member length, inflated length)] of the file's BGZF members, BSIZE checked against where the next begins."""
    blocks = list(bgzf_blocks(raw))
    out = []
    for (at, _, n), nxt in zip(blocks, [b[0] for b in blocks[1:]] + [len(raw)]):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04" and raw[at + 12:at + 16] == b"BC\x02\x00"
        assert struct.unpack_from("<H", raw, at + 16)[0] + 1 == nxt - at
        out.append((at, nxt - at, n))
    return out


def assert_structure(case, raw, payload_bytes, file_bytes):
    """The header part ends a member; every member of the records part holds 0xff00 bytes but possibly its last; no empty member
    but the EOF block, which is last; the members' lengths sum to the file's size."""
    mem = members(raw)
    n_head = -(-len(case["header"]) // BLOCK)
    sizes = [n for _, _, n in mem]
    assert sizes[:n_head] == [BLOCK] * (n_head - 1) + [len(case["header"]) - (n_head - 1) * BLOCK]
    body = sizes[n_head:-1]
    assert body == [BLOCK] * (payload_bytes // BLOCK) + ([payload_bytes % BLOCK] if payload_bytes % BLOCK else [])
    assert sizes[-1] == 0 and raw[-28:] == EOF_BLOCK and 0 not in sizes[:-1]
    assert sum(m for _, m, _ in mem) == len(raw) == file_bytes
    return mem


def in_memory(case, tmp_path, key, *args, **kw):
    """The in-memory path's file for a selection (made once per selection)."""
    if key not in case["memo"]:
        p = str(case["dir"] / ("mem_%d.bam" % len(case["memo"])))
        bam.extract_records(case["path"], *args, device=GPU, n_threads=2, batch_bytes=SMALL_BATCH, index=False, **kw).write(p, device=GPU)
        case["memo"][key] = read_file(p)
    return case["memo"][key]


# ---- 1. the inflated content ---------------------------------------------------------------------------------------------------
SELECTIONS = {
    "everything": dict(),
    "regions": dict(regions=REGIONS),
    "regions, 0x900 excluded": dict(regions=REGIONS, exclude_flags=0x900),
    "names": dict(names=["r1", "chim", "huge", "noseq", "z", "not_there", name_of_size(BLOCK), name_of_size(FILLER_SIZES[7])]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(SELECTIONS))
def test_inflated_content_and_member_structure(case, tmp_path, which):
    kw = SELECTIONS[which]
    st, raw = view(case, tmp_path / "out.bam", **kw)
    assert bam.LAST_DECODE["where"] == "gpu" and bam.LAST_DECODE["batches"] == 3
    names, blobs = want_records(case, kw.get("regions"), set(kw["names"]) if "names" in kw else None, kw.get("exclude_flags", 0))
    payload = b"".join(blobs)
    assert len(blobs) > 3 and gzip.decompress(raw) == case["header"] + payload
    assert st == bam.ViewStats(len(blobs), len(payload), len(raw))
    assert_structure(case, raw, len(payload), st.file_bytes)


@pytest.mark.gpu
def test_record_filter_acts_first(case, tmp_path):
    st, raw = view(case, tmp_path / "out.bam", REGIONS, record_filter=bam.RecordFilter(min_mapq=5, min_seq_length=30))
    kept = [r for r in case["parsed"].recs if r["mapq"] >= 5 and r["l_seq"] >= 30]
    names, blobs = want_records(case, REGIONS, None, 0, recs=kept)
    assert 3 < len(blobs) < len(want_records(case, REGIONS)[1])
    assert gzip.decompress(raw) == case["header"] + b"".join(blobs) and st.records == len(blobs)


# ---- 3. byte identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_byte_identical_to_the_in_memory_path_whatever_the_batches_and_chunks(case, tmp_path):
    want = in_memory(case, tmp_path, "everything")
    assert gzip.decompress(want) == case["raw"]
    batches = set()
    for batch_bytes, chunk_blocks in ((MIB, 1), (MIB, 3), (MIB, 0), (2 * MIB, 1), (2 * MIB, 0), (0, 3), (0, 0), (MIB, 0)):
        st, raw = view(case, tmp_path / "out.bam", batch_bytes=batch_bytes, chunk_blocks=chunk_blocks)
        batches.add(bam.LAST_DECODE["batches"])
        assert raw == want, (batch_bytes, chunk_blocks, len(raw), len(want))
    assert {3, 1} <= batches                                     # (a batch is also bounded by its compressed bytes: 2 MiB may still be three)
    sel = dict(regions=REGIONS + [("chr8", 10_000, 31_000)], exclude_flags=0x400)
    assert view(case, tmp_path / "out.bam", **sel)[1] == in_memory(case, tmp_path, "regions", sel["regions"], None, 0x400)


# ---- 4. the carry's corners ----------------------------------------------------------------------------------------------------
CORNERS = {
    BLOCK - 1: [BLOCK - 1],
    BLOCK: [BLOCK],
    BLOCK + 1: [BLOCK + 1],
    2 * BLOCK: [BLOCK - 1, BLOCK + 1],
}


@pytest.mark.gpu
@pytest.mark.parametrize("total", sorted(CORNERS))
def test_selections_that_end_at_a_block_boundary_or_one_byte_off(case, tmp_path, total):
    names = {name_of_size(s) for s in CORNERS[total]}
    got_names, blobs = want_records(case, None, names)
    assert sum(len(b) for b in blobs) == total and len(blobs) == len(names)      # the case is met on the parsed file
    st, raw = view(case, tmp_path / "out.bam", names=sorted(names))
    assert gzip.decompress(raw) == case["header"] + b"".join(blobs) and st.bytes == total
    mem = assert_structure(case, raw, total, st.file_bytes)
    assert len(mem) == 1 + -(-total // BLOCK) + 1                # an exact multiple leaves no tail member
    assert raw == in_memory(case, tmp_path, ("corner", total), None, sorted(names))


@pytest.mark.gpu
def test_the_smallest_record_fills_a_block_to_the_byte(case, tmp_path):
    names = {"z", name_of_size(BLOCK - SMALLEST)}
    got_names, blobs = want_records(case, None, names)
    assert sorted(len(b) for b in blobs) == [SMALLEST, BLOCK - SMALLEST]
    st, raw = view(case, tmp_path / "out.bam", names=sorted(names))
    assert gzip.decompress(raw) == case["header"] + b"".join(blobs)
    assert [n for _, _, n in assert_structure(case, raw, BLOCK, st.file_bytes)][-2:] == [BLOCK, 0]
    st, raw = view(case, tmp_path / "out.bam", names=["z"])      # and alone: one member of 38 bytes
    assert st[:2] == (1, SMALLEST) and gzip.decompress(raw)[len(case["header"]):] == blobs[got_names.index("z")]


def ends_in(case, names):
    """Where each selected record ends in the inflated stream (a record belongs to the batch it ends in)."""
    return sorted(r["start"] + r["size"] for r in case["parsed"].recs if r["name"] in names)


@pytest.mark.gpu
def test_a_batch_that_writes_nothing_between_two_that_write_and_batches_below_one_block(case, tmp_path):
    recs, once = case["parsed"].recs, lambda r: case["count"][r["name"]] == 1
    early = [r["name"] for r in recs if once(r) and r["start"] + r["size"] < MIB - 100_000 and r["size"] < 2_000][:3]
    late = [r["name"] for r in recs if once(r) and r["start"] > 2 * MIB + 200_000 and r["size"] < 2_000][:2]
    late_big = [r["name"] for r in recs if once(r) and r["start"] > 2 * MIB + 200_000 and r["size"] > BLOCK // 2][:2]
    middle = [r["name"] for r in recs if once(r) and MIB + 200_000 < r["start"] and r["start"] + r["size"] < 2 * MIB - 200_000 and r["size"] < 2_000][:1]
    assert len(early) == 3 and len(late) == 2 and len(late_big) == 2 and len(middle) == 1
    # (a) the first and the last batch write, the middle one nothing: the carry (less than a block) survives it
    names = set(early + late_big)
    ends = ends_in(case, names)
    assert not [e for e in ends if MIB - 100_000 <= e <= 2 * MIB + 200_000] and ends[0] < MIB < 2 * MIB < ends[-1]
    got_names, blobs = want_records(case, None, names)
    assert 0 < sum(len(b) for b in blobs[:3]) < BLOCK < sum(len(b) for b in blobs)
    st, raw = view(case, tmp_path / "out.bam", names=sorted(names))
    assert bam.LAST_DECODE["batches"] == 3 and gzip.decompress(raw) == case["header"] + b"".join(blobs)
    assert_structure(case, raw, st.bytes, st.file_bytes)
    # (b) every batch writes less than one block, all three together too: no member until `finish`, the carry grows
    names = set(early + middle + late)
    got_names, blobs = want_records(case, None, names)
    assert len(blobs) == 6 and sum(len(b) for b in blobs) < BLOCK
    st, raw = view(case, tmp_path / "out.bam", names=sorted(names))
    assert gzip.decompress(raw) == case["header"] + b"".join(blobs)
    assert len(assert_structure(case, raw, st.bytes, st.file_bytes)) == 3


@pytest.mark.gpu
def test_a_record_over_several_blocks_and_the_batch_boundary(case, tmp_path):
    by_name = {r["name"]: r for r in case["parsed"].recs}
    huge, wide = by_name["huge"], by_name[name_of_size(WIDE)]
    assert huge["start"] < MIB - 20_000 and huge["start"] + huge["size"] > MIB + 20_000 and huge["size"] > 2 * BLOCK
    assert wide["size"] == WIDE
    for names in (["huge"], ["huge", wide["name"], "z"]):
        got_names, blobs = want_records(case, None, set(names))
        st, raw = view(case, tmp_path / "out.bam", names=names)
        assert gzip.decompress(raw) == case["header"] + b"".join(blobs) and st.records == len(names)
        assert_structure(case, raw, st.bytes, st.file_bytes)


# ---- 5. empty selections -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_empty_selections_write_header_and_eof(case, tmp_path):
    st, raw = view(case, tmp_path / "none.bam", names=["not_in_the_file"])
    assert st[:2] == (0, 0) and bam.LAST_DECODE["batches"] == 3 and gzip.decompress(raw) == case["header"]
    assert [n for _, _, n in assert_structure(case, raw, 0, st.file_bytes)] == [len(case["header"]), 0]
    bam.LAST_DECODE.clear()
    for kw in (dict(names=[]), dict(regions=[])):
        st2, raw2 = view(case, tmp_path / "empty.bam", **kw)
        assert raw2 == raw and st2 == st and not bam.LAST_DECODE   # the same file, without a decode
    assert read_bam(str(tmp_path / "empty.bam")).recs == []


# ---- 6. the index and the way back ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_index_and_round_trip(case, tmp_path):
    out, mem = str(tmp_path / "out.bam"), str(tmp_path / "mem.bam")
    st, raw = view(case, out, exclude_flags=0x400, index=True)
    bam.extract_records(case["path"], None, None, 0x400, device=GPU, batch_bytes=SMALL_BATCH).write(mem, device=GPU)
    bam.build_index(mem, device="cpu")
    assert read_file(out + ".bai") == read_file(mem + ".bai") and raw == read_file(mem)
    idx = bam.read_index(out + ".bai")
    first = min(int(c[0][0]) for b in idx.bins for c in b.values())
    assert first & 0xFFFF == 0 and first >> 16 > 0               # the header ends a block
    region = [("chr8", 100_000, 100_200)]
    got = bam.extract_records(out, region, device="cpu", index=idx)
    names, blobs = want_records(case, region, None, 0x400)
    assert got.names() == names and got.data.tobytes() == b"".join(blobs) and len(blobs) > 5
    assert_same_records(bam.load_bam(out, device="cpu"), bam.load_bam(mem, device="cpu"))


# ---- 7. span decode ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_an_index_beside_the_source_cuts_the_decode_down_to_the_regions(case, tmp_path):
    src = str(tmp_path / "src.bam")
    shutil.copyfile(case["path"], src)
    bam.build_index(src, device="cpu")
    whole, raw = view_of(src, tmp_path / "whole.bam", REGIONS, bam_index=False)
    blocks_whole = bam.LAST_DECODE["blocks"]
    spans, raw2 = view_of(src, tmp_path / "spans.bam", REGIONS, bam_index=None)
    assert 0 < bam.LAST_DECODE["blocks"] < blocks_whole and bam.LAST_DECODE["index"] == src + ".bai"
    assert raw2 == raw and spans == whole
    assert gzip.decompress(raw2) == case["header"] + b"".join(want_records(case, REGIONS)[1])


def view_of(src, out, *args, **kw):
    st = bam.view_bam(src, str(out), *args, device=GPU, n_threads=2, batch_bytes=SMALL_BATCH, **kw)
    return st, read_file(out)


# ---- 8. nothing is kept on the host (the C ABI) ----------------------------------------------------------------------------------
def open_bam_sink(path, out_path, header, chunk_blocks=0, batch_bytes=SMALL_BATCH, **request):
    """coral_bamgpu_open_request with a BAM sink alone -> (rc, handle, ws_bytes, message, the request - it owns the arrays)."""
    L, req = _lib.lib(), _lib.bam_request(**request)
    rc, h, ws_bytes = open_handle(L, path, 2, batch_bytes, req, BamFile(out_path, header, chunk_blocks))
    return rc, h, ws_bytes, L.coral_bam_last_error().decode(), req


@pytest.mark.gpu
def test_the_c_abi_keeps_nothing_on_the_host(case, tmp_path):
    L, out = _lib.lib(), str(tmp_path / "abi.bam")
    names = sorted({"huge", "z", name_of_size(BLOCK + 1)})
    with gpu_decode_started(case["path"], 2, SMALL_BATCH, BamFile(out, case["header"], 2), reads=(0, None, [n.encode() for n in names], 2)) as d:
        d.run()
        assert read_file(out)[-28:] != EOF_BLOCK                 # not before `finish`
        dh, h = d.finish(), d.h
        blobs = want_records(case, None, set(names))[1]
        sz, stats = (C.c_int64 * 2)(), (C.c_int64 * 4)()
        _ok(L, "reads_sizes", L.coral_bam_reads_sizes(dh, sz))
        assert list(sz) == [3, sum(len(b) for b in blobs)]
        text, off = np.zeros(int(sz[1]), dtype=np.uint8), np.zeros(int(sz[0]) + 1, dtype=np.int64)
        assert L.coral_bam_reads_fill(dh, text.ctypes.data, off.ctypes.data) == CORAL_ERR_ARG and "file" in L.coral_bam_last_error().decode()
        _ok(L, "sink_stats", L.coral_bamgpu_sink_stats(h, stats))
        raw = read_file(out)
        assert list(stats) == [3, int(sz[1]), len(raw), len(members(raw))]
        assert gzip.decompress(raw) == case["header"] + b"".join(blobs)


# ---- 9. refusals at open (no GPU work) -------------------------------------------------------------------------------------------
def test_open_refuses(case, tmp_path):
    L, out = _lib.lib(), str(tmp_path / "refused.bam")
    records = (0, None, None, 2)
    bad = {
        "want_reads = 0": (dict(), {}, "want_reads"),
        "want_reads = 1": (dict(reads=(0, None, None, 1)), {}, "want_reads"),
        "with an index request": (dict(reads=records, index=True), {}, "want_reads"),
        "coordinate order": (dict(reads=records + (1,)), {}, "reads_order"),
        "a byte range": (dict(reads=records, rank=0, world=2), {}, "world"),
        "chunk_blocks = -1": (dict(reads=records), dict(chunk_blocks=-1), "chunk_blocks"),
        "chunk_blocks = 16 385": (dict(reads=records), dict(chunk_blocks=16385), "chunk_blocks"),
        "no header": (dict(reads=records), dict(header=None), "header"),
        "no output path": (dict(reads=records), dict(out_path=None), "path"),
        "a path that cannot be created": (dict(reads=records), dict(out_path=str(tmp_path / "no_such_dir" / "x.bam")), "cannot create"),
    }
    for name, (request, args, word) in bad.items():
        a = dict(out_path=out, header=case["header"])
        a.update(args)
        rc, h, ws_bytes, message, keep = open_bam_sink(case["path"], a["out_path"], a["header"], a.get("chunk_blocks", 0), **request)
        assert rc == CORAL_ERR_ARG and h.value is None and ws_bytes == 0, name
        assert word in message, (name, message)
        assert not os.path.exists(out), name                     # nothing is created for a request that is refused
    stats = (C.c_int64 * 4)()
    assert L.coral_bamgpu_sink_stats(None, stats) == CORAL_ERR_ARG


def test_a_request_without_a_sink_carves_what_it_carved(case, tmp_path):
    """The sink's arrays are part of the workspace only for a sink request (NULL and CORAL_SINK_HOST are the same: no sink)."""
    L = _lib.lib()
    req, h, plain = _lib.bam_request(reads=(0, None, None, 2)), C.c_void_p(), C.c_int64(0)
    assert L.coral_bamgpu_open_request(case["path"].encode(), 1, SMALL_BATCH, C.byref(req), None, C.byref(h), C.byref(plain)) == CORAL_OK
    stats = (C.c_int64 * 4)()
    assert L.coral_bamgpu_sink_stats(h, stats) == CORAL_ERR_ARG and "no file" in L.coral_bam_last_error().decode()
    L.coral_bamgpu_close(h)
    sizes = {}
    for chunk in (1, 8):
        rc, h, ws_bytes, message, keep = open_bam_sink(case["path"], str(tmp_path / "x.bam"), case["header"], chunk, reads=(0, None, None, 2))
        assert rc == CORAL_OK, message
        L.coral_bamgpu_close(h)
        sizes[chunk] = ws_bytes
    # per block of a chunk: a slot, its packed bytes, 4 bytes per input byte of tokens, a descriptor, a length, an offset
    per_block = 2 * 65536 + 4 * BLOCK + 16 + 4 + 4
    assert plain.value + BLOCK + per_block <= sizes[1] < sizes[8] and abs((sizes[8] - sizes[1]) - 7 * per_block) <= 8 * 256
    assert read_file(tmp_path / "x.bam") == b""                  # closed without a decode: no EOF block, a truncated file


# ---- 10. the command line ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_view_stream_on_the_command_line(case, tmp_path):
    out, names_file = str(tmp_path / "cli.bam"), str(tmp_path / "names.txt")
    with open(names_file, "w") as fp:
        fp.write("r1\nhuge\nz\nnot_there\n")
    argv = ["view", "--lr_bam", case["path"], "--output", out, "--names_file", names_file, "--reads_exclude_flags", "0x10", "--filter_min_mapq", "1"]
    assert CoRAL.main(argv + ["--stream", "--device", "cpu"]) == out
    streamed = read_file(out)
    flt = bam.RecordFilter(min_mapq=1)
    st = bam.view_bam(case["path"], str(tmp_path / "api.bam"), None, ["r1", "huge", "z", "not_there"], 0x10, record_filter=flt)
    assert streamed == read_file(tmp_path / "api.bam") and st.records > 0
    assert CoRAL.main(argv + ["--device", "cpu"]) == out         # without --stream: what it wrote before
    rec = bam.extract_records(case["path"], None, ["r1", "huge", "z", "not_there"], 0x10, device="cpu", record_filter=flt)
    rec.write(str(tmp_path / "before.bam"))
    assert read_file(out) == read_file(tmp_path / "before.bam") and gzip.decompress(streamed) == gzip.decompress(read_file(out))
    with pytest.raises(ValueError):
        CoRAL.main(argv + ["--stream", "--level", "5"])


# ---- 11. the same sink for FASTQ text --------------------------------------------------------------------------------------------
def want_fastq(case, names=None, exclude_flags=0x900):
    recs = [r for r in case["parsed"].recs if r["l_seq"] > 0 and not r["flag"] & exclude_flags and (names is None or r["name"] in names)]
    return recs, b"".join(fastq_of(r) for r in recs)


@pytest.mark.gpu
@pytest.mark.parametrize("batch_bytes", [MIB, 2 * MIB, 0])
def test_fastq_text_goes_to_the_file_batch_by_batch(case, tmp_path, batch_bytes):
    out, mem = str(tmp_path / "out.fastq"), str(tmp_path / "mem.fastq")
    recs, text = want_fastq(case)
    assert any(r["flag"] & 0x10 for r in recs) and any(r["qual"][0] == 0xFF for r in recs) and len(recs) > 100      # reverse strand, no QUAL
    got = bam.extract_reads(case["path"], device=GPU, n_threads=2, batch_bytes=batch_bytes, index=False, output=out)
    assert bam.LAST_DECODE["batches"] == {MIB: 3, 2 * MIB: 2, 0: 1}[batch_bytes]
    assert got == (len(recs), len(text)) and read_file(out) == text
    bam.extract_reads(case["path"], device=GPU, n_threads=2, batch_bytes=batch_bytes, index=False).write(mem)
    assert read_file(mem) == text
    if batch_bytes == MIB:                                       # a selection, an empty one, and the command line
        names = ["huge", "r1", "z", "codes_r", "unmapped_edge"]
        recs, text = want_fastq(case, set(names), 0x10)
        assert bam.extract_reads(case["path"], None, names, 0x10, device=GPU, batch_bytes=batch_bytes, output=out) == (len(recs), len(text))
        assert read_file(out) == text and 0 < len(recs) < len(names) + 2
        assert bam.extract_reads(case["path"], names=[], device=GPU, output=out) == (0, 0) and read_file(out) == b""
        assert bam.extract_reads(case["path"], names=["not_in_the_file"], device=GPU, batch_bytes=batch_bytes, output=out) == (0, 0) and read_file(out) == b""
        assert CoRAL.main(["fastq", "--lr_bam", case["path"], "--output", out, "--stream", "--device", "cpu"]) == out
        assert read_file(out) == want_fastq(case)[1]


def test_fastq_output_argument_rules(case, tmp_path):
    out = str(tmp_path / "x.fastq")
    with pytest.raises(ValueError, match="write"):
        bam.extract_reads(case["path"], device="cpu", output=out)
    with pytest.raises(ValueError):
        bam.extract_reads(case["path"], rank=1, world=2, output=out)
    assert not os.path.exists(out)
    L = _lib.lib()
    for request, out_path, word in ((dict(reads=(0, None, None, 2)), out, "want_reads"), (dict(), out, "want_reads"), (dict(reads=(0, None, None, 1), world=2), out, "world"),
                                    (dict(reads=(0, None, None, 1)), None, "path"), (dict(reads=(0, None, None, 1)), str(tmp_path / "no_dir" / "x"), "cannot create")):
        rc, h, ws_bytes = open_handle(L, case["path"], 1, 0, _lib.bam_request(**request), TextFile(out_path))
        assert rc == CORAL_ERR_ARG and h.value is None and word in L.coral_bam_last_error().decode(), (request, L.coral_bam_last_error().decode())
    assert not os.path.exists(out)
    a = CoRAL.build_parser().parse_args(["fastq", "--lr_bam", "x.bam", "--output", "o.fastq", "--stream"])
    assert a.stream is True and CoRAL.build_parser().parse_args(["fastq", "--lr_bam", "x.bam", "--output", "o.fastq"]).stream is False


# ---- without a GPU -------------------------------------------------------------------------------------------------------------
def test_python_argument_rules(case, tmp_path):
    out = str(tmp_path / "x.bam")
    with pytest.raises(ValueError, match="extract_records"):
        bam.view_bam(case["path"], out, device="cpu")
    for kw in (dict(chunk_blocks=-1), dict(chunk_blocks=16385), dict(chunk_blocks=True), dict(chunk_blocks=1.5), dict(batch_bytes=-1),
               dict(exclude_flags=-1), dict(exclude_flags=0x10000), dict(names=[""]), dict(names=["a" * 255]), dict(regions=[("chrNone", 0, 5)])):
        with pytest.raises(ValueError):
            bam.view_bam(case["path"], out, **kw)
    assert not os.path.exists(out)
    assert bam.ViewStats(1, 2, 3).file_bytes == 3


def test_stream_parses():
    p = CoRAL.build_parser()
    a = p.parse_args(["view", "--lr_bam", "x.bam", "--output", "o.bam", "--stream"])
    assert a.stream is True and a.level == 1 and a.gpu_compress is False
    assert p.parse_args(["view", "--lr_bam", "x.bam", "--output", "o.bam"]).stream is False
