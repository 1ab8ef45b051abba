"""Coordinate order during the BAM decode (bam.extract_records(order="coordinate"), bam.sort_bam, the `sort` mode; reads_order = 1
of the request, coral_bam_decode_request / coral_bamgpu_open_request; coral_bam_records_merge), on both pipelines.

The contract is one key and stability:
    key = (uint32)tid << 32 | (uint32)(pos + 1) << 1 | (flag >> 4 & 1)
tid = -1 is 0xffffffff (records without coordinates last), forward before reverse at an equal position, records with equal keys
in file order.  Every expected byte comes from tests/bamfile.parse, the selection rule restated in test_extract_records and
Python's stable `sorted` with the key restated here.  Nothing expected has passed through either decoder.  Byte identity with
`samtools sort` is not claimed."""
import ctypes as C
import gzip
import os
import random
import struct

import numpy as np
import pytest
import torch  # noqa: F401

from coral_amd import CoRAL, _lib, bam, synth
from tests.bamfile import parse, read_bam
from tests.decode_support import CORAL_ERR_ARG, CORAL_OK, DEVICE, PIPELINES, _pipeline_by_device, gpu_open_only  # noqa: F401
from tests.test_extract_reads import patch_codes, qual_of, write_raw
from tests.test_extract_records import (EDGE_SIZES, REGIONS, SMALL_BATCH, SMALLEST, assert_records, bytes_of, gunzip, more_alignments,
                                        selected)

MIB = 1 << 20
BATCH = MIB // 1500 * 1500                     # inflated bytes of a smallest GPU batch of this file: whole blocks of 1500 bytes
ALL_REGIONS = REGIONS + [("chr8", 0, 1_000_000)]
FILTER = bam.RecordFilter(min_mapq=11, min_seq_length=16, exclude_flags=0x400)
NAMES = ["tie_a", "tie_b", "tie_c", "far_a", "far_b", "huge", "r1", "chim", "nowhere", "u1", "rev_first", "fwd_second", "z", "not_there"]


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def sort_key(r):
    return ((r["tid"] & 0xFFFFFFFF) << 32) | (((r["pos"] + 1) & 0xFFFFFFFF) << 1) | ((r["flag"] >> 4) & 1)


def passes(r, f):
    return f is None or (r["mapq"] >= f.min_mapq and r["l_seq"] >= f.min_seq_length and r["flag"] & f.require_flags == f.require_flags
                         and not r["flag"] & f.exclude_flags)


def want_sorted(case, regions=None, names=None, exclude_flags=0, record_filter=None, recs=None):
    """(names, bytes) of the selection in coordinate order: `sorted` is stable, so equal keys stay in file order."""
    kept = [r for r in (case["parsed"].recs if recs is None else recs) if passes(r, record_filter)]
    sel = sorted(selected(case, regions, None if names is None else set(names), exclude_flags, recs=kept), key=sort_key)
    return [r["name"] for r in sel], [bytes_of(case, r) for r in sel]


# ---- the file ------------------------------------------------------------------------------------------------------------------
def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def raw_record(tid, pos, flag, name, l_seq, mapq=30):
    """One record's bytes, block_size word first: a single M op when it is placed and mapped, SEQ of A/C/G/T, QUAL, no tag."""
    cigar = [(l_seq << 4)] if l_seq and tid >= 0 and not flag & 4 else []
    k = np.arange(l_seq + (l_seq & 1), dtype=np.int64)
    codes = (1 << ((k * 7 + len(name)) % 4)).astype(np.uint8)
    qual = ((np.arange(l_seq, dtype=np.int64) * 5 + len(name)) % 41).astype(np.uint8)
    name_b = name.encode() + b"\0"
    bin_ = reg2bin(pos, pos + (l_seq if cigar else 1)) if tid >= 0 else 4680
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name_b), mapq, bin_, len(cigar), flag, l_seq, -1, -1, 0) + name_b
    body += struct.pack("<%dI" % len(cigar), *cigar) + ((codes[0::2] << 4) | codes[1::2]).astype(np.uint8).tobytes() + qual.tobytes()
    return struct.pack("<i", len(body)) + body


def source_stream():
    """(header bytes, [record bytes]) of test_extract_records' file: the copy kernel's edge sizes, the smallest record, the
    long-CIGAR record and `huge` come with it."""
    import tempfile
    rec = synth.records_from_alignments(more_alignments())
    names = rec.materialise_names()
    name_of = lambda i: names[int(rec.name_id[i])]
    l_seq = lambda i: int(rec.qlen[i]) if int(rec.has_seq[i]) else 0
    with tempfile.TemporaryDirectory() as d:
        first = os.path.join(d, "first.bam")
        bam.write_bam(rec, first, seed=11, fast_seq=True, qual=lambda i: qual_of(name_of(i), l_seq(i)),
                      nm_type=lambda i: None if name_of(i) == "z" else "i")
        raw = gunzip(first)
    raw = patch_codes(raw, parse(raw))
    parsed = parse(raw)
    return raw[:parsed.recs[0]["start"]], [raw[r["start"]:r["start"] + r["size"]] for r in parsed.recs]


def build_stream():
    header, recs = source_stream()
    random.Random(20240607).shuffle(recs)
    # unplaced records among the first ten
    recs.insert(2, raw_record(-1, -1, 4, "u1", 40))
    recs.insert(6, raw_record(-1, -1, 4, "u2", 0))
    # three records of one key under different names, apart from each other; reverse in front of forward at one (tid, pos)
    for at, name in ((12, "tie_a"), (30, "tie_b"), (55, "tie_c")):
        recs.insert(at, raw_record(7, 50_000, 0, name, 30))
    recs.insert(20, raw_record(7, 60_000, 0x10, "rev_first", 25))
    recs.insert(40, raw_record(7, 60_000, 0, "fwd_second", 26))
    recs.insert(4, raw_record(7, 70_000, 0, "far_a", 50))
    # a stretch without a forward record, from where the records above end to behind the end of the third smallest batch:
    # positions all over chr8 and chr3 so that the records interleave with everything else, some on keys that forward records have
    stretch_at = len(header) + sum(len(r) for r in recs)
    assert stretch_at < 2 * BATCH - 4096, stretch_at
    k = 0
    while len(header) + sum(len(r) for r in recs) < 3 * BATCH + 4096:
        tid, pos = ((7, 50_000), (7, 60_000), (2, 1_500 - k), (7, 10_000 + 37 * k), (7, 900_000 - k), (2, 7_000 + k))[k % 6]
        recs.append(raw_record(tid, pos, 0x10 if k % 5 else 0x14, "s%03d" % k, 30_000 - 401 * (k % 7)))
        k += 1
    stretch_end = len(header) + sum(len(r) for r in recs)
    recs += [raw_record(7, 70_000, 0, "far_b", 60), raw_record(0, 5, 0, "first_of_all", 10), raw_record(-1, -1, 4, "u3", 12),
             raw_record(7, 50_000, 0x10, "tie_rev", 30)]
    return header, recs, stretch_at, stretch_end


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("sort_records")
    header, recs, stretch_at, stretch_end = build_stream()
    raw = header + b"".join(recs)
    path = str(d / "shuffled.bam")
    write_raw(raw, path, block_size=1500, empty_block_every=5)
    parsed = read_bam(path)
    R = parsed.recs
    assert len(R) == len(recs) and parsed.n_bytes == len(raw) > 2 * MIB
    by_name = {}
    for r in R:
        by_name.setdefault(r["name"], []).append(r)
    sizes = {r["size"] for r in R}
    assert set(EDGE_SIZES) <= sizes and min(sizes) == SMALLEST and "huge" in by_name and len(by_name["longcigar"][0]["ops"]) == 66001
    keys = [sort_key(r) for r in R]
    assert keys != sorted(keys)
    ties = [r for r in R if sort_key(r) == sort_key(by_name["tie_a"][0])]
    assert len({r["name"] for r in ties}) >= 3 and [r["name"] for r in ties[:3]] == ["tie_a", "tie_b", "tie_c"]
    rev, fwd = by_name["rev_first"][0], by_name["fwd_second"][0]
    assert (rev["tid"], rev["pos"]) == (fwd["tid"], fwd["pos"]) and rev["flag"] & 0x10 and not fwd["flag"] & 0x10 and rev["start"] < fwd["start"]
    assert sum(1 for r in R[:10] if r["tid"] == -1) >= 2
    far_a, far_b = by_name["far_a"][0], by_name["far_b"][0]
    assert sort_key(far_a) == sort_key(far_b) and far_b["start"] - far_a["start"] > MIB
    # the stretch: at least 1 MiB, covering the whole third batch at the smallest batch size, no record that survives 0x10
    assert stretch_end - stretch_at >= MIB and stretch_at <= 2 * BATCH and stretch_end >= 3 * BATCH
    inside = [r for r in R if stretch_at <= r["start"] < stretch_end]
    assert inside and all(r["flag"] & 0x10 for r in inside) and inside[-1]["start"] + inside[-1]["size"] == stretch_end
    assert any(not r["flag"] & 0x10 for r in R if r["start"] >= stretch_end)
    return dict(dir=d, raw=raw, path=path, parsed=parsed, header=header, sorted_header=bam.sorted_header_bytes(header))


def extract(pipe, path, *args, **kw):
    if pipe == "gpu":
        kw.setdefault("batch_bytes", SMALL_BATCH)
    kw.setdefault("index", False)
    kw.setdefault("order", "coordinate")
    got = bam.extract_records(path, *args, device=DEVICE[pipe], n_threads=2, **kw)
    if pipe == "gpu":
        assert bam.LAST_DECODE.get("where") == "gpu"
    return got


def same(a, b):
    return a.n == b.n and np.array_equal(a.data, b.data) and np.array_equal(a.offsets, b.offsets) and a.header == b.header and a.order == b.order


# ---- 1. the whole file and the selections ----------------------------------------------------------------------------------------
SELECTIONS = {
    "everything": dict(),
    "forward only": dict(exclude_flags=0x10),
    "record filter": dict(record_filter=FILTER),
    "names": dict(names=NAMES),
    "regions": dict(regions=ALL_REGIONS),
    "names and regions": dict(regions=ALL_REGIONS, names=NAMES, exclude_flags=0x100),
}


@pytest.mark.parametrize("what", list(SELECTIONS))
@pytest.mark.parametrize("pipe", PIPELINES)
def test_selection_in_coordinate_order(case, pipe, what):
    kw = SELECTIONS[what]
    want = want_sorted(case, **kw)
    got = extract(pipe, case["path"], **kw)
    assert_records(got, want, what)
    assert got.order == "coordinate" and got.header == case["sorted_header"] and len(want[0]) >= 8
    if pipe == "gpu":
        assert bam.LAST_DECODE["batches"] >= 3                   # at least three sorted runs were merged
    if what == "everything":
        assert got.n == len(case["parsed"].recs) and want[0][0] == "first_of_all" and set(want[0][-4:]) == {"nowhere", "u1", "u2", "u3"}
        at = want[0].index("tie_a")
        assert want[0][at:at + 3] == ["tie_a", "tie_b", "tie_c"] and want[0].index("tie_rev") > at + 2
        assert want[0].index("fwd_second") < want[0].index("rev_first") and want[0].index("far_a") + 1 == want[0].index("far_b")
    if what == "forward only":                                   # (a batch of the GPU decode contributes an empty run)
        assert "far_b" in want[0] and not any(n.startswith("s0") for n in want[0])


@pytest.mark.gpu
def test_one_run_equals_many_runs_equals_the_host(case):
    for kw in (dict(), dict(exclude_flags=0x10)):
        one = extract("gpu", case["path"], batch_bytes=0, **kw)
        assert bam.LAST_DECODE["batches"] == 1
        many = extract("gpu", case["path"], **kw)
        assert bam.LAST_DECODE["batches"] >= 3
        host = extract("host", case["path"], **kw)
        assert same(one, many) and same(one, host)
        assert_records(one, want_sorted(case, **kw))


@pytest.mark.parametrize("pipe", PIPELINES)
def test_sorted_byte_ranges_merge_to_the_whole(case, pipe):
    for kw in (dict(), dict(names=NAMES, exclude_flags=0x900)):
        parts = [extract(pipe, case["path"], rank=r, world=3, **kw) for r in range(3)]
        assert sum(p.n > 0 for p in parts) >= 2
        whole = bam.merge_sorted_record_bytes(parts)
        assert_records(whole, want_sorted(case, **kw), kw)
        assert whole.order == "coordinate" and whole.header == case["sorted_header"]
        with pytest.raises(ValueError):
            bam.merge_record_bytes(parts)
    in_file_order = extract(pipe, case["path"], order="file")
    with pytest.raises(ValueError):
        bam.merge_record_bytes([in_file_order, parts[0]])
    with pytest.raises(ValueError):
        bam.merge_sorted_record_bytes([in_file_order])
    with pytest.raises(ValueError):
        bam.merge_sorted_record_bytes([])


@pytest.mark.parametrize("pipe", PIPELINES)
def test_a_sorted_file_stays_as_it_is(case, pipe, tmp_path):
    blobs = want_sorted(case)[1]
    path = str(tmp_path / "sorted.bam")
    write_raw(case["header"] + b"".join(blobs), path, block_size=1500, empty_block_every=5)
    a, b = extract(pipe, path), extract(pipe, path, order="file")
    assert a.n == b.n == len(blobs) and a.data.tobytes() == b.data.tobytes() == b"".join(blobs) and np.array_equal(a.offsets, b.offsets)
    assert (a.order, b.order) == ("coordinate", "file") and b.header == case["header"] and a.header == case["sorted_header"]


@pytest.mark.parametrize("pipe", PIPELINES)
def test_nothing_and_one_record(case, pipe, tmp_path):
    empty, one = str(tmp_path / "header_only.bam"), str(tmp_path / "one.bam")
    write_raw(case["header"], empty)
    record = raw_record(3, 77, 0x10, "only", 19)
    write_raw(case["header"] + record, one)
    got = extract(pipe, empty)
    assert got.n == 0 and got.offsets.tolist() == [0] and len(got.data) == 0 and got.header == case["sorted_header"]
    got = extract(pipe, one)
    assert got.n == 1 and got.offsets.tolist() == [0, len(record)] and got.data.tobytes() == record and got.names() == ["only"]
    for kw in (dict(names=["not_in_the_file"]), dict(regions=[("chr4", 0, 1000)]), dict(names=["rev_first", "tie_rev"], exclude_flags=0x10)):
        got = extract(pipe, case["path"], **kw)
        assert got.n == 0 and got.offsets.tolist() == [0] and len(got.data) == 0 and got.order == "coordinate"
    got = bam.extract_records(str(tmp_path / "no_such_file.bam"), names=[], device=DEVICE[pipe], order="coordinate")
    assert got.n == 0 and got.header is None and got.order == "coordinate"


# ---- 2. the header ---------------------------------------------------------------------------------------------------------------
def test_sorted_header_bytes():
    contigs = struct.pack("<i", 2) + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 1000) + struct.pack("<i", 3) + b"cX\0" + struct.pack("<i", 7)
    sq = b"@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:cX\tLN:7\n"
    shapes = {
        b"@HD\tVN:1.5\tSO:unsorted\tGO:none\n" + sq: b"@HD\tVN:1.5\tSO:coordinate\tGO:none\n" + sq,
        b"@HD\tVN:1.6\n" + sq: b"@HD\tVN:1.6\tSO:coordinate\n" + sq,
        sq + b"@CO\tSO:queryname is only a comment\n": b"@HD\tVN:1.6\tSO:coordinate\n" + sq + b"@CO\tSO:queryname is only a comment\n",
        b"": b"@HD\tVN:1.6\tSO:coordinate\n",
    }
    for text, want in shapes.items():
        got = bam.sorted_header_bytes(b"BAM\x01" + struct.pack("<i", len(text)) + text + contigs)
        l_text = struct.unpack_from("<i", got, 4)[0]
        assert got[:4] == b"BAM\x01" and l_text == len(want) and got[8:8 + l_text] == want and got[8 + l_text:] == contigs, text
        assert bam.sorted_header_bytes(got) == got                # (nothing more to change)
    for bad in (b"", b"BAM\x01", b"SAM\x01" + bytes(8), b"BAM\x01" + struct.pack("<i", 50) + b"@HD\n"):
        with pytest.raises(ValueError):
            bam.sorted_header_bytes(bad)


# ---- 3. the file, its index, the command line --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", PIPELINES)
def test_the_source_cannot_be_indexed(case, pipe):
    with pytest.raises(_lib.CoralHipError, match="coordinate order"):
        bam.build_index(case["path"], str(case["dir"] / ("never_%s.bai" % pipe)), device=DEVICE[pipe])
    assert not os.path.exists(str(case["dir"] / ("never_%s.bai" % pipe)))


@pytest.mark.parametrize("pipe", PIPELINES)
def test_sort_bam_writes_an_indexed_file(case, pipe, tmp_path):
    out = str(tmp_path / "sorted.bam")
    kw = dict(batch_bytes=SMALL_BATCH) if pipe == "gpu" else {}
    assert bam.sort_bam(case["path"], out, device=DEVICE[pipe], n_threads=2, **kw) == out and os.path.exists(out + ".bai")
    names, blobs = want_sorted(case)
    assert gunzip(out) == case["sorted_header"] + b"".join(blobs)
    back = read_bam(out)
    assert [r["name"] for r in back.recs] == names and back.refs == case["parsed"].refs and back.lens == case["parsed"].lens
    assert [sort_key(r) for r in back.recs] == sorted(sort_key(r) for r in case["parsed"].recs)
    assert bam.build_index(out, str(tmp_path / "again.bai"), device=DEVICE[pipe]) == str(tmp_path / "again.bai")
    with open(out + ".bai", "rb") as a, open(str(tmp_path / "again.bai"), "rb") as b:
        assert a.read() == b.read()
    # a region query on the sorted file, through its index: the restated selection of the sorted records, in their order
    sorted_case = dict(parsed=back, raw=gunzip(out))
    for regions in (REGIONS, [("chr8", 49_990, 60_010)]):
        got = bam.extract_records(out, regions, device=DEVICE[pipe], n_threads=2, index=out + ".bai", **kw)
        sel = selected(sorted_case, regions)
        assert bam.LAST_DECODE["index"] == out + ".bai" and len(sel) >= 6
        assert_records(got, ([r["name"] for r in sel], [bytes_of(sorted_case, r) for r in sel]), regions)
        again = bam.extract_records(out, regions, device=DEVICE[pipe], n_threads=2, index=out + ".bai", order="coordinate", **kw)
        assert again.data.tobytes() == got.data.tobytes()
    # index=False and a selection through sort_bam's own arguments
    out2 = str(tmp_path / "forward.bam")
    bam.sort_bam(case["path"], out2, index=False, level=0, record_filter=FILTER, exclude_flags=0x10, device=DEVICE[pipe], n_threads=2, **kw)
    assert gunzip(out2) == case["sorted_header"] + b"".join(want_sorted(case, exclude_flags=0x10, record_filter=FILTER)[1])
    assert not os.path.exists(out2 + ".bai")


@pytest.mark.parametrize("pipe", PIPELINES)
def test_sort_mode_writes_what_sort_bam_writes(case, pipe, tmp_path):
    out, ref = str(tmp_path / "cli.bam"), str(tmp_path / "api.bam")
    argv = ["sort", "--lr_bam", case["path"], "--output", out, "--device", DEVICE[pipe], "--filter_min_mapq", "11", "--index"]
    assert CoRAL.main(argv) == out
    bam.sort_bam(case["path"], ref, record_filter=bam.RecordFilter(min_mapq=11), device=DEVICE[pipe])
    for suffix in ("", ".bai"):
        with open(out + suffix, "rb") as a, open(ref + suffix, "rb") as b:
            assert a.read() == b.read(), suffix
    want = want_sorted(case, record_filter=bam.RecordFilter(min_mapq=11))
    assert gunzip(out) == case["sorted_header"] + b"".join(want[1]) and 8 < len(want[0]) < len(case["parsed"].recs)
    a = CoRAL.build_parser().parse_args(["sort", "--lr_bam", "x.bam", "--output", "o.bam"])
    assert a.reads_exclude_flags == 0 and a.level == 1 and a.index is False and a.filter_min_length == 0 and a.device == "cuda:0"


# ---- 4. the entry points' rules (neither call needs a GPU) --------------------------------------------------------------------------
BAD_ORDERS = {
    "reads_order = 2": (dict(reads=(0, None, None, 2)), 2),
    "reads_order = -1": (dict(reads=(0, None, None, 2)), -1),
    "coordinate order without a reads request": (dict(), 1),
    "coordinate order of FASTQ text": (dict(reads=(0, None, None, 1)), 1),
}


def test_both_entry_points_refuse_a_bad_order(case):
    L = _lib.lib()
    path = case["path"].encode()
    for name, (kw, order) in BAD_ORDERS.items():
        req, h, ws = _lib.bam_request(**kw), C.c_void_p(), C.c_int64(0)
        req.reads_order = order
        assert L.coral_bam_decode_request(path, 1, C.byref(req), C.byref(h)) == CORAL_ERR_ARG and h.value is None, name
        assert "reads_order" in L.coral_bam_last_error().decode(), (name, L.coral_bam_last_error().decode())
        assert L.coral_bamgpu_open_request(path, 1, 0, C.byref(req), None, C.byref(h), C.byref(ws)) == CORAL_ERR_ARG, name
        assert h.value is None and ws.value == 0 and "reads_order" in L.coral_bam_last_error().decode(), name
    # the other rules of the request still come first, and order 0 is what a zeroed field asks for
    req, h = _lib.bam_request(reads=(0, None, None, 3, 1)), C.c_void_p()
    assert L.coral_bam_decode_request(path, 1, C.byref(req), C.byref(h)) == CORAL_ERR_ARG and "want_reads" in L.coral_bam_last_error().decode()
    req = _lib.bam_request(reads=(0, None, [b"tie_a", b"tie_b"], 2))
    assert L.coral_bam_decode_request(path, 2, C.byref(req), C.byref(h)) == CORAL_OK
    sz = (C.c_int64 * 2)()
    assert L.coral_bam_reads_sizes(h, sz) == CORAL_OK and sz[0] == 2
    L.coral_bam_decode_close(h)
    assert _lib.bam_request(reads=(0, None, None, 2, 1)).reads_order == 1 and _lib.bam_request(reads=(0, None, None, 2)).reads_order == 0
    for kw in (dict(order="x"), dict(order=1), dict(order=None)):
        with pytest.raises(ValueError):
            bam.extract_records(case["path"], device="cpu", **kw)
    with pytest.raises(ValueError):
        bam.RecordBytes(order="sorted")


@pytest.mark.gpu
def test_only_coordinate_order_carves_the_sort_arrays(case):
    L = _lib.lib()
    sizes = {}
    for order in (0, 1):
        req, h, ws = _lib.bam_request(reads=(0, None, None, 2, order)), C.c_void_p(), C.c_int64(0)
        assert L.coral_bamgpu_open_request(case["path"].encode(), 1, 0, C.byref(req), None, C.byref(h), C.byref(ws)) == CORAL_OK
        L.coral_bamgpu_close(h)
        sizes[order] = ws.value
    assert sizes[0] == gpu_open_only(case["path"], reads=(0, None, None, 2))[2] < sizes[1]
    # 40 bytes per record of a batch (two key and two ordinal buffers, two permuted plan arrays) and hipcub's temporary storage;
    # a batch of this file has (64 MiB carried + 16 MiB + ...) / 36 record slots at most
    assert sizes[1] - sizes[0] >= 40 * ((80 << 20) // 36)


# ---- 5. the merge on its own -------------------------------------------------------------------------------------------------------
def merge(runs, n_threads):
    """runs: lists of record bytes -> (rc, [record bytes])"""
    L = _lib.lib()
    k = len(runs)
    blobs = [np.frombuffer(b"".join(r) + b"\0", dtype=np.uint8) for r in runs]
    offs = [np.concatenate([[0], np.cumsum([len(x) for x in r])]).astype(np.int64) for r in runs]
    data = (C.c_void_p * max(k, 1))(*[b.ctypes.data for b in blobs])
    off = (C.c_void_p * max(k, 1))(*[o.ctypes.data for o in offs])
    n = (C.c_int64 * max(k, 1))(*[len(r) for r in runs])
    total = sum(len(r) for r in runs)
    out, out_off = np.full(sum(len(b) - 1 for b in blobs) + 1, 0xAB, dtype=np.uint8), np.full(total + 1, -1, dtype=np.int64)
    rc = L.coral_bam_records_merge(k, data, off, n, out.ctypes.data, out_off.ctypes.data, n_threads)
    o = out_off.tolist()
    assert rc != CORAL_OK or (o[0] == 0 and o[-1] == len(out) - 1 and out[-1] == 0xAB)
    return rc, [out[o[j]:o[j + 1]].tobytes() for j in range(total)] if rc == CORAL_OK else None


def test_records_merge(case):
    rec = lambda tid, pos, flag, name: raw_record(tid, pos, flag, name, 5 + len(name))
    run0 = [rec(0, 10, 0, "a0"), rec(0, 20, 0, "tie_run0"), rec(0, 20, 0x10, "rev0"), rec(-1, -1, 4, "un0")]
    run1 = [rec(0, 20, 0, "tie_run1_first"), rec(0, 20, 0, "tie_run1_second"), rec(1, 0, 0, "b1"), rec(-1, -1, 4, "un1")]
    run2 = [rec(0, 5, 0x10, "c2"), rec(0, 20, 0, "tie_run2"), rec(2, 7, 0, "d2")]
    name = lambda b: b[36:36 + b[12] - 1].decode()
    rc, got = merge([run0, run1, run2], 1)
    assert rc == CORAL_OK
    assert [name(b) for b in got] == ["c2", "a0", "tie_run0", "tie_run1_first", "tie_run1_second", "tie_run2", "rev0", "b1", "d2", "un0", "un1"]
    assert got == sorted(run0 + run1 + run2, key=lambda b: sort_key(parse_fixed(b)))
    # an empty run between two others, one run, no run; the bytes do not depend on the thread count
    for runs in ([run0, [], run2], [run1], [[], []], []):
        one, four = merge(runs, 1), merge(runs, 4)
        assert one[0] == four[0] == CORAL_OK and one[1] == four[1] == sorted([b for r in runs for b in r], key=lambda b: sort_key(parse_fixed(b)))
    # the file's own records as three runs, 1 thread against 4 and against the restatement
    R = case["parsed"].recs
    runs = [[bytes_of(case, r) for r in sorted(R[a:b], key=sort_key)] for a, b in ((0, 40), (40, 41), (41, len(R)))]
    one, four = merge(runs, 1), merge(runs, 4)
    assert one[0] == four[0] == CORAL_OK and one[1] == four[1] == want_sorted(case)[1]
    L = _lib.lib()
    assert L.coral_bam_records_merge(-1, None, None, None, None, None, 1) == CORAL_ERR_ARG
    assert L.coral_bam_records_merge(0, None, None, None, None, None, 1) == CORAL_ERR_ARG          # (out_off always gets its first 0)
    zero = np.full(1, -1, dtype=np.int64)
    assert L.coral_bam_records_merge(0, None, None, None, None, zero.ctypes.data, 0) == CORAL_OK and zero.tolist() == [0]


def parse_fixed(b):
    tid, pos = struct.unpack_from("<ii", b, 4)
    return dict(tid=tid, pos=pos, flag=struct.unpack_from("<H", b, 18)[0])
