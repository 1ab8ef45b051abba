"""The records request of the BAM decode (bam.extract_records, want_reads = 2 of a coral_bam_request_t): the selected records as
their own bytes, on both pipelines, and the BAM file written around them (RecordBytes.write, coral_bgzf_write).

Every expected byte comes from tests/bamfile.py (`raw[r["start"] : r["start"] + r["size"]]` of the records it parses out of the
gzip-inflated file) and from a restatement of the rule in this module: a record is written when flag & exclude_flags == 0, with
regions: tid >= 0 and [pos, bam_endpos) meets a region, with names: its name is listed.  SEQ is not required.  Nothing expected
here has passed through either decoder."""
import ctypes as C
import gzip
import os
import struct

import numpy as np
import pytest
import torch  # noqa: F401

from coral_amd import CoRAL, _lib, bam, synth
from tests.bamfile import M, bgzf_blocks, parse, read_bam
from tests.decode_support import (CORAL_ERR_ARG, CORAL_OK, DEVICE, PIPELINES, _pipeline_by_device, assert_same_qc,  # noqa: F401
                                  assert_same_records, gpu_open_only)
from tests.test_extract_reads import alignments, end_of, patch_codes, qual_of, write_raw

SLICE = 32768                                  # record bytes per work item of the GPU copy (READS_COPY_SLICE)
EDGE_SIZES = (SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 1)
SMALLEST = 4 + 32 + 2                          # block_size word, fixed fields, a 1-byte name and its NUL: no CIGAR, SEQ, QUAL, tag
REGIONS = [("chr3", 1000, 2000), ("chr3", 1500, 1800), ("chr3", 5000, 6000), ("chr5", 100, 200), ("chr4", 0, 1000)]
SMALL_BATCH = 1 << 16                          # (the decoder's smallest batch is 1 MiB)
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def written(r, refs, regions, names, exclude_flags):
    if r["flag"] & exclude_flags:
        return False
    if regions is not None:
        end = end_of(r)
        if r["tid"] < 0 or not any(refs[r["tid"]] == c and a < b and r["pos"] < b and end > a for c, a, b in regions):
            return False
    return names is None or r["name"] in names


def selected(case, regions=None, names=None, exclude_flags=0, recs=None):
    parsed = case["parsed"]
    return [r for r in (parsed.recs if recs is None else recs) if written(r, parsed.refs, regions, names, exclude_flags)]


def bytes_of(case, r):
    return case["raw"][r["start"]:r["start"] + r["size"]]


def want_records(case, regions=None, names=None, exclude_flags=0, recs=None):
    """(names of the written records, their bytes)"""
    sel = selected(case, regions, names, exclude_flags, recs)
    return [r["name"] for r in sel], [bytes_of(case, r) for r in sel]


def assert_records(got, want, what=""):
    names, blobs = want
    assert got.n == len(blobs), (what, got.n, len(blobs), got.names()[:20], names[:20])
    off, raw = got.offsets.tolist(), got.data.tobytes()
    for k, t in enumerate(blobs):                      # record by record first: a failure names the record
        assert raw[off[k]:off[k + 1]] == t, (what, k, names[k][:20], len(t))
    assert raw == b"".join(blobs) and off[-1] == len(raw) and got.offsets.dtype == np.int64 and got.data.dtype == np.uint8, what
    assert got.names() == names and len(got) == got.n, what


# ---- the file ------------------------------------------------------------------------------------------------------------------
def edge_record(size, pos):
    """A forward record of exactly `size` bytes: 36 + (name + NUL) + one CIGAR op + ceil(l_seq / 2) + l_seq + NM:i (7 bytes).
    l_seq + ceil(l_seq / 2) takes every value that is not 1 mod 3; the name's length takes care of the rest.  (The fixture asserts
    the sizes on the parsed file.)"""
    for name_len in (6, 7, 8):
        v = size - 36 - (name_len + 1) - 4 - 7
        if v % 3 != 1:
            l_seq = 2 * v // 3 if v % 3 == 0 else (2 * v - 1) // 3
            return dict(tid=7, pos=pos, cigar=[(M, l_seq)], name=("e%d" % size).ljust(name_len, "_"))
    raise AssertionError(size)


def more_alignments():
    """The alignments of test_extract_reads plus, on chr8 behind `huge`, the records that hit the copy kernel's edges."""
    alns = alignments()
    at = [k for k, a in enumerate(alns) if a.get("name") == "huge"][0] + 1
    extra = [edge_record(size, 30_000 + 10 * k) for k, size in enumerate(EDGE_SIZES)]
    extra.append(dict(tid=7, pos=30_100, cigar=[], flag=4, has_seq=0, qlen=0, name="z"))      # the smallest record there is
    # short records of many sizes, one in four on the reverse strand: with flag 0x10 excluded the gaps shift the destination
    extra += [dict(tid=7, pos=30_200 + k, cigar=[(M, 20 + 2 * k)], flag=0x10 if k % 4 == 2 else 0, name="f%02d" % k) for k in range(24)]
    return alns[:at] + extra + alns[at:]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("extract_records")
    rec = synth.records_from_alignments(more_alignments())
    names = rec.materialise_names()
    name_of = lambda i: names[int(rec.name_id[i])]
    l_seq = lambda i: int(rec.qlen[i]) if int(rec.has_seq[i]) else 0
    first = str(d / "first.bam")
    bam.write_bam(rec, first, seed=11, fast_seq=True, qual=lambda i: qual_of(name_of(i), l_seq(i)),
                  nm_type=lambda i: None if name_of(i) == "z" else "i")
    with gzip.open(first, "rb") as fp:
        raw = fp.read()
    raw = patch_codes(raw, parse(raw))
    path, plain = str(d / "records.bam"), str(d / "records_plain.bam")
    write_raw(raw, path, block_size=1500, empty_block_every=5)
    write_raw(raw, plain)
    parsed = read_bam(path)
    assert len(parsed.recs) == rec.n and parsed.n_bytes == len(raw)
    by_name = {r["name"]: r for r in parsed.recs}
    assert by_name["longcigar"]["n_cig"] == 2 and len(by_name["longcigar"]["ops"]) == 66001      # its CIGAR sits in the CG tag
    sizes = sorted(r["size"] for r in parsed.recs)
    assert set(EDGE_SIZES) <= set(sizes) and sizes[0] == SMALLEST == by_name["z"]["size"]
    assert (by_name["z"]["l_seq"], by_name["z"]["n_cig"], by_name["noseq"]["l_seq"]) == (0, 0, 0)
    huge = by_name["huge"]                            # straddles the first 1 MiB of the inflated stream: two GPU batches
    assert huge["start"] < (1 << 20) - 20_000 and huge["start"] + huge["size"] > (1 << 20) + 20_000
    return dict(dir=d, raw=raw, path=path, plain=plain, parsed=parsed, header=raw[:parsed.recs[0]["start"]])


def extract(pipe, path, *args, **kw):
    if pipe == "gpu":
        kw.setdefault("batch_bytes", SMALL_BATCH)
    kw.setdefault("index", False)
    got = bam.extract_records(path, *args, device=DEVICE[pipe], n_threads=2, **kw)
    if pipe == "gpu":                                  # (an index that names no block for the regions: nothing is decoded at all)
        assert bam.LAST_DECODE.get("where") == "gpu" or (bam.LAST_DECODE["blocks"] == 0 and got.n == 0 and kw["index"])
    return got


def alignments_met(case, sel):
    """(source offsets mod 16, destination offsets mod 16, shifts mod 16) of a selection, from the parsed file."""
    src = [r["start"] for r in sel]
    dst = np.concatenate([[0], np.cumsum([r["size"] for r in sel])])[:-1].tolist()
    return {s % 16 for s in src}, {t % 16 for t in dst}, {(s - t) % 16 for s, t in zip(src, dst)}


# ---- 1. everything, concatenated -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", PIPELINES)
def test_every_record_is_everything_concatenated(case, pipe):
    """No limit, no flag excluded: every record's bytes joined - every l_seq forward and reverse, names of 1 and 254 bytes, the
    CG-tag record, the record that straddles two GPU batches, records of SLICE - 1, SLICE, SLICE + 1 and 2 SLICE + 1 bytes, the
    smallest record, and the record without SEQ that the FASTQ request leaves out.  A second request (flag 0x10 excluded) leaves
    gaps of many sizes, so that source and destination alignments differ from record to record."""
    parsed = case["parsed"]
    everything = b"".join(bytes_of(case, r) for r in parsed.recs)
    assert everything == case["raw"][len(case["header"]):]
    for path in (case["path"], case["plain"]):
        got = extract(pipe, path)
        assert_records(got, want_records(case), path)
        assert got.data.tobytes() == everything and got.n == len(parsed.recs) and got.header == case["header"]
        if pipe == "gpu" and path == case["path"]:
            assert bam.LAST_DECODE["batches"] >= 2            # the 300 000-base record straddles two of them
        forward = extract(pipe, path, exclude_flags=0x10)
        assert_records(forward, want_records(case, exclude_flags=0x10), path)
    src, dst, _ = alignments_met(case, parsed.recs)
    assert src == dst == set(range(16))
    sel = selected(case, exclude_flags=0x10)
    src, dst, shifts = alignments_met(case, sel)
    assert src == dst == set(range(16)) and len(shifts) >= 8, (sorted(src), sorted(dst), sorted(shifts))
    assert set(EDGE_SIZES) | {SMALLEST} <= {r["size"] for r in sel}
    # the difference to the FASTQ request: records without SEQ are records
    fastq = bam.extract_reads(case["plain"], exclude_flags=0, device=DEVICE[pipe], n_threads=2, index=False,
                              **(dict(batch_bytes=SMALL_BATCH) if pipe == "gpu" else {}))
    no_seq = [r["name"] for r in parsed.recs if r["l_seq"] == 0]
    assert sorted(no_seq) == ["noseq", "z"] and fastq.n == got.n - 2 and not set(no_seq) & set(fastq.names()) and set(no_seq) <= set(got.names())


# ---- 2. selection --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exclude_flags", [0x900, 0, 0xF04])
@pytest.mark.parametrize("pipe", PIPELINES)
def test_regions_and_flags(case, pipe, exclude_flags):
    """Several segments on two contigs (two of them overlap and are merged), a contig without records; records that end exactly at
    a segment's start or start exactly at its end, unmapped records at a region's edge, a record without SEQ (written)."""
    want = want_records(case, REGIONS, None, exclude_flags)
    assert_records(extract(pipe, case["path"], REGIONS, exclude_flags=exclude_flags), want, exclude_flags)
    base = ["r1", "r1", "spliced", "last_base", "on_chr5", "noseq"]
    extra = {0x900: ["unmapped_edge", "r1a"], 0: ["r10", "chim", "r1a", "unmapped_edge"], 0xF04: []}[exclude_flags]
    assert sorted(want[0]) == sorted(base + extra)
    for absent in ("ends_at_start", "starts_at_end", "unmapped_before", "unmapped_after", "off_chr5"):
        assert absent not in want[0]


@pytest.mark.parametrize("pipe", PIPELINES)
def test_names(case, pipe):
    # the supplementary of `chim` lies in the region, its primary elsewhere: by name both records are found
    got = extract(pipe, case["path"], names=["chim"])
    assert_records(got, want_records(case, names={"chim"}))
    assert got.n == 2 and extract(pipe, case["path"], names=["chim"], exclude_flags=0x900).n == 1
    assert extract(pipe, case["path"], [("chr3", 1000, 2000)]).names().count("chim") == 1
    # names that are prefixes of each other, a name that is not in the file, duplicates, str and bytes, the 1-byte and 254-byte names
    long3 = ("N%03d" % 3) + "x" * 250
    for names in (["r1"], ["r10"], ["r1a", "r1"], ["r1", "r10", "r1a", "r", "r1b", "zzz"], [b"r10", "r10", "A", "z", long3, long3[:-1]], ["noseq", "z"]):
        want = want_records(case, names={n.decode() if isinstance(n, bytes) else n for n in names})
        assert_records(extract(pipe, case["path"], names=names), want, names)
        assert len(want[0]) > 0
    assert want[0] == ["noseq", "z"]
    # regions and names intersect
    want = want_records(case, REGIONS, {"r1", "on_chr5", "mito", "starts_at_end", "noseq"})
    assert_records(extract(pipe, case["path"], REGIONS, ["r1", "on_chr5", "mito", "starts_at_end", "noseq"]), want)
    assert want[0] == ["r1", "noseq", "r1", "on_chr5"]


@pytest.mark.parametrize("pipe", PIPELINES)
def test_empty_selections(case, pipe, tmp_path):
    for got in (extract(pipe, case["path"], names=["not_in_the_file"]), extract(pipe, case["path"], [("chr4", 0, 1000)]),
                extract(pipe, case["path"], REGIONS, ["mito"]), extract(pipe, case["path"], [("chr3", 10, 10)]),
                extract(pipe, case["path"], names=["r10"], exclude_flags=0x100)):
        assert got.n == 0 and len(got.data) == 0 and got.offsets.tolist() == [0] and got.names() == [] and got.header == case["header"]
    # an empty list selects nothing and the file is not opened
    for kw in (dict(regions=[]), dict(names=[]), dict(regions=[], names=["A"])):
        got = bam.extract_records(str(tmp_path / "no_such_file.bam"), device=DEVICE[pipe], **kw)
        assert got.n == 0 and got.header is None
    # a file whose records are all unselected
    recs = [r for r in case["parsed"].recs if r["name"] in ("noseq", "r10", "chim") and r["tid"] == 2]
    raw = case["header"] + b"".join(bytes_of(case, r) for r in recs)
    path = str(tmp_path / "unselected.bam")
    write_raw(raw, path)
    assert [r["name"] for r in read_bam(path).recs] == ["r10", "chim", "noseq"]
    assert extract(pipe, path, exclude_flags=0x900).names() == ["noseq"] and extract(pipe, path, names=["noseq"], exclude_flags=0x900).n == 1
    assert extract(pipe, path, names=["r10", "chim"], exclude_flags=0x900).n == 0 and extract(pipe, path).n == 3


# ---- 3. composition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", PIPELINES)
def test_record_filter_acts_first(case, pipe, tmp_path):
    """The result is that of a file that holds only the kept records (cut out of the inflated stream by the test)."""
    parsed, f = case["parsed"], bam.RecordFilter(min_mapq=11, min_seq_length=16, exclude_flags=0x400)
    kept = [r for r in parsed.recs if r["mapq"] >= 11 and r["l_seq"] >= 16 and not r["flag"] & 0x400]
    assert 0 < len(kept) < len(parsed.recs)
    path = str(tmp_path / "kept.bam")
    write_raw(case["header"] + b"".join(bytes_of(case, r) for r in kept), path, block_size=1500, empty_block_every=5)
    for kw in (dict(), dict(regions=REGIONS + [("chr8", 0, 1_000_000)], exclude_flags=0x100)):
        want = want_records(case, kw.get("regions"), None, kw.get("exclude_flags", 0), recs=kept)
        assert_records(extract(pipe, case["path"], record_filter=f, **kw), want, kw)
        assert_records(extract(pipe, path, **kw), want, kw)
        assert len(want[0]) > 3 and "noseq" not in want[0]


@pytest.mark.parametrize("world", [2, 3, 5])
@pytest.mark.parametrize("pipe", PIPELINES)
def test_byte_ranges_concatenate(case, pipe, world):
    for kw in (dict(), dict(names=["r1", "huge", "A", "mito", "z"], exclude_flags=0x900)):
        parts = [extract(pipe, case["path"], rank=r, world=world, **kw) for r in range(world)]
        names = set(kw["names"]) if "names" in kw else None
        whole = bam.merge_record_bytes(parts)
        assert_records(whole, want_records(case, None, names, kw.get("exclude_flags", 0)), (world, kw))
        assert whole.header == case["header"]


@pytest.mark.parametrize("pipe", PIPELINES)
def test_index_cuts_the_decode_down_to_the_regions(case, pipe, tmp_path):
    path = str(tmp_path / "indexed.bam")
    write_raw(case["raw"], path, block_size=1500, empty_block_every=5)
    bai = bam.build_index(path, device="cpu")
    whole = extract(pipe, path, REGIONS)
    blocks_whole = bam.LAST_DECODE["blocks"]
    for index in (bai, None):                          # given, and found beside the file
        got = extract(pipe, path, REGIONS, index=index)
        assert bam.LAST_DECODE["index"] == bai and 0 < bam.LAST_DECODE["blocks"] < blocks_whole
        assert got.n == whole.n > 0 and np.array_equal(got.data, whole.data) and np.array_equal(got.offsets, whole.offsets)
    assert_records(got, want_records(case, REGIONS))
    empty = extract(pipe, path, [("chr4", 0, 1000)], index=bai)
    assert empty.n == 0 and empty.header == case["header"]


@pytest.mark.parametrize("pipe", PIPELINES)
def test_rides_with_read_qc_and_a_pileup(case, pipe):
    """One decode with three requests gives what each gives alone (on the GPU they borrow the same scratch arrays in turn)."""
    dev = DEVICE[pipe]
    kw = dict(batch_bytes=SMALL_BATCH) if pipe == "gpu" else {}
    refs = bam.bam_reference_names(case["path"])
    _, segs = bam.pileup_regions(REGIONS + [("chr8", 10_000, 21_000)], refs)
    _, rsegs = bam.pileup_regions(REGIONS, refs)
    names = [b"A", b"huge", b"noseq", b"r1"]
    both = bam._decode(case["path"], dev, n_threads=2, qc=True, coverage=(segs, 10, 0), per_base=True, reads=(0, None, names, 2), records=False, **kw)
    qc = bam._decode(case["path"], dev, n_threads=2, qc=True, records=False, **kw).qc
    pile = bam._decode(case["path"], dev, n_threads=2, coverage=(segs, 10, 0), per_base=True, records=False, **kw)
    alone = bam._decode(case["path"], dev, n_threads=2, reads=(0, None, names, 2), records=False, **kw).reads
    assert_same_qc(both.qc, qc)
    assert np.array_equal(both.pileup, pile.pileup) and np.array_equal(both.counts, pile.counts) and int(pile.counts.sum()) > 0
    assert np.array_equal(both.reads[0], alone[0]) and np.array_equal(both.reads[1], alone[1])
    assert_records(bam.RecordBytes(*both.reads), want_records(case, None, {"A", "huge", "noseq", "r1"}))
    with_regions = bam._decode(case["path"], dev, n_threads=2, qc=True, coverage=(segs, 10, 0), per_base=True, reads=(0, rsegs, names, 2), **kw)
    assert_records(bam.RecordBytes(*with_regions.reads), want_records(case, REGIONS, {"A", "huge", "noseq", "r1"}))
    assert with_regions.records.n == len(case["parsed"].recs) and np.array_equal(with_regions.pileup, pile.pileup)


# ---- 4. the file ---------------------------------------------------------------------------------------------------------------
def blocks_of(path):
    """[(inflated offset, inflated length)] of the file's BGZF blocks, each block's BSIZE checked against where the next begins."""
    with open(path, "rb") as fp:
        raw = fp.read()
    blocks = list(bgzf_blocks(raw))
    for (at, _, _), nxt in zip(blocks, [b[0] for b in blocks[1:]] + [len(raw)]):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04" and raw[at + 12:at + 16] == b"BC\x02\x00"
        assert struct.unpack_from("<H", raw, at + 16)[0] + 1 == nxt - at
    return raw, [(u, n) for _, u, n in blocks]


def gunzip(path):
    with gzip.open(path, "rb") as fp:
        return fp.read()


@pytest.mark.parametrize("pipe", PIPELINES)
def test_the_written_file(case, pipe, tmp_path):
    regions = REGIONS + [("chr8", 10_000, 31_000)]
    got = extract(pipe, case["path"], regions, exclude_flags=0x400)
    sel = selected(case, regions, None, 0x400)
    assert_records(got, want_records(case, regions, None, 0x400))
    assert {"huge", "longcigar", "noseq", "z"} <= set(got.names()) and set(EDGE_SIZES) <= {r["size"] for r in sel}
    out, out4, out0 = (str(tmp_path / n) for n in ("out.bam", "out4.bam", "out0.bam"))
    assert got.write(out, n_threads=1) == out and got.write(out4, n_threads=4) == out4 and got.write(out0, level=0) == out0
    assert not os.path.exists(out + ".bai")
    raw, blocks = blocks_of(out)
    with open(out4, "rb") as fp:
        assert fp.read() == raw                                  # the bytes do not depend on n_threads
    payload = case["header"] + got.data.tobytes()
    for path in (out, out0):
        assert gunzip(path) == payload
        file_bytes, blk = blocks_of(path)
        assert all(0 < n <= 0xFF00 for _, n in blk[:-1]) and blk[-1][1] == 0 and file_bytes[-28:] == EOF_BLOCK
        assert len(case["header"]) in [u for u, _ in blk]        # the header ends a block
        assert sum(n for _, n in blk) == len(payload) and len(blk) > 10
    assert os.path.getsize(out0) > len(payload) > os.path.getsize(out)
    # field by field, through the plain-Python reader
    back = read_bam(out)
    assert back.refs == case["parsed"].refs and back.lens == case["parsed"].lens and len(back.recs) == len(sel)
    for a, b in zip(back.recs, sel):
        for k in ("tid", "pos", "flag", "mapq", "name", "l_seq", "n_cig", "size"):
            assert a[k] == b[k], (k, b["name"])
        for k in ("ops", "codes", "qual"):
            assert np.array_equal(a[k], b[k]), (k, b["name"])
        assert len(a["tags"]) == len(b["tags"]) and all(x[:2] == y[:2] and np.array_equal(x[2], y[2]) for x, y in zip(a["tags"], b["tags"]))
    # decoded again: the Records of a file the test cut by hand
    cut = str(tmp_path / "cut.bam")
    write_raw(case["header"] + b"".join(bytes_of(case, r) for r in sel), cut)
    want = bam.load_bam(cut, device="cpu")
    for dev in {"cpu", DEVICE[pipe]}:
        assert_same_records(bam.load_bam(out, device=dev), want)
    assert want.n == len(sel)


@pytest.mark.parametrize("pipe", PIPELINES)
def test_the_written_index(case, pipe, tmp_path):
    got = extract(pipe, case["path"])
    out = str(tmp_path / "all.bam")
    got.write(out, index=True)
    idx = bam.read_index(out + ".bai")
    assert len(idx.bins) == len(case["parsed"].refs)
    plain = extract(pipe, out, REGIONS)
    blocks_whole = bam.LAST_DECODE["blocks"]
    for index in (idx, None):
        indexed = extract(pipe, out, REGIONS, index=index)
        assert 0 < bam.LAST_DECODE["blocks"] < blocks_whole
        assert indexed.n == plain.n > 0 and np.array_equal(indexed.data, plain.data) and np.array_equal(indexed.offsets, plain.offsets)
    assert_records(indexed, want_records(case, REGIONS))
    # the first record's virtual offset has a zero low half: the header ends a block
    first = min(int(c[0][0]) for b in idx.bins for c in b.values())
    assert first & 0xFFFF == 0 and first >> 16 > 0


def test_an_empty_selection_writes_header_and_eof(case, tmp_path):
    got = bam.extract_records(case["plain"], names=["not_in_the_file"], device="cpu")
    out = got.write(str(tmp_path / "empty.bam"), index=True)
    raw, blocks = blocks_of(out)
    assert gunzip(out) == case["header"] and raw[-28:] == EOF_BLOCK and [n for _, n in blocks] == [len(case["header"]), 0]
    assert read_bam(out).recs == [] and bam.extract_records(out, device="cpu").n == 0
    assert bam.extract_records(out, [("chr3", 0, 10_000)], device="cpu", index=out + ".bai").n == 0
    with pytest.raises(ValueError):
        bam.extract_records(case["plain"], names=[], device="cpu").write(str(tmp_path / "no_header.bam"))


# ---- 5. the request's rules, equal on both pipelines (neither call needs a GPU) ---------------------------------------------------
I32 = lambda *rows: np.array(rows, dtype=np.int32)
BAD_REQUESTS = {
    "want_reads = 3": (dict(reads=(0, None, None, 3)), "want_reads"),
    "want_reads = -1": (dict(reads=(0, None, None, -1)), "want_reads"),
    "with an index request": (dict(reads=(0, None, None, 2), index=True), "want_reads"),
    "unsorted segments": (dict(reads=(0, I32([2, 2], [500, 100], [600, 200]), None, 2)), "reads_seg"),
    "segments out of contig order": (dict(reads=(0, I32([3, 2], [0, 0], [10, 10]), None, 2)), "reads_seg"),
    "overlapping segments": (dict(reads=(0, I32([2, 2], [100, 150], [200, 300]), None, 2)), "reads_seg"),
    "segment with end < start": (dict(reads=(0, I32([2], [100], [50]), None, 2)), "reads_seg"),
    "unsorted names": (dict(reads=(0, None, [b"b", b"a"], 2)), "reads_names"),
    "a prefix behind its extension": (dict(reads=(0, None, [b"r10", b"r1"], 2)), "reads_names"),
    "duplicate names": (dict(reads=(0, None, [b"a", b"a"], 2)), "reads_names"),
    "a name of 0 bytes": (dict(reads=(0, None, [b"", b"a"], 2)), "reads_names"),
    "a name of 255 bytes": (dict(reads=(0, None, [b"a", b"b" * 255], 2)), "reads_names"),
    "exclude_flags < 0": (dict(reads=(-1, None, None, 2)), "reads_exclude_flags"),
    "exclude_flags > 0xffff": (dict(reads=(0x10000, None, None, 2)), "reads_exclude_flags"),
}
GOOD_REQUESTS = [dict(reads=(0xFFFF, I32([2, 2, 4], [100, 200, 0], [200, 300, 5]), [b"a", b"a" * 254, b"ab", b"b"], 2)),
                 dict(reads=(0, I32([2], [7], [7]), None, 2), spans=np.zeros((0, 2), dtype=np.uint64)),
                 dict(reads=(0, None, [b"r1", b"r10", b"r1a"], 2), qc=True, depth=(1000, 0, 0, 1), keep=(1, 2, 0, 4)),
                 dict(reads=(0, None, None, 1)), dict(reads=(0, None, None))]


def test_the_mode_is_the_fourth_element(case):
    assert _lib.bam_request(reads=(0, None, None)).want_reads == 1 and _lib.bam_request(reads=(0, None, None, 1)).want_reads == 1
    assert _lib.bam_request(reads=(5, None, None, 2)).want_reads == 2 and _lib.bam_request().want_reads == 0


def test_host_refuses_bad_requests(case):
    L = _lib.lib()
    for name, (kw, word) in BAD_REQUESTS.items():
        req, h = _lib.bam_request(**kw), C.c_void_p()
        assert L.coral_bam_decode_request(case["plain"].encode(), 1, C.byref(req), C.byref(h)) == CORAL_ERR_ARG and h.value is None, name
        assert word in L.coral_bam_last_error().decode(), (name, L.coral_bam_last_error().decode())
    for kw in GOOD_REQUESTS:
        req, h = _lib.bam_request(**kw), C.c_void_p()
        assert L.coral_bam_decode_request(case["plain"].encode(), 2, C.byref(req), C.byref(h)) == CORAL_OK, kw
        L.coral_bam_decode_close(h)


def test_gpu_open_refuses_the_same_requests(case):
    for name, (kw, word) in BAD_REQUESTS.items():
        rc, h, ws_bytes, message = gpu_open_only(case["plain"], **kw)
        assert rc == CORAL_ERR_ARG and h is None and ws_bytes == 0, name
        assert word in message, (name, message)
    for kw in GOOD_REQUESTS:
        rc, h, ws_bytes, message = gpu_open_only(case["plain"], **kw)
        assert rc == CORAL_OK and h is not None and ws_bytes > 0, (kw, message)


def test_workspace_one_batch_for_records_four_thirds_for_fastq(case):
    plain = gpu_open_only(case["plain"])[2]
    assert plain == gpu_open_only(case["plain"], qc=False)[2] > 0          # without a request nothing is carved
    records = gpu_open_only(case["plain"], reads=(0, None, None, 2))[2]
    fastq = gpu_open_only(case["plain"], reads=(0, None, None, 1))[2]
    assert plain < records < fastq
    # one batch's capacity, the 64 MiB of carried bytes included, + 256: three quarters of what the FASTQ request carves
    assert (64 << 20) + (16 << 20) + 256 <= records - plain and abs((fastq - plain) * 3 - (records - plain) * 4) <= 4 * 4096


def test_bgzf_write_refuses_bad_arguments(tmp_path):
    L = _lib.lib()
    data = np.arange(100, dtype=np.uint8)
    parts, sizes = (C.c_void_p * 1)(data.ctypes.data), (C.c_int64 * 1)(100)
    path = str(tmp_path / "x.gz").encode()
    for level in (-1, 10):
        assert L.coral_bgzf_write(path, parts, sizes, 1, level, 1) == CORAL_ERR_ARG and "level" in L.coral_bam_last_error().decode()
    assert L.coral_bgzf_write(path, parts, sizes, -1, 1, 1) == CORAL_ERR_ARG and "n_parts" in L.coral_bam_last_error().decode()
    assert L.coral_bgzf_write(path, parts, (C.c_int64 * 1)(-5), 1, 1, 1) == CORAL_ERR_ARG
    assert not os.path.exists(path.decode())
    assert L.coral_bgzf_write(path, parts, sizes, 1, 9, 0) == CORAL_OK and gunzip(path.decode()) == data.tobytes()
    assert L.coral_bgzf_write(path, None, None, 0, 1, 1) == CORAL_OK
    with open(path, "rb") as fp:
        assert fp.read() == EOF_BLOCK


# ---- 6. the command line -------------------------------------------------------------------------------------------------------
def test_view_mode_writes_the_restated_bytes(case, tmp_path):
    out, names_file, empty_file = str(tmp_path / "out.bam"), str(tmp_path / "names.txt"), str(tmp_path / "none.txt")
    with open(names_file, "w") as fp:
        fp.write("r1\n\nchim\nhuge\nnoseq\nnot_there\n")
    open(empty_file, "w").close()
    argv = ["view", "--lr_bam", case["path"], "--device", "cpu", "--output", out]
    payload = lambda *a, **kw: case["header"] + b"".join(want_records(case, *a, **kw)[1])
    assert CoRAL.main(argv) == out
    assert gunzip(out) == case["raw"] and not os.path.exists(out + ".bai")
    CoRAL.main(argv + ["--names_file", names_file, "--reads_exclude_flags", "0x800", "--level", "0"])
    assert gunzip(out) == payload(None, {"r1", "chim", "huge", "noseq"}, 0x800)
    CoRAL.main(argv + ["--region", "chr3:1000-2000", "--region", "chr5:100-200", "--filter_min_mapq", "5"])
    kept = [r for r in case["parsed"].recs if r["mapq"] >= 5]
    want = want_records(case, [("chr3", 1000, 2000), ("chr5", 100, 200)], None, 0, recs=kept)
    assert gunzip(out) == case["header"] + b"".join(want[1]) and "on_chr5" not in want[0] and len(want[0]) >= 6
    CoRAL.main(argv + ["--region", "chr8:10,000-31,000", "--index"])
    sel = want_records(case, [("chr8", 10_000, 31_000)])
    assert gunzip(out) == case["header"] + b"".join(sel[1]) and len(sel[0]) > 40
    idx = bam.read_index(out + ".bai")
    assert_records(bam.extract_records(out, [("chr8", 30_000, 30_300)], device="cpu", index=idx), want_records(case, [("chr8", 30_000, 30_300)]))
    CoRAL.main(argv + ["--names_file", empty_file])
    assert gunzip(out) == case["header"]
    a = CoRAL.build_parser().parse_args(["view", "--lr_bam", "x.bam", "--output", "o.bam"])
    assert a.reads_exclude_flags == 0 and a.level == 1 and a.index is False and a.region is None and a.names_file is None and a.filter_min_length == 0


# ---- 7. Python argument rules --------------------------------------------------------------------------------------------------
def test_python_argument_rules(case, tmp_path):
    for kw in (dict(exclude_flags=-1), dict(exclude_flags=0x10000), dict(exclude_flags=True), dict(names=[""]), dict(names=["a" * 255]),
               dict(regions=[("chrNone", 0, 5)]), dict(regions=[("chr3", 5, 1)])):
        with pytest.raises(ValueError):
            bam.extract_records(case["plain"], device="cpu", **kw)
    with pytest.raises(ValueError):
        bam.merge_record_bytes([])
    a = bam.extract_records(case["plain"], names=["r1"], device="cpu")
    with pytest.raises(ValueError):
        bam.merge_record_bytes([a, bam.RecordBytes(a.data, a.offsets, a.header + b"\0")])
    with pytest.raises(ValueError):
        bam.merge_record_bytes([a, bam.RecordBytes()])
    assert bam.merge_record_bytes([a, a]).n == 2 * a.n == 4
    with pytest.raises(ValueError):
        bam.RecordBytes(np.zeros(3, dtype=np.uint8), np.array([0, 2]))
    for level in (-1, 10, True, 1.5):
        with pytest.raises(ValueError):
            a.write(str(tmp_path / "x.bam"), level=level)
