"""The reads request of the BAM decode (bam.extract_reads, want_reads of a coral_bam_request_t): the selected records as FASTQ
text, on both pipelines.

Every expected byte comes from a restatement of the rule in this module, on records read with tests/bamfile.py (gzip + struct):
a record is written when l_seq > 0, flag & exclude_flags == 0, with regions: tid >= 0 and [pos, bam_endpos) meets a region,
with names: its name is listed; its text is `@name\\nSEQ\\n+\\nQUAL\\n` with "=ACMGRSVTWYHKDBN"[code], min(q, 93) + 33, '"' for a
record whose first QUAL byte is 0xff, and for flag 0x10 SEQ reversed and complemented (the 4 bits of a code reversed), QUAL
reversed.  Nothing here has passed through either decoder."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest
import torch

from coral_amd import CoRAL, _lib, bam, synth
from tests.bamfile import D, EQ, H, I, M, N, S, X, parse, read_bam
from tests.decode_support import (CORAL_ERR_ARG, CORAL_OK, DEVICE, PIPELINES, _pipeline_by_device, assert_same_qc,  # noqa: F401
                                  gpu_open_only)

SEQ_CHARS = "=ACMGRSVTWYHKDBN"
COMPLEMENT = [int("{:04b}".format(c)[::-1], 2) for c in range(16)]
LENGTHS = (1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 16383, 16384, 16385, 32769)
HUGE = 300_000
EDGE_QUAL = (0, 93, 94, 200, 254)
NO_QUAL_LENGTHS = (3, 64, 16385)              # forward records written without QUAL (0xff throughout)
REGIONS = [("chr3", 1000, 2000), ("chr3", 1500, 1800), ("chr3", 5000, 6000), ("chr5", 100, 200), ("chr4", 0, 1000)]
SMALL_BATCH = 1 << 16                          # (the decoder's smallest batch is 1 MiB)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def end_of(r):
    rlen = sum(int(w >> 4) for w in r["ops"] if int(w & 15) in (M, D, N, EQ, X))
    if r["flag"] & 4 or len(r["ops"]) == 0:
        rlen = 0
    return r["pos"] + max(rlen, 1)


def fastq_of(r):
    codes, qual = np.asarray(r["codes"], dtype=np.int64), np.asarray(r["qual"], dtype=np.int64)
    absent = qual[0] == 0xFF
    if r["flag"] & 0x10:
        codes, qual = np.array(COMPLEMENT)[codes[::-1]], qual[::-1]
    seq = np.frombuffer(SEQ_CHARS.encode(), dtype=np.uint8)[codes].tobytes()
    q = b'"' * len(codes) if absent else (np.minimum(qual, 93) + 33).astype(np.uint8).tobytes()
    return b"@" + r["name"].encode() + b"\n" + seq + b"\n+\n" + q + b"\n"


def written(r, refs, regions, names, exclude_flags):
    if r["l_seq"] == 0 or r["flag"] & exclude_flags:
        return False
    if regions is not None:
        end = end_of(r)
        if r["tid"] < 0 or not any(refs[r["tid"]] == c and a < b and r["pos"] < b and end > a for c, a, b in regions):
            return False
    return names is None or r["name"] in names


def want_reads(parsed, regions=None, names=None, exclude_flags=0x900, recs=None):
    """(names of the written records, their texts)"""
    sel = [r for r in (parsed.recs if recs is None else recs) if written(r, parsed.refs, regions, names, exclude_flags)]
    return [r["name"] for r in sel], [fastq_of(r) for r in sel]


def assert_reads(got, want, what=""):
    names, texts = want
    assert got.n == len(texts), (what, got.n, len(texts), got.names()[:20], names[:20])
    off = got.offsets.tolist()
    raw = got.text.tobytes()
    for k, t in enumerate(texts):                      # record by record first: a failure names the record
        assert raw[off[k]:off[k + 1]] == t, (what, k, names[k][:20], len(t))
    assert raw == b"".join(texts) and off[-1] == len(raw) and got.offsets.dtype == np.int64 and got.text.dtype == np.uint8, what


# ---- the file ------------------------------------------------------------------------------------------------------------------
def long_name(k):
    return ("N%03d" % k) + "x" * 250                  # 254 bytes


def alignments():
    big = [(M, 3), (I, 1), (D, 2)] * 22000 + [(M, 5)]            # 66001 ops -> CG tag; the record's own n_cigar_op is 2
    alns = [
        # chr3 (tid 2): selection by region [1000, 2000), [5000, 6000)
        dict(tid=2, pos=900, cigar=[(M, 100)], name="ends_at_start"),                    # [900, 1000): not in
        dict(tid=2, pos=950, cigar=[(M, 100)], name="r1"),
        dict(tid=2, pos=999, cigar=[(M, 60)], flag=4, name="unmapped_before"),          # [999, 1000) whatever its CIGAR: not in
        dict(tid=2, pos=1100, cigar=[(M, 50)], flag=0x100, name="r10"),
        dict(tid=2, pos=1200, cigar=[(H, 20), (M, 30)], flag=0x800, name="chim"),        # the supplementary: its primary is on chr8
        dict(tid=2, pos=1300, cigar=[(M, 33)], flag=0x400, name="r1a"),
        dict(tid=2, pos=1400, cigar=[(M, 200)], has_seq=0, name="noseq"),
        dict(tid=2, pos=1500, cigar=[(S, 3), (M, 40), (D, 10), (M, 7)], flag=0x10, name="r1"),
        dict(tid=2, pos=1999, cigar=[(M, 60)], flag=4, name="unmapped_edge"),           # [1999, 2000): in
        dict(tid=2, pos=2000, cigar=[(M, 100)], name="starts_at_end"),                   # [2000, 2100): not in
        dict(tid=2, pos=2000, cigar=[(M, 60)], flag=4, name="unmapped_after"),
        dict(tid=2, pos=4990, cigar=[(M, 5), (N, 100), (M, 5)], name="spliced"),         # [4990, 5100): in by its N
        dict(tid=2, pos=5999, cigar=[(M, 1)], flag=0x10, name="last_base"),
        dict(tid=2, pos=7000, cigar=[(M, 37)], name="codes_f"),
        dict(tid=2, pos=7001, cigar=[(M, 37)], flag=0x10, name="codes_r"),
        dict(tid=2, pos=7002, cigar=[(M, 21)], flag=0x10, name="ff_first"),
        # chr5 (tid 4)
        dict(tid=4, pos=150, cigar=[(M, 20)], name="on_chr5", mapq=3),
        dict(tid=4, pos=300, cigar=[(M, 20)], name="off_chr5"),
    ]
    k = 0
    for ln in LENGTHS:                                # chr8 (tid 7): every length forward (1-byte name) and reverse (254-byte name)
        alns.append(dict(tid=7, pos=10_000 + 2 * k, cigar=[(M, ln)], name=chr(65 + k), mapq=10 + k))
        alns.append(dict(tid=7, pos=10_001 + 2 * k, cigar=[(M, ln)], flag=0x10, name=long_name(k)))
        k += 1
    alns += [dict(tid=7, pos=20_000, cigar=big, flag=0x10, name="longcigar"),
             dict(tid=7, pos=20_010, cigar=[(S, 100), (M, HUGE - 100)], flag=0x10, name="huge"),
             dict(tid=7, pos=900_000, cigar=[(M, 500)], name="chim"),
             dict(tid=24, pos=16000, cigar=[(M, 50)], name="mito"),
             dict(tid=-1, pos=-1, cigar=[], flag=4, qlen=45, name="nowhere")]
    return alns


def qual_of(name, n):
    """The QUAL bytes the file is written with; None: absent."""
    if name in ("unmapped_edge", "spliced") or (len(name) == 1 and n in NO_QUAL_LENGTHS):
        return None
    k = np.arange(n, dtype=np.int64)
    q = np.where(k % 3 == 0, np.array(EDGE_QUAL)[(k // 3) % 5], (7 * k + 3 + len(name)) % 95)
    if name == "ff_first":
        q[0] = 0xFF                                   # a real QUAL whose first byte is 0xff: absent by the rule
    return q.astype(np.uint8).tobytes()


def patch_codes(raw, parsed):
    """All 16 SEQ codes into the two codes_* records (write_bam only makes A, C, G, T and N)."""
    raw = bytearray(raw)
    for r in parsed.recs:
        if r["name"].startswith("codes_"):
            codes = [(7 * k + 3) % 16 for k in range(r["l_seq"])] + [0]
            assert set(codes[:-1]) == set(range(16))
            at = r["start"] + 36 + len(r["name"]) + 1 + 4 * r["n_cig"]
            for k in range((r["l_seq"] + 1) // 2):
                raw[at + k] = (codes[2 * k] << 4) | codes[2 * k + 1]
    return bytes(raw)


def write_raw(raw, path, **kw):
    with open(path, "wb") as fp:
        for blk in bam._bgzf_blocks(raw, **kw):
            fp.write(blk)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("extract_reads")
    rec = synth.records_from_alignments(alignments())
    names = rec.materialise_names()
    name_of = lambda i: names[int(rec.name_id[i])]
    l_seq = lambda i: int(rec.qlen[i]) if int(rec.has_seq[i]) else 0
    first = str(d / "first.bam")
    bam.write_bam(rec, first, seed=11, fast_seq=True, qual=lambda i: qual_of(name_of(i), l_seq(i)))
    with gzip.open(first, "rb") as fp:
        raw = fp.read()
    raw = patch_codes(raw, parse(raw))
    path, plain = str(d / "reads.bam"), str(d / "reads_plain.bam")
    write_raw(raw, path, block_size=1500, empty_block_every=5)
    write_raw(raw, plain)
    parsed = read_bam(path)
    assert len(parsed.recs) == rec.n and read_bam(plain).recs[5]["name"] == parsed.recs[5]["name"]
    by_name = {r["name"]: r for r in parsed.recs}
    assert by_name["longcigar"]["n_cig"] == 2 and len(by_name["longcigar"]["ops"]) == 66001
    assert set(by_name["codes_f"]["codes"].tolist()) == set(range(16)) and by_name["ff_first"]["qual"][0] == 0xFF
    huge = by_name["huge"]                            # straddles the first 1 MiB of the inflated stream: two GPU batches
    assert huge["l_seq"] == HUGE and huge["start"] < (1 << 20) - 20_000 and huge["start"] + huge["size"] > (1 << 20) + 20_000
    return dict(dir=d, raw=raw, path=path, plain=plain, parsed=parsed)


def extract(pipe, path, *args, **kw):
    if pipe == "gpu":
        kw.setdefault("batch_bytes", SMALL_BATCH)
    kw.setdefault("index", False)
    got = bam.extract_reads(path, *args, device=DEVICE[pipe], n_threads=2, **kw)
    if pipe == "gpu":                                  # (an index that names no block for the regions: nothing is decoded at all)
        assert bam.LAST_DECODE.get("where") == "gpu" or (bam.LAST_DECODE["blocks"] == 0 and got.n == 0 and kw["index"])
    return got


# ---- 1. the text ---------------------------------------------------------------------------------------------------------------
def test_complement_is_an_involution():
    assert sorted(COMPLEMENT) == list(range(16)) and all(COMPLEMENT[COMPLEMENT[c]] == c for c in range(16))
    assert [SEQ_CHARS[COMPLEMENT[SEQ_CHARS.index(c)]] for c in "ACGTN=MRWSYKVHDB"] == list("TGCAN=KYWSRMBDHV")


@pytest.mark.parametrize("pipe", PIPELINES)
def test_every_read_is_everything_concatenated(case, pipe):
    """Neither regions nor names, no flag excluded: every record with SEQ, in file order - every length forward and reverse,
    names of 1 and 254 bytes, QUAL real / absent / absent by its first byte, all 16 codes, the CG-tag record."""
    parsed = case["parsed"]
    for path in (case["path"], case["plain"]):
        got = extract(pipe, path, exclude_flags=0)
        want = want_reads(parsed, exclude_flags=0)
        assert_reads(got, want, path)
        assert len(want[1]) == len(parsed.recs) - 1 and b"".join(want[1]) == b"".join(fastq_of(r) for r in parsed.recs if r["l_seq"])
        if pipe == "gpu" and path == case["path"]:
            assert bam.LAST_DECODE["batches"] >= 2            # the 300 000-base record straddles two of them
    lens = {r["l_seq"] for r in parsed.recs}
    assert set(LENGTHS) | {HUGE} <= lens
    assert got.names() == want[0] and len(got) == got.n
    for (name, seq, qual), wname, text in zip(got, want[0], want[1]):
        assert (name, len(seq), len(qual)) == (wname, (len(text) - len(wname) - 6) // 2, len(seq))
    by_name = dict(zip(want[0], want[1]))
    assert by_name["ff_first"].endswith(b"\n+\n" + b'"' * 21 + b"\n")        # pinned: a first QUAL byte of 0xff means no quality
    assert by_name["D"].count(b"~") >= 3                                       # 93, and 94, 200 and 254 clamped to it: '~'


@pytest.mark.parametrize("pipe", PIPELINES)
def test_default_leaves_out_secondary_and_supplementary(case, pipe):
    got = extract(pipe, case["path"])
    want = want_reads(case["parsed"])
    assert_reads(got, want)
    assert "r10" not in want[0] and want[0].count("chim") == 1


# ---- 2. selection --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exclude_flags", [0x900, 0, 0xF04])
@pytest.mark.parametrize("pipe", PIPELINES)
def test_regions_and_flags(case, pipe, exclude_flags):
    """Several segments on two contigs (two of them overlap and are merged), a contig without reads; records that end exactly at a
    segment's start or start exactly at its end, unmapped records at a region's edge, a record without SEQ."""
    want = want_reads(case["parsed"], REGIONS, None, exclude_flags)
    assert_reads(extract(pipe, case["path"], REGIONS, exclude_flags=exclude_flags), want, exclude_flags)
    base = ["r1", "r1", "spliced", "last_base", "on_chr5"]
    extra = {0x900: ["unmapped_edge", "r1a"], 0: ["r10", "chim", "r1a", "unmapped_edge"], 0xF04: []}[exclude_flags]
    assert sorted(want[0]) == sorted(base + extra)
    for absent in ("ends_at_start", "starts_at_end", "unmapped_before", "unmapped_after", "noseq", "off_chr5"):
        assert absent not in want[0]


@pytest.mark.parametrize("pipe", PIPELINES)
def test_names(case, pipe):
    parsed = case["parsed"]
    # the supplementary of `chim` lies in the region, its primary (the whole read) does not: by name it is found
    got = extract(pipe, case["path"], names=["chim"])
    assert_reads(got, want_reads(parsed, names={"chim"}))
    assert got.n == 1 and len(got.text) == 2 * 500 + 4 + 6
    assert extract(pipe, case["path"], [("chr3", 1000, 2000)], exclude_flags=0).names().count("chim") == 1
    # names that are prefixes of each other, a name that is not in the file, duplicates, str and bytes
    for names in (["r1"], ["r10"], ["r1a", "r1"], ["r1", "r10", "r1a", "r", "r1b", "zzz"], [b"r10", "r10", "A", long_name(3), long_name(3)[:-1]]):
        want = want_reads(parsed, names={n.decode() if isinstance(n, bytes) else n for n in names}, exclude_flags=0)
        assert_reads(extract(pipe, case["path"], names=names, exclude_flags=0), want, names)
        assert len(want[0]) > 0
    assert want[0] == ["r10", "A", long_name(3)]
    # regions and names intersect
    want = want_reads(parsed, REGIONS, {"r1", "on_chr5", "mito", "starts_at_end"}, 0)
    assert_reads(extract(pipe, case["path"], REGIONS, ["r1", "on_chr5", "mito", "starts_at_end"], 0), want)
    assert want[0] == ["r1", "r1", "on_chr5"]


@pytest.mark.parametrize("pipe", PIPELINES)
def test_empty_selections(case, pipe, tmp_path):
    for got in (extract(pipe, case["path"], names=["not_in_the_file"]), extract(pipe, case["path"], [("chr4", 0, 1000)]),
                extract(pipe, case["path"], REGIONS, ["mito"]), extract(pipe, case["path"], [("chr3", 10, 10)]),
                extract(pipe, case["path"], names=["r10"])):
        assert got.n == 0 and len(got.text) == 0 and got.offsets.tolist() == [0] and list(got) == []
    # an empty list selects nothing and the file is not opened
    for kw in (dict(regions=[]), dict(names=[]), dict(regions=[], names=["A"])):
        assert bam.extract_reads(str(tmp_path / "no_such_file.bam"), device=DEVICE[pipe], **kw).n == 0
    # a file whose records are all unselected
    recs = [r for r in case["parsed"].recs if r["name"] in ("noseq", "r10", "chim") and r["tid"] == 2]
    first = case["parsed"].recs[0]["start"]
    raw = case["raw"][:first] + b"".join(case["raw"][r["start"]:r["start"] + r["size"]] for r in recs)
    path = str(tmp_path / "unselected.bam")
    write_raw(raw, path)
    assert [r["name"] for r in read_bam(path).recs] == ["r10", "chim", "noseq"]
    assert extract(pipe, path).n == 0 and extract(pipe, path, exclude_flags=0).n == 2


# ---- 3. composition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", PIPELINES)
def test_record_filter_acts_first(case, pipe, tmp_path):
    """The result is that of a file that holds only the kept records (cut out of the inflated stream by the test)."""
    parsed, f = case["parsed"], bam.RecordFilter(min_mapq=11, min_seq_length=16, exclude_flags=0x400)
    kept = [r for r in parsed.recs if r["mapq"] >= 11 and r["l_seq"] >= 16 and not r["flag"] & 0x400]
    assert 0 < len(kept) < len(parsed.recs)
    raw = case["raw"][:parsed.recs[0]["start"]] + b"".join(case["raw"][r["start"]:r["start"] + r["size"]] for r in kept)
    path = str(tmp_path / "kept.bam")
    write_raw(raw, path, block_size=1500, empty_block_every=5)
    for kw in (dict(exclude_flags=0), dict(regions=REGIONS + [("chr8", 0, 1_000_000)], exclude_flags=0x100)):
        want = want_reads(parsed, kw.get("regions"), None, kw["exclude_flags"], recs=kept)
        assert_reads(extract(pipe, case["path"], record_filter=f, **kw), want, kw)
        assert_reads(extract(pipe, path, **kw), want, kw)
        assert len(want[0]) > 3


@pytest.mark.parametrize("world", [2, 3, 5])
@pytest.mark.parametrize("pipe", PIPELINES)
def test_byte_ranges_concatenate(case, pipe, world):
    for kw in (dict(exclude_flags=0), dict(names=["r1", "huge", "A", "mito"], exclude_flags=0x900)):
        parts = [extract(pipe, case["path"], rank=r, world=world, **kw) for r in range(world)]
        names = set(kw["names"]) if "names" in kw else None
        assert_reads(bam.merge_reads(parts), want_reads(case["parsed"], None, names, kw["exclude_flags"]), (world, kw))


@pytest.mark.parametrize("pipe", PIPELINES)
def test_index_cuts_the_decode_down_to_the_regions(case, pipe, tmp_path):
    path = str(tmp_path / "indexed.bam")
    write_raw(case["raw"], path, block_size=1500, empty_block_every=5)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("CORAL_BAM_DECODE", "cpu")
        bai = bam.build_index(path, device="cpu")
    whole = extract(pipe, path, REGIONS, exclude_flags=0)
    blocks_whole = bam.LAST_DECODE["blocks"]
    for index in (bai, None):                          # given, and found beside the file
        got = extract(pipe, path, REGIONS, exclude_flags=0, index=index)
        assert bam.LAST_DECODE["index"] == bai and 0 < bam.LAST_DECODE["blocks"] < blocks_whole
        assert got.n == whole.n > 0 and np.array_equal(got.text, whole.text) and np.array_equal(got.offsets, whole.offsets)
    assert_reads(got, want_reads(case["parsed"], REGIONS, None, 0))
    assert extract(pipe, path, [("chr4", 0, 1000)], index=bai).n == 0


@pytest.mark.parametrize("pipe", PIPELINES)
def test_rides_with_read_qc_and_a_pileup(case, pipe):
    """One decode with three requests gives what each gives alone (on the GPU they borrow the same scratch arrays in turn)."""
    dev = DEVICE[pipe]
    kw = dict(batch_bytes=SMALL_BATCH) if pipe == "gpu" else {}
    refs = bam.bam_reference_names(case["path"])
    _, segs = bam.pileup_regions(REGIONS + [("chr8", 10_000, 21_000)], refs)
    _, rsegs = bam.pileup_regions(REGIONS, refs)
    reads = (0, rsegs, [b"A", b"huge", b"r1"])
    both = bam._decode(case["path"], dev, n_threads=2, qc=True, coverage=(segs, 10, 0), per_base=True, reads=(0, None, reads[2]), records=False, **kw)
    qc = bam._decode(case["path"], dev, n_threads=2, qc=True, records=False, **kw).qc
    pile = bam._decode(case["path"], dev, n_threads=2, coverage=(segs, 10, 0), per_base=True, records=False, **kw)
    alone = bam._decode(case["path"], dev, n_threads=2, reads=(0, None, reads[2]), records=False, **kw).reads
    assert_same_qc(both.qc, qc)
    assert np.array_equal(both.pileup, pile.pileup) and np.array_equal(both.counts, pile.counts) and int(pile.counts.sum()) > 0
    assert np.array_equal(both.reads[0], alone[0]) and np.array_equal(both.reads[1], alone[1])
    assert_reads(bam.Reads(*both.reads), want_reads(case["parsed"], None, {"A", "huge", "r1"}, 0))
    with_regions = bam._decode(case["path"], dev, n_threads=2, qc=True, coverage=(segs, 10, 0), per_base=True, reads=reads, **kw)
    assert_reads(bam.Reads(*with_regions.reads), want_reads(case["parsed"], REGIONS, {"A", "huge", "r1"}, 0))
    assert with_regions.records.n == len(case["parsed"].recs) and np.array_equal(with_regions.pileup, pile.pileup)
    assert bam._decode(case["path"], dev, n_threads=2, records=False, **kw).reads is None


# ---- 4. the request's rules, equal on both pipelines (neither call needs a GPU) ---------------------------------------------------
I32 = lambda *rows: np.array(rows, dtype=np.int32)
BAD_REQUESTS = {
    "unsorted segments": (dict(reads=(0, I32([2, 2], [500, 100], [600, 200]), None)), "reads_seg"),
    "segments out of contig order": (dict(reads=(0, I32([3, 2], [0, 0], [10, 10]), None)), "reads_seg"),
    "overlapping segments": (dict(reads=(0, I32([2, 2], [100, 150], [200, 300]), None)), "reads_seg"),
    "segment with end < start": (dict(reads=(0, I32([2], [100], [50]), None)), "reads_seg"),
    "unsorted names": (dict(reads=(0, None, [b"b", b"a"])), "reads_names"),
    "a prefix behind its extension": (dict(reads=(0, None, [b"r10", b"r1"])), "reads_names"),
    "duplicate names": (dict(reads=(0, None, [b"a", b"a"])), "reads_names"),
    "a name of 0 bytes": (dict(reads=(0, None, [b"", b"a"])), "reads_names"),
    "a name of 255 bytes": (dict(reads=(0, None, [b"a", b"b" * 255])), "reads_names"),
    "exclude_flags < 0": (dict(reads=(-1, None, None)), "reads_exclude_flags"),
    "exclude_flags > 0xffff": (dict(reads=(0x10000, None, None)), "reads_exclude_flags"),
    "with an index request": (dict(reads=(0, None, None), index=True), "want_reads"),
}
GOOD_REQUESTS = [dict(reads=(0xFFFF, I32([2, 2, 4], [100, 200, 0], [200, 300, 5]), [b"a", b"a" * 254, b"ab", b"b"])),
                 dict(reads=(0, I32([2], [7], [7]), None), spans=np.zeros((0, 2), dtype=np.uint64)),
                 dict(reads=(0, None, [b"r1", b"r10", b"r1a"]), qc=True, depth=(1000, 0, 0, 1), keep=(1, 2, 0, 4)), dict()]


def test_a_zero_struct_requests_nothing(case):
    zero = _lib.coral_bam_request_t()
    names = [f[0] for f in _lib.coral_bam_request_t._fields_]
    assert names[names.index("depth_count_deletions") + 1] == "want_reads" and names[names.index("keep_min_mapq") - 1] == "reads_name_off"
    assert (zero.want_reads, zero.reads_exclude_flags, zero.reads_n_seg, zero.reads_n_names) == (0, 0, 0, 0)
    req = _lib.bam_request()
    assert (req.want_reads, req.reads_n_seg, req.reads_n_names, req.reads_names) == (0, 0, 0, None)
    L, h = _lib.lib(), C.c_void_p()
    assert L.coral_bam_decode_request(case["plain"].encode(), 2, C.byref(req), C.byref(h)) == CORAL_OK
    try:
        sz = (C.c_int64 * 2)()
        assert L.coral_bam_reads_sizes(h, sz) == CORAL_ERR_ARG and "no reads request" in L.coral_bam_last_error().decode()
    finally:
        L.coral_bam_decode_close(h)


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


def test_workspace_grows_only_with_the_request(case):
    plain = gpu_open_only(case["plain"])[2]
    assert plain == gpu_open_only(case["plain"], qc=False)[2] == gpu_open_only(case["plain"], batch_bytes=0)[2] > 0
    asked = gpu_open_only(case["plain"], reads=(0x900, None, None))[2]
    # one output buffer of 4/3 of a batch's capacity, the 64 MiB of carried bytes included, + 256 (a batch is at least 16 MiB and
    # never more than six times the file + 64 MiB + a block)
    size = os.path.getsize(case["plain"])
    assert ((64 << 20) + (16 << 20)) // 3 * 4 + 256 <= asked - plain <= ((128 << 20) + 6 * size + (1 << 16)) // 3 * 4 + 4096
    assert gpu_open_only(case["plain"], reads=(0x900, I32([2], [0], [9]), [b"abc"]))[2] > asked


# ---- 5. the command line -------------------------------------------------------------------------------------------------------
def test_fastq_mode_writes_the_restated_bytes(case, tmp_path):
    out, names_file = str(tmp_path / "out.fastq"), str(tmp_path / "names.txt")
    with open(names_file, "w") as fp:
        fp.write("r1\n\nchim\nhuge\nnot_there\n")
    argv = ["fastq", "--lr_bam", case["path"], "--device", "cpu", "--output", out]
    assert CoRAL.main(argv) == out
    assert open(out, "rb").read() == b"".join(want_reads(case["parsed"])[1])
    CoRAL.main(argv + ["--names_file", names_file, "--reads_exclude_flags", "0x100"])
    assert open(out, "rb").read() == b"".join(want_reads(case["parsed"], None, {"r1", "chim", "huge"}, 0x100)[1])
    CoRAL.main(argv + ["--region", "chr3:1000-2000", "--region", "chr5:100-200", "--reads_exclude_flags", "0", "--filter_min_mapq", "5"])
    kept = [r for r in case["parsed"].recs if r["mapq"] >= 5]
    want = want_reads(case["parsed"], [("chr3", 1000, 2000), ("chr5", 100, 200)], None, 0, recs=kept)
    assert open(out, "rb").read() == b"".join(want[1]) and "on_chr5" not in want[0] and len(want[0]) >= 5
    a = CoRAL.build_parser().parse_args(["fastq", "--lr_bam", "x.bam", "--output", "o.fq"])
    assert a.reads_exclude_flags == 0x900 and a.region is None and a.names_file is None and a.filter_min_length == 0


def test_python_argument_rules(case):
    for kw in (dict(exclude_flags=-1), dict(exclude_flags=0x10000), dict(exclude_flags=True), dict(names=[""]), dict(names=["a" * 255]),
               dict(regions=[("chrNone", 0, 5)]), dict(regions=[("chr3", 5, 1)])):
        with pytest.raises(ValueError):
            bam.extract_reads(case["plain"], device="cpu", **kw)
    with pytest.raises(ValueError):
        bam.merge_reads([])
    with pytest.raises(ValueError):
        bam.Reads(np.zeros(3, dtype=np.uint8), np.array([0, 2]))
