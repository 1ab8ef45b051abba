"""The GPU BAM decoder's record-boundary search (k_bam_find / k_bam_verify / k_bam_starts) against files BUILT to break it: QUAL
bytes that hold chains of well-formed record images ("decoys") at every 128 KiB segment edge, record starts placed byte-exactly
around segment and batch edges, a record longer than the 64-segment window of k_bam_verify, and a malformed record on the true
chain.  The expected result of every whole-file decode is the input itself (``assert_same`` against the Records handed to
``write_bam``), on the host pipeline and on the GPU.

That the plants bite is proven without a GPU by a restatement in this module (``Stream``): the true record starts by hopping
along block_size, ``plausible_record`` and the chained check of k_bam_find restated in plain Python over the gzip-read bytes,
hence the guess (first, land, count) of every segment of a single-batch decode - which puts the file at buffer offset CARRY_CAP,
a multiple of the segment size, so that segment edges are multiples of 128 KiB of the uncompressed stream.

Two shapes the cases could NOT take, and why:
  * a decoy in front of the first record (in the header's @CO text): ``plausible_record`` wants refID in [-1, n_ref), whose four
    little-endian bytes are ff ff ff ff or hold three NUL bytes - printable bytes cannot pass, so there is no such case;
  * records of 36 bytes, and record starts 35 / 36 bytes in front of the end of the FILE's data: a record that both pipelines
    accept has a name of at least one character plus its NUL (l_read_name 0 is "record fields overrun the record"), so the
    shortest one is 38 bytes (block_size 34, the lower bound of ``plausible_record``) and no record starts nearer to the end of
    the file than that.  The minimum records here are those 38 bytes, the file ends with one, and the 35 / 36 byte distances
    (and 2: a block_size word cut in two) are taken from the end of a BATCH's data instead, where they can occur: with
    ``batch_bytes = 1 << 20`` and BGZF blocks of 0xff00 bytes a batch holds 16 blocks, so batches end at multiples of 1 044 480
    (the file's last, shorter block is kept above the 4 096 bytes that would still fit behind them)."""
import bisect
import gzip
import re
import struct

import numpy as np
import pytest

from coral_amd import _lib, bam, synth
from tests.bamfile import M, bgzf_blocks
from tests.decode_support import DEVICE, PIPELINES, _pipeline_by_device, assert_same_records as assert_same  # noqa: F401

SEG = 128 << 10                                # SEG_BYTES of coral_bamgpu.hip
BATCH = 16 * 0xff00                            # inflated bytes of a batch of batch_bytes = 1 << 20 (16 whole BGZF blocks)
DECOY_FILES = ("tail_tags", "tail_rejoins", "tail_zeros")
FILES = DECOY_FILES + ("edges", "long")
SMALL_BATCH = {"tail_tags": 1 << 20, "tail_rejoins": 1 << 20, "tail_zeros": 1 << 20, "edges": 1 << 20, "long": 2 << 20}
N_BIG, BIG_L_SEQ, MEDIUM_L_SEQ, ZEROS = 8, 650_000, 150_000, 256
MIN_RECORD = 38                                # 4 + 32 fixed bytes + the name "x" and its NUL

# a decoy: the 64-byte image of a well-formed record (block_size 60, refID 0, pos 5, name "x", no CIGAR, no SEQ, mates -1, one Z tag)
DECOY = struct.pack("<iiiBBHHHiiii", 60, 0, 5, 2, 0, 4680, 0, 0, 0, -1, -1, 0) + b"x\0" + b"XDZ" + b"decoy-decoy-decoy-deco" + b"\0"
assert len(DECOY) == 64

_HEADER_TEXT = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % cl for cl in zip(synth.CHROMS, synth.CHR_SIZES))
HEADER_BYTES = 12 + len(_HEADER_TEXT) + sum(len(c) + 9 for c in synth.CHROMS)      # what write_bam puts in front of the first record


# ---- the restatement -----------------------------------------------------------------------------------------------------------
class Guess:
    """What k_bam_find leaves for one segment: the first position from which 3..8 plausible records chain, where the hop along
    block_size from there lands, how many records it counts - ``withdrawn`` when that hop meets a length below 36 (seg_first = -1)."""

    def __init__(self, first, land, count, withdrawn):
        self.first, self.land, self.count, self.withdrawn = first, land, count, withdrawn


class Stream:
    """The uncompressed stream of a BAM file and what a single-batch GPU decode makes of it, restated."""

    def __init__(self, path):
        raw = self.raw = gzip.open(path, "rb").read()
        self.n = len(raw)
        assert raw[:4] == b"BAM\x01"
        o = 8 + struct.unpack_from("<i", raw, 4)[0]
        self.n_ref = struct.unpack_from("<i", raw, o)[0]
        o += 4
        for _ in range(self.n_ref):
            o += 8 + struct.unpack_from("<i", raw, o)[0]
        self.first = o
        self.starts = []
        while o < self.n:
            self.starts.append(o)
            o += 4 + struct.unpack_from("<I", raw, o)[0]
        assert o == self.n
        # positions that can pass the first lines of `plausible` at all (block_size <= 2^29: top byte <= 0x20; refID in [-1, n_ref)) -
        # a necessary condition only, searched at C speed; the rule itself is `plausible`
        assert 0 < self.n_ref < 128
        maybe = re.compile(rb"(?s)(?=...[\x00-\x20](?:[\x00-" + re.escape(bytes([self.n_ref - 1])) + rb"]\x00\x00\x00|\xff\xff\xff\xff))")
        self.candidates = [m.start() for m in maybe.finditer(raw)]
        self._guess = {}

    def u32(self, q):
        return struct.unpack_from("<I", self.raw, q)[0]

    def plausible(self, q):
        """plausible_record (coral_bam_common.h) at q: the record's length, or None."""
        raw, avail = self.raw, self.n - q
        if avail < 36:
            return None
        bs, ref, pos, l_name, _mapq, _bin, n_cig, _flag, l_seq, mate, mpos = struct.unpack_from("<IiiBBHHHIii", raw, q)
        if bs < 34 or bs > 1 << 29:
            return None
        if ref < -1 or ref >= self.n_ref or mate < -1 or mate >= self.n_ref or pos < -1 or mpos < -1:
            return None
        if l_name < 2 or l_seq > 1 << 29:
            return None
        if 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
            return None
        if avail >= 36 + l_name:
            name = raw[q + 36:q + 36 + l_name]
            if name[-1] != 0 or any(c < 33 or c > 126 for c in name[:-1]):
                return None
        return 4 + bs

    def chains(self, q):
        """At least 3 and at most 8 plausible records in a row from q; the chain stops where fewer than 36 bytes remain."""
        k = 0
        while k < 8 and q + 36 <= self.n:
            ln = self.plausible(q)
            if ln is None:
                return False
            q += ln
            k += 1
        return k >= 3

    def hop(self, x, seg_end):
        """Along block_size from x while the record starts in front of seg_end and is complete: (landing, count, met a length < 36)."""
        count = 0
        while x < seg_end:
            if x + 4 > self.n:
                break
            ln = 4 + self.u32(x)
            if ln < 36:
                return x, count, True
            if x + ln > self.n:
                break
            count += 1
            x += ln
        return x, count, False

    def seg_end(self, s):
        return min((s + 1) * SEG, self.n)

    def guess(self, s):
        if s not in self._guess:
            a, b = max(s * SEG, self.first), self.seg_end(s)
            g = None
            for x in self.candidates[bisect.bisect_left(self.candidates, a):]:
                if x >= b or x + 36 > self.n:
                    break
                if self.chains(x):
                    g = Guess(x, *self.hop(x, b))
                    break
            self._guess[s] = g
        return self._guess[s]

    def entries(self):
        """{segment: the position the true chain enters it at} - its first record start; a segment without one is never entered."""
        out = {}
        for x in self.starts:
            out.setdefault(x // SEG, x)
        return out

    def verdicts(self):
        """(wrong, withdrawn, rewalked): the segments the true chain enters whose guess exists and is not the entry position; those
        whose guess was withdrawn; and every segment k_bam_verify has to walk itself (these and the ones without any guess)."""
        wrong = withdrawn = rewalked = 0
        for s, entry in self.entries().items():
            g = self.guess(s)
            if g is not None and g.withdrawn:
                withdrawn += 1
            elif g is not None and g.first != entry:
                wrong += 1
            rewalked += g is None or g.withdrawn or g.first != entry
        return wrong, withdrawn, rewalked


# ---- the files -----------------------------------------------------------------------------------------------------------------
class Layout:
    """Alignments for ``write_bam`` with every byte accounted for: ``off`` is where the next record starts in the uncompressed
    stream.  (The accounting is this module's claim about the writer; ``Stream`` reads the offsets back from the bytes.)"""

    def __init__(self):
        self.alns, self.behind, self.qual, self.nm_type = [], {}, {}, {}
        self.off = HEADER_BYTES
        self.marks = {}                            # name of a claim -> stream offset
        self.reads = []                            # the decoy reads: dict(tail, prefix, qual0, qual_end, end, l_seq)

    def add(self, name=None, cigar=(), l_seq=0, flag=0, end_at=None, qual=None, with_tags=False):
        """One record; ``end_at``: a trailing Z tag sized so that the record ends exactly there.  Returns its start."""
        i, start = len(self.alns), self.off
        name = "r%d" % i if name is None else name
        sa = [(1, 900, 1, 30, 10, 0, 0, 60, 1)] if with_tags else []
        size = 36 + len(name) + 1 + 4 * len(cigar) + (l_seq + 1) // 2 + l_seq
        if with_tags:                              # NM:i and SA:Z behind QUAL
            self.nm_type[i] = "i"
            size += 7 + 3 + len(synth.sa_entry_string(sa[0][:8], sa[0][8]) + ";") + 1
        if end_at is not None:
            pad = end_at - start - size
            assert pad >= 4, "no room for the padding tag"
            self.behind[i] = b"XPZ" + b"p" * (pad - 4) + b"\0"
            size += pad
        if qual is not None:
            assert len(qual) == l_seq
            self.qual[i] = qual
        self.alns.append(dict(tid=0, pos=1000 + 50 * i, cigar=list(cigar), name=name, flag=flag, has_seq=int(l_seq > 0),
                              nm=7 if with_tags else 0, sa=sa))
        self.off += size
        return start

    def short(self, count=1, end_at=None):
        for _ in range(count):
            i = len(self.alns)
            ln = 20 + i % 7
            start = self.add(cigar=[(M, ln)], l_seq=ln if i % 5 == 0 and end_at is None else 0, end_at=end_at)
        return start

    def minimal(self, count=1):
        for _ in range(count):
            start = self.add(name="x", flag=4)
        return start

    def fill_to(self, target):
        """Records up to ``target``, the last one ending exactly there: the next record starts at ``target``."""
        while target - self.off > 60_000:
            self.add(cigar=[(M, 30_000)], l_seq=30_000)
        while target - self.off > 200:
            self.short()
        self.short(end_at=target)
        assert self.off == target

    def decoy_read(self, tail, prefix, l_about):
        """A read whose QUAL is ``prefix`` bytes of 0x01 and then decoys back to back up to its end (tail "zeros": up to 256 zero
        bytes at its end).  ``prefix`` "edge": the length that puts a decoy's first byte on every segment edge.  l_seq is the
        largest one <= l_about at which the decoys tile QUAL exactly and QUAL ends 4 KiB or more away from a segment edge (so
        that the segment the read ends in starts with more than 8 decoys)."""
        name = "decoy%d" % len(self.alns)
        fixed = self.off + 36 + len(name) + 1 + 4
        for l_seq in range(l_about, l_about - 20_000, -1):
            qual0 = fixed + (l_seq + 1) // 2
            p = (-qual0) % 64 if prefix == "edge" else prefix
            if l_seq % 64 == p and 4096 <= (qual0 + l_seq) % SEG <= SEG - 4096:
                break
        else:
            raise AssertionError("no fitting l_seq")
        zeros = ZEROS if tail == "zeros" else 0
        qual = b"\x01" * p + DECOY * ((l_seq - p - zeros) // 64) + b"\0" * zeros
        self.add(name=name, cigar=[(M, l_seq)], l_seq=l_seq, qual=qual, with_tags=tail == "tags")
        self.reads.append(dict(tail=tail, prefix=p, qual0=qual0, qual_end=qual0 + l_seq, end=self.off, l_seq=l_seq, edge=prefix == "edge"))

    def records(self):
        return synth.records_from_alignments(self.alns)

    def write(self, path, decoys=True):
        bam.write_bam(self.records(), path, seed=5, fast_seq=True, nm_type=lambda i: self.nm_type.get(i),
                      aux=lambda i: (b"", self.behind.get(i, b"")), qual=(lambda i: self.qual.get(i)) if decoys else None)


def decoy_layout(kind):
    """Eight reads of about 1 MiB (650 000 bases) with decoy QUAL and the tail ``kind``, prefixes 0, "edge" and six others, short
    records between them and one run of 3 500 minimal records.  "tail_zeros" also holds eight reads of 150 000 bases whose
    decoys run into the next true record: its own tails withdraw their guesses, these give it wrong ones as well."""
    tail = kind[len("tail_"):]
    L = Layout()
    L.short(5)
    for j in range(N_BIG):
        L.decoy_read(tail, 0 if j == 0 else "edge" if j == 1 else (11 * j + 5) % 64, BIG_L_SEQ)
        L.short(30)
        if j == 3:
            L.minimal(3500)
        if tail == "zeros":
            L.decoy_read("rejoins", (5 * j + 1) % 64, MEDIUM_L_SEQ)
            L.short(20)
    L.short(10)
    return L


def edges_layout():
    L = Layout()
    L.short(3)
    for k, back in ((1, 0), (2, 1), (3, 2), (4, 3)):         # a start at byte 0 of a segment; 1, 2 and 3 bytes in front of an edge
        L.fill_to(k * SEG - back)
        L.marks["edge-%d" % back] = L.short()
    L.marks["minimal"] = L.minimal(3500)                      # more than a segment of the shortest records there are
    for k, back in ((1, 35), (2, 36), (3, 2)):                # in front of the end of a batch's data
        L.fill_to(k * BATCH - back)
        L.marks["batch-%d" % back] = L.short()
        if k == 1:
            L.fill_to(10 * SEG - 1000)
            L.marks["spanning"] = L.add(cigar=[(M, 200_000)], l_seq=200_000)      # 300 KB: segments 10 and 11 hold no record start
    L.fill_to(3 * BATCH + 20_000)                             # a last BGZF block too large to join the 16 blocks of the third batch
    L.short(20)
    L.marks["last"] = L.minimal()
    return L


def long_layout():
    L = Layout()
    L.short(50)
    L.fill_to(SEG + 70_000)
    L.marks["long"] = L.add(name="long", cigar=[(M, 6_000_000)], l_seq=6_000_000)      # 9 000 045 bytes: 68.7 segments
    L.short(50)
    return L


class Case:
    def __init__(self, kind, tmp):
        self.kind = kind
        self.layout = decoy_layout(kind) if kind in DECOY_FILES else edges_layout() if kind == "edges" else long_layout()
        self.records = self.layout.records()
        self.path = str(tmp / (kind + ".bam"))
        self.layout.write(self.path)
        self._tmp, self._stream, self._twin = tmp, None, None

    @property
    def stream(self):
        if self._stream is None:
            self._stream = Stream(self.path)
        return self._stream

    @property
    def twin(self):
        """The same records without decoys: QUAL all 0xff."""
        if self._twin is None:
            self._twin = str(self._tmp / (self.kind + ".twin.bam"))
            self.layout.write(self._twin, decoys=False)
        return self._twin


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    tmp, made = tmp_path_factory.mktemp("boundaries"), {}

    def get(kind):
        if kind not in made:
            made[kind] = Case(kind, tmp)
        return made[kind]
    return get


# ---- 1. the plants are what they claim (no GPU) --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", DECOY_FILES)
def test_decoy_plants_bite(kind, case):
    """Per decoy read, from the bytes: every segment wholly inside its QUAL has a guess within 64 bytes of its edge (on a decoy)
    and is never entered by the true chain; the segment the read ends in is entered at the next true record and its guess is a
    decoy that, by tail: stops inside the segment on the NM tag read as a block_size ("tags"), runs into the true records and
    lands where they do with another first and another count ("rejoins"), or is withdrawn on a length of 0 ("zeros").  So the
    file has at least 8 wrong guesses on the true chain; the "edge" read has a decoy starting on a segment edge, the first read
    no prefix; some segment holds thousands of records."""
    c = case(kind)
    S, entries = c.stream, c.stream.entries()
    assert S.first == HEADER_BYTES and len(S.starts) == c.records.n
    ignored = 0
    for r in c.layout.reads:
        assert S.raw[r["qual0"]:r["qual0"] + r["prefix"] + 64] == b"\x01" * r["prefix"] + DECOY
        tail_seg = r["qual_end"] // SEG
        inner = range(-(-(r["qual0"] + r["prefix"]) // SEG), tail_seg)
        assert len(inner) >= (3 if r["l_seq"] > 4 * SEG else 0)
        for s in inner:
            g = S.guess(s)
            assert s not in entries and g is not None and 0 <= g.first - s * SEG < 64 and S.raw[g.first:g.first + 64] == DECOY
            assert (g.first == s * SEG) == r["edge"]
            ignored += 1
        assert r["edge"] or r["prefix"] != (-r["qual0"]) % 64
        entry, g = entries[tail_seg], S.guess(tail_seg)
        assert entry == r["end"] and entry in S.starts
        assert g is not None and 0 <= g.first - tail_seg * SEG < 64 and g.first != entry
        true_land, true_count, _ = S.hop(entry, S.seg_end(tail_seg))
        decoys = (r["qual_end"] - (ZEROS if r["tail"] == "zeros" else 0) - g.first) // 64
        if r["tail"] == "tags":
            assert not g.withdrawn and (g.land, g.count) == (r["qual_end"], decoys) and S.raw[g.land:g.land + 3] == b"NMi"
            assert g.land < S.seg_end(tail_seg) and true_land >= S.seg_end(tail_seg)
        elif r["tail"] == "rejoins":
            assert r["end"] == r["qual_end"]
            assert not g.withdrawn and g.land == true_land and g.count == decoys + true_count and decoys >= 8
        else:
            assert r["end"] == r["qual_end"] and S.raw[r["qual_end"] - ZEROS:r["qual_end"]] == b"\0" * ZEROS
            assert g.withdrawn and (g.land, g.count) == (r["qual_end"] - ZEROS, decoys)
    big = [r for r in c.layout.reads if r["l_seq"] > 4 * SEG]
    assert len(big) == N_BIG and big[0]["prefix"] == 0 and big[1]["edge"] and len({r["prefix"] for r in big}) >= 6
    assert ignored >= 3 * N_BIG
    wrong, withdrawn, rewalked = S.verdicts()
    print("%s: %d bytes, %d records, wrong=%d withdrawn=%d rewalked(model)=%d" % (kind, S.n, len(S.starts), wrong, withdrawn, rewalked))
    assert wrong >= N_BIG
    assert withdrawn >= (N_BIG if kind == "tail_zeros" else 0)
    assert max(np.bincount(np.array(S.starts) // SEG)) >= 2000


def test_edge_plants_land_on_their_offsets(case):
    """The exact-offset claims of the "edges" and "long" files, read back from the bytes."""
    c = case("edges")
    S, mk, starts = c.stream, c.layout.marks, set(c.stream.starts)
    assert S.first == HEADER_BYTES and len(S.starts) == c.records.n
    assert mk["edge-0"] == SEG and mk["edge-1"] == 2 * SEG - 1 and mk["edge-2"] == 3 * SEG - 2 and mk["edge-3"] == 4 * SEG - 3
    assert mk["batch-35"] == BATCH - 35 and mk["batch-36"] == 2 * BATCH - 36 and mk["batch-2"] == 3 * BATCH - 2
    assert all(x in starts for x in mk.values())
    assert S.n // BATCH == 3 and S.n % BATCH > (1 << 20) - BATCH             # the last block does not fit behind a batch's 16: the third batch ends at 3 * BATCH
    prev = S.starts[S.starts.index(SEG) - 1]
    assert prev + 4 + S.u32(prev) == SEG                                    # a record ends exactly on the edge
    sizes = np.diff(np.array(S.starts + [S.n]))
    assert int(sizes.min()) == MIN_RECORD and int((sizes == MIN_RECORD).sum()) >= 3500
    assert mk["last"] == S.starts[-1] == S.n - MIN_RECORD                   # the nearest a record start gets to the end of the data
    entered = S.entries()
    assert mk["spanning"] // SEG == 9 and 9 in entered and 10 not in entered and 11 not in entered and 12 in entered
    c = case("long")
    S, at = c.stream, c.layout.marks["long"]
    size = 4 + S.u32(at)
    assert at in S.starts and size > 64 * SEG
    assert (at + size) // SEG - at // SEG > 64                              # k_bam_verify reloads its window of 64 segments on the way
    entered = S.entries()
    assert entered[at // SEG] < at and (at + size) // SEG in entered and S.starts[-1] > at + size


# ---- 2 + 3. whole files, both pipelines ----------------------------------------------------------------------------------------
def _decode(path, pipeline, **kw):
    res = bam._decode(path, DEVICE[pipeline], **kw)
    if pipeline == "gpu":
        assert bam.LAST_DECODE["where"] == "gpu"
    return res


@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("kind", FILES)
def test_decode_gives_the_records_back(kind, pipeline, case):
    """The round trip of every file; on the GPU in one batch - where k_bam_verify must have walked at least the segments the
    restatement says it has to - and in batches of 1 MiB (2 MiB for the 9 MiB record), where the big reads straddle batches, the
    chain starts from a carried known_start and (file "edges") records start 35, 36 and 2 bytes in front of a batch's end."""
    c = case(kind)
    assert_same(c.records, _decode(c.path, pipeline).records)
    if pipeline != "gpu":
        return
    one = dict(bam.LAST_DECODE)
    wrong, withdrawn, rewalked = c.stream.verdicts()
    print("%s: rewalked_segments=%d wrong=%d withdrawn=%d rewalked(model)=%d" % (kind, one["rewalked_segments"], wrong, withdrawn, rewalked))
    assert one["batches"] == 1
    assert one["rewalked_segments"] >= wrong + withdrawn
    if kind in DECOY_FILES:
        assert wrong >= 8
    assert_same(c.records, _decode(c.path, pipeline, batch_bytes=SMALL_BATCH[kind]).records)
    assert bam.LAST_DECODE["batches"] >= 2
    if kind == "edges":
        assert bam.LAST_DECODE["batches"] == -(-c.stream.n // BATCH)         # the batches end where the "batch-" records were put


def _linear(path, voff):
    """Virtual offsets -> offsets in the uncompressed stream (the twin's blocks compress differently; ~0 stays)."""
    data = open(path, "rb").read()
    table = {at: u for at, u, _ in bgzf_blocks(data)}
    table[len(data)] = sum(n for _, _, n in bgzf_blocks(data))
    return [v if v == 0xffffffffffffffff else table[v >> 16] + (v & 0xffff) for v in np.asarray(voff, dtype=np.uint64).tolist()]


@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("kind", DECOY_FILES)
def test_ride_alongs_equal_the_decoy_free_twin(kind, pipeline, case):
    """Window coverage, BAI index, read QC and binned depth of ONE decode of the decoy file against the same request on its twin
    (same records, QUAL all 0xff): a wrong rec_start corrupts these even where the record fields survive.  Left out: what
    legitimately differs - QC's QUAL sums, histogram and no-quality counter; the index's virtual offsets are compared as offsets
    in the uncompressed stream (and are record starts)."""
    c = case(kind)
    segs = bam.coverage_segments([("chr1", 0, 3_000_000), ("chr1", 1500, 40_000), ("chr1", 300_000, 300_001), ("chr2", 0, 1000)], synth.CHROMS)[0]
    ask = dict(coverage=(segs, 0, 0), index=True, qc=True, depth=(1000, 0, 0x704, 1))
    got, want = _decode(c.path, pipeline, **ask), _decode(c.twin, pipeline, **ask)
    assert_same(c.records, got.records)
    assert got.counts.sum() > 0 and np.array_equal(got.counts, want.counts)
    for a, b in zip(got.depth, want.depth):
        assert np.array_equal(a, b)
    assert got.depth[1].sum() > 0
    for k in ("length", "mapq", "flag"):
        assert np.array_equal(getattr(got.qc, k), getattr(want.qc, k)), k
    assert {k: v for k, v in got.qc.counters.items() if k != "n_no_qual"} == {k: v for k, v in want.qc.counters.items() if k != "n_no_qual"}
    assert got.qc.n_no_qual == want.qc.n_no_qual - len(c.layout.reads) and want.qc.n_no_qual == want.qc.n_reads == got.qc.n_reads > 0
    gi, wi = got.index, want.index
    for k in ("head_key", "n_mapped", "n_unmapped"):
        assert np.array_equal(gi[k], wi[k]), k
    for k in ("n_records", "n_no_coor", "first_sort", "last_sort"):
        assert gi[k] == wi[k], k
    for k in ("head_voff", "lin"):
        assert _linear(c.path, gi[k]) == _linear(c.twin, wi[k]), k
    assert _linear(c.path, [gi["end_voff"]]) == _linear(c.twin, [wi["end_voff"]]) == [c.stream.n]
    assert set(_linear(c.path, gi["head_voff"])) <= set(c.stream.starts)


# ---- 4. a malformed record on the true chain -----------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_malformed_record_on_the_true_chain(pipeline, tmp_path):
    """block_size = 20 in the 26th record (the stream re-blocked, so every CRC is valid): both pipelines say so, and decode a good
    file afterwards."""
    L = Layout()
    L.short(60)
    good, bad = str(tmp_path / "good.bam"), str(tmp_path / "bad.bam")
    L.write(good)
    S = Stream(good)
    raw = bytearray(S.raw)
    raw[S.starts[25]:S.starts[25] + 4] = struct.pack("<i", 20)
    with open(bad, "wb") as fp:
        for blk in bam._bgzf_blocks(bytes(raw)):
            fp.write(blk)
    with pytest.raises(_lib.CoralHipError, match="record shorter than its fixed fields"):
        _decode(bad, pipeline)
    assert_same(L.records(), _decode(good, pipeline).records)
