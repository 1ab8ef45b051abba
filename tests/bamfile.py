"""The one plain-Python BAM reader of the test suite, and the two rule restatements that more than one test module checks against.

INDEPENDENT of the product: this module imports gzip, zlib, struct, bisect and numpy, and nothing from coral_amd.  What the test
modules restate on top of these records is evidence about the decoders only because no byte here has passed through them - keep
it that way.  The reader itself is pinned by tests/test_bamfile.py on a file assembled from literal bytes."""
import bisect
import gzip
import struct
import zlib

import numpy as np

M, I, D, N, S, H, P, EQ, X = range(9)
_INT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


class Bam:
    """refs / lens: contig names and lengths; recs: one dict per record, in file order; n_bytes: length of the inflated stream.
    From read_bam_bgzf also blocks [(file offset, inflated offset, inflated length)], file_size, voffset(u) and end_voff."""

    def voffset(self, u):
        """Virtual offset of byte u of the inflated stream."""
        if u < self.n_bytes:                         # the block that holds byte u (an empty block holds none)
            at, first, _ = self.blocks[bisect.bisect_right(self.starts, u) - 1]
            return (at << 16) | (u - first)
        b = bisect.bisect_left(self.starts, u)           # behind the last byte: the block that follows the last byte
        return (self.blocks[b][0] if b < len(self.blocks) else self.file_size) << 16


def pairs(ops):
    """CIGAR words -> [(op, len)]"""
    return list(zip((ops & 15).tolist(), (ops >> 4).tolist()))


def many_ops(n):
    """A CIGAR of exactly n >= 16 ops: leading H and S, every op of M I D N S H P = X, zero-length ops in between."""
    cycle = [(M, 5), (I, 2), (M, 0), (D, 3), (EQ, 4), (X, 1), (I, 0), (N, 7), (P, 2), (M, 6), (D, 0)]
    ops = [(H, 3), (S, 4)]
    while len(ops) < n - 3:
        ops.append(cycle[(len(ops) - 2) % len(cycle)])
    return ops + [(M, 9), (S, 2), (H, 1)]


def _tags(raw, p, end):
    """[(key, type, value)] of the tags in raw[p:end]; a B array comes back as a numpy array of its subtype."""
    tags = []
    while p < end:
        key, ty = raw[p:p + 2].decode(), chr(raw[p + 2])
        p += 3
        if ty == "A":
            val, p = chr(raw[p]), p + 1
        elif ty in _INT or ty == "f":
            fmt = _INT.get(ty, "<f")
            val, p = struct.unpack_from(fmt, raw, p)[0], p + struct.calcsize(fmt)
        elif ty in "ZH":
            z = raw.index(b"\0", p)
            val, p = raw[p:z].decode(), z + 1
        elif ty == "B":
            sub, cnt = chr(raw[p]), struct.unpack_from("<I", raw, p + 1)[0]
            dt = np.dtype("<f4" if sub == "f" else _INT[sub])
            val = np.frombuffer(raw, dtype=dt, count=cnt, offset=p + 5).copy()
            p += 5 + dt.itemsize * cnt
        else:
            raise AssertionError("tag type %r" % ty)
        tags.append((key, ty, val))
    assert p == end
    return tags


def parse(raw):
    """The inflated stream -> Bam.  Per record: tid, pos, flag, mapq, name, l_seq, n_cig (the record's own n_cigar_op), ops (the
    real CIGAR as uint32 words: the first CG:B,I tag where the record's own CIGAR is the placeholder of two ops, S of length l_seq
    and N), codes (the 4-bit SEQ codes) and qual (both of length l_seq), tags [(key, type, value)], start (byte offset in the
    stream) and size (block_size + 4)."""
    raw = bytes(raw)
    assert raw[:4] == b"BAM\x01"
    out = Bam()
    out.refs, out.lens, out.recs, out.n_bytes = [], [], [], len(raw)
    o = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, o)[0]
    o += 4
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", raw, o)[0]
        out.refs.append(raw[o + 4:o + 4 + ln - 1].decode())
        out.lens.append(struct.unpack_from("<i", raw, o + 4 + ln)[0])
        o += 8 + ln
    while o < len(raw):
        bs, tid, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", raw, o)
        p = o + 36
        name = raw[p:p + l_name - 1].decode()
        p += l_name
        assert raw[p - 1] == 0
        ops = np.frombuffer(raw, dtype="<u4", count=n_cig, offset=p).copy()
        p += 4 * n_cig
        packed = np.frombuffer(raw, dtype=np.uint8, count=(l_seq + 1) // 2, offset=p)
        codes = np.empty(2 * len(packed), dtype=np.uint8)
        codes[0::2], codes[1::2] = packed >> 4, packed & 15
        p += (l_seq + 1) // 2
        qual = np.frombuffer(raw, dtype=np.uint8, count=l_seq, offset=p)
        tags = _tags(raw, p + l_seq, o + 4 + bs)
        if n_cig == 2 and ops[0] & 15 == S and ops[0] >> 4 == l_seq and ops[1] & 15 == N:
            cg = [v for k, ty, v in tags if k == "CG" and ty == "B" and v.dtype == np.dtype("<u4")]
            ops = cg[0] if cg else ops
        out.recs.append(dict(tid=tid, pos=pos, flag=flag, mapq=mapq, name=name, l_seq=l_seq, n_cig=n_cig, ops=ops, codes=codes[:l_seq],
                             qual=qual, tags=tags, start=o, size=bs + 4))
        o += 4 + bs
    assert o == len(raw)
    return out


def read_bam(path):
    """The file through the gzip module (BGZF is multi-member gzip, empty members included)."""
    with gzip.open(path, "rb") as fp:
        return parse(fp.read())


def bgzf_blocks(raw):
    """(file offset, inflated offset, inflated length) of every BGZF block of the file's bytes, empty blocks included."""
    at = u = 0
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04"
        xlen = struct.unpack_from("<H", raw, at + 10)[0]
        bsize, x = None, at + 12
        while x < at + 12 + xlen:
            if raw[x:x + 2] == b"BC":
                bsize = struct.unpack_from("<H", raw, x + 4)[0]
            x += 4 + struct.unpack_from("<H", raw, x + 2)[0]
        isize = struct.unpack_from("<I", raw, at + bsize + 1 - 4)[0]
        yield at, u, isize
        at, u = at + bsize + 1, u + isize


def read_bam_bgzf(path):
    """The file block by block, so that every record carries voff, its virtual offset; end_voff is the one behind the last."""
    with open(path, "rb") as fp:
        raw = fp.read()
    blocks = list(bgzf_blocks(raw))
    ends = [b[0] for b in blocks[1:]] + [len(raw)]
    data = b"".join(zlib.decompress(raw[at:end], 31) for (at, _, _), end in zip(blocks, ends))
    assert [len(data)] == [u + n for _, u, n in blocks[-1:]]
    out = parse(data)
    out.blocks, out.starts, out.file_size = blocks, [u for _, u, _ in blocks], len(raw)
    for r in out.recs:
        r["voff"] = out.voffset(r["start"])
    out.end_voff = out.voffset(out.n_bytes)
    return out


# ---- the rules that two test modules check against: restated once, here, from the records above -------------------------------
def oracle_coverage(parsed, windows, threshold, read_callback):
    """pysam AlignmentFile.count_coverage summed over the four bases (tests/test_window_coverage.py, tests/test_bam_index.py).
    For every window: #(read, qpos, refpos) with the read on the contig (and, with 'all', none of the flags 0x704), SEQ
    present, (qpos, refpos) an aligned pair of an M / = / X op inside the window, SEQ code A/C/G/T, and threshold 0 or QUAL
    present (first byte not 0xff) and QUAL[qpos] >= threshold.  parsed = (refs, recs)."""
    refs, recs = parsed
    hits = {}
    for r in recs:
        if r["tid"] < 0 or len(r["codes"]) == 0 or (read_callback == "all" and r["flag"] & 0x704):
            continue
        if threshold > 0 and r["qual"][0] == 0xFF:
            continue
        q, ref, qs, rs = 0, r["pos"], [], []
        for w in r["ops"]:
            op, ln = int(w & 15), int(w >> 4)
            if op in (M, EQ, X):
                qs.append(np.arange(q, q + ln))
                rs.append(np.arange(ref, ref + ln))
            q += ln if op in (M, I, S, EQ, X) else 0
            ref += ln if op in (M, D, N, EQ, X) else 0
        if not qs:
            continue
        qp, rp = np.concatenate(qs), np.concatenate(rs)
        keep = qp < len(r["codes"])
        qp, rp = qp[keep], rp[keep]
        c = r["codes"][qp]
        ok = (c == 1) | (c == 2) | (c == 4) | (c == 8)
        if threshold > 0:
            ok &= r["qual"][qp] >= threshold
        hits.setdefault(r["tid"], []).append(rp[ok])
    hits = {t: np.sort(np.concatenate(v)) for t, v in hits.items()}
    out = []
    for chrom, a, b in windows:
        h = hits.get(refs.index(chrom), np.zeros(0, dtype=np.int64))
        out.append(int(np.searchsorted(h, b) - np.searchsorted(h, a)))
    return np.array(out, dtype=np.int64)


def restate_read_qc(recs):
    """What the reference's scripts/report_nanopore_qc.py collects (lines 35-48) over the reads, plus the counters and the
    histogram as bam.read_qc words them (tests/test_read_qc.py, tests/test_bam_request.py)."""
    reads = [r for r in recs if r["flag"] & 0x900 == 0 and r["l_seq"] > 0]          # `if sequence:`
    mean_lengths = [r["l_seq"] for r in reads]                                        # len(sequence)
    with_q = [r for r in reads if r["qual"][0] != 0xFF]
    mean_qualities = [np.mean(np.array(r["qual"].tolist())) for r in with_q]          # np.mean(np.array([ints]))
    hist = np.zeros(256, dtype=np.int64)
    for r in with_q:
        hist += np.bincount(r["qual"], minlength=256)
    counters = dict(n_records=len(recs), n_reads=len(reads), n_secondary=sum(1 for r in recs if r["flag"] & 0x100),
                    n_supplementary=sum(1 for r in recs if r["flag"] & 0x800), n_unmapped=sum(1 for r in reads if r["flag"] & 4),
                    n_no_seq=sum(1 for r in recs if r["flag"] & 0x900 == 0 and r["l_seq"] == 0), n_no_qual=len(reads) - len(with_q),
                    total_bases=sum(mean_lengths))
    return dict(reads=reads, mean_lengths=mean_lengths, mean_qualities=mean_qualities, hist=hist, counters=counters,
                length=np.array(mean_lengths, dtype=np.int32),
                qual_sum=np.array([int(r["qual"].astype(np.int64).sum()) if r["qual"][0] != 0xFF else -1 for r in reads], dtype=np.int64),
                mapq=np.array([r["mapq"] for r in reads], dtype=np.int32), flag=np.array([r["flag"] for r in reads], dtype=np.int32))
