"""tests/bamfile.py, the reader every BAM test module trusts, on a BAM assembled here from literal bytes (struct.pack, raw deflate
and hand-made BGZF headers - no writer of the product): one tag of every type and B subtype, a CG tag that is taken and one that
is not, a record without SEQ, a record that straddles two BGZF blocks, an empty block in the middle, the EOF block."""
import struct
import zlib

import numpy as np

from tests.bamfile import D, I, M, N, S, bgzf_blocks, pairs, read_bam, read_bam_bgzf


def bgzf(payload):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(payload) + c.flush()
    size = 18 + len(body) + 8
    return (bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0]) + b"BC" + struct.pack("<HH", 2, size - 1) + body
            + struct.pack("<II", zlib.crc32(payload), len(payload)))


def record(tid, pos, name, mapq, flag, cigar, codes, qual, tags=b""):
    seq = bytes((a << 4) | b for a, b in zip(codes[0::2], codes[1::2] + [0]))
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name) + 1, mapq, 4680, len(cigar), flag, len(codes), -1, -1, 0) + name.encode() + b"\0"
    body += b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cigar) + seq + bytes(qual) + tags
    return struct.pack("<i", len(body)) + body


def B(key, sub, fmt, values):
    return key + b"B" + sub + struct.pack("<I", len(values)) + b"".join(struct.pack(fmt, v) for v in values)


EVERY_TAG = (b"XAAq" + b"Xcc" + struct.pack("<b", -7) + b"XCC" + struct.pack("<B", 250) + b"Xss" + struct.pack("<h", -30000)
             + b"XSS" + struct.pack("<H", 65000) + b"Xii" + struct.pack("<i", -(1 << 30)) + b"XII" + struct.pack("<I", (1 << 32) - 5)
             + b"Xff" + struct.pack("<f", -1.5) + b"XZZhi\0" + b"XHH1AE3\0"
             + B(b"Bc", b"c", "<b", [-1, 2]) + B(b"BC", b"C", "<B", [3]) + B(b"Bs", b"s", "<h", [-300]) + B(b"BS", b"S", "<H", [60000, 1])
             + B(b"Bi", b"i", "<i", [-70000]) + B(b"BI", b"I", "<I", [4000000000]) + B(b"Bf", b"f", "<f", [0.5, -2.0]) + B(b"B0", b"S", "<H", []))
HEADER = b"BAM\x01" + struct.pack("<i", 4) + b"@CO\n" + struct.pack("<i", 2) + struct.pack("<i", 3) + b"c0\0" + struct.pack("<i", 1000) \
    + struct.pack("<i", 3) + b"c1\0" + struct.pack("<i", 500)
RECORDS = [
    record(0, 10, "all", 60, 0, [(M, 4)], [1, 2, 4, 8], [10, 20, 30, 40], EVERY_TAG),
    record(0, 20, "taken", 7, 16, [(S, 3), (N, 8)], [15, 1, 2], [0xFF] * 3, b"NMC\x05" + B(b"CG", b"I", "<I", [(2 << 4) | M, (1 << 4) | I, (6 << 4) | D, (0 << 4) | M])),
    record(0, 30, "not_taken", 0, 0, [(S, 2), (N, 4)], [8, 4, 2], [1, 2, 3], B(b"CG", b"I", "<I", [(3 << 4) | M])),
    record(1, 0, "e", 255, 4, [], [], []),
    record(1, 40, "straddles", 1, 0x900, [(M, 50)], [1, 2] * 25, list(range(50))),
    record(-1, -1, "last", 0, 4, [], [4], [9], b"XZZ\0"),
]
STREAM = HEADER + b"".join(RECORDS)
STARTS = [len(HEADER) + sum(len(r) for r in RECORDS[:k]) for k in range(len(RECORDS))]
CUT = STARTS[4] + 2                              # not even the straddling record's length field fits into the first block
# block 0: header, four records and two bytes; 1: the rest of the straddling record; 2: empty; 3: the last record; 4: EOF
PAYLOADS = [STREAM[:CUT], STREAM[CUT:STARTS[5]], b"", STREAM[STARTS[5]:], b""]
BLOCKS = [bgzf(p) for p in PAYLOADS]
AT = [sum(len(b) for b in BLOCKS[:k]) for k in range(6)]          # file offsets of the blocks; AT[5]: the file's size


def plain(x):
    """numpy values as (dtype, list): the dicts compare with ==."""
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.tolist())
    if isinstance(x, (list, tuple)):
        return type(x)(plain(v) for v in x)
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    return x


def u4(pairs_):
    return ("<u4", [(ln << 4) | op for op, ln in pairs_])


def u1(values):
    return ("|u1", list(values))


WANT = [
    dict(tid=0, pos=10, flag=0, mapq=60, name="all", l_seq=4, n_cig=1, ops=u4([(M, 4)]), codes=u1([1, 2, 4, 8]), qual=u1([10, 20, 30, 40]),
         start=STARTS[0], size=len(RECORDS[0]), voff=STARTS[0],
         tags=[("XA", "A", "q"), ("Xc", "c", -7), ("XC", "C", 250), ("Xs", "s", -30000), ("XS", "S", 65000), ("Xi", "i", -(1 << 30)),
               ("XI", "I", (1 << 32) - 5), ("Xf", "f", -1.5), ("XZ", "Z", "hi"), ("XH", "H", "1AE3"), ("Bc", "B", ("|i1", [-1, 2])),
               ("BC", "B", ("|u1", [3])), ("Bs", "B", ("<i2", [-300])), ("BS", "B", ("<u2", [60000, 1])), ("Bi", "B", ("<i4", [-70000])),
               ("BI", "B", ("<u4", [4000000000])), ("Bf", "B", ("<f4", [0.5, -2.0])), ("B0", "B", ("<u2", []))]),
    dict(tid=0, pos=20, flag=16, mapq=7, name="taken", l_seq=3, n_cig=2, ops=u4([(M, 2), (I, 1), (D, 6), (M, 0)]), codes=u1([15, 1, 2]),
         qual=u1([255] * 3), start=STARTS[1], size=len(RECORDS[1]), voff=STARTS[1],
         tags=[("NM", "C", 5), ("CG", "B", u4([(M, 2), (I, 1), (D, 6), (M, 0)]))]),
    dict(tid=0, pos=30, flag=0, mapq=0, name="not_taken", l_seq=3, n_cig=2, ops=u4([(S, 2), (N, 4)]), codes=u1([8, 4, 2]), qual=u1([1, 2, 3]),
         start=STARTS[2], size=len(RECORDS[2]), voff=STARTS[2], tags=[("CG", "B", u4([(M, 3)]))]),
    dict(tid=1, pos=0, flag=4, mapq=255, name="e", l_seq=0, n_cig=0, ops=u4([]), codes=u1([]), qual=u1([]), start=STARTS[3], size=38,
         voff=STARTS[3], tags=[]),
    dict(tid=1, pos=40, flag=0x900, mapq=1, name="straddles", l_seq=50, n_cig=1, ops=u4([(M, 50)]), codes=u1([1, 2] * 25), qual=u1(range(50)),
         start=STARTS[4], size=36 + 10 + 4 + 25 + 50, voff=STARTS[4], tags=[]),
    dict(tid=-1, pos=-1, flag=4, mapq=0, name="last", l_seq=1, n_cig=0, ops=u4([]), codes=u1([4]), qual=u1([9]), start=STARTS[5],
         size=len(RECORDS[5]), voff=AT[3] << 16, tags=[("XZ", "Z", "")]),
]


def test_reader_on_a_hand_made_file(tmp_path):
    path = str(tmp_path / "hand.bam")
    with open(path, "wb") as fp:
        fp.write(b"".join(BLOCKS))
    assert len(BLOCKS[2]) == len(BLOCKS[4]) == 28 and STARTS[4] < CUT < STARTS[4] + 4 and AT[1] < 1 << 16
    assert list(bgzf_blocks(b"".join(BLOCKS))) == [(AT[0], 0, CUT), (AT[1], CUT, STARTS[5] - CUT), (AT[2], STARTS[5], 0),
                                                   (AT[3], STARTS[5], len(RECORDS[5])), (AT[4], len(STREAM), 0)]
    got = read_bam_bgzf(path)
    assert (got.refs, got.lens, got.n_bytes, got.file_size) == (["c0", "c1"], [1000, 500], len(STREAM), AT[5])
    assert [plain(r) for r in got.recs] == WANT
    # the offsets: inside the first block; in the first byte of a block behind an empty one (not in the empty one); behind the last
    # byte of the data, the block that follows it; and behind the last block, the file's size
    assert [r["voff"] for r in got.recs[:5]] == STARTS[:5] and got.recs[5]["voff"] == AT[3] << 16
    assert got.voffset(CUT - 1) == CUT - 1 and got.voffset(CUT) == AT[1] << 16 and got.voffset(CUT + 7) == (AT[1] << 16) | 7
    assert got.end_voff == got.voffset(len(STREAM)) == AT[4] << 16 and got.voffset(len(STREAM) + 1) == AT[5] << 16
    through_gzip = read_bam(path)
    assert (through_gzip.refs, through_gzip.lens, through_gzip.n_bytes) == (got.refs, got.lens, got.n_bytes)
    assert [plain(r) for r in through_gzip.recs] == [{k: v for k, v in w.items() if k != "voff"} for w in WANT]
    assert pairs(got.recs[1]["ops"]) == [(M, 2), (I, 1), (D, 6), (M, 0)] and pairs(got.recs[3]["ops"]) == []
