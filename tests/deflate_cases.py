"""Input blocks for the DEFLATE compressor core (coral_amd/csrc/coral_deflate_core.h), shared by tests/test_deflate_core.py (the
host build against zlib) and tests/test_bgzf_deflate_gpu.py (the kernel against the host build): the smallest shapes at which
each part of the compressor can go wrong.  Everything but the one os.urandom block is made from seeded generators.  Also the
readers the two modules check members with: BGZF member fields, and the dynamic block's header (the compressor writes the
code-length code as sixteen 4-bit codes, which is all `dynamic_header` reads)."""
import gzip
import os
import random
import struct
import zlib

BLOCK_MAX = 0xff00
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
FIB = [1, 1]
while len(FIB) < 22:
    FIB.append(FIB[-1] + FIB[-2])
assert sum(FIB) == 46367


def no_repeat(rnd, n, weights):
    """n bytes drawn with the given weights in which no three consecutive bytes occur twice."""
    seen, out = set(), []
    syms = list(range(len(weights)))
    while len(out) < n:
        s = rnd.choices(syms, weights)[0]
        if len(out) >= 2:
            tri = (out[-2], out[-1], s)
            if tri in seen:
                continue
            seen.add(tri)
        out.append(s)
    return bytes(out)


def inflate_core_cases():
    """The list of tests/test_inflate_core.py::test_core_equals_zlib."""
    rnd = random.Random(1)
    cases = [b"", b"a", b"hello hello hello hello", bytes(65280), b"\xff" * 65280, rnd.randbytes(65280),
             bytes(rnd.choice(b"ACGT") for _ in range(65280)), bytes(rnd.getrandbits(8) & 0x33 for _ in range(30000)),
             b"".join(b"%d,%d;" % (rnd.randrange(1000), rnd.randrange(10 ** 6)) for _ in range(5000))[:65280],
             b"".join(struct.pack("<I", (rnd.randrange(1, 40) << 4) | rnd.choice([0, 0, 0, 1, 2])) for _ in range(16000))]
    for n in (1, 2, 3, 5, 100, 1000, 40000):
        cases += [rnd.randbytes(n), bytes(rnd.choice(b"ab") for _ in range(n))]
    return cases


def acgt_payload():
    rnd = random.Random(7)
    return bytes(rnd.choice(b"ACGT") for _ in range(BLOCK_MAX))


def bam_payload(directory):
    """The inflated record bytes of a tests/bamfile.py-readable file with real QUAL bytes: 60 reads of 3 000 bases."""
    from coral_amd import bam, synth
    from tests.bamfile import M, read_bam
    path = os.path.join(str(directory), "payload.bam")
    rec = synth.records_from_alignments([dict(tid=k % 3, pos=1000 + 37 * k, cigar=[(M, 3000)], name="read%04d" % k) for k in range(60)])
    bam.write_bam(rec, path, seed=5, with_qual=True)
    with gzip.open(path, "rb") as fp:
        raw = fp.read()
    parsed = read_bam(path)
    assert all(r["l_seq"] == 3000 for r in parsed.recs) and len(parsed.recs) == 60
    return raw[parsed.recs[0]["start"]:]


def cases():
    """[(name, block)]: every block at most 0xff00 bytes."""
    rnd = random.Random(2024)
    text = lambda n: bytes(rnd.choice(b"ACGTACGTN\n") for _ in range(n))
    motif = bytes(rnd.randrange(1, 256) for _ in range(300))                # (no zero byte: the filler below is zeros)
    out = [("len_%d" % n, text(n)) for n in (0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129)]
    out += [("run_%d" % n, b"a" * n) for n in (1, 2, 3, 4)]
    out.append(("largest_text", b"".join(b"%d\t%d\tchr%d\n" % (rnd.randrange(10 ** 6), rnd.randrange(100), rnd.randrange(24)) for _ in range(9000))[:BLOCK_MAX]))
    out.append(("urandom", os.urandom(BLOCK_MAX)))
    out.append(("one_byte", b"\x5a" * BLOCK_MAX))
    out += [("period_%d" % p, (rnd.randbytes(p) * (5000 // p + 1))[:5000]) for p in (2, 3, 64, 65)]
    # the zeros between the two motifs are one long run: found at distance 1, never hashed, so the first motif stays in the table
    out += [("motif_at_%d" % d, motif + bytes(d - 300) + motif) for d in (32768, 32769, 40000)]
    out.append(("no_distance_code", no_repeat(rnd, 3000, [1.0 / (1 + k) ** 2 for k in range(256)])))
    out.append(("one_distance_code", b"".join(bytes([k]) * 10 for k in range(1, 200))))
    fib = [s for s, f in enumerate(FIB) for _ in range(f)]
    rnd.shuffle(fib)
    out.append(("fibonacci", bytes(fib)))
    tail = rnd.randbytes(100)
    out.append(("match_ends_on_last_byte", rnd.randbytes(500) + tail + rnd.randbytes(300) + tail))
    out.append(("candidate_runs_past_end", rnd.randbytes(500) + tail + rnd.randbytes(300) + tail[:50]))
    out.append(("acgt", acgt_payload()))
    out += [("inflate_core_%d" % k, c) for k, c in enumerate(inflate_core_cases())]
    assert all(len(c) <= BLOCK_MAX for _, c in out) and len(set(n for n, _ in out)) == len(out)
    return out


# ---- readers --------------------------------------------------------------------------------------------------------------------
def member_fields(member):
    """(raw DEFLATE stream, crc, isize) of one BGZF member, with its fixed fields and BSIZE asserted."""
    assert member[:16] == bytes.fromhex("1f8b08040000000000ff060042430200"), member[:16].hex()
    assert struct.unpack_from("<H", member, 16)[0] == len(member) - 1
    crc, isize = struct.unpack_from("<II", member, len(member) - 8)
    return member[18:-8], crc, isize


def check_member(member, data):
    """The member holds `data`: every field, the stream through zlib, the member through gzip.  Returns the stream's BTYPE."""
    stream, crc, isize = member_fields(member)
    assert isize == len(data) and crc == (zlib.crc32(data) & 0xffffffff)
    assert zlib.decompress(stream, -15) == data and gzip.decompress(member) == data
    assert len(member) <= len(data) + 5 + 26
    assert stream[0] & 1 == 1                                    # one block, marked final
    return (stream[0] >> 1) & 3


def dynamic_header(stream):
    """(hlit, hdist, literal / length code lengths, distance code lengths) of a dynamic block as the compressor writes it."""
    bits = int.from_bytes(stream[:400], "little")
    take = lambda at, n: (bits >> at) & ((1 << n) - 1)
    assert take(0, 3) == 0b101                                   # BFINAL, BTYPE = 2
    hlit, hdist, hclen = take(3, 5) + 257, take(8, 5) + 1, take(13, 4) + 4
    assert hclen == 19 and [take(17 + 3 * k, 3) for k in range(19)] == [0, 0, 0] + [4] * 16
    rev4 = lambda x: int("{:04b}".format(x)[::-1], 2)
    lens = [rev4(take(74 + 4 * k, 4)) for k in range(hlit + hdist)]
    return hlit, hdist, lens[:hlit], lens[hlit:]


def kraft(lens):
    return sum(2.0 ** -l for l in lens if l)
