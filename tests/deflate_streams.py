"""Raw DEFLATE test streams (with their plain text) shared by the host test of the decoder core (tests/test_inflate_core.py) and
the GPU test of the inflate kernel (tests/test_bam_gpu.py): every block type, levels and strategies, sizes around the 64-lane
boundaries, two-letter texts (very long matches, code sets with 11- and 12-bit codes), several blocks per stream; and streams
built block by block with a writer of their own (Deflate: dynamic_streams, rejected_streams, incomplete_streams; also run by the
GPU tests of tests/test_inflate_streams_gpu.py)."""
import bisect
import os
import random
import struct
import zlib


def streams():
    rnd = random.Random(7)
    cases = [b"", b"a", b"hello hello hello hello", bytes(65280), b"\xff" * 65280, os.urandom(65280),
             bytes(rnd.choice(b"ACGT") for _ in range(65280)), bytes(rnd.getrandbits(8) & 0x33 for _ in range(30000)),
             b"".join(b"%d,%d;" % (rnd.randrange(1000), rnd.randrange(10 ** 6)) for _ in range(5000))[:65280],
             b"".join(struct.pack("<I", (rnd.randrange(1, 40) << 4) | rnd.choice([0, 0, 0, 1, 2])) for _ in range(16000))]
    # Fibonacci-like symbol frequencies: Huffman code lengths up to the 15-bit limit (the canonical loop behind the 10-bit table)
    fib, a, b = [], 1, 1
    for sym in range(24):
        fib.append(bytes([65 + sym]) * a)
        a, b = b, a + b
    skew = bytearray(b"".join(fib))
    rnd.shuffle(skew)
    cases.append(bytes(skew[:65000]))
    for n in (1, 2, 3, 5, 63, 64, 65, 100, 1000, 40000):
        cases.append(os.urandom(n))
        cases.append(bytes(rnd.choice(b"ab") for _ in range(n)))
    out = []
    for data in cases:
        for level in (0, 1, 6, 9):
            for strat in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE):
                co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strat)
                out.append((co.compress(data) + co.flush(), data))
    out += crafted_streams()
    for _ in range(20):                                 # several DEFLATE blocks per stream, empty stored blocks in between
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        data, comp = b"", b""
        for _k in range(rnd.randrange(1, 6)):
            piece = os.urandom(rnd.randrange(0, 3000)) if rnd.random() < 0.5 else bytes(rnd.choice(b"ACGTN") for _ in range(rnd.randrange(0, 9000)))
            data += piece
            comp += co.compress(piece) + co.flush(rnd.choice([zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH, zlib.Z_NO_FLUSH]))
        out.append((comp + co.flush(), data))
    return out


# ---- streams written token by token (fixed Huffman codes, RFC 1951 §3.2.6): matches of exactly chosen length and distance,
# around every boundary of the GPU kernel's hand-written loop (coral_bamgpu.hip, DevWaveT::fast): the 2 KiB ring and its
# "source has left the ring" limit (distance 1984 / 1985), 64-byte copy chunks, matches that overlap their source, the longest
# match, the 256-byte output lines, the last 260 bytes of a block.
_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):                       # LSB first (extra bits, header fields)
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, nbits):                      # a Huffman code: most significant bit first
        self.put(int(format(value, "0%db" % nbits)[::-1], 2), nbits)

    def done(self):
        if self.n:
            self.put(0, 8 - self.n)
        return bytes(self.out)


def fixed_block(tokens):
    """tokens: ('L', byte) | ('M', length, distance)  ->  (raw DEFLATE stream of one final fixed-Huffman block, its plain text)."""
    b, text = _Bits(), bytearray()
    b.put(1, 1)
    b.put(1, 2)

    def sym(x):
        if x < 144: b.code(0x30 + x, 8)
        elif x < 256: b.code(0x190 + x - 144, 9)
        elif x < 280: b.code(x - 256, 7)
        else: b.code(0xc0 + x - 280, 8)
    for t in tokens:
        if t[0] == "L":
            sym(t[1])
            text.append(t[1])
        else:
            _, n, d = t
            assert 3 <= n <= 258 and 1 <= d <= len(text) and d <= 32768
            i = max(k for k in range(29) if _LBASE[k] <= n)
            if n == 258: i = 28
            sym(257 + i)
            b.put(n - _LBASE[i], _LEXT[i])
            j = max(k for k in range(30) if _DBASE[k] <= d)
            b.code(j, 5)
            b.put(d - _DBASE[j], _DEXT[j])
            for _k in range(n):
                text.append(text[-d])
    sym(256)
    return b.done(), bytes(text)


def crafted_streams():
    rnd = random.Random(17)
    out = []
    lens = (3, 4, 5, 63, 64, 65, 66, 127, 128, 129, 257, 258)
    dists = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1983, 1984, 1985, 2047, 2048, 2049, 4031, 4032, 4033, 4999)
    for order in range(3):
        toks = [("L", rnd.randrange(256)) for _ in range(5000)]            # history longer than any ring
        combos = [(n, d) for n in lens for d in dists]
        rnd.shuffle(combos)
        for n, d in combos:
            toks.append(("M", n, d))
            for _ in range(rnd.randrange(0, 3) if order else 1):           # literal runs of 0..2 between the matches
                toks.append(("L", rnd.randrange(256)))
        out.append(fixed_block(toks))
    # matches only (no literal in between), every output-line phase; the block ends with a match
    toks = [("L", 65 + k % 7) for k in range(300)]
    for k in range(400):
        toks.append(("M", 3 + (k * 7) % 256, 1 + (k * 13) % 299))
    out.append(fixed_block(toks))
    # very short blocks and blocks shorter than the 260 bytes the hand-written loop leaves to the general one
    for n in (1, 2, 3, 100, 259, 260, 261, 300, 600):
        toks = [("L", rnd.randrange(256)) for _ in range(min(n, 40))]
        while sum(1 if t[0] == "L" else t[1] for t in toks) + 3 <= n:
            left = n - sum(1 if t[0] == "L" else t[1] for t in toks)
            have = sum(1 if t[0] == "L" else t[1] for t in toks)
            toks.append(("M", min(left, rnd.choice((3, 17, 70, 258))), rnd.randrange(1, have + 1)))
        out.append(fixed_block(toks))
    for comp, text in out:
        assert zlib.decompress(comp, -15) == text
    return out


# ---- a block-level DEFLATE writer: stored, fixed and dynamic blocks appended to one stream, the plain text tracked across
# blocks (matches may reach into earlier blocks, up to distance 32768).  A dynamic block's code lengths, alphabet sizes,
# code-length code and run-length ops can each be given, so a stream can hold what no compressor emits: a repeat op across the
# literal / distance boundary, code 16 behind a zero run, chosen symbols on codes longer than the decoder's look-up tables.
# Tokens: ('L', byte) | ('M', length, distance[, length symbol]) | ('R', ll symbol[, length extra, distance symbol, distance
# extra]) raw symbols that the text does not follow (for streams a decoder must reject) | ('B', value, nbits) raw bits.
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def kraft(lens):
    """Sum of 2^-l over the non-zero lengths, in units of 2^-15 (a complete code: 32768)."""
    return sum(1 << (15 - l) for l in lens if l)


def limited_lengths(freqs, limit):
    """Optimal code lengths of at most `limit` bits (package-merge); Kraft sum exactly 1 (two codes at the least)."""
    freqs = list(freqs)
    syms = [s for s, f in enumerate(freqs) if f > 0]
    for s in range(len(freqs)):                                   # a complete code needs two symbols
        if len(syms) >= 2: break
        if s not in syms: syms.append(s)
    assert len(syms) <= 1 << limit
    lens = [0] * len(freqs)
    leaves = sorted((max(freqs[s], 1), [s]) for s in syms)
    packages = leaves
    for _ in range(limit - 1):
        merged = [(packages[i][0] + packages[i + 1][0], packages[i][1] + packages[i + 1][1]) for i in range(0, len(packages) - 1, 2)]
        packages = sorted(leaves + merged, key=lambda p: p[0])
    for _, ss in packages[:2 * len(syms) - 2]:
        for s in ss: lens[s] += 1
    assert kraft(lens) == 32768 and max(lens) <= limit
    return lens


def canonical_codes(lens):
    """symbol -> code value (RFC 1951 §3.2.2); values of an over-subscribed set are cut to their length."""
    count = [0] * 17
    for l in lens: count[l] += 1
    count[0], code, nxt = 0, 0, [0] * 17
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        out.append(nxt[l] & ((1 << l) - 1))
        nxt[l] += 1
    return out


def zlib_rle(seq):
    """The run-length ops a compressor writes: [(symbol, repeat)], a plain length with repeat 1."""
    ops, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]: j += 1
        run, v = j - i, seq[i]
        if v:
            ops.append((v, 1))
            run -= 1
        while run >= 3:
            n = min(run, 138 if v == 0 else 6)
            if v == 0 and n < 11: n = min(run, 10)
            ops.append((18 if n >= 11 else 17, n) if v == 0 else (16, n))
            run -= n
        ops += [(v, 1)] * run
        i = j
    return ops


def plain_rle(seq):
    return [(v, 1) for v in seq]


def expand_ops(ops):
    seq = []
    for s, rep in ops:
        seq += [s] if s < 16 else [seq[-1] if s == 16 else 0] * rep
    return seq


_LSYM = [0, 0, 0] + [257 + max(k for k in range(28) if _LBASE[k] <= n) for n in range(3, 258)] + [285]


def length_symbol(n):
    return _LSYM[n]


def distance_symbol(d):
    return bisect.bisect_right(_DBASE, d) - 1


class Deflate:
    def __init__(self):
        self.b, self.text, self.blocks = _Bits(), bytearray(), []

    def done(self):
        return self.b.done(), bytes(self.text)

    def _begin(self, kind, final, btype):
        info = dict(type=kind, start=len(self.text), uses=[], bit=8 * len(self.b.out) + self.b.n)
        self.blocks.append(info)
        self.b.put(1 if final else 0, 1)
        self.b.put(btype, 2)
        return info

    def raw(self, value, nbits):
        self.b.put(value, nbits)

    def stored(self, data, final, nlen=None, length=None):
        info = self._begin("stored", final, 0)
        if self.b.n: self.b.put(0, 8 - self.b.n)
        n = len(data) if length is None else length
        self.b.put(n, 16)
        self.b.put((n ^ 0xffff) if nlen is None else nlen, 16)
        self.b.out += data
        self.text += data
        info["end"] = len(self.text)
        return info

    def _symbols(self, tokens, info, ll, dd):
        """tokens through the codes ll / dd ([(value, nbits)] by symbol); follows the text, records every length and distance
        symbol used as (kind, symbol, code length, extra value, extra bits, text position)."""
        b, text = self.b, self.text
        lit = [(int(format(v, "0%db" % n)[::-1], 2), n) if n else (0, 0) for v, n in ll[:256]]      # (bit-reversed once, not per token)
        for t in tokens:
            if t[0] == "L":
                b.put(*lit[t[1]])
                text.append(t[1])
            elif t[0] == "B":
                b.put(t[1], t[2])
            elif t[0] == "R":
                b.code(*ll[t[1]])
                if len(t) > 2:
                    b.put(t[2], _LEXT[t[1] - 257])
                    b.code(*dd[t[3]])
                    b.put(t[4], _DEXT[t[3]] if t[3] < 30 else 0)
            else:
                n, d = t[1], t[2]
                assert 3 <= n <= 258 and 1 <= d <= len(text) and d <= 32768
                s = t[3] if len(t) > 3 else length_symbol(n)
                i = s - 257
                assert 0 <= n - _LBASE[i] < 1 << _LEXT[i] or (n, s) == (258, 285)
                j = distance_symbol(d)
                assert ll[s][1] and dd[j][1], "no code for a symbol in use"
                info["uses"] += [("len", s, ll[s][1], n - _LBASE[i], _LEXT[i], len(text)), ("dist", j, dd[j][1], d - _DBASE[j], _DEXT[j], len(text))]
                b.code(*ll[s])
                b.put(n - _LBASE[i], _LEXT[i])
                b.code(*dd[j])
                b.put(d - _DBASE[j], _DEXT[j])
                for _k in range(n):
                    text.append(text[-d])
        b.code(*ll[256])
        info["end"] = len(text)

    def fixed(self, tokens, final):
        info = self._begin("fixed", final, 1)
        lens = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
        self._symbols(tokens, info, list(zip(canonical_codes(lens), lens)), [(j, 5) for j in range(32)])
        return info

    def dynamic(self, tokens, final, ll_lens=None, d_lens=None, hlit=None, hdist=None, cl_lens=None, hclen=None, rle=zlib_rle, strict=True):
        """Returns the code-length ops written as [(symbol, repeat, position)] (also in self.blocks[-1]).  strict=False drops the
        consistency checks (streams that a decoder must reject)."""
        info = self._begin("dynamic", final, 2)
        if ll_lens is None or d_lens is None:
            fl, fd = [0] * 286, [0] * 30
            fl[256] = 1
            for t in tokens:
                if t[0] == "L": fl[t[1]] += 1
                elif t[0] == "M":
                    fl[t[3] if len(t) > 3 else length_symbol(t[1])] += 1
                    fd[distance_symbol(t[2])] += 1
            if ll_lens is None: ll_lens = limited_lengths(fl, 15)
            if d_lens is None: d_lens = limited_lengths(fd, 15) if any(fd) else [0]
        ll_lens, d_lens = list(ll_lens) + [0] * (288 - len(ll_lens)), list(d_lens) + [0] * (32 - len(d_lens))
        if hlit is None: hlit = max([257] + [1 + s for s in range(288) if ll_lens[s]])
        if hdist is None: hdist = max([1] + [1 + s for s in range(32) if d_lens[s]])
        seq = ll_lens[:hlit] + d_lens[:hdist]
        ops = rle(seq) if callable(rle) else list(rle)
        if strict:
            assert expand_ops(ops) == seq and not any(ll_lens[hlit:]) and not any(d_lens[hdist:])
            assert all(3 <= r <= 6 if s == 16 else 3 <= r <= 10 if s == 17 else 11 <= r <= 138 if s == 18 else r == 1 for s, r in ops)
        if cl_lens is None:
            f = [0] * 19
            for s, _ in ops: f[s] += 1
            cl_lens = limited_lengths(f, 7)
        if hclen is None: hclen = max(4, 1 + max(k for k in range(19) if cl_lens[_CL_ORDER[k]]))
        if strict: assert not any(cl_lens[_CL_ORDER[k]] for k in range(hclen, 19)) and all(cl_lens[s] for s, _ in ops)
        b = self.b
        b.put(hlit - 257, 5)
        b.put(hdist - 1, 5)
        b.put(hclen - 4, 4)
        for k in range(hclen): b.put(cl_lens[_CL_ORDER[k]], 3)
        cl, pos, placed = list(zip(canonical_codes(cl_lens), cl_lens)), 0, []
        for s, rep in ops:
            b.code(*cl[s])
            if s == 16: b.put(rep - 3, 2)
            elif s == 17: b.put(rep - 3, 3)
            elif s == 18: b.put(rep - 11, 7)
            placed.append((s, rep, pos))
            pos += rep
        info.update(hlit=hlit, hdist=hdist, hclen=hclen, ops=placed, ll_lens=ll_lens[:hlit], d_lens=d_lens[:hdist], cl_lens=list(cl_lens))
        self._symbols(tokens, info, list(zip(canonical_codes(ll_lens), ll_lens)), list(zip(canonical_codes(d_lens), d_lens)))
        return placed


# ---- named cases built with the writer.  A valid case is checked against zlib when it is built and carries `edge`, a function
# that asserts from the header and the lengths actually written that the stream reaches the edge it is named after.
def _case(name, w, edge=None, reference=True):
    comp, text = w.done()
    assert len(text) <= 65536, name
    if reference:
        assert zlib.decompress(comp, -15) == text, name
    return dict(name=name, comp=comp, text=text, blocks=w.blocks, edge=edge or (lambda: None))


def _ops_block(w, ops, hlit, tokens, final=True, **kw):
    """A dynamic block whose code lengths are what the ops [(symbol, repeat)] expand to."""
    seq = expand_ops(ops)
    return w.dynamic(tokens, final, ll_lens=seq[:hlit], d_lens=seq[hlit:], hlit=hlit, hdist=len(seq) - hlit, rle=ops, **kw)


def _types_are(w, want):
    def edge(blocks=w.blocks):
        assert [b["type"] for b in blocks] == want
    return edge


def _crossing(blk, sym):
    return [(s, r, p) for s, r, p in blk["ops"] if s == sym and p < blk["hlit"] < p + r]


def _pattern(kind, bits):
    """Extra-bit patterns: zeros, ones, alternating (both phases for the distances)."""
    mask = (1 << bits) - 1
    return [0, mask, 0x15 & mask] if kind == "len" else [0, mask, 0x1555 & mask, 0x2aaa & mask]


LONG_LL = [0] * 286                      # literals 0..9 at lengths 1..10, 32 symbols at length 15: every length symbol and
for _s in range(10): LONG_LL[_s] = _s + 1    # the end-of-block code lie behind the 10-bit table
for _s in (10, 11, *range(256, 286)): LONG_LL[_s] = 15
SHORT_LL = [0] * 286                     # every length symbol, the end-of-block code and three literals in the table
SHORT_LL[0] = 1
for _s in (1, 2, *range(256, 286)): SHORT_LL[_s] = 6
SHORT_D = [5] * 28 + [4] * 2


def long_d(rotation):
    """Eight distance symbols at lengths 1..8, the 22 others behind the 8-bit table (2 x 11, 4 x 12, 16 x 13 bits)."""
    short = list(range(8 * rotation, 8 * rotation + 8))
    lens, rest = [0] * 30, [s for s in range(30) if s not in short]
    for k, s in enumerate(short): lens[s] = k + 1
    for k, s in enumerate(rest): lens[s] = 11 if k < 2 else 12 if k < 6 else 13
    return lens


def _history(rnd, n, alphabet=range(256)):
    alphabet = list(alphabet)
    return bytes(rnd.choice(alphabet) for _ in range(n))


def _all_length_tokens(rnd, hist):
    toks = []
    for i in range(29):
        for x in _pattern("len", _LEXT[i]):
            toks.append(("M", _LBASE[i] + x, rnd.randrange(1, hist), 257 + i))
    toks.append(("M", 258, 7, 284))                                # 258 as symbol 284 with all extra bits set
    return toks


def _all_distance_tokens(rnd, lengths=(3, 4, 5, 9)):
    toks = []
    for j in range(30):
        for x in _pattern("dist", _DEXT[j]):
            toks.append(("M", rnd.choice(lengths), _DBASE[j] + x))
    return toks


def dynamic_streams():
    rnd = random.Random(23)
    A, out = 65, []
    used = lambda blk, kind: {(s, x, e) for k, s, _, x, e, _ in blk["uses"] if k == kind}

    # -- the code-length sequence
    w = Deflate()                                          # 16 over a non-zero length, across the boundary, repeat 6
    _ops_block(w, [(18, 65), (1, 1), (18, 138), (18, 52), (3, 1), (16, 6), (16, 5)], 260,
               [("L", A)] * 20 + [("M", n, d) for n in (3, 4, 5) for d in (1, 2, 3, 4, 5, 7, 9, 13)])
    def edge(b=w.blocks[0]):
        assert _crossing(b, 16) == [(16, 6, 257)] and b["ll_lens"][256] == 3 and b["d_lens"] == [3] * 8
    out.append(_case("cl_16_across_boundary", w, edge))

    w = Deflate()                                          # 17 across the boundary
    _ops_block(w, [(18, 65), (1, 1), (18, 138), (18, 52), (2, 1), (2, 1), (17, 8), (1, 1), (1, 1)], 263,
               [("L", A)] * 9 + [("M", 3, 4), ("M", 3, 5), ("M", 3, 6), ("L", A)])
    def edge(b=w.blocks[0]):
        assert _crossing(b, 17) == [(17, 8, 258)] and b["d_lens"] == [0, 0, 0, 1, 1]
    out.append(_case("cl_17_across_boundary", w, edge))

    w = Deflate()                                          # 18 across the boundary
    _ops_block(w, [(18, 65), (1, 1), (18, 138), (18, 52), (2, 1), (2, 1), (18, 22), (1, 1), (1, 1)], 270,
               [("L", A)] * 70 + [("M", 3, 33), ("M", 3, 48), ("M", 3, 49), ("M", 3, 64), ("L", A)])
    def edge(b=w.blocks[0]):
        assert _crossing(b, 18) == [(18, 22, 258)] and b["hdist"] == 12
    out.append(_case("cl_18_across_boundary", w, edge))

    w = Deflate()                                          # 16 behind 17 and behind 18 (repeats "previous = 0" although the
    ops = [(18, 65), (2, 1), (17, 3), (16, 3), (2, 1), (18, 11), (16, 6), (2, 1), (17, 10), (16, 6), (18, 138), (18, 11),    # last
           (3, 1), (3, 1), (1, 1), (1, 1)]                 # length written was 2); every repeat count at both ends of its range
    _ops_block(w, ops, 258, [("L", A), ("L", 72), ("L", 90)] * 5 + [("M", 3, 1), ("M", 3, 2)])
    def edge(b=w.blocks[0]):
        o = b["ops"]
        for first, then in ((17, 16), (18, 16)):
            assert any(o[k][0] == first and o[k + 1][0] == then and o[k - 1][0] not in (0, 16, 17, 18) for k in range(1, len(o) - 1))
        assert {(18, 138), (18, 11), (17, 10), (17, 3), (16, 6), (16, 3)} <= {(s, r) for s, r, _ in o}
        assert [s for s in range(258) if b["ll_lens"][s]] == [65, 72, 90, 256, 257]
    out.append(_case("cl_16_after_zero_runs", w, edge))

    w = Deflate()                                          # hlit 257, hdist 1 with length 0, end-of-block code of 1 bit
    w.dynamic([("L", A)] * 300, True, ll_lens=[0] * 65 + [1] + [0] * 190 + [1], d_lens=[0])
    def edge(b=w.blocks[0]):
        assert (b["hlit"], b["hdist"], b["d_lens"], b["ll_lens"][256]) == (257, 1, [0], 1)
    out.append(_case("hlit_257_no_distance_code", w, edge))

    w = Deflate()                                          # hclen 5 (the least that can carry an end-of-block code): 256 codes of 8 bits
    w.dynamic([("L", rnd.randrange(1, 256)) for _ in range(400)], True, ll_lens=[0] + [8] * 256, d_lens=[0], cl_lens=[1] + [0] * 7 + [1] + [0] * 10, rle=plain_rle)
    def edge(b=w.blocks[0]):
        assert b["hclen"] == 5
    out.append(_case("hclen_5", w, edge))

    w = Deflate()                                          # a code-length code with 7-bit codes, in use
    cl = [2, 3, 4, 5, 6, 7, 7] + [0] * 11 + [1]
    w.dynamic([("L", A + k) for k in (0, 0, 0, 0, 1, 1, 2, 3, 4, 5)] * 30, True, ll_lens=[0] * 65 + [1, 2, 3, 4, 5, 6] + [0] * 185 + [6], d_lens=[0], cl_lens=cl)
    def edge(b=w.blocks[0]):
        assert b["cl_lens"][5] == b["cl_lens"][6] == 7 and {5, 6} <= {s for s, _, _ in b["ops"]} and kraft(b["cl_lens"]) == 32768
    out.append(_case("code_length_code_of_7_bits", w, edge))

    # -- distance alphabet corners
    w = Deflate()
    w.dynamic([("L", A), ("L", 66)] + [("M", n, 1) for n in (3, 64, 65, 258)] + [("L", 67), ("M", 200, 1)], True, d_lens=[1])
    def edge(b=w.blocks[0]):
        assert b["d_lens"] == [1] and b["hdist"] == 1
    out.append(_case("one_distance_code_symbol_0", w, edge))

    w = Deflate()
    w.stored(_history(rnd, 32768), False)
    w.dynamic([("L", A)] + [("M", n, d) for d in (24577, 32768) for n in (3, 65, 258)] + [("L", A)], True, d_lens=[0] * 29 + [1])
    def edge(b=w.blocks[1]):
        assert b["d_lens"] == [0] * 29 + [1] and b["hdist"] == 30 and {(29, 0, 13), (29, 8191, 13)} <= used(b, "dist")
    out.append(_case("one_distance_code_symbol_29", w, edge))

    # -- every length and distance symbol on both decode paths (in the look-up table; behind it), chosen extra bits, in the
    # block's last 260 bytes and well in front of them
    lits12 = range(12)
    for name, ll, dl in (("lengths_behind_table", LONG_LL, SHORT_D), ("lengths_in_table", SHORT_LL, SHORT_D),
                         ("lengths_and_distances_behind_table", LONG_LL, long_d(0))):
        w = Deflate()
        hist = [("L", b) for b in _history(rnd, 700, lits12 if ll is LONG_LL else range(3))]
        tail = [("M", 3, 5), ("M", 12, 300), ("M", 42, 513), ("M", 130, 650), ("M", 19, 200)]          # 206 bytes
        w.dynamic(hist + _all_length_tokens(rnd, 600) + hist[:320] + tail, True, ll_lens=ll, d_lens=dl)
        out.append(_case(name, w))
    for rot in range(3):
        w = Deflate()
        w.stored(_history(rnd, 32768), False)
        tail = [("M", 5, d) for d in (1, 2, 4, 8, 24, 100, 700, 3000, 9000, 17000, 32768)] + [("M", 9, 12289 + 0xaaa)]
        w.dynamic(_all_distance_tokens(rnd) + [("L", 0)] * 320 + tail, True, ll_lens=SHORT_LL, d_lens=long_d(rot))
        out.append(_case("distances_behind_table_%d" % rot, w))
    w = Deflate()
    w.stored(_history(rnd, 32768), False)
    w.dynamic(_all_distance_tokens(rnd) + [("L", 0)] * 320 + [("M", 5, 32768), ("M", 9, 1)], True, ll_lens=SHORT_LL, d_lens=SHORT_D)
    out.append(_case("distances_in_table", w))

    # -- far distances, in a fixed and in a dynamic block, behind 32768 stored bytes
    far = [(n, d) for d in (4999, 5000, 6144, 6145, 8192, 8193, 12288, 12289, 16384, 16385, 24576, 24577, 32767, 32768) for n in (3, 64, 65, 258)]
    for kind in ("fixed", "dynamic"):
        w = Deflate()
        w.stored(_history(rnd, 32768), False)
        order = far[:]
        rnd.shuffle(order)
        toks = []
        for n, d in order:
            toks += [("M", n, d)] + [("L", rnd.randrange(256))] * rnd.randrange(0, 3)
        w.fixed(toks, True) if kind == "fixed" else w.dynamic(toks, True)
        def edge(b=w.blocks[1], kind=kind):
            got = {(u[5], u[1], u[3]) for u in b["uses"] if u[0] == "dist"}
            assert b["type"] == kind and len(got) == len(far) and {_DBASE[s] + x for _, s, x in got} == {d for _, d in far}
        out.append(_case("far_distances_%s" % kind, w, edge))

    # -- stored blocks: every bit phase in front of the header (k literals of 9 bits behind a 3-bit header and in front of a
    # 7-bit end-of-block code), lengths around the ring and the 256-byte lines; then matches into the stored bytes
    for k in range(9):
        for n in (0, 1, 2, 3, 4, 5, 6, 7, 8, 255, 256, 257, 2047, 2048, 2049, 5000):
            w = Deflate()
            w.fixed([("L", 200 + k)] * k, False)
            w.stored(_history(rnd, n), False)
            h = k + n
            toks = [("L", 1)] if h == 0 else [("M", min(258, max(h, 3)), h)]               # one match covers the whole history
            toks += [("L", 2), ("L", 3), ("M", 7, 3)]
            h = len(w.text) + sum(1 if t[0] == "L" else t[1] for t in toks)
            if h >= 1990: toks += [("M", 100, 1990), ("L", 4), ("M", 3, 1985)]
            w.fixed(toks, True)
            def edge(b=w.blocks, k=k, n=n):
                assert b[1]["type"] == "stored" and b[1]["bit"] % 8 == (2 + k) % 8 and b[1]["end"] - b[1]["start"] == n
            out.append(_case("stored_phase%d_len%d" % (k, n), w, edge))
    w = Deflate()
    w.dynamic([("L", b) for b in b"abcabcabd"] + [("M", 30, 3)], False)
    w.stored(b"", False)
    w.fixed([("M", 20, 39), ("L", 9)], True)
    out.append(_case("empty_stored_between_huffman_blocks", w, _types_are(w, ["dynamic", "stored", "fixed"])))
    w = Deflate()
    w.stored(_history(rnd, 300), False)
    w.dynamic([("M", 258, 300), ("L", 7)], False)
    w.stored(_history(rnd, 77), True)
    out.append(_case("stored_first_and_last", w, _types_are(w, ["stored", "dynamic", "stored"])))
    w = Deflate()
    w.fixed([("L", 250)] * 3, False)
    w.stored(_history(rnd, 1000), False)
    w.stored(_history(rnd, 1301), False)
    w.stored(b"", False)
    w.stored(_history(rnd, 2), False)
    w.fixed([("M", 258, 2306), ("M", 3, 2)], True)
    out.append(_case("stored_blocks_in_a_row", w, _types_are(w, ["fixed"] + ["stored"] * 4 + ["fixed"])))
    return out


def check_coverage(cases):
    """What the cases cover together: every length and distance symbol on both decode paths with every extra-bit pattern, in
    the block's last 260 bytes and well in front of them; alphabet sizes at both ends; the end-of-block code at 15 bits and at 1."""
    LL_BITS, D_BITS = 10, 8                                                      # coral_inflate_core.h
    blocks = [b for c in cases for b in c["blocks"] if b["type"] == "dynamic"]
    seen, place = set(), set()
    for b in blocks:
        for kind, s, nbits, x, e, pos in b["uses"]:
            behind = nbits > (LL_BITS if kind == "len" else D_BITS)
            seen.add((kind, s, behind, x))
            if behind:
                place.add((kind, "tail" if pos >= b["end"] - 260 else "body" if pos < b["end"] - 600 else "between"))
    for i in range(29):
        for behind in (False, True):
            for x in _pattern("len", _LEXT[i]):
                assert ("len", 257 + i, behind, x) in seen, (257 + i, behind, x)
    for j in range(30):
        for behind in (False, True):
            for x in _pattern("dist", _DEXT[j]):
                assert ("dist", j, behind, x) in seen, (j, behind, x)
    assert {("len", "tail"), ("len", "body"), ("dist", "tail"), ("dist", "body")} <= place
    assert {257, 286} <= {b["hlit"] for b in blocks} and {1, 30} <= {b["hdist"] for b in blocks} and {5, 19} <= {b["hclen"] for b in blocks}
    assert {1, 15} <= {b["ll_lens"][256] for b in blocks}
    assert any(7 in [b["cl_lens"][s] for s, _, _ in b["ops"]] for b in blocks)


def rejected_streams():
    """[(name, stream, declared size)]: streams that a decoder must refuse.  zlib refuses each (or, for the two with a wrong
    declared size, gives another number of bytes), asserted here."""
    rnd = random.Random(29)
    A, out = 65, []

    def add(name, w, size=None):
        comp, text = w.done() if isinstance(w, Deflate) else w
        out.append((name, comp, len(text) if size is None else size))

    lits = [("L", A), ("L", 66), ("L", 67)] * 4
    ok_ll = [0] * 65 + [2, 2, 2] + [0] * 188 + [2]                     # A B C and the end-of-block code
    w = Deflate()
    w.fixed(lits, False)
    w.raw(1, 1)
    w.raw(3, 2)
    add("btype_3", w)
    w = Deflate()
    w.stored(b"abcdefgh", True, nlen=0xfff6)
    add("nlen_mismatch", w)
    for beyond, n in ((1, 1), (1, 2), (1, 6), (3, 9), (1, 300), (1000, 3000)):
        w = Deflate()
        w.stored(_history(rnd, n - beyond), True, length=n)
        add("stored_%d_bytes_beyond_input_of_%d" % (beyond, n), w, n)
    for field in (30, 31):
        w = Deflate()
        w.dynamic(lits, True, ll_lens=ok_ll, d_lens=[1, 1], hlit=257 + field, strict=False)
        add("hlit_field_%d" % field, w)
        w = Deflate()
        w.dynamic(lits, True, ll_lens=ok_ll, d_lens=[1, 1], hdist=1 + field, strict=False)
        add("hdist_field_%d" % field, w)
    w = Deflate()
    w.dynamic(lits, True, ll_lens=ok_ll, d_lens=[0], rle=[(16, 3)] + plain_rle(ok_ll[3:] + [0]), strict=False)
    add("code_16_first", w)
    w = Deflate()
    w.dynamic(lits, True, ll_lens=ok_ll, d_lens=[0, 0], rle=plain_rle(ok_ll) + [(17, 3)], strict=False)
    add("repeat_past_the_last_length", w)
    w = Deflate()
    w.dynamic(lits, True, ll_lens=ok_ll, d_lens=[0, 0], rle=plain_rle(ok_ll[:250]) + [(18, 138)], strict=False)
    add("zero_run_past_the_last_length", w)
    w = Deflate()
    w.dynamic(lits + [("B", 0, 16)], True, ll_lens=[0] * 65 + [1, 2, 2] + [0] * 189, d_lens=[0], hlit=257, strict=False)
    add("no_end_of_block_code", w)
    w = Deflate()                                                        # hclen 4: only lengths of 0 can be written
    w.dynamic([], True, ll_lens=[0] * 257, d_lens=[0], cl_lens=[1] + [0] * 17 + [1], hclen=4, rle=[(18, 138), (18, 120)], strict=False)
    add("hclen_4", w, 7)
    w = Deflate()
    w.dynamic(lits, True, ll_lens=ok_ll, d_lens=[0], cl_lens=[1, 1, 1] + [0] * 16, rle=plain_rle, strict=False)
    add("oversubscribed_code_length_code", w)
    w = Deflate()
    w.dynamic(lits, True, ll_lens=[0] * 65 + [1, 1, 2] + [0] * 188 + [2], d_lens=[1, 1], strict=False)
    add("oversubscribed_literal_code", w)
    w = Deflate()
    w.dynamic(lits, True, ll_lens=ok_ll, d_lens=[1, 1, 1], strict=False)
    add("oversubscribed_distance_code", w)
    w = Deflate()                                                        # code-length code 0:2 2:2 18:2, the pattern 11 belongs to no symbol
    w._begin("dynamic", True, 2)
    for v, n in ((0, 5), (0, 5), (15, 4), (0, 3), (0, 3), (2, 3), (2, 3)) + ((0, 3),) * 11 + ((2, 3), (0, 3), (0, 3), (0, 3), (3, 2), (3, 2)):
        w.raw(v, n)
    add("unused_code_length_pattern", w, 5)
    for s in (286, 287):
        w = Deflate()
        w.fixed(lits + [("R", s)] + lits, True)
        add("literal_length_symbol_%d" % s, w)
    for s in (30, 31):
        w = Deflate()
        w.fixed(lits + [("R", 257, 0, s, 0)] + lits, True)
        add("distance_symbol_%d" % s, w, 27)
    for n in (0, 1, 5, 300, 3000):
        w = Deflate()
        d = distance_symbol(n + 1)
        w.fixed([("L", rnd.randrange(256)) for _ in range(n)] + [("R", 257, 0, d, n + 1 - _DBASE[d]), ("L", A)], True)
        add("distance_%d_after_%d_bytes" % (n + 1, n), w, n + 4)
    toks = [("L", rnd.choice(b"ACGT")) for _ in range(20000)]
    w = Deflate()
    w.dynamic(toks + [("M", 50, 4000)], True)
    valid = w.done()
    add("text_longer_than_declared", valid, len(valid[1]) - 1)
    add("text_shorter_than_declared", valid, len(valid[1]) + 1)
    for cut in range(1, 41):
        add("cut_after_%d_bytes" % cut, (valid[0][:cut], valid[1]))
    for name, comp, size in incomplete_streams():
        if name.endswith("pattern_used"):
            out.append((name, comp, size))
    for name, comp, size in out:
        try:
            assert len(zlib.decompress(comp, -15)) != size and name.startswith("text_"), name
        except zlib.error:
            pass
    return out


def incomplete_streams():
    """[(name, stream, text or declared size)]: literal / length and distance codes that leave bit patterns unused.  zlib refuses
    such a header; this decoder takes it (Inflater::build) as long as no unused pattern occurs: the `..._accepted` streams carry
    their text, their `..._pattern_used` siblings (a size) hold one unused pattern and must be refused."""
    A, out = 65, []
    ll = [0] * 65 + [2, 2] + [0] * 189 + [3, 3]                          # A = 00, B = 01, end of block = 100, length 3 = 101; 11x is no code
    body = [("L", A), ("L", 66), ("L", A), ("M", 3, 2), ("L", 66)]
    for used in (False, True):
        w = Deflate()
        w.dynamic(body + ([("B", 3, 2)] if used else []) + body, True, ll_lens=ll, d_lens=[1, 1])
        comp, text = w.done()
        out.append(("incomplete_literal_code_" + ("pattern_used" if used else "accepted"), comp, len(text) if used else text))
    for used in (False, True):                                           # distance symbols 0 1 2 at 2 bits: 11 is no code
        w = Deflate()
        w.dynamic(body + [("M", 3, 3)] + ([("R", 257), ("B", 3, 2)] if used else []) + body, True,
                  ll_lens=[0] * 65 + [2, 2] + [0] * 189 + [2, 2], d_lens=[2, 2, 2])
        comp, text = w.done()
        out.append(("incomplete_distance_code_" + ("pattern_used" if used else "accepted"), comp, len(text) if used else text))
    for name, comp, text in out:
        try:
            zlib.decompress(comp, -15)
            raise AssertionError("zlib accepts " + name)
        except zlib.error:
            pass
    return out


def dump(path):
    """Every hand-built stream for tests/native/inflate_streams_host.cpp: u32 length, stream, u32 size, u8 valid, text when valid."""
    with open(path, "wb") as fp:
        def entry(comp, size, text=None):
            fp.write(struct.pack("<I", len(comp)) + comp + struct.pack("<IB", size, text is not None) + (text or b""))
        for c in dynamic_streams():
            entry(c["comp"], len(c["text"]), c["text"])
        for name, comp, want in incomplete_streams():
            if name.endswith("accepted"):
                entry(comp, len(want), want)
        for _, comp, size in rejected_streams():
            entry(comp, size)


if __name__ == "__main__":
    import sys
    dump(sys.argv[1])
