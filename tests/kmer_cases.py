"""The k-mer counter's rule restated in plain Python - split the text into lines, drop the header lines, cut at every byte that is
no base, count the windows with a ``collections.Counter``, the ``distinct=`` threshold in Python integers - and the table of FASTA
byte strings that the CPU tests (tests/test_kmer_core.py: the host backend against this restatement) and the GPU tests
(tests/test_kmer_gpu.py: the device against the host backend) share.  Nothing here calls the library but ``feed_in_pieces``."""
import collections
import ctypes as C
import functools
import re

import numpy as np

KS = (1, 2, 3, 8, 11, 12)
_CODE = bytes.maketrans(b"ACGT", b"0123")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def parse(data: bytes):
    """-> (the runs of consecutive bases, upper case; the number of header lines)."""
    clean, headers = [], 0
    for line in data.split(b"\n"):                       # a line starts at the first byte and behind every '\n'
        if line.startswith(b">"):
            headers += 1
            clean.append(b"#")                           # a header line is one break
        else:
            clean.append(line.replace(b"\r", b""))       # '\n' and '\r' are skipped, not breaks
    return tuple(re.findall(rb"[ACGT]+", b"".join(clean).upper())), headers


def kmer_int(s: bytes) -> int:
    return int(s.translate(_CODE), 4)


def revcomp(s: bytes) -> bytes:
    return s[::-1].translate(_COMP)


@functools.lru_cache(maxsize=None)
def restate(data: bytes, k: int, canonical: bool):
    """-> (counts: k-mer integer -> count, stats dict, histogram: sorted list of (count value, distinct k-mers with it))."""
    runs, headers = parse(data)
    by_text = collections.Counter()
    for run in runs:
        by_text.update(run[i:i + k] for i in range(len(run) - k + 1))
    counts = collections.Counter()
    for s, c in by_text.items():
        counts[kmer_int(min(s, revcomp(s)) if canonical else s)] += c      # (equal lengths, A < C < G < T: the smaller text is the smaller integer)
    stats = dict(n_sequences=headers, n_bases=sum(len(r) for r in runs), total=sum(by_text.values()), distinct=len(counts))
    return dict(counts), stats, sorted(collections.Counter(counts.values()).items())


def threshold(hist, p_text: str) -> int:
    """hist: (count value, number) pairs; p_text: decimal text.  p = P / 10^d exactly; need = ceil(P * distinct / 10^d); the
    smallest c >= 0 with at least `need` distinct k-mers of a count <= c."""
    whole, _, frac = p_text.partition(".")
    P, scale = int((whole or "0") + frac), 10 ** len(frac)
    distinct = sum(n for _v, n in hist)
    need = (P * distinct + scale - 1) // scale
    c = 0
    while sum(n for v, n in hist if v <= c) < need:
        c = min(v for v, _n in hist if v > c)                # (nothing changes between two count values)
    return c


def expected_lines(counts: dict, k: int, t: int, both_strands: bool = False) -> bytes:
    out = []
    for v in sorted(counts):
        if counts[v] <= t:
            continue
        s = "".join("ACGT"[(v >> (2 * (k - 1 - i))) & 3] for i in range(k)).encode()
        out.append(b"%s\t%d\n" % (s, counts[v]))
        if both_strands and revcomp(s) != s:
            out.append(b"%s\t%d\n" % (revcomp(s), counts[v]))
    return b"".join(out)


# ---- the library, fed in pieces ---------------------------------------------------------------------------------------------------
def feed_in_pieces(data: bytes, k: int, canonical: bool, piece: int):
    """The host backend through the C ABI, ``piece`` bytes a feed (0: the whole text at once) -> (non-zero entries as a dict, stats
    dict, histogram pairs)."""
    from coral_amd import _lib
    L = _lib.lib()
    table = np.zeros(1 << (2 * k), dtype=np.uint32)
    h = C.c_void_p()
    assert L.coral_kmer_open(k, int(canonical), -1, table.ctypes.data, 0, None, 0, None, 0, C.byref(h)) == 0
    try:
        buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8)
        base = buf.ctypes.data
        for at in range(0, len(data), piece or max(len(data), 1)):
            assert L.coral_kmer_feed(h, base + at, min(piece or len(data), len(data) - at)) == 0
        stats = (C.c_int64 * 8)()
        assert L.coral_kmer_finish(h, stats, None) == 0
        values, nums = np.zeros(stats[4], dtype=np.int64), np.zeros(stats[4], dtype=np.int64)
        assert L.coral_kmer_histogram(h, stats[4], values.ctypes.data, nums.ctypes.data) == 0
    finally:
        L.coral_kmer_close(h)
    return nonzero(table), dict(zip(("n_sequences", "n_bases", "total", "distinct"), (int(x) for x in stats[:4]))), list(zip(values.tolist(), nums.tolist()))


def nonzero(table: np.ndarray) -> dict:
    at = np.flatnonzero(table)
    return dict(zip(at.tolist(), table[at].tolist()))


def results_of(kc):
    """A ``kmers.KmerCounts`` -> (non-zero entries, stats, histogram pairs), as ``restate`` gives them."""
    values, nums = kc.histogram()
    return nonzero(kc.table()), dict(n_sequences=kc.n_sequences, n_bases=kc.n_bases, total=kc.total, distinct=kc.distinct), list(zip(values.tolist(), nums.tolist()))


# ---- the case table ---------------------------------------------------------------------------------------------------------------
def wrap(seq: bytes, width: int, end: bytes = b"\n") -> bytes:
    return b"".join(seq[i:i + width] + end for i in range(0, len(seq), width))


def random_bases(rng, n: int) -> bytes:
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, n)])


@functools.lru_cache(maxsize=None)
def random_megabase() -> bytes:
    """1 Mb, seeded, with planted repeats (a 3 kb element 30 times, a 7-mer tandem of 2 kb, a 40 kb duplication, poly-A and N
    blocks), split over 40 records of 60-column lines."""
    rng = np.random.RandomState(20150)
    seq = bytearray(random_bases(rng, 1_000_000))
    element = random_bases(rng, 3000)
    for at in rng.randint(0, 990_000, 30):
        seq[at:at + 3000] = element
    seq[500_000:502_002] = (b"ACGGTCA" * 286)
    seq[700_000:740_000] = seq[100_000:140_000]
    seq[250_000:250_400] = b"A" * 400
    for at in (0, 333_333, 999_900):
        seq[at:at + 100] = b"N" * 100
    cuts = [0] + sorted(rng.choice(np.arange(1, 1_000_000), 39, replace=False).tolist()) + [1_000_000]
    return b"".join(b">record%d some words\n" % i + wrap(bytes(seq[a:b]), 60) for i, (a, b) in enumerate(zip(cuts, cuts[1:])))


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    rng = np.random.RandomState(7)
    lengths = (0, 1, 2, 3, 4, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17)       # k-1, k and k+1 bases of every k the tests use
    body = random_bases(rng, 700)
    out = {}
    out["empty"] = b""
    out["lengths_around_k"] = b"".join(b">len%d\n" % n + random_bases(rng, n) + b"\n" for n in lengths)
    out["empty_sequences_and_last_header"] = b">a\n>b\n>c\nACGTACGTTGCAGGATCCA\n>d\n\n>e\nGGGATTACAGATTACA\n>last header"
    out["no_trailing_newline"] = b">x\n" + wrap(body, 60)[:-1]
    out["no_header"] = body[:200] + b"\n" + body[200:333]
    out["crlf"] = b">x desc\r\n" + wrap(body, 60, b"\r\n") + b">y\r\n" + wrap(body[::-1], 61, b"\r\n")
    out["cr_inside_and_alone"] = b">x\nACGT\rACGTTGCA\r\rGGA\n\rTTACAGATTACA\r>TT\nAC"
    out["blank_lines"] = b"\n\n>x\n\n" + wrap(body[:150], 60) + b"\n\n\n" + wrap(body[150:300], 60) + b"\n>y\n\n\n" + body[300:350] + b"\n\n"
    out["width_1"] = b">x\n" + wrap(body[:120], 1)
    out["width_60"] = b">x\n" + wrap(body, 60)
    out["width_61"] = b">x\n" + wrap(body, 61)
    out["mixed_widths"] = b">x\n" + wrap(body[:100], 1) + wrap(body[100:400], 61) + wrap(body[400:], 60)
    out["lower_and_mixed_case"] = b">x\n" + wrap(body.lower()[:300], 60) + wrap(bytes(c + 32 if i % 3 == 0 else c for i, c in enumerate(body[300:])), 60)
    n_every = b"".join(b">every%d\n" % n + wrap(b"".join(random_bases(rng, n) + b"N" * (1 + j % 3) for j in range(12)), 60) for n in lengths[1:])
    out["n_runs"] = b">x\nNNNNNNNN" + body[:90] + b"\nNNNN\n" + body[90:180] + b"NNNNNNNNNNNN\n" + n_every
    out["iupac_and_symbols"] = b">x\nACGTRYACGTTGCAKMSWACGGTTAACCBDHVGATTACA*ACGTACGTTGCA-ACGGTTAACCGG ACGTACGT\tTTGACCA.ACGGTTAAU\n"
    out["gt_in_header_and_sequence"] = b">x > y >z\nACGTTGCAGG>ACGTTGCAGGATCCAAG\nAC>GT\n >notaheader\nACGTTGCAGGATC\n"
    out["long_header"] = b">" + b"h" * 5000 + b" ACGTACGTACGTACGTACGT\n" + wrap(body[:240], 60) + b">" + b"ACGT" * 2000 + b"\n" + body[240:300] + b"\n"
    out["poly_a"] = b">polyA\n" + b"A" * 100_000 + b"\n"
    out["tandem_ac"] = b">ac\n" + wrap(b"AC" * 50_000, 60)
    out["tandem_acg"] = b">acg\n" + wrap(b"ACG" * 30_000, 61)
    out["palindromes"] = b">pal\n" + wrap(b"ACGT" * 300, 60) + b">pal2\nAATT\nGGCC\nTTAAN\nGAATTC\n"
    out["random_megabase"] = random_megabase()
    return out


SMALL = tuple(n for n in ("lengths_around_k", "empty_sequences_and_last_header", "crlf", "n_runs", "long_header", "palindromes"))
