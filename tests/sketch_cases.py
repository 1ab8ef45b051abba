"""The minimizer sketch's rule restated in plain Python by brute force, O(n w), straight from its definition - split the text into
contigs, give every position of a contig its key or +infinity, list the windows, take every position whose key is the minimum of a
window that holds it - and the table of FASTA byte strings that the CPU tests (tests/test_sketch_core.py: the host backend against
this restatement) and the GPU tests (tests/test_sketch_gpu.py: the device against the host backend) share.  Nothing here calls the
library but ``feed_in_pieces``."""
import ctypes as C
import functools

import numpy as np

from tests import kmer_cases

KW = ((5, 4), (8, 1), (11, 5), (15, 50), (3, 256))
INF = float("inf")
REFUSED = "refused"                  # what `restate` gives for a text with a sequence byte in front of the first header line
_CODE = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def hash64(x: int, k: int) -> int:
    mask = 4 ** k - 1
    x = (~x + (x << 21)) & mask
    x = x ^ (x >> 24)
    x = (x + (x << 3) + (x << 8)) & mask
    x = x ^ (x >> 14)
    x = (x + (x << 2) + (x << 4)) & mask
    x = x ^ (x >> 28)
    x = (x + (x << 31)) & mask
    return x


@functools.lru_cache(maxsize=None)
def contigs_of(data: bytes):
    """-> a list of (name, positions: the bytes of the contig's sequence lines without '\\n' and '\\r'), or REFUSED."""
    out, lines = [], data.split(b"\n")                   # a line starts at the first byte and behind every '\n'
    for line in lines:
        if line.startswith(b">"):
            name = line[1:]
            for stop in b" \t\r":
                name = name.split(bytes([stop]))[0]
            out.append([name.decode(), bytearray()])
        else:
            kept = line.replace(b"\r", b"")
            if kept and not out:
                return REFUSED
            if kept:
                out[-1][1].extend(kept)
    return [(n, bytes(s)) for n, s in out]


def keys_of(seq: bytes, k: int, repetitive=frozenset()):
    """(key or INF, strand) of every k-mer position of a contig."""
    out = []
    for p in range(len(seq) - k + 1):
        codes = [_CODE.get(c) for c in seq[p:p + k]]
        if None in codes:
            out.append((INF, 0))
            continue
        fwd = rev = 0
        for c in codes:
            fwd = fwd << 2 | c
        for c in reversed(codes):
            rev = rev << 2 | (3 - c)
        if fwd == rev:
            out.append((INF, 0))
            continue
        canon = min(fwd, rev)
        out.append((hash64(canon, k) | (int(canon in repetitive) << (2 * k)), int(rev < fwd)))
    return out


def minimizers_of(seq: bytes, k: int, w: int, repetitive=frozenset()):
    """The minimizers of one contig as (pos, strand, key), by the definition."""
    keys = keys_of(seq, k, repetitive)
    n = len(keys)
    if n < 1:
        return []
    ww = min(w, n)
    chosen = set()
    for j in range(n - ww + 1):                          # the windows that lie wholly inside the contig
        window = [keys[j + i][0] for i in range(ww)]
        m = min(window)
        if m != INF:
            chosen.update(j + i for i in range(ww) if window[i] == m)
    return [(p, keys[p][1], keys[p][0]) for p in sorted(chosen)]


@functools.lru_cache(maxsize=None)
def restate(data: bytes, k: int, w: int, repetitive=frozenset()):
    """-> (names, lengths, rows: (key, contig, pos, strand) in (contig, pos) order), or REFUSED."""
    contigs = contigs_of(data)
    if contigs == REFUSED:
        return REFUSED
    rows = [(key, c, p, s) for c, (_n, seq) in enumerate(contigs) for p, s, key in minimizers_of(seq, k, w, repetitive)]
    return [n for n, _s in contigs], [len(s) for _n, s in contigs], rows


def sorted_rows(rows):
    """The index order: by key, ties in (contig, pos) order."""
    return sorted(rows, key=lambda r: (r[0], r[1], r[2]))


def bitmap_of(canon_kmers, k: int) -> np.ndarray:
    bitmap = np.zeros(max(1, 4 ** k // 32), dtype=np.uint32)
    for v in canon_kmers:
        bitmap[v >> 5] |= np.uint32(1 << (v & 31))
    return bitmap


def canonical(seq: bytes) -> int:
    return min(kmer_cases.kmer_int(seq.upper()), kmer_cases.kmer_int(kmer_cases.revcomp(seq.upper())))


# ---- the library, fed in pieces ---------------------------------------------------------------------------------------------------
def feed_in_pieces(data: bytes, k: int, w: int, piece: int, capacity: int, bitmap=None):
    """The host backend through the C ABI, ``piece`` bytes a feed (0: the whole text at once) -> (rc of the first call that failed
    or of finish, stats list, rows, names, lengths)."""
    from coral_amd import _lib
    L = _lib.lib()
    keys, values = np.zeros(max(capacity, 1), dtype=np.uint64), np.zeros(max(capacity, 1), dtype=np.uint64)
    h = C.c_void_p()
    assert L.coral_sketch_open(k, w, -1, bitmap.ctypes.data if bitmap is not None else None, keys.ctypes.data, values.ctypes.data, capacity, 0, None, 0, None, C.byref(h)) == 0
    stats = (C.c_int64 * 8)()
    try:
        buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8)
        base = buf.ctypes.data
        for at in range(0, len(data), piece or max(len(data), 1)):
            rc = L.coral_sketch_feed(h, base + at, min(piece or len(data), len(data) - at))
            if rc != 0:
                return rc, list(stats), [], [], []
        rc = L.coral_sketch_finish(h, stats, None)
        if rc not in (0, -3):
            return rc, list(stats), [], [], []
        n_contigs, names_bytes = int(stats[0]), int(stats[6])
        lengths, name_off, blob = np.zeros(n_contigs, dtype=np.int64), np.zeros(n_contigs + 1, dtype=np.int64), np.zeros(max(names_bytes, 1), dtype=np.uint8)
        if rc == 0:
            assert L.coral_sketch_contigs(h, n_contigs, lengths.ctypes.data, names_bytes, blob.ctypes.data, name_off.ctypes.data) == 0
    finally:
        L.coral_sketch_close(h)
    text = blob.tobytes()
    names = [text[name_off[c]:name_off[c + 1]].decode() for c in range(n_contigs)]
    return rc, list(stats), rows_of(keys[:stats[3]], values[:stats[3]]), names, lengths.tolist()


def rows_of(keys, values):
    keys, values = np.asarray(keys, dtype=np.uint64), np.asarray(values, dtype=np.uint64)
    return list(zip(keys.tolist(), (values >> np.uint64(32)).tolist(), ((values & np.uint64(0xFFFFFFFF)) >> np.uint64(1)).tolist(), (values & np.uint64(1)).tolist()))


def index_rows(idx):
    """A ``minimizers.MinimizerIndex`` -> its rows (key, contig, pos, strand) in index order."""
    keys, contigs, positions, strands = idx.arrays()
    return list(zip(keys.tolist(), contigs.tolist(), positions.tolist(), strands.tolist()))


# ---- the case table ---------------------------------------------------------------------------------------------------------------
KNOWN_TEXT = b"ACGTTGCAGGATCCAAGTCTAGGCATTACAGATTACA"
KNOWN_ANSWER = [(3, 1, 243), (4, 1, 239), (8, 1, 34), (9, 0, 34), (11, 0, 51), (14, 0, 10), (17, 1, 411), (19, 1, 87), (21, 1, 50), (23, 0, 247), (27, 0, 283), (28, 1, 93),
                (32, 1, 339)]                            # (pos, strand, key) at k = 5, w = 4, no weights


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    """The byte strings of tests/kmer_cases.py (the two large tandems cut to 3 kb: the restatement is O(n w)) and the sketch's own."""
    rng = np.random.RandomState(11)
    rb, wrap = kmer_cases.random_bases, kmer_cases.wrap
    out = {name: data for name, data in kmer_cases.cases().items() if name not in ("random_megabase", "poly_a", "tandem_ac", "tandem_acg")}
    around = []
    for k, w in KW:
        around += [k - 1, k, k + 1, k + w - 2, k + w - 1, k + w]
    out["contigs_around_k_and_w"] = b"".join(b">c%d_%d\n" % (i, n) + wrap(rb(rng, n), 60) for i, n in enumerate(around))
    body = rb(rng, 1200)
    for k, w in KW:
        out["n_runs_around_w%d" % w] = b">n\n" + wrap(body[:300] + b"N" * (w - 1) + body[300:600] + b"N" * w + body[600:900] + b"N" * (w + 1) + body[900:], 70)
    out["poly_a"] = b">polyA\n" + wrap(b"A" * 3000, 60)      # every position is chosen
    out["tandem_ac"] = b">ac\n" + wrap(b"AC" * 1500, 60)     # every second one (odd k), or every one
    out["tandem_acg"] = b">acg\n" + wrap(b"ACG" * 1000, 61)
    out["acgt_palindromes"] = b">pal\n" + wrap(b"ACGT" * 200, 60) + b">pal8\nACGTACGTAATTCCGGAATTACGT\n"
    pair = rb(rng, 15)
    out["reverse_complement_tie"] = b">tie\n" + pair + kmer_cases.revcomp(pair) + b"\n" + rb(rng, 40) + pair + b"T" + kmer_cases.revcomp(pair) + b"\n"
    out["known_answer"] = b">known\n" + KNOWN_TEXT + b"\n"
    out["lower_case_crlf"] = b">x desc\r\n" + wrap(body[:400].lower(), 60, b"\r\n") + b">y\r\n" + wrap(body[400:800], 61, b"\r\n")
    out["header_last"] = b">a\n" + wrap(body[:200], 60) + b">b"
    out["many_short_contigs"] = b"".join(b">s%d\n" % i + rb(rng, int(n)) + b"\n" for i, n in enumerate(rng.randint(0, 70, 200)))
    return out


@functools.lru_cache(maxsize=None)
def six_records() -> bytes:
    """20 kb in 6 records with an N run, a tandem and lower case: the text of the piece-independence tests."""
    rng = np.random.RandomState(12)
    seq = bytearray(kmer_cases.random_bases(rng, 20_000))
    seq[5000:5120] = b"N" * 120
    seq[9000:9400] = b"AC" * 200
    seq[15000:15600] = bytes(seq[15000:15600]).lower()
    cuts = [0, 40, 3000, 3049, 11000, 11064, 20_000]
    return b"".join(b">rec%d words\n" % i + kmer_cases.wrap(bytes(seq[a:b]), 60) for i, (a, b) in enumerate(zip(cuts, cuts[1:])))


@functools.lru_cache(maxsize=None)
def anchor_setup(contig_len: int = 20_000, n_reads: int = 50, read_len: int = 2000):
    """A reference of 3 contigs (an N run, a tandem, a duplication) and reads that are exact substrings, every second one reverse
    complemented -> (FASTA bytes, [(contig, start, reverse, read bytes)])."""
    rng = np.random.RandomState(13)
    contigs = [bytearray(kmer_cases.random_bases(rng, contig_len)) for _ in range(3)]
    contigs[0][4000:4100] = b"N" * 100
    contigs[1][6000:6600] = b"ACGGTCA" * 85 + b"ACGGT"
    contigs[2][12000:15000] = contigs[0][8000:11000]
    reads = []
    for i in range(n_reads):
        c, a = int(rng.randint(0, 3)), int(rng.randint(0, contig_len - read_len + 1))
        read = bytes(contigs[c][a:a + read_len])
        reads.append((c, a, i % 2 == 1, kmer_cases.revcomp(read.replace(b"N", b"#")).replace(b"#", b"N") if i % 2 else read))
    fasta = b"".join(b">ref%d\n" % c + kmer_cases.wrap(bytes(s), 80) for c, s in enumerate(contigs))
    return fasta, reads


def check_anchor_property(index, reads, k: int, seqs_sketch, max_occ: int):
    """Every minimizer (p, s, key) of a forward read ref[a : a + L] has (a + p, s, key) in the reference sketch, of a reverse-
    complemented one (a + L - k - p, s ^ 1, key): asserted for every minimizer of every read through ``anchors``; returns the
    number of minimizers checked."""
    query, pos, strand, key = seqs_sketch
    aq, aqpos, acontig, arpos, astrand = index.anchors((query, pos, strand, key), max_occ=max_occ)
    have = set(zip(aq.tolist(), aqpos.tolist(), acontig.tolist(), arpos.tolist(), astrand.tolist()))
    assert len(query) > 0
    for q, p in zip(query.tolist(), pos.tolist()):
        c, a, reverse, read = reads[q]
        want = (q, p, c, a + len(read) - k - p, 1) if reverse else (q, p, c, a + p, 0)
        assert want in have, "read %d: its minimizer at %d has no anchor %r" % (q, p, want)
    return len(query)
