"""The minimizer sketch's rule restated in plain Python by brute force, O(n w), straight from its definition - split the text into
contigs, give every position of a contig its key or +infinity, list the windows, take every position whose key is the minimum of a
window that holds it - and the table of FASTA byte strings that the CPU tests (tests/test_sketch_core.py: the host backend against
this restatement) and the GPU tests (tests/test_sketch_gpu.py and tests/test_sketch_limits_gpu.py: the device against the host
backend) share.  Nothing here calls the library but ``geometry`` and ``feed_in_pieces``, which runs a session on the host or, with
guard entries behind its arrays and its workspace, on a GPU."""
import ctypes as C
import functools

import numpy as np

from tests import kmer_cases

KW = ((5, 4), (8, 1), (11, 5), (15, 50), (3, 256))
EDGE_KW = ((16, 256), (16, 255), (16, 1), (16, 50), (1, 1), (1, 256), (2, 3))      # the limits of k and w; kept out of KW, which multiplies the whole case table
MANY_HEADERS_KW = ((3, 4), (16, 256), (1, 1))        # of the texts with more header lines than a device piece holds
GUARD = 64                           # untouched entries asked for behind every device output array,
WS_GUARD = 4096                      # and bytes of GUARD_BYTE behind every device workspace
SENTINEL, GUARD_BYTE = 0x5A5A5A5A5A5A5A5A, 0xA5
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
WHOLE = 2 << 20                      # a staging size that holds every text here


def guarded(n: int, device):
    """A device int64 tensor of n + GUARD entries, every one SENTINEL: an output array of n entries with its guard behind it."""
    import torch
    return torch.full((n + GUARD,), SENTINEL, dtype=torch.int64, device=device)


def guarded_workspace(n_bytes: int, device):
    """A device workspace of n_bytes + WS_GUARD bytes, every one GUARD_BYTE (the library is told of n_bytes)."""
    import torch
    assert n_bytes >= 0
    return torch.full((n_bytes + WS_GUARD,), GUARD_BYTE, dtype=torch.uint8, device=device)


def assert_untouched(array, n: int, what=""):
    """Everything from entry n on of a ``guarded`` array is still SENTINEL."""
    assert bool((array[n:] == SENTINEL).all()), "entries behind the first %d were written: %s" % (n, what)


def assert_workspace_guard(ws, n_bytes: int, what=""):
    assert ws.numel() == n_bytes + WS_GUARD and bool((ws[n_bytes:] == GUARD_BYTE).all()), "bytes behind the workspace were written: %s" % (what,)


def feed_in_pieces(data: bytes, k: int, w: int, piece: int, capacity: int, bitmap=None, device=None):
    """One session through the C ABI, ``piece`` bytes a feed (0: the whole text at once) -> (rc of the first call that failed or of
    finish, stats list, rows, names, lengths).  ``device`` None: the host backend.  Else the same session on that GPU at staging
    ``piece or WHOLE``: the arrays have GUARD entries behind the capacity and hold SENTINEL, the workspace has WS_GUARD bytes of
    GUARD_BYTE behind it, and after finish nothing behind the written entries and behind the workspace has changed.  Capacity 0: no
    arrays."""
    from coral_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    if device is None:
        keys, values = np.zeros(max(capacity, 1), dtype=np.uint64), np.zeros(max(capacity, 1), dtype=np.uint64)
        assert L.coral_sketch_open(k, w, -1, bitmap.ctypes.data if bitmap is not None else None, keys.ctypes.data if capacity else None, values.ctypes.data if capacity else None, capacity,
                                   0, None, 0, None, C.byref(h)) == 0
    else:
        import torch
        dev = torch.device(device)
        torch.cuda.set_device(dev)
        staging = piece or WHOLE
        dkeys, dvalues = guarded(capacity, dev), guarded(capacity, dev)
        ws_bytes = int(L.coral_sketch_workspace_bytes(staging))
        ws = guarded_workspace(ws_bytes, dev)
        dbitmap = torch.from_numpy(bitmap.view(np.int32)).to(dev) if bitmap is not None else None
        stream = torch.cuda.current_stream(dev)
        stream.synchronize()
        assert L.coral_sketch_open(k, w, dev.index or 0, dbitmap.data_ptr() if dbitmap is not None else None, dkeys.data_ptr() if capacity else None, dvalues.data_ptr() if capacity else None,
                                   capacity, staging, ws.data_ptr(), ws_bytes, stream.cuda_stream, C.byref(h)) == 0
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
    if device is not None:
        torch.cuda.synchronize(dev)
        what = (k, w, piece, capacity)
        assert 0 <= stats[3] <= capacity
        assert_untouched(dkeys, int(stats[3]), what)
        assert_untouched(dvalues, int(stats[3]), what)
        assert_workspace_guard(ws, ws_bytes, what)
        keys, values = dkeys.cpu().numpy().view(np.uint64), dvalues.cpu().numpy().view(np.uint64)
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
def limits_text() -> bytes:
    """One contig of 6 000 random bases with an N at 2000 and 300 x AC from 4000 on, in lines of 60: the text of the extreme k and w
    (EDGE_KW), short enough for the O(n w) restatement at w = 256."""
    seq = bytearray(kmer_cases.random_bases(np.random.RandomState(31), 6000))
    seq[2000:2001] = b"N"
    seq[4000:4600] = b"AC" * 300
    return b">limits\n" + kmer_cases.wrap(bytes(seq), 60)


def many_headers_text(geometry) -> bytes:
    """More header lines than one piece of the device session holds, several times over, sized from coral_sketch_geometry
    (``geometry``: its 8 entries): 3 max_bound + 928 empty contigs of one name, a contig of 300 bases, max_bound + 476 empty contigs,
    and a contig of 8 bases without a final newline.  Fed whole, the device cuts a piece at every max_bound header lines; the
    second piece finds the carry full of contig starts and adds max_bound of its own, which fills the contig table as far as it
    is ever filled (1 + carry + max_bound entries)."""
    max_bound, carry = int(geometry[4]), int(geometry[1])
    assert max_bound > carry                             # (the first piece ends on more than `carry` empty contigs)
    return _many_headers_text(max_bound)


@functools.lru_cache(maxsize=None)
def _many_headers_text(max_bound: int) -> bytes:
    rng = np.random.RandomState(32)
    return b">x\n" * (3 * max_bound + 928) + b">last\n" + kmer_cases.random_bases(rng, 300) + b"\n" + b">y\n" * (max_bound + 476) + b">z\nACGTTGCA"


@functools.lru_cache(maxsize=None)
def one_base_contigs() -> bytes:
    """3 000 contigs of one random base each: contig boundaries and bases alternate in everything the device carries."""
    bases = kmer_cases.random_bases(np.random.RandomState(33), 3000)
    return b"".join(b">s\n%c\n" % c for c in bases)


@functools.lru_cache(maxsize=None)
def poly_a_6200() -> bytes:
    """6 200 x A in lines of 61: at (k, w) = (5, 4) every one of its 6 196 k-mer positions is a minimizer, so output rank r is
    contig position r - the text of the capacity tests."""
    return b">p\n" + kmer_cases.wrap(b"A" * 6200, 61)


def geometry() -> tuple:
    """coral_sketch_geometry's 8 entries: tile, carry, block, items, max_bound, table_cap, the smallest staging size, the largest w."""
    from coral_amd import _lib
    g = (C.c_int32 * 8)()
    assert _lib.lib().coral_sketch_geometry(g) == 0
    return tuple(g)


@functools.lru_cache(maxsize=None)
def k16_weights_case():
    """-> (text, k, w, listed): limits_text() at (16, 50) and three canonical k-mers to list as repetitive.  The one of the
    smallest key outside the tandem: it is a minimizer, so listing it changes or removes its row.  The two of the
    AC tandem at 4000: the windows inside the tandem are repetitive as a whole and still yield their minimum, so rows with the
    repetitive bit - bit 32 at k = 16 - stay in the sketch."""
    data, k, w = limits_text(), 16, 50
    seq = contigs_of(data)[0][1]
    _key, _contig, pos, _strand = min(r for r in restate(data, k, w)[2] if not 4000 <= r[2] <= 4600 - k)
    listed = frozenset([canonical(seq[pos:pos + k]), canonical(b"AC" * 8), canonical(b"CA" * 8)])
    assert len(listed) == 3 and seq[4000:4600] == b"AC" * 300
    return data, k, w, listed


def assert_bit_32_marks_the_listed(data: bytes, rows, listed, k: int = 16):
    """In a sketch at k = 16 some rows carry bit 32, and they are exactly the rows of the listed k-mers."""
    seq = contigs_of(data)[0][1]
    marked = [r for r in rows if r[0] >> 32]
    assert len(marked) > 100 and all(r[0] >> 32 == 1 for r in marked)
    assert marked == [r for r in rows if canonical(seq[r[2]:r[2] + k]) in listed]


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
