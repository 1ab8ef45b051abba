"""The composition rule of coral_amd/csrc/coral_comp_core.h restated in plain Python, the shared small cases, and a driver of the
C ABI's session (coral_comp_*) that tests/test_comp_core.py (host backend) and tests/test_comp_gpu.py (device) both use."""
import ctypes as C

import numpy as np

from coral_amd import _lib


class Refused(Exception):
    pass


def restate(data: bytes, bin_size: int):
    """(names, lengths, gc, at, masked) of the FASTA bytes, line by line; ``Refused`` where the rule refuses the text."""
    names, lengths, seqs = [], [], []
    lines = data.split(b"\n")                      # a line starts at the first byte and behind every '\n'
    if lines and lines[-1] == b"" and data.endswith(b"\n"):
        lines.pop()                                # (no line behind the last '\n')
    for line in lines:
        if line[:1] == b">":
            name = line[1:]
            for stop in (b" ", b"\t", b"\r"):
                name = name.split(stop)[0]
            if not name:
                raise Refused("empty name")
            names.append(name.decode("latin-1"))
            seqs.append(bytearray())
        else:
            body = line.replace(b"\r", b"")
            if body and not seqs:
                raise Refused("sequence in front of the first header")
            if body:
                seqs[-1] += body
    gc, at, masked = [], [], []
    for s in seqs:
        lengths.append(len(s))
        for a in range(0, len(s), bin_size):
            part = bytes(s[a:a + bin_size])
            gc.append(sum(part.count(x) for x in (b"G", b"C", b"g", b"c")))
            at.append(sum(part.count(x) for x in (b"A", b"T", b"a", b"t")))
            masked.append(sum(1 for x in part if 97 <= x <= 122))
    return names, lengths, gc, at, masked


def random_sequence(rng, n, alphabet=b"ACGTacgtNn"):
    return bytes(np.frombuffer(alphabet, dtype=np.uint8)[rng.randint(0, len(alphabet), n)])


def wrap(seq: bytes, width: int, end: bytes = b"\n") -> bytes:
    return b"".join(seq[a:a + width] + end for a in range(0, len(seq), width))


def cases():
    """name -> (FASTA bytes, bin sizes): the inputs the issue of the feature lists, small enough to be cut at every byte."""
    rng = np.random.RandomState(11)
    seq = lambda n, alphabet=b"ACGTacgtNn": random_sequence(rng, n, alphabet)
    out = {}
    out["crlf"] = (b">one first contig\r\n" + wrap(seq(130), 30, b"\r\n") + b">two\r\n" + wrap(seq(45), 30, b"\r\n"), (1, 7, 30, 50))
    out["lowercase_runs"] = (b">lc\n" + wrap(b"ACGT" * 5 + b"acgtnnnn" * 6 + b"GGCC" * 4 + b"atat" * 7, 25), (8, 10, 16))
    out["n_runs"] = (b">gaps\n" + wrap(b"N" * 40 + seq(33, b"ACGT") + b"N" * 7 + b"n" * 21 + seq(19, b"ACGT"), 20), (10, 20, 21))
    out["iupac_and_star"] = (b">codes\nACGTRYSWKMBDHVN*-acgtryswkmbdhvn.xX>\nUu*A\n", (4, 5, 1000))
    out["shorter_than_a_bin"] = (b">tiny\nACG\n>next\n" + wrap(seq(64), 16), (16, 50))
    out["ends_on_a_bin_edge"] = (b">edge\n" + wrap(seq(64), 16) + b">after\n" + wrap(seq(17), 16), (16, 32, 64))
    out["empty_contig_between"] = (b">a\n" + wrap(seq(20), 10) + b">empty\n>b desc\n" + wrap(seq(21), 10) + b">e2\n\n\r\n>c\nAC\n", (5, 10))
    out["header_as_last_line"] = (b">a\nACGTTGCA\n>last one", (3,))
    out["header_last_with_newline"] = (b">a\nACGTTGCA\n>last\n", (3,))
    out["no_trailing_newline"] = (b">a\nACGTTGCA\nacgtn", (4, 5))
    out["names_with_descriptions"] = (b">chr1 homo sapiens\nACGT\n>chr2\tx y\nGGCCA\n>chr3|a=b more\r\nTT\n>chr4\n\n", (2, 4))
    out["bin_size_one"] = (b">one\n" + wrap(seq(37), 9) + b">two\nNacgt\n", (1,))
    out["bin_larger_than_the_file"] = (b">a\n" + wrap(seq(50), 12) + b">b\n" + wrap(seq(9), 12), (100000, (1 << 31) - 1))
    out["leading_blank_lines"] = (b"\n\r\n\n>a\nACGT\n", (3,))
    out["gt_inside_a_line"] = (b">a>b c\nAC>GT\nA\r>x\n", (2, 4))
    return out


def run_session(pieces, bin_size, capacity, device=-1, staging=0, stream_setup=None):
    """The C ABI's session over the given pieces -> (rc of the failing call or 0, stats[8], names, lengths, gc, at, masked).  Host
    tables for device < 0; for a device session ``stream_setup(capacity, staging)`` returns (tables tensor [3][capacity], workspace
    tensor, workspace bytes, stream handle, download function)."""
    L = _lib.lib()
    h = C.c_void_p()
    stats = (C.c_int64 * 8)()
    if device < 0:
        tables = np.zeros((3, max(capacity, 1)), dtype=np.uint32)
        rc = L.coral_comp_open(bin_size, -1, tables[0].ctypes.data, tables[1].ctypes.data, tables[2].ctypes.data, capacity, 0, None, 0, None, C.byref(h))
        download = lambda: tables
    else:
        dev_tables, ws, ws_bytes, stream, download = stream_setup(capacity, staging)
        rc = L.coral_comp_open(bin_size, device, dev_tables[0].data_ptr(), dev_tables[1].data_ptr(), dev_tables[2].data_ptr(), capacity, staging, ws.data_ptr(), ws_bytes, stream,
                               C.byref(h))
    if rc != 0:
        return rc, list(stats), None, None, None, None, None
    try:
        for p in pieces:
            rc = L.coral_comp_feed(h, bytes(p), len(p))
            if rc != 0:
                return rc, list(stats), None, None, None, None, None
        rc = L.coral_comp_finish(h, stats, None)
        st = list(stats)
        if rc != 0:
            return rc, st, None, None, None, None, None
        lengths, off, blob = np.zeros(st[0], dtype=np.int64), np.zeros(st[0] + 1, dtype=np.int64), np.zeros(max(st[6], 1), dtype=np.uint8)
        assert L.coral_comp_contigs(h, st[0], lengths.ctypes.data, st[6], blob.ctypes.data, off.ctypes.data) == 0
        t = download()
        text = blob.tobytes()
        names = [text[off[c]:off[c + 1]].decode("latin-1") for c in range(st[0])]
        return 0, st, names, lengths.tolist(), t[0][:st[2]].tolist(), t[1][:st[2]].tolist(), t[2][:st[2]].tolist()
    finally:
        L.coral_comp_close(h)


def expected(data, bin_size):
    """``run_session``'s tuple as the restatement gives it."""
    names, lengths, gc, at, masked = restate(data, bin_size)
    stats = [len(names), sum(lengths), len(gc), sum(gc), sum(at), sum(masked), sum(len(n.encode("latin-1")) for n in names), 0]
    return 0, stats, names, lengths, gc, at, masked


# ---- the GC rule of the copy-number segmenter (coral_cn_core.h), restated over tests/cnv_cases.py's pieces -----------------------
def restate_gc(case, gc, at, strata=100, min_bins=256, permille=500, margins=None):
    """-> (rows, counts, bias [strata + 1], stratum_bins [strata + 1]) of a cnv_cases.Case with the composition (gc, at) per bin:
    cnv_cases.restate with the called-base mask, the strata, the pooled lower medians and s' = s - bias in front of the details."""
    import math
    from tests import cnv_cases as cn
    bases = [int(v) for v in case.bases]
    ref = None if case.ref is None else [int(v) for v in case.ref]
    gc, at = [int(v) for v in gc], [int(v) for v in at]
    flags, size = case.centre_flags(), case.bin_size
    contig_bins = [range(int(case.bin_off[c]), int(case.bin_off[c + 1])) for c in range(len(case.chroms))]
    cand, uncalled = set(), 0
    for c, bins in enumerate(contig_bins):
        for b in bins:
            if ((b - bins.start) + 1) * size <= case.lengths[c] and bases[b] > 0 and (ref is None or ref[b] > 0):
                acgt = gc[b] + at[b]
                if acgt > 0 and acgt * 1000 >= size * permille:
                    cand.add(b)
                else:
                    uncalled += 1
    counts = {"kept": 0, "centre": 0, "ref_centre": 0, "breakpoints": 0, "uncalled": uncalled}
    bias, stratum_bins = [0] * (strata + 1), [0] * (strata + 1)
    mid = [b for c, bins in enumerate(contig_bins) if flags[c] for b in bins if b in cand]
    if not mid:
        return [], counts, bias, stratum_bins
    C = counts["centre"] = cn.lower_median([bases[b] for b in mid])
    Cr = counts["ref_centre"] = cn.lower_median([ref[b] for b in mid]) if ref is not None else 0
    kept = [[b for b in bins if b in cand and bases[b] * 32 >= C and (ref is None or ref[b] * 32 >= Cr)] for bins in contig_bins]
    s = {b: cn.log2_q16(bases[b]) - cn.log2_q16(C) - ((cn.log2_q16(ref[b]) - cn.log2_q16(Cr)) if ref is not None else 0) for k in kept for b in k}
    g = {b: gc[b] * strata // (gc[b] + at[b]) for b in s}
    pool = [b for c, k in enumerate(kept) if flags[c] for b in k]
    for b in pool:
        stratum_bins[g[b]] += 1
    need = min(min_bins, len(pool))
    for t in range(strata + 1):
        w = 0
        while True:
            lo, hi = max(0, t - w), min(strata, t + w)
            inside = [s[b] for b in pool if lo <= g[b] <= hi]
            if len(inside) >= need:
                break
            w += 1
        bias[t] = cn.lower_median(inside) if inside else 0
    rows = []
    for c, bins in enumerate(contig_bins):
        n = len(kept[c])
        if n == 0:
            continue
        counts["kept"] += n
        x = [s[b] - bias[g[b]] for b in kept[c]]
        found = set()
        if n >= 2:
            d = cn.lower_median([abs(x[k] - x[k - 1]) for k in range(1, n)])
            sigma = 1.4826 * d / math.sqrt(2.0)
            for l in range(1, case.levels + 1):
                h = 1 << l
                if h > n:
                    continue
                pk = cn.peaks(cn.details(x, h))
                cut = cn.fdr_cut(sorted(pk.values(), reverse=True), h, sigma, case.q, margins)
                before = set(found)
                for k, m in pk.items():
                    if m >= cut and not any(abs(k - b) <= 1 << (l - 1) for b in before):
                        found.add(k)
        counts["breakpoints"] += len(found)
        edges = [0] + sorted(found) + [n]
        for a, b in zip(edges[:-1], edges[1:]):
            first, last = kept[c][a] - bins.start, kept[c][b - 1] - bins.start
            rows.append((c, first * size, min((last + 1) * size, case.lengths[c]), b - a, sum(x[a:b]), sum(bases[j] for j in kept[c][a:b])))
    return rows, counts, bias, stratum_bins


def gc_cases():
    """name -> (cnv_cases.Case, gc, at, strata, min_bins, permille): the tables the issue of the feature lists."""
    from tests import cnv_cases as cn
    rng = np.random.RandomState(77)
    out = {}

    def comp(n, size, lo=0.3, hi=0.6, called=1.0):
        acgt = np.full(n, int(size * called), dtype=np.int64)
        gc = (acgt * rng.uniform(lo, hi, n)).astype(np.int64)
        return gc.astype(np.uint32), (acgt - gc).astype(np.uint32)

    def wave(case_bases, gc, at, amp=0.4):
        """depth multiplied by a smooth function of the bin's GC fraction"""
        f = gc.astype(np.float64) / np.maximum(gc.astype(np.float64) + at, 1)
        return np.maximum((case_bases * (1.0 + amp * np.sin(8.0 * f))).astype(np.int64), 0)

    out["g4_three_bins"] = (cn.Case(["chr1"], [300], 100, [1000, 1100, 900]), np.array([10, 50, 100], dtype=np.uint32), np.array([90, 50, 0], dtype=np.uint32), 4, 1, 500)
    gc, at = comp(50, 100, 0.05, 0.95)
    out["g1000_fifty_bins"] = (cn.Case(["chr1"], [5000], 100, wave(cn.noisy(rng, 50, 4000, [(20, 30, 2.0)]), gc, at)), gc, at, 1000, 8, 500)
    n = 400
    out["one_stratum"] = (cn.Case(["chr1"], [n * 100], 100, cn.noisy(rng, n, 3000, [(100, 160, 2.0)])), np.full(n, 41, dtype=np.uint32), np.full(n, 59, dtype=np.uint32), 100, 256, 500)
    gc = np.full(n, 100, dtype=np.uint32)
    gc[::3] = 50
    out["gc_equals_acgt"] = (cn.Case(["chr1"], [n * 100], 100, cn.noisy(rng, n, 3000, [(100, 160, 0.5)])), gc, (100 - gc).astype(np.uint32), 10, 16, 500)
    gc, at = comp(300, 100)
    out["min_bins_above_p"] = (cn.Case(["chr1"], [300 * 100], 100, wave(cn.noisy(rng, 300, 5000, [(50, 90, 3.0)]), gc, at)), gc, at, 100, 100000, 500)
    gc, at = comp(600, 100, 0.30, 0.34)
    flat = np.full(600, 2000, dtype=np.int64)
    flat[200:260] = 4000
    flat[::7] += 16
    out["ties"] = (cn.Case(["chr1"], [600 * 100], 100, flat), gc, at, 20, 32, 500)
    gc, at = comp(1500, 1000)
    b = wave(np.concatenate([cn.noisy(rng, 1000, 8000, [(300, 420, 0.5), (700, 720, 4.0)]), cn.noisy(rng, 500, 8000, [(100, 200, 1.5)])]), gc, at, 0.7)
    out["both_signs"] = (cn.Case(["chr1", "chr2"], [1000 * 1000, 500 * 1000], 1000, b), gc, at, 100, 64, 500)
    gc1, at1 = comp(800, 100, 0.35, 0.5)
    gcx, atx = comp(300, 100, 0.6, 0.9)                 # chrX is no centring contig, and its strata lie above the pool's
    gc, at = np.concatenate([gc1, gcx]), np.concatenate([at1, atx])
    out["strata_the_pool_lacks"] = (cn.Case(["chr1", "chrX"], [800 * 100, 300 * 100], 100,
                                            wave(np.concatenate([cn.noisy(rng, 800, 3000, [(100, 180, 2.0)]), cn.noisy(rng, 300, 1500, [(120, 160, 2.0)])]), gc, at)), gc, at, 100, 64, 500)
    gc, at = comp(500, 100)
    gc[40:60], at[40:60] = gc[40:60] // 4, at[40:60] // 4     # a quarter called
    gc[200:203], at[200:203] = 0, 0
    gc[300], at[300] = 25, 25                               # exactly half
    base = cn.Case(["chr1"], [500 * 100], 100, wave(cn.noisy(rng, 500, 3000, [(350, 420, 2.0)]), gc, at))
    out["min_called_0"] = (base, gc, at, 50, 32, 0)
    out["min_called_500"] = (base, gc, at, 50, 32, 500)
    out["min_called_1000"] = (base, gc, at, 50, 32, 1000)
    gc, at = comp(600, 100)
    one = cn.cases()["reference"]
    out["with_a_reference"] = (cn.Case(["chr1"], [600 * 100], 100, wave(one.bases, gc, at), ref=one.ref), gc, at, 100, 128, 500)
    return out


def segment_gc(case, gc, at, strata, min_bins, permille, gpu=None, entry="gc"):
    """coral_cn_segment_gc_host (or, with ``gpu`` = a torch device, coral_cn_segment_gc_gpu) on a case -> (rows, counts dict, bias,
    stratum_bins) as ``restate_gc`` gives them; gc = None: no composition.  ``entry`` = "old": the entry points without one."""
    L = _lib.lib()
    nc, n_bins = len(case.chroms), int(case.bin_off[-1])
    lengths, centre = np.array(case.lengths, dtype=np.int64), np.array(case.centre_flags(), dtype=np.uint8)
    bases = np.ascontiguousarray(case.bases, dtype=np.int64)
    ref = None if case.ref is None else np.ascontiguousarray(case.ref, dtype=np.int64)
    cap = max(n_bins, 1)
    rows = [np.zeros(cap, dtype=np.int32)] + [np.zeros(cap, dtype=np.int64) for _ in range(5)]
    counts = (C.c_int64 * 8)()
    bias, sbins = np.full(strata + 1, -7, dtype=np.int64), np.full(strata + 1, -7, dtype=np.int64)
    common = [nc, case.bin_off.ctypes.data, lengths.ctypes.data, case.bin_size, bases.ctypes.data, None if ref is None else ref.ctypes.data, centre.ctypes.data, case.levels,
              case.q, cap] + [a.ctypes.data for a in rows] + [counts]
    if gc is not None:
        gc, at = np.ascontiguousarray(gc, dtype=np.uint32), np.ascontiguousarray(at, dtype=np.uint32)
        extra = [gc.ctypes.data, at.ctypes.data, strata, min_bins, permille, bias.ctypes.data, sbins.ctypes.data]
    else:
        extra = [None, None, 0, 0, 0, None, None]
    if gpu is None:
        rc = L.coral_cn_segment_host(*common) if entry == "old" else L.coral_cn_segment_gc_host(*common, *extra)
    else:
        import torch
        ws_bytes = int(L.coral_cn_workspace_bytes(n_bins, nc, case.levels, int(ref is not None), cap) if entry == "old" else
                       L.coral_cn_workspace_gc_bytes(n_bins, nc, case.levels, int(ref is not None), cap, int(gc is not None), strata))
        assert ws_bytes > 0
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=gpu)
        stream = torch.cuda.current_stream(gpu)
        stream.synchronize()
        secs = (C.c_double * 7)()
        head = [torch.device(gpu).index or 0] + common + [ws.data_ptr(), ws_bytes, stream.cuda_stream, secs]
        rc = L.coral_cn_segment_gpu(*head) if entry == "old" else L.coral_cn_segment_gc_gpu(*head, *extra)
        stream.synchronize()
    assert rc == 0, (rc, L.coral_bam_last_error().decode())
    n = int(counts[0])
    out_rows = list(zip(*(a[:n].tolist() for a in rows)))
    names = ("kept", "centre", "ref_centre", "breakpoints", "uncalled")
    return out_rows, {k: int(counts[i + 1]) for i, k in enumerate(names)}, bias.tolist(), sbins.tolist()
