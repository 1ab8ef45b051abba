"""The FASTQ rule of coral_amd/csrc/coral_fastq_core.h restated in plain Python, the shared small cases, and a driver of the C ABI's
session (coral_fastq_*) that tests/test_fastq_core.py (host backend) and tests/test_fastq_gpu.py (device) both use.  The
restatement walks the text line by line and shares nothing with the native byte-wise state machine."""
import ctypes as C
import functools
import tempfile

import numpy as np

from coral_amd import _lib, fastq  # noqa: F401  (the module under test: everything here drives its session)

NO_THRESHOLDS = (0, 0, 0)            # min_length, max_length, min_mean_q100
FORMAT = -4                          # CORAL_ERR_FORMAT


class Refused(Exception):
    def __init__(self, offset):
        super().__init__("refused at byte %d" % offset)
        self.offset = offset


def lines_of(data: bytes):
    """[(first byte, the byte behind the last one that is no '\\n', ends with '\\n')]: a line starts at the first byte and behind
    every '\\n'."""
    out, start = [], 0
    for i in range(len(data)):
        if data[i] == 10:
            out.append((start, i, True))
            start = i + 1
    if start < len(data):
        out.append((start, len(data), False))
    return out


def keeps(thresholds, length, qual_sum):
    min_length, max_length, q100 = thresholds
    return length >= min_length and (max_length == 0 or length <= max_length) and 100 * qual_sum >= q100 * length


def restate_records(data: bytes):
    """[(length, [quality values], first byte, byte behind the last)] of every record; ``Refused`` where the rule refuses the text."""
    lines = lines_of(data)
    recs, length, begin = [], 0, 0
    for k, (a, b, newline) in enumerate(lines):
        phase = k % 4
        if phase == 0:
            if data[a] != 64:                              # '@' (of an empty line data[a] is its '\n')
                raise Refused(a)
            begin = a
        elif phase == 1:
            length = sum(1 for i in range(a, b) if data[i] != 13)
        elif phase == 2:
            if data[a] != 43:                              # '+'
                raise Refused(a)
        else:
            quals = []
            for i in range(a, b):
                if data[i] == 13:
                    continue
                if not 33 <= data[i] <= 126:
                    raise Refused(i)
                quals.append(data[i] - 33)
            if len(quals) != length:
                raise Refused(b)                           # the byte that closes the record: its '\n', or the end of the stream
            recs.append((length, quals, begin, b + 1 if newline else b))
    if lines and not lines[-1][2]:
        if (len(lines) - 1) % 4 != 3:
            raise Refused(len(data))                       # the stream ends inside lines 0-2
    elif len(lines) % 4 == 3:                              # right behind the '\n' of a separator line: an empty quality line
        if length != 0:
            raise Refused(len(data))
        recs.append((0, [], begin, len(data)))
    elif len(lines) % 4 != 0:
        raise Refused(len(data))
    return recs


@functools.lru_cache(maxsize=None)
def expected(data: bytes, thresholds=NO_THRESHOLDS):
    """``run_session``'s dict as the restatement gives it."""
    try:
        recs = restate_records(data)
    except Refused as e:
        return dict(rc=FORMAT, offset=e.offset)
    hist = [0] * 256
    listed, out, n_kept, kept_bases = [], bytearray(), 0, 0
    for length, quals, a, b in recs:
        for q in quals:
            hist[q] += 1
        k = keeps(thresholds, length, sum(quals))
        if k:
            out += data[a:b]
            n_kept += 1
            kept_bases += length
        if length:
            listed.append((length, sum(quals), int(k)))
    return dict(rc=0, offset=-1, records=len(recs), reads=len(listed), no_seq=len(recs) - len(listed), bases=sum(r[0] for r in listed), n_kept=n_kept,
                kept_bases=kept_bases, length=[r[0] for r in listed], qual_sum=[r[1] for r in listed], kept=[r[2] for r in listed], hist=hist, output=bytes(out))


def quality_lists(data: bytes):
    """(lengths, quality lists) of the listed reads: what the reference's script collects (its lines 38-48)."""
    recs = [r for r in restate_records(data) if r[0]]
    return [r[0] for r in recs], [r[1] for r in recs]


def record(name: bytes, seq: bytes, qual: bytes, end: bytes = b"\n", plus: bytes = b"+") -> bytes:
    return b"@" + name + end + seq + end + plus + end + qual + end


def random_record(rng, name: bytes, n: int, end: bytes = b"\n", lo: int = 33, hi: int = 126) -> bytes:
    seq = bytes(np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.randint(0, 5, n)])
    return record(name, seq, bytes(rng.randint(lo, hi + 1, n).astype(np.uint8)), end)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> FASTQ bytes: the legal inputs the issue of the feature lists."""
    rng = np.random.RandomState(31)
    out = {}
    out["unix"] = b"".join(random_record(rng, b"r%d" % k, n) for k, n in enumerate((5, 17, 1, 64, 33)))
    out["crlf"] = b"".join(random_record(rng, b"r%d" % k, n, b"\r\n") for k, n in enumerate((5, 17, 1, 64, 33)))
    out["no_trailing_newline"] = (random_record(rng, b"a", 12) + random_record(rng, b"b", 7))[:-1]
    out["no_trailing_newline_crlf"] = (random_record(rng, b"a", 12, b"\r\n") + random_record(rng, b"b", 7, b"\r\n"))[:-2]
    out["empty_sequence_in_the_middle"] = random_record(rng, b"a", 9) + b"@r\n\n+\n\n" + random_record(rng, b"b", 4)
    out["empty_sequence_at_the_end"] = random_record(rng, b"a", 9) + b"@r\n\n+\n"
    out["empty_sequence_at_the_end_with_quality_line"] = random_record(rng, b"a", 9) + b"@r\n\n+\n\n"
    out["quality_extremes"] = record(b"lo", b"ACGT", b"!!!!") + record(b"hi", b"ACGTA", b"~~~~~") + record(b"mix", b"ACG", b"!~I")
    out["plus_repeats_the_name"] = record(b"read1 x", b"ACGTT", b"IIIII", plus=b"+read1 x") + record(b"read2", b"AC", b"#I", plus=b"+read2")
    out["quality_starts_with_at_and_plus"] = record(b"a", b"ACGT", b"@III") + record(b"b", b"ACGT", b"+@@+") + record(b"c", b"A", b"@") + record(b"d", b"C", b"+")
    out["names_with_blanks"] = record(b"read 1 runid=abc ch=5\tstart=1", b"ACGTACGT", b"IIIIHHHH") + record(b" ", b"T", b"5")
    out["one_long_read"] = random_record(rng, b"short", 3) + random_record(rng, b"long", 300_000) + random_record(rng, b"tail", 2)
    out["many_short_reads"] = b"".join(random_record(rng, b"s%d" % k, (k * 5 + k // 7) % 7) for k in range(5000))
    out["empty_stream"] = b""
    return out


def refused():
    """name -> (text, the stream offset of the first offending byte)."""
    a = record(b"a", b"AC", b"II")                     # 11 bytes
    return {
        "blank_line_between_records": (a + b"\n" + record(b"b", b"G", b"I"), 11),
        "blank_line_behind_the_last_record": (a + b"\n", 11),
        "fasta_record": (a + b">b\nACGT\n", 11),
        "wrapped_sequence": (b"@a\nAC\nGT\n+\nIIII\n", 6),
        "quality_one_short": (b"@a\nACG\n+\nII\n" + record(b"b", b"A", b"I"), 11),
        "quality_one_long": (b"@a\nACG\n+\nIIII\n" + record(b"b", b"A", b"I"), 13),
        "quality_one_short_at_the_end": (b"@a\nACG\n+\nII", 11),
        "quality_character_32": (b"@a\nACG\n+\nI I\n", 10),
        "quality_character_127": (b"@a\nACG\n+\nI\x7fI\n", 10),
        "ends_after_one_line": (a + b"@b\n", 14),
        "ends_inside_the_first_line": (a + b"@b", 13),
        "ends_after_two_lines": (a + b"@b\nA\n", 16),
        "ends_after_three_lines": (a + b"@b\nA\n+\n", 18),
        "ends_inside_the_third_line": (a + b"@b\n\n+", 16),
    }


def cut(data: bytes, how, seed: int = 0):
    """The pieces of a feeding: "whole", "bytes" (1 byte each) or "random" (seeded)."""
    if how == "whole":
        return [data]
    if how == "bytes":
        return [data[i:i + 1] for i in range(len(data))]
    rng = np.random.RandomState(seed)
    out, at = [], 0
    while at < len(data):
        n = int(rng.choice([1, 2, 3, 5, 16, 17, 100, 4097, 70_000]))
        out.append(data[at:at + n])
        at += n
    return out


def run_session(pieces, thresholds=NO_THRESHOLDS, device=-1, staging=0, stream_setup=None, output=True):
    """The C ABI's session over the given pieces -> dict(rc of the first failing call or 0, offset, and for a legal text the
    counters, length, qual_sum, kept, hist [256] and the output's bytes).  Host histogram for device < 0; for a device session
    ``stream_setup(staging)`` returns (histogram tensor, workspace tensor, workspace bytes, stream handle, download function)."""
    L = _lib.lib()
    h = C.c_void_p()
    stats = (C.c_int64 * 8)()
    with tempfile.TemporaryFile() as fp:
        fd = fp.fileno() if output else -1
        if device < 0:
            hist = np.zeros(256, dtype=np.uint64)
            rc = L.coral_fastq_open(-1, thresholds[0], thresholds[1], thresholds[2], fd, 0, hist.ctypes.data, None, 0, None, C.byref(h))
            download = lambda: hist
        else:
            dev_hist, ws, ws_bytes, stream, download = stream_setup(staging)
            rc = L.coral_fastq_open(device, thresholds[0], thresholds[1], thresholds[2], fd, staging, dev_hist.data_ptr(), ws.data_ptr(), ws_bytes, stream, C.byref(h))
        assert rc == 0, (rc, L.coral_bam_last_error().decode())
        try:
            rc = 0
            for p in pieces:
                rc = L.coral_fastq_feed(h, p, len(p))
                if rc != 0:
                    break
            rc_finish = L.coral_fastq_finish(h, stats, None)
            st = list(stats)
            if rc != 0 or rc_finish != 0:
                assert rc_finish != 0
                return dict(rc=rc or rc_finish, offset=st[6])
            length, qual_sum, kept = np.zeros(st[1], dtype=np.int32), np.zeros(st[1], dtype=np.int64), np.zeros(st[1], dtype=np.uint8)
            assert L.coral_fastq_rows(h, st[1], length.ctypes.data, qual_sum.ctypes.data, kept.ctypes.data) == 0
            fp.seek(0)
            return dict(rc=0, offset=st[6], records=st[0], reads=st[1], no_seq=st[2], bases=st[3], n_kept=st[4], kept_bases=st[5], length=length.tolist(),
                        qual_sum=qual_sum.tolist(), kept=kept.tolist(), hist=[int(v) for v in download()[:256]], output=fp.read() if output else b"")
        finally:
            L.coral_fastq_close(h)


def assert_same(got, want, what=""):
    assert (got["rc"], got["offset"]) == (want["rc"], want["offset"]), (what, got["rc"], got["offset"], want["rc"], want["offset"])
    if want["rc"] != 0:
        return
    for k in ("records", "reads", "no_seq", "bases", "n_kept", "kept_bases"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("length", "qual_sum", "kept", "hist"):
        assert got[k] == want[k], (what, k, [i for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b][:10], len(got[k]), len(want[k]))
    assert got["output"] == want["output"], (what, "output", len(got["output"]), len(want["output"]))
