"""The SAM -> BAM encoding core (coral_amd/csrc/coral_sam_core.h) compiled for the HOST (tests/native/sam_host.cpp: the same
logic, lanes as loops) against a plain-Python restatement of the rules - htslib's sam_parse1 + bam_write1 as the header states
them -, which lives in this module, uses struct only and takes its floats from libc's strtof.  The restatement itself is pinned by
a record assembled from literal bytes.  The product's host path (bam.import_sam with device "cpu") is checked on top: a round trip
through the project's own independent BAM writer, the record filter, the command line and a pipe.  The device build of the same
code is compared byte for byte with the host's in tests/test_sam_import_gpu.py."""
import ctypes as C
import gzip
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests import bamfile
from tests import sam_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "sam_host.cpp")


# ---- the rules, restated -------------------------------------------------------------------------------------------------------
class Refused(Exception):
    def __init__(self, line_no, field):
        Exception.__init__(self, "line %d field %d" % (line_no, field))
        self.line_no, self.field = line_no, field


_INT_RE = re.compile(rb"^[+-]?[0-9]+$")
_FLOAT_RE = re.compile(rb"^[+-]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?$")
_CIGAR_RE = re.compile(rb"([0-9]*)([^0-9])")
_SEQ_CODE = {ord(ch): k for k, ch in enumerate("=ACMGRSVTWYHKDBN")}
_SEQ_CODE.update({ord(ch.lower()): k for k, ch in enumerate("=ACMGRSVTWYHKDBN") if ch != "="})
_B_TYPES = {b"c": ("<b", -128, 127), b"C": ("<B", 0, 255), b"s": ("<h", -32768, 32767), b"S": ("<H", 0, 65535), b"i": ("<i", -2 ** 31, 2 ** 31 - 1),
            b"I": ("<I", 0, 2 ** 32 - 1)}


def _number(field, lo, hi):
    if not _INT_RE.match(field) or not lo <= int(field) <= hi:
        return None
    return int(field)


def _float_bits(field):
    return struct.pack("<I", sc.strtof_bits(field.decode("latin-1"))) if _FLOAT_RE.match(field) else None


def _reg2bin(beg, end):
    end -= 1
    for shift, off in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return off + (beg >> shift)
    return 0


def _tag(field):
    """One tag's bytes in the record, or None for a malformed one."""
    if len(field) < 5 or field[2:3] != b":" or field[4:5] != b":" or not re.match(rb"^[A-Za-z][A-Za-z0-9]$", field[:2]):
        return None
    key, ty, val = field[:2], field[3:4], field[5:]
    if ty == b"A":
        return key + b"A" + val if len(val) == 1 and 33 <= val[0] <= 126 else None
    if ty == b"i":
        v = _number(val, -2 ** 31, 2 ** 32 - 1)
        if v is None:
            return None
        if v < 0:
            code = ("c", "<b") if v >= -128 else ("s", "<h") if v >= -32768 else ("i", "<i")
        else:
            code = ("C", "<B") if v <= 255 else ("S", "<H") if v <= 65535 else ("I", "<I")
        return key + code[0].encode() + struct.pack(code[1], v)
    if ty == b"f":
        bits = _float_bits(val)
        return None if bits is None else key + b"f" + bits
    if ty == b"Z":
        return key + b"Z" + val + b"\0"
    if ty == b"H":
        return key + b"H" + val + b"\0" if len(val) % 2 == 0 and re.match(rb"^[0-9A-Fa-f]*$", val) else None
    if ty == b"B":
        sub = val[:1]
        if sub not in _B_TYPES and sub != b"f":
            return None
        rest = val[1:]
        if rest and rest[:1] != b",":
            return None
        items = rest.split(b",")[1:]
        out = []
        for it in items:
            if sub == b"f":
                b = _float_bits(it)
            else:
                fmt, lo, hi = _B_TYPES[sub]
                v = _number(it, lo, hi)
                b = None if v is None else struct.pack(fmt, v)
            if b is None:
                return None
            out.append(b)
        return key + b"B" + sub + struct.pack("<I", len(items)) + b"".join(out)
    return None


def restate_record(ln, line_no, refs):
    """One record line (bytes, no newline) -> (the record's bytes, flag, mapq, l_seq)."""
    if ln == b"":
        raise Refused(line_no, sc.F_EMPTY)
    if ln[:1] == b"@":
        raise Refused(line_no, sc.F_HEADER_LINE)
    f = ln.split(b"\t")
    if len(f) < 11:
        raise Refused(line_no, sc.F_FIELDS)
    qname, rname, cigar, rnext, seq, qual = f[0], f[2], f[5], f[6], f[9], f[10]

    def need(v, field):
        if v is None or v is False:
            raise Refused(line_no, field)
        return v
    need(1 <= len(qname) <= 254, sc.F_QNAME)
    flag = need(_number(f[1], 0, 65535), sc.F_FLAG)
    tid = -1 if rname == b"*" else need(refs.get(rname), sc.F_RNAME)
    pos = need(_number(f[3], 0, 2 ** 31 - 1), sc.F_POS) - 1
    mapq = need(_number(f[4], 0, 255), sc.F_MAPQ)
    ops = []
    if cigar != b"*":
        need(len(cigar) > 0, sc.F_CIGAR)
        at = 0
        for m in _CIGAR_RE.finditer(cigar):
            need(m.start() == at and m.group(1) != b"" and m.group(2) in b"MIDNSHP=X" and int(m.group(1)) < 2 ** 28, sc.F_CIGAR)
            ops.append((b"MIDNSHP=X".index(m.group(2)), int(m.group(1))))
            at = m.end()
        need(at == len(cigar), sc.F_CIGAR)
    next_tid = tid if rnext == b"=" else -1 if rnext == b"*" else need(refs.get(rnext), sc.F_RNEXT)
    pnext = need(_number(f[7], 0, 2 ** 31 - 1), sc.F_PNEXT) - 1
    tlen = need(_number(f[8], -2 ** 31, 2 ** 31 - 1), sc.F_TLEN)
    ref_len = sum(n for op, n in ops if op in (0, 2, 3, 7, 8))
    query_len = sum(n for op, n in ops if op in (0, 1, 4, 7, 8))
    l_seq = 0 if seq == b"*" else len(seq)
    need(len(seq) > 0 and (seq == b"*" or not ops or query_len == l_seq), sc.F_SEQ)
    need(len(qual) > 0 and (qual == b"*" or (seq != b"*" and len(qual) == l_seq)), sc.F_QUAL)
    tags = b"".join(need(_tag(t), sc.F_TAG) for t in f[11:])
    words = [(n << 4) | op for op, n in ops]
    if len(ops) > 65535:
        need(l_seq < 2 ** 28 and ref_len < 2 ** 28, sc.F_CIGAR)
        tags += b"CGBI" + struct.pack("<I", len(words)) + struct.pack("<%dI" % len(words), *words)
        words = [(l_seq << 4) | 4, (ref_len << 4) | 3]
    end = pos + (ref_len if not flag & 4 and ops and ref_len > 0 else 1)
    codes = [_SEQ_CODE.get(b, 15) for b in (seq if seq != b"*" else b"")] + [0]
    packed = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, l_seq, 2))
    q = b"\xff" * l_seq if qual == b"*" else bytes((b - 33) & 255 for b in qual)
    body = (struct.pack("<iiBBHHHiiii", tid, pos, len(qname) + 1, mapq, _reg2bin(pos, end) & 0xffff, len(words), flag, l_seq, next_tid, pnext, tlen) + qname + b"\0" +
            struct.pack("<%dI" % len(words), *words) + packed + q + tags)
    return struct.pack("<i", len(body)) + body, flag, mapq, l_seq


def restate(text, keep=(0, 0, 0, 0)):
    """A whole SAM text -> (the inflated BAM stream, lines, records written, records dropped)."""
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    n_head = 0
    while n_head < len(lines) and lines[n_head][:1] == b"@":
        n_head += 1
    head_text = text[:sum(len(ln) + 1 for ln in lines[:n_head])] if n_head < len(lines) or text.endswith(b"\n") else text
    names, lens = [], []
    for ln in lines[:n_head]:
        if ln.startswith(b"@SQ\t"):
            kv = dict((x[:2], x[3:]) for x in ln.split(b"\t")[1:] if x[2:3] == b":")
            names.append(kv[b"SN"])
            lens.append(int(kv[b"LN"]))
    refs = {nm: k for k, nm in enumerate(names)}
    out = [b"BAM\x01" + struct.pack("<i", len(head_text)) + head_text + struct.pack("<i", len(names))]
    for nm, ln in zip(names, lens):
        out.append(struct.pack("<i", len(nm) + 1) + nm + b"\0" + struct.pack("<i", ln))
    written = dropped = 0
    for k, ln in enumerate(lines[n_head:]):
        rec, flag, mapq, l_seq = restate_record(ln, n_head + k + 1, refs)
        if mapq >= keep[0] and l_seq >= keep[1] and flag & keep[2] == keep[2] and flag & keep[3] == 0:
            out.append(rec)
            written += 1
        else:
            dropped += 1
    return b"".join(out), len(lines) - n_head, written, dropped


# ---- the host build of the core ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("sam_host")), "libsam_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC], check=True)
    L = C.CDLL(so)
    L.coral_test_sam.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.coral_test_sam_float.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]

    def run(text, keep=(0, 0, 0, 0)):
        out = np.zeros(3 * len(text) + 36 * (text.count(b"\n") + 1) + 64, dtype=np.uint8)
        res = (C.c_int64 * 8)()
        k = np.array(keep, dtype=np.int32)
        L.coral_test_sam(text, len(text), k.ctypes.data, out.ctypes.data, len(out), res)
        res = [int(v) for v in res]
        return res, out[:res[1] + res[2]].tobytes() if res[0] == 0 else b""
    run.L = L
    return run


@pytest.fixture(scope="module")
def table():
    return sc.cases()


def test_the_restatement_on_a_record_of_literal_bytes():
    """The SAM line beside the record's bytes, written out by hand: this pins the restatement, as tests/test_bamfile.py pins the reader."""
    sam = b"r1\t83\tchr10\t16385\t60\t2S3M1D1M\t=\t101\t-7\tACGTNa\t!+5?I~\tNM:i:300\tXS:A:+\tde:f:0.5\tXZ:Z:hi\tXB:B:s,-2,3"
    rec = bytes.fromhex(
        "5e000000"                      # block_size = 94
        "01000000" "00400000"           # refID 1 (chr10), pos 16384
        "03" "3c" "4a12"                # l_read_name 3, mapq 60, bin 4682 = 4681 + (16384 >> 14)
        "0400" "5300" "06000000"        # 4 ops, flag 83, l_seq 6
        "01000000" "64000000" "f9ffffff"    # next_refID 1, next_pos 100, tlen -7
        "723100"                        # r1 NUL
        "24000000" "30000000" "12000000" "10000000"     # 2S 3M 1D 1M
        "1248f1"                        # A C | G T | N a
        "000a141e285d"                  # ! + 5 ? I ~  minus 33
        "4e4d53" "2c01"                 # NM S 300
        "585341" "2b"                   # XS A +
        "646566" "0000003f"             # de f 0.5
        "585a5a" "686900"               # XZ Z hi NUL
        "584242" "73" "02000000" "feff" "0300")         # XB B s 2: -2, 3
    got, flag, mapq, l_seq = restate_record(sam, 1, {b"chr1": 0, b"chr10": 1})
    assert got == rec and (flag, mapq, l_seq) == (83, 60, 6)
    header = restate(b"@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chr10\tLN:70000\n" + sam)[0][:-len(rec)]
    assert header == (b"BAM\x01" + struct.pack("<i", 53) + b"@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chr10\tLN:70000\n" + struct.pack("<i", 2) +
                      struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 1000) + struct.pack("<i", 6) + b"chr10\0" + struct.pack("<i", 70000))
    p = bamfile.parse(header + rec).recs[0]          # and the suite's reader reads it back
    assert (p["name"], p["tid"], p["pos"], p["flag"], bamfile.pairs(p["ops"])) == ("r1", 1, 16384, 83, [(4, 2), (0, 3), (2, 1), (0, 1)])


def test_host_core_equals_the_restatement_on_the_case_table(host, table):
    for name, (text, keep) in table.items():
        want, lines, written, dropped = restate(text, keep)
        res, got = host(text, keep)
        assert res[0] == 0, (name, res)
        assert (res[3], res[4], res[5]) == (lines, written, dropped), name
        assert got == want, (name, next(i for i in range(min(len(got), len(want)) + 1) if got[i:i + 1] != want[i:i + 1]))
    big = bamfile.parse(host(*table["cigar"])[1])
    assert [r["n_cig"] for r in big.recs if r["name"].startswith("ops655")] == [65535, 2, 2]
    assert [len(r["ops"]) for r in big.recs if r["name"].startswith("ops655")] == [65535, 65536, 65537]
    sizes = {r["name"]: r["size"] for r in bamfile.parse(host(*table["short_and_long"])[1]).recs}
    lens = {ln.split(b"\t")[0].decode(): len(ln) + 1 for ln in table["short_and_long"][0].split(b"\n")[sc.N_HEADER_LINES:-1]}
    assert sizes["longer_than_text"] > lens["longer_than_text"] and sizes["shorter_than_text"] < lens["shorter_than_text"]
    for name in ("filter_mapq", "filter_len", "filter_flags", "filter_all"):
        assert 0 < host(*table[name])[0][5] <= 48 and (name != "filter_all" or host(*table[name])[0][4] == 0)


def test_floats_are_strtof_bit_for_bit(host):
    """Every value, around float midpoints above all: the exact fast path of the core (what the device computes itself) and the
    values it leaves to strtof."""
    fast = slow = 0
    for s in sc.float_strings():
        for text in (s, "-" + s.lstrip("+-")):
            bits = C.c_uint32(0)
            how = host.L.coral_test_sam_float(text.encode(), len(text), bits)
            assert how in (1, 2), text
            assert bits.value == sc.strtof_bits(text), (text, how, hex(bits.value), hex(sc.strtof_bits(text)))
            fast, slow = fast + (how == 1), slow + (how == 2)
    assert fast > 200 and slow > 200
    # a double at a float midpoint with the decimal beside it: rounding the double would go to the even float, the wrong one
    for text, want in (("16777217.000001", 0x4b800001), ("16777216.999999", 0x4b800000), ("16777217", 0x4b800000), ("16777219", 0x4b800002)):
        bits = C.c_uint32(0)
        assert host.L.coral_test_sam_float(text.encode(), len(text), bits) == 1 and bits.value == want == sc.strtof_bits(text), text


def test_every_refusal_names_its_line_and_field(host):
    for name, text, line_no, field in sc.refusals():
        with pytest.raises(Refused) as e:
            restate(text)
        assert (e.value.line_no, e.value.field) == (line_no, field), name
        res, _ = host(text)
        assert (res[0], res[6], res[7]) == (1, line_no, field), (name, res)


def test_sanitizer_run_of_the_stand_alone_program(tmp_path, host, table):
    """The case table and the refusals through the stand-alone program (its own main) under AddressSanitizer and UBSan, on the
    CPU: every text is an allocation of exactly its size.  Its answers are the library's."""
    exe, cases_bin, results_bin = str(tmp_path / "sam_host"), str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DSAM_HOST_MAIN", SRC, "-o", exe], check=True)
    todo = [(text, keep) for text, keep in table.values()] + [(text, (0, 0, 0, 0)) for _n, text, _l, _f in sc.refusals()]
    with open(cases_bin, "wb") as fp:
        for text, keep in todo:
            fp.write(struct.pack("<I", len(text)) + text + struct.pack("<4i", *keep))
    run = subprocess.run([exe, cases_bin, results_bin], capture_output=True, text=True)
    assert run.returncode == 0 and "sam_host: %d cases" % len(todo) in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    with open(results_bin, "rb") as fp:
        raw = fp.read()
    at = 0
    for text, keep in todo:
        res = list(struct.unpack_from("<8q", raw, at))
        n = res[1] + res[2] if res[0] == 0 else 0
        want_res, want = host(text, keep)
        assert res == want_res and raw[at + 64:at + 64 + n] == want
        at += 64 + n
    assert at == len(raw)


# ---- the product's host path ---------------------------------------------------------------------------------------------------
def sam_text_of(path):
    """The file ``path`` as SAM text, rendered from tests/bamfile.parse plus the three fields it does not return."""
    with gzip.open(path, "rb") as fp:
        raw = fp.read()
    b = bamfile.parse(raw)
    l_text = struct.unpack_from("<i", raw, 4)[0]
    lines = []
    for r in b.recs:
        next_tid, next_pos, tlen = struct.unpack_from("<iii", raw, r["start"] + 24)
        cg = r["n_cig"] == 2 and len(r["ops"]) > 2
        cigar = "".join("%d%s" % (n, "MIDNSHP=X"[op]) for op, n in bamfile.pairs(r["ops"])) or "*"
        seq = "".join("=ACMGRSVTWYHKDBN"[c] for c in r["codes"]) or "*"
        qual = "*" if r["l_seq"] == 0 or r["qual"][0] == 0xff else "".join(chr(int(q) + 33) for q in r["qual"])
        tags = []
        for key, ty, val in r["tags"]:
            if key == "CG" and cg:
                continue
            if ty == "B":
                sub = {"int8": "c", "uint8": "C", "int16": "s", "uint16": "S", "int32": "i", "uint32": "I", "float32": "f"}[val.dtype.name]
                tags.append("%s:B:%s%s" % (key, sub, "".join("," + (repr(float(v)) if sub == "f" else str(int(v))) for v in val)))
            elif ty == "f":
                tags.append("%s:f:%s" % (key, repr(float(np.float32(val)))))         # (a double's shortest text reads back as the same float)
            else:
                tags.append("%s:%s:%s" % (key, "i" if ty in "cCsSiI" else ty, val))
        rnext = "*" if next_tid < 0 else "=" if next_tid == r["tid"] else b.refs[next_tid]
        lines.append("\t".join([r["name"], str(r["flag"]), b.refs[r["tid"]] if r["tid"] >= 0 else "*", str(r["pos"] + 1), str(r["mapq"]), cigar, rnext, str(next_pos + 1),
                                str(tlen), seq, qual] + tags))
    return raw[8:8 + l_text] + ("\n".join(lines) + "\n").encode("latin-1"), raw


def roundtrip_records():
    """Alignments for the project's own writer, in coordinate order: every CIGAR op, 66 001 ops (the CG shape), flags, a record
    without SEQ, NM values of every width."""
    from coral_amd import synth
    M, I, D, N, S, H, P, EQ, X = range(9)
    big = [(M, 3), (I, 1), (D, 2)] * 22000 + [(M, 5)]
    alns = [dict(tid=0, pos=0, cigar=[(M, 30)], name="first", nm=0),
            dict(tid=2, pos=1000, cigar=[(S, 7), (M, 150), (D, 40), (M, 100)], name="c3b", nm=255, mapq=0),
            dict(tid=7, pos=150_010, cigar=[(H, 9), (EQ, 10), (X, 2), (N, 90), (P, 1), (M, 30), (I, 2), (H, 7)], name="b", flag=0x10, nm=256),
            dict(tid=7, pos=150_020, cigar=[(M, 60)], flag=4, name="unmapped", nm=65535),
            dict(tid=7, pos=150_030, cigar=[(M, 200)], has_seq=0, name="noseq", nm=65536),
            dict(tid=7, pos=150_040, cigar=[(M, 121)], flag=0x900, name="odd_len", nonacgt=[150_041], nm=2 ** 31 - 1, mapq=255),
            dict(tid=7, pos=150_070, cigar=big, name="longcigar", nm=7),
            dict(tid=7, pos=150_080, cigar=bamfile.many_ops(129), name="ops129", nm=1,
                 sa=[(3, 500, 0, 7, 40, 0, 0, 60, 1)]),
            dict(tid=24, pos=16000, cigar=[(M, 500)], name="mito", nm=3)]
    return synth.records_from_alignments(alns)


def test_round_trip_through_the_projects_own_writer(tmp_path):
    """write_bam (real QUAL on two records of three; aux tags of every type; NM in the smallest type; a CIGAR above 65 535 ops as
    CG:B,I behind the last tag) -> SAM text -> import on the host: the inflated stream comes back byte for byte."""
    from coral_amd import bam
    rec = roundtrip_records()
    nm = rec.nm.cpu().numpy()
    front = (b"XAA!" + b"Xcc\x80" + b"XCC\xff" + b"Xss\x00\x80" + b"XSS\xff\xff" + b"Xii\x00\x00\x00\x80" + b"XII\xff\xff\xff\xff" + b"Xff" + struct.pack("<f", 0.1) +
             b"XZZtext here\0" + b"XHH1AE3\0" + b"XBBc\x02\x00\x00\x00\x80\x7f" + b"XGBf\x02\x00\x00\x00" + struct.pack("<ff", 1.5, -0.0123) + b"XEBS\x00\x00\x00\x00")
    src, out, sam = str(tmp_path / "src.bam"), str(tmp_path / "imported.bam"), str(tmp_path / "src.sam")
    bam.write_bam(rec, src, with_qual=lambda i: i % 3 != 0, aux=lambda i: (front if i % 2 == 0 else b"", b""),
                  nm_type=lambda i: "C" if nm[i] <= 255 else "S" if nm[i] <= 65535 else "I")
    text, raw = sam_text_of(src)
    parsed = bamfile.parse(raw)
    assert b"CG:B" not in text and max(len(r["ops"]) for r in parsed.recs) == 66001 and [r["n_cig"] for r in parsed.recs if r["name"] == "longcigar"] == [2]
    with open(sam, "wb") as fp:
        fp.write(text)
    st = bam.import_sam(sam, out, device="cpu")
    with gzip.open(out, "rb") as fp:
        got = fp.read()
    assert got == raw
    assert (st.lines, st.records, st.dropped, st.text_bytes) == (rec.n, rec.n, 0, len(text) - struct.unpack_from("<i", raw, 4)[0])
    assert got == restate(text)[0]
    assert bamfile.read_bam_bgzf(out).recs[-1]["name"] == "mito"


def test_the_filter_equals_the_import_of_the_kept_lines(tmp_path, table):
    from coral_amd import bam
    text = table["filter_mapq"][0]
    lines = text.split(b"\n")[:-1]
    for k, rf in enumerate((bam.RecordFilter(min_mapq=25), bam.RecordFilter(min_seq_length=3), bam.RecordFilter(require_flags=16, exclude_flags=0x900),
                            bam.RecordFilter(min_mapq=24, min_seq_length=2, exclude_flags=4))):
        kept = [ln for ln in lines[sc.N_HEADER_LINES:] if (lambda f: int(f[4]) >= rf.min_mapq and (0 if f[9] == b"*" else len(f[9])) >= rf.min_seq_length and
                                                           int(f[1]) & rf.require_flags == rf.require_flags and int(f[1]) & rf.exclude_flags == 0)(ln.split(b"\t"))]
        assert 0 < len(kept) < 48
        a, b, c = (str(tmp_path / ("%s%d" % (x, k))) for x in ("all.sam", "kept.sam", "out"))
        with open(a, "wb") as fp:
            fp.write(text)
        with open(b, "wb") as fp:
            fp.write(b"\n".join(lines[:sc.N_HEADER_LINES] + kept) + b"\n")
        st = bam.import_sam(a, c + "_a.bam", record_filter=rf, device="cpu")
        bam.import_sam(b, c + "_b.bam", device="cpu")
        assert (st.records, st.dropped) == (len(kept), 48 - len(kept))
        with open(c + "_a.bam", "rb") as fa, open(c + "_b.bam", "rb") as fb:
            assert fa.read() == fb.read()


def test_a_refusal_removes_the_output_and_names_the_line(tmp_path):
    from coral_amd import _lib, bam
    name, text, line_no, field = next(r for r in sc.refusals() if r[0] == "two_bad_lines")
    sam, out = str(tmp_path / "bad.sam"), str(tmp_path / "bad.bam")
    with open(sam, "wb") as fp:
        fp.write(text)
    with pytest.raises(_lib.CoralHipError, match="SAM line %d: MAPQ" % line_no) as e:
        bam.import_sam(sam, out, device="cpu")
    assert e.value.code == -4 and not os.path.exists(out)


def test_sam_header_bytes_is_the_restated_header(table):
    from coral_amd import bam
    for name in ("tags", "contigs3000", "no_header", "header_only", "header_unterminated"):
        text = table[name][0]
        want = restate(text)[0]
        got = bam.sam_header_bytes(text)
        assert want[:len(got)] == got and (name not in ("header_only", "header_unterminated") or got == want), name


def test_the_command_line_parses_and_reads_a_pipe(tmp_path, table):
    from coral_amd import CoRAL
    args = CoRAL.build_parser().parse_args(["import", "--sam", "-", "--output", "x.bam", "--filter_min_mapq", "25", "--device", "cpu", "--level", "6", "--gpu_compress"])
    assert (args.mode, args.sam, args.output, args.filter_min_mapq, args.device, args.level, args.gpu_compress) == ("import", "-", "x.bam", 25, "cpu", 6, True)
    text = table["tags"][0] + table["seq"][0].split(b"\n", sc.N_HEADER_LINES)[sc.N_HEADER_LINES]
    out = str(tmp_path / "piped.bam")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "coral_amd.CoRAL", "import", "--sam", "-", "--output", out, "--device", "cpu"], input=text, capture_output=True, env=env, cwd=ROOT)
    assert run.returncode == 0 and b"Wrote" in run.stdout, (run.stdout[-2000:], run.stderr[-4000:])
    with gzip.open(out, "rb") as fp:
        assert fp.read() == restate(text)[0]
