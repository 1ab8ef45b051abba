"""The case table of the SAM -> BAM import: whole SAM texts (header and record lines) that tests/test_sam_core.py gives to the
host build of the encoding core, beside its plain-Python restatement of the rules, and tests/test_sam_import_gpu.py to the device
- and the texts every rule refuses, with the line and the field the refusal must name.  Nothing here imports the product."""
import ctypes
import ctypes.util
import random
import struct
from fractions import Fraction

# the field a refusal names (coral_amd/csrc/coral_sam_core.h: Field)
F_FIELDS, F_EMPTY, F_HEADER_LINE, F_QNAME, F_FLAG, F_RNAME, F_POS, F_MAPQ, F_CIGAR, F_RNEXT, F_PNEXT, F_TLEN, F_SEQ, F_QUAL, F_TAG = range(1, 16)

HEADER = ("@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:248956422\n@SQ\tSN:chr10\tLN:133797422\n@SQ\tSN:chr1_alt\tLN:5000\n"
          "@PG\tID:mapper\tPN:mapper\tCL:mapper -ax map-ont ref.fa reads.fq\n")
N_HEADER_LINES = 5
ALPHABET = "=ACMGRSVTWYHKDBN"
OPS = "MIDNSHP=X"
INTS = [-2 ** 31, -32769, -32768, -129, -128, -1, 0, 255, 256, 65535, 65536, 2 ** 31 - 1, 2 ** 32 - 1]

_libc = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6")
_libc.strtof.restype = ctypes.c_float
_libc.strtof.argtypes = [ctypes.c_char_p, ctypes.c_void_p]


def strtof_bits(text: str) -> int:
    """The bits of libc's strtof (binary32, correctly rounded) - not of Python's float, which is a double."""
    return struct.unpack("<I", struct.pack("<f", _libc.strtof(text.encode(), None)))[0]


def line(qname="r", flag=0, rname="chr1", pos=1, mapq=60, cigar="*", rnext="*", pnext=0, tlen=0, seq="*", qual="*", tags=()):
    return "\t".join([qname, str(flag), rname, str(pos), str(mapq), cigar, rnext, str(pnext), str(tlen), seq, qual] + list(tags))


def quals(n, salt=0):
    return "".join(chr(33 + (7 * i + 13 * salt) % 94) for i in range(n))


def text_of(lines, header=HEADER, last_newline=True):
    return (header + "\n".join(lines) + ("\n" if last_newline and lines else "")).encode("latin-1")


def decimal(x: Fraction, digits: int, up: bool) -> str:
    """x > 0 to ``digits`` significant digits, rounded down or up, in plain or scientific notation as its size suggests."""
    e = 0
    while x >= 10 ** (e + 1):
        e += 1
    while x < Fraction(10) ** e:
        e -= 1
    scaled = x / Fraction(10) ** (e - digits + 1)
    w = scaled.numerator // scaled.denominator + (1 if up and scaled.denominator != 1 else 0)
    s = str(w)
    if -5 <= e < 16:
        if e - digits + 1 >= 0:
            return s + "0" * (e - digits + 1)
        if e < 0:
            return "0." + "0" * (-e - 1) + s
        return s[:e + 1] + "." + s[e + 1:]
    return s[0] + "." + s[1:] + "e%d" % e


def float_strings():
    """Decimals around the midpoints of neighbouring floats - where a conversion through a double rounds twice -, the midpoints
    themselves (ties), and values as mappers print them.  Deterministic."""
    rnd = random.Random(20240607)
    out = ["0", "-0", "0.0", "1", "-1", "0.5", "1e5", "1E-3", "+2.5e+3", ".5", "5.", "0.0123", "0.1034", "0.0000", "1e22", "1e23", "1e-22", "1e-23", "3.4028235e38",
           "1e-45", "1.4e-45", "7e-46", "1.17549435e-38", "123456789012345678901234567890", "0.000000000000000000000000000001", "16777217", "16777219",
           "9007199254740993", "9007199254740992", "1.00000005960464477539062500", "1.000000059604644775390625", "1.00000005960464477539062501",
           "1.0000000596046447", "1.0000000596046448", "33554434", "33554438", "8388608.5", "8388609.5", "0.30000001192092896", "4e-320", "1e39", "1e400"]
    out += ["%.4f" % (rnd.random() * 0.3) for _ in range(40)]          # de:f as minimap2 / winnowmap print it
    for _ in range(60):
        bits = rnd.randrange(0x00800000, 0x7f000000)
        f = Fraction(struct.unpack("<f", struct.pack("<I", bits))[0])
        g = Fraction(struct.unpack("<f", struct.pack("<I", bits + 1))[0])
        mid = (f + g) / 2
        for digits in (8, 9, 15, 16, 17, 19, 21):
            for up in (False, True):
                out.append(decimal(mid, digits, up))
    for k in range(20):                                                  # midpoints that are short decimals: exact ties and their neighbours
        v = 2 ** 24 + 2 * k + 1
        out += [str(v), "%d.000001" % v, "%d.999999" % (v - 1), "%de1" % v, "%d.0e-1" % v]
    return out


def cases():
    """name -> (text, keep): keep = (min_mapq, min_seq_length, require_flags, exclude_flags)."""
    c = {}
    no = (0, 0, 0, 0)
    tags = ["XA:A:!", "XB:A:~", "XZ:Z:", "XY:Z:a string with spaces, and commas", "XH:H:", "XI:H:1AE301ff", "Xf:f:3.25", "Xg:f:-1e-3", "XE:B:c", "X0:B:c,-128,127,0",
            "X1:B:C,0,255", "X2:B:s,-32768,32767", "X3:B:S,0,65535", "X4:B:i,-2147483648,2147483647", "X5:B:I,0,4294967295", "X6:B:f,1,0.5,-2.5e3,0.0123",
            "ML:B:C," + ",".join(str((37 * k) % 256) for k in range(300))] + ["i%d:i:%d" % (k, v) for k, v in enumerate(INTS[:10])] + ["j%d:i:%d" % (k, v) for k, v in enumerate(INTS[10:])]
    c["tags"] = (text_of([line("tagged", tags=tags), line("plus", tags=["NM:i:+7", "s1:i:-0"]), line("none"), line("z_long", tags=["MD:Z:" + "10A5^AC6" * 700, "NM:i:3"])]), no)
    lens = (0, 1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1031)
    seqs = []
    for n in lens:
        s = "".join(ALPHABET[(i * 5 + n) % 16] for i in range(n)) or "*"
        seqs.append(line("len%d" % n, seq=s, qual=quals(n, n) if n and n % 2 else "*", cigar="%dM" % n if n % 3 == 1 else "*"))
    seqs.append(line("codes", seq=ALPHABET, qual=quals(16)))
    seqs.append(line("lower", seq=ALPHABET.lower(), qual="*", cigar="8M8S"))
    seqs.append(line("outside", seq="AC.GT-XZ0123acgt\x7f", qual=quals(17, 3)))
    seqs.append(line("q_edge", seq="ACGT", qual="!~ \x7f"))
    c["seq"] = (text_of(seqs), no)
    cig = [line("star"), line("one", cigar="5M", seq="ACGTA"), line("nine", cigar="1M2I3D4N5S6H7P8=9X", seq="A" * (1 + 2 + 5 + 8 + 9)), line("zero", cigar="0M3M0I", seq="ACG"),
           line("max_len", cigar="268435455N1M", seq="A"),
           line("ops64", cigar="1M1D" * 32), line("ops65", cigar="1M1D" * 32 + "1M"), line("ops63_digits", cigar="".join("%d%s" % (10 ** (k % 7), OPS[k % 9]) for k in range(63))),
           line("ops65535", cigar="2M1I" * 32767 + "1M"), line("ops65536", cigar="1M1I" * 32768, seq="AC" * 32768, qual="*", tags=["NM:i:5", "XA:Z:behind"]),
           line("ops65537_noseq", cigar="1=2X" * 32768 + "1S"), line("after")]
    c["cigar"] = (text_of(cig), no)
    c["fields"] = (text_of([line("unmapped_ops", flag=4, cigar="10M", pos=100), line("unmapped", flag=4, rname="*", pos=0, mapq=0), line("pos0", pos=0, cigar="4M"),
                            line("eq", rname="chr10", rnext="=", pnext=77, tlen=-2 ** 31), line("rnext_star", rname="chr1_alt", rnext="*", tlen=2 ** 31 - 1),
                            line("rnext_name", rname="chr1", rnext="chr10", pnext=2 ** 31 - 1, pos=2 ** 31 - 1, flag=65535, mapq=255), line("star_eq", rname="*", rnext="="),
                            line("x" * 254), line("*"), line("bin", pos=2 ** 29 - 5, cigar="10M"), line("bin2", pos=16384, cigar="1M"), line("bin3", pos=16385, cigar="16384D"),
                            line("reflen0", cigar="5I", pos=10)]), no)
    many = "@HD\tVN:1.6\n" + "".join("@SQ\tSN:ctg%d\tLN:%d\n" % (k, 1000 + k) for k in range(3000))
    c["contigs3000"] = (text_of([line("a", rname="ctg0"), line("b", rname="ctg2999", rnext="ctg1"), line("c", rname="ctg1500", rnext="="), line("d", rname="ctg29", rnext="ctg299")],
                                header=many), no)
    c["no_last_newline"] = (text_of([line("a"), line("last", seq="ACGT", qual="IIII", tags=["NM:i:1"])], last_newline=False), no)
    c["no_last_newline_f"] = (text_of([line("last", tags=["de:f:0.30000001192092896"])], last_newline=False), no)
    c["header_only"] = (text_of([]), no)
    c["header_unterminated"] = (HEADER.rstrip("\n").encode(), no)
    c["no_header"] = (text_of([line("a", rname="*", pos=0), line("b", rname="*", pos=0, seq="AC", qual="II")], header=""), no)
    c["empty"] = (b"", no)
    c["short_and_long"] = (text_of([line("longer_than_text", tags=["XF:B:f" + ",1" * 50, "XE:B:i"]), line("shorter_than_text", seq="ACGT" * 50, qual="I" * 200, cigar="200M")]), no)
    fl = float_strings()
    c["floats"] = (text_of([line("f%d" % k, tags=["de:f:" + v]) for k, v in enumerate(fl)] + [line("fb", tags=["XF:B:f," + ",".join(fl)])]), no)
    filt = [line("q%d" % k, flag=(0, 4, 16, 256, 2048, 2064)[k % 6], mapq=(0, 24, 25, 60)[k % 4], seq="ACGTA"[:k % 6] or "*", tags=["NM:i:%d" % k]) for k in range(48)]
    c["filter_mapq"] = (text_of(filt), (25, 0, 0, 0))
    c["filter_len"] = (text_of(filt), (0, 3, 0, 0))
    c["filter_flags"] = (text_of(filt), (0, 0, 16, 0x900))
    c["filter_all"] = (text_of(filt), (61, 0, 0, 0))
    return c


def refusals():
    """[(name, text, the 1-based line the refusal names, its field)]"""
    good = line("good", seq="ACGT", qual="IIII", cigar="4M", tags=["NM:i:0"])
    r = []

    def one(name, bad, field, before=1):
        r.append((name, text_of([good] * before + [bad, good]), N_HEADER_LINES + before + 1, field))
    one("ten_fields", "\t".join(line("a").split("\t")[:10]), F_FIELDS)
    one("one_field", "a", F_FIELDS, before=0)
    one("empty_line", "", F_EMPTY, before=2)
    one("header_behind_record", "@CO\tlate", F_HEADER_LINE)
    one("qname_255", line("q" * 255), F_QNAME)
    one("qname_empty", line(""), F_QNAME)
    for name, kw, field in (("flag_text", dict(flag="0x10"), F_FLAG), ("flag_big", dict(flag=65536), F_FLAG), ("flag_neg", dict(flag=-1), F_FLAG), ("flag_empty", dict(flag=""), F_FLAG),
                            ("pos_digit", dict(pos="12a"), F_POS), ("pos_big", dict(pos=2 ** 31), F_POS), ("pos_neg", dict(pos=-1), F_POS), ("pos_huge", dict(pos="9" * 30), F_POS),
                            ("mapq_big", dict(mapq=256), F_MAPQ), ("mapq_text", dict(mapq="6 0"), F_MAPQ), ("pnext_digit", dict(pnext="1.0"), F_PNEXT),
                            ("pnext_big", dict(pnext=2 ** 31), F_PNEXT), ("tlen_big", dict(tlen=2 ** 31), F_TLEN), ("tlen_small", dict(tlen=-2 ** 31 - 1), F_TLEN),
                            ("tlen_sign", dict(tlen="-"), F_TLEN), ("rname_unknown", dict(rname="chr100"), F_RNAME), ("rname_prefix", dict(rname="chr"), F_RNAME),
                            ("rname_longer", dict(rname="chr1_"), F_RNAME), ("rname_empty", dict(rname=""), F_RNAME), ("rnext_unknown", dict(rnext="chrX"), F_RNEXT),
                            ("cigar_op", dict(cigar="4Q"), F_CIGAR), ("cigar_lower", dict(cigar="4m"), F_CIGAR), ("cigar_no_len", dict(cigar="M"), F_CIGAR),
                            ("cigar_no_len2", dict(cigar="3MM"), F_CIGAR), ("cigar_tail", dict(cigar="3M4"), F_CIGAR), ("cigar_len", dict(cigar="268435456M"), F_CIGAR),
                            ("cigar_empty", dict(cigar=""), F_CIGAR), ("cigar_no_len_64", dict(cigar="1M" * 32 + "M"), F_CIGAR), ("cigar_star2", dict(cigar="**"), F_CIGAR),
                            ("qual_len", dict(seq="ACGT", qual="III"), F_QUAL), ("qual_no_seq", dict(qual="III"), F_QUAL), ("qual_empty", dict(seq="ACGT", qual=""), F_QUAL),
                            ("seq_cigar", dict(seq="ACGT", qual="IIII", cigar="3M"), F_SEQ), ("seq_empty", dict(seq=""), F_SEQ)):
        one(name, line("bad", **kw), field)
    for name, tag in (("tag_key", "1A:i:1"), ("tag_key2", "A_:i:1"), ("tag_type", "XX:q:1"), ("tag_short", "XX:i"), ("tag_colon", "XX;i:1"), ("tag_empty", ""), ("tag_a2", "XX:A:ab"),
                      ("tag_a0", "XX:A:"), ("tag_h_odd", "XX:H:ABC"), ("tag_h_digit", "XX:H:AG"), ("tag_b_range", "XX:B:c,128"), ("tag_b_range2", "XX:B:C,-1"),
                      ("tag_b_range3", "XX:B:S,65536"), ("tag_b_range4", "XX:B:I,4294967296"), ("tag_b_sub", "XX:B:x,1"), ("tag_b_none", "XX:B:"), ("tag_b_empty", "XX:B:c,"),
                      ("tag_b_empty2", "XX:B:c,1,,2"), ("tag_b_nocomma", "XX:B:c1"), ("tag_b_float", "XX:B:f,1,x"), ("tag_i_big", "XX:i:4294967296"),
                      ("tag_i_small", "XX:i:-2147483649"), ("tag_i_text", "XX:i:1.5"), ("tag_i_empty", "XX:i:"), ("tag_f_inf", "XX:f:inf"), ("tag_f_nan", "XX:f:nan"),
                      ("tag_f_hex", "XX:f:0x1p3"), ("tag_f_empty", "XX:f:"), ("tag_f_e", "XX:f:1e"), ("tag_f_dot", "XX:f:."), ("tag_f_space", "XX:f: 1")):
        one(name, line("bad", tags=["NM:i:1", tag]), F_TAG)
    r.append(("two_bad_lines", text_of([good, line("b1", mapq=300), good, line("b2", flag="x")]), N_HEADER_LINES + 2, F_MAPQ))
    r.append(("bad_last_line_unterminated", text_of([good, line("b", tags=["XX:B:c,1,"])], last_newline=False), N_HEADER_LINES + 2, F_TAG))
    r.append(("bad_first_of_many", text_of([line("b", pos="x")] + [good] * 200), N_HEADER_LINES + 1, F_POS))
    r.append(("bad_last_of_many", text_of([good] * 200 + [line("b", pos="x")]), N_HEADER_LINES + 201, F_POS))
    return r
