"""Chimeric-alignment tables written as real SA text (``rname,pos,strand,CIGAR,mapQ,NM;`` as a BAM holds it), and what the
reference makes of them - the inputs and expectations of tests/test_sa_table_reference.py.

A case is a list of records (``rec``) in file order.  ``load`` writes them as a BAM file with the SA strings verbatim and reads
the file back with the product's host decoder, so the tokens the kernels get are the product's tokeniser's own; the expectation
is the oracle's ``fetch()`` over the decoded records with the ORIGINAL strings in ``sa_str`` (oracle/hostrecords.py rebuilds the
strings from the tokens and cannot express an unknown CIGAR shape), turned into arrays by tests/product_check.oracle_sa_table.
Everything here is plain Python and runs without a GPU.  The asserts inside the builders show that a case is what its name says.
"""
import json
import os

import numpy as np

from coral_amd import bam, synth
from oracle import coral_oracle as O
from tests.bamfile import M
from tests.canon import uncanon_unit
from tests.product_check import oracle_sa_table

RL = 100                                            # read length of the hand-made reads, unless a record says otherwise
SHAPES = ("SM", "MS", "SMS", "SMD", "MDS", "SMDS", "SMI", "MIS", "SMIS")
STRANDS = (("fwd", "+"), ("rev", "-"))
BAD = "chr1,500,+,1S2M3S4M,60,1"                    # S and M, but none of the nine shapes: KeyError (cp:255)
NO_S = "chr1,300,+,100M,60,0"                       # no S: the read fails as a whole (cp:248-253)
NO_M = "chr1,400,-,20S30I50S,60,0"                  # no M: the same
ZERO = "chr2,3000,+,20S1M79S,60,1"                  # SMS of one base: qs == qe whatever the read length (cp:268)
FILLER = "zz_plain"                                 # a plain MAPQ-60 record without SA: fetch() divides by their number


def ent(rname, pos, strand, cigar, mapq=60, nm=1):
    return "%s,%d,%s,%s,%d,%d" % (rname, pos, strand, cigar, mapq, nm)


def shape_of(entry):
    return O.split_cigar(entry.split(",")[3])[0]


def q(entry, rl=RL):
    """(qs, qe) of an SA entry by the oracle's cigar2pos."""
    f = entry.split(",")
    return tuple(O.cigar2pos(f[3], f[2], rl)[:2])


def at(qs, qe, rl=RL, strand="+", rname="chr1", pos=1000, mapq=60, nm=1):
    """An SMS entry with the query interval [qs, qe]."""
    assert 0 < qs <= qe < rl - 1
    c5, c3 = (qs, rl - 1 - qe) if strand == "+" else (rl - 1 - qe, qs)
    e = ent(rname, pos, strand, "%dS%dM%dS" % (c5, qe - qs + 1, c3), mapq, nm)
    assert q(e, rl) == (qs, qe)
    return e


def rec(name, sa=None, flag=0, qlen=RL, tid=0):
    """One record: ``sa`` is its SA tag as a list of entries (None: no tag); tid -1 is an unplaced record (they end the file)."""
    return dict(name=name, sa=list(sa) if sa is not None else None, flag=flag, qlen=qlen, tid=tid)


def supp(name, sa=None, flag=2048):
    """A supplementary (or, with flag 256, secondary) record; its hard-clipped length must never become the read length."""
    return rec(name, sa, flag=flag, qlen=30)


def _pair(k):
    """Two well-formed entries of a good read, different for every k."""
    return [at(10, 29 + k % 7, pos=1000 * (k + 1), mapq=60 - k % 50), at(40, 69 + k % 11, rname="chr2", pos=1000 * (k + 1) + 500, strand="-", nm=k % 9)]


# ---- the reference's recorded vectors -------------------------------------------------------------------------------------------
def unit_vectors():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unit_vectors.json")) as fp:
        vec = json.load(fp)
    return vec["cigar2pos"], [dict(v, out=uncanon_unit(v["out"])) for v in vec["alignment_from_satags"]]


def cigar2pos_entry(k, v):
    return ent("chr1", 1000 + 13 * k, v["strand"], v["cigar"], 60, 1)


def _cigar2pos_vectors():
    """One read per vector: a primary of the vector's read length, one SA entry with its CIGAR and strand."""
    vec, _ = unit_vectors()
    assert len(vec) == 108 and all(v["out"][0] != v["out"][1] for v in vec)          # (no zero-length interval: no error)
    assert {(shape_of(cigar2pos_entry(0, v)), v["strand"]) for v in vec} == {(s, st) for s in SHAPES for _, st in STRANDS}
    return [rec("c2p%03d" % k, [cigar2pos_entry(k, v)], qlen=v["read_length"]) for k, v in enumerate(vec)]


def _satags_vectors():
    _, vec = unit_vectors()
    assert len(vec) == 40 and all(2 <= len(v["sa_list"]) <= 5 and len(set(v["sa_list"])) == len(v["sa_list"]) for v in vec)
    return [rec("afs%02d" % k, v["sa_list"], qlen=v["read_length"]) for k, v in enumerate(vec)]


# ---- hand-made reads -------------------------------------------------------------------------------------------------------------
def _ties():
    a, b, c = at(20, 49, pos=1000, mapq=10), at(20, 49, pos=2000, strand="-", mapq=20), at(20, 49, rname="chr2", pos=3000, mapq=30)
    lo, hi = at(5, 15, pos=4000), at(60, 80, pos=5000)
    assert q(a) == q(b) == q(c) and len({a, b, c}) == 3 and q(lo) < q(a) < q(hi)
    orders = [[a, lo, b, hi, c], [c, hi, b, lo, a], [hi, b, a, lo, c]]
    assert len({tuple(o) for o in orders}) == 3
    desc = [at(20, 80, pos=6000), at(20, 60, pos=7000), at(20, 40, pos=8000)]
    assert [q(e)[0] for e in desc] == [20, 20, 20] and [q(e)[1] for e in desc] == [80, 60, 40]
    return [rec("tie%d" % k, o) for k, o in enumerate(orders)] + [rec("same_qs", desc)]


def _ties_verify(x):
    a, b, c = 999, 2028, 2999                    # where the three tied entries start on the reference ('-': pos + al - 2)
    assert [x.ra("tie%d" % k)[1:4] for k in range(3)] == [[a, b, c], [c, b, a], [b, a, c]]
    assert x.qe("same_qs") == [40, 60, 80]


def _dedup():
    x, y, z, p = at(10, 29, pos=1000), at(30, 59, pos=2000, strand="-"), at(60, 89, pos=3000), at(2, 9, pos=4000)
    x_nm, x_mq = at(10, 29, pos=1000, nm=2), at(10, 29, pos=1000, mapq=59)
    assert x.rsplit(",", 1)[0] == x_nm.rsplit(",", 1)[0] and x != x_nm                 # all eight token fields equal, NM not
    assert x.split(",")[:4] == x_mq.split(",")[:4] and x.split(",")[5] == x_mq.split(",")[5] and x != x_mq
    return [rec("shared", [x, y]), supp("shared", [p, x]),                             # x on the primary's and the supplementary's list
            rec("apart", [x, y, x, z, y]),                                             # duplicates that are not adjacent
            rec("nm_differs", [x, x_nm]), rec("mapq_differs", [x, x_mq]),
            rec("all_one", [z, z, z]), supp("all_one", [z])]


def _dedup_verify(x):
    assert [x.n_rows(n) for n in ("shared", "apart", "nm_differs", "mapq_differs", "all_one")] == [3, 3, 2, 2, 1]
    assert x.col("nm_differs", 7) == [1, 2] and x.col("mapq_differs", 6) == [60, 59]


def _dict_order():
    recs = [rec("late"), supp("b", _pair(1)), rec("a", _pair(2)), rec("b"), supp("late", _pair(3))]
    first = lambda pred: list(dict.fromkeys(r["name"] for r in recs if pred(r)))
    by_id, by_sa, by_primary = first(lambda r: True), first(lambda r: r["sa"]), first(lambda r: r["flag"] < 256)
    assert by_sa == ["b", "a", "late"] and len({tuple(by_id), tuple(by_sa), tuple(by_primary)}) == 3
    assert recs.index(supp("b", _pair(1))) < recs.index(rec("b"))                      # a supplementary with SA ahead of its primary
    assert [r["sa"] is None for r in recs if r["name"] == "late" and r["flag"] < 256] == [True]      # its primary has no SA
    return recs


def _dict_order_verify(x):
    assert x.reads == ["b", "a", "late"] and not x.e["failed"].any()


def _read_length():
    sm = lambda pos: [ent("chr1", pos, "+", "40S7M"), ent("chr2", pos, "-", "7M20S")]      # both end at read length - 1
    assert all(q(e, 100) != q(e, 80) for e in sm(1))
    return [rec("after", qlen=100), rec("after", flag=16, qlen=80), supp("after", sm(1000)),
            supp("before", sm(2000)), rec("before", flag=16, qlen=90), rec("before", qlen=70),
            rec("unmapped_first", flag=4, qlen=55), rec("unmapped_first", sm(3000), qlen=100)]      # flag 4 < 256, placed: it counts


def _read_length_verify(x):
    assert [x.read_length(n) for n in ("after", "before", "unmapped_first")] == [100, 90, 55]
    assert [x.qe(n) for n in ("after", "before", "unmapped_first")] == [[99, 99], [89, 89], [54, 54]]


def _orphans():
    return [rec("good1", _pair(1)), supp("no_primary", _pair(2)), supp("unplaced_primary", _pair(3)), supp("orphan_bad", [BAD]),
            supp("orphan_zero", [ZERO], flag=256), rec("good2", _pair(4)),
            rec("unplaced_primary", flag=4, qlen=RL, tid=-1),                          # its only flag < 256 record is unplaced
            rec("good2", [at(70, 89, pos=9000)], flag=4, qlen=40, tid=-1),             # an SA-bearing unplaced record: ignored
            rec("ghost", [BAD], flag=4, qlen=40, tid=-1)]


def _orphans_verify(x):
    assert x.reads == ["good1", "good2"] and x.n_rows("good2") == 2 and x.read_length("unplaced_primary") == -1
    assert x.read_length("good2") == RL


def _failed():
    return [rec("good1", _pair(1)), rec("no_s_then_bad", [NO_S, BAD]), rec("good2", _pair(2)), rec("zero_then_no_s", [ZERO, NO_S]),
            rec("no_m", [_pair(3)[0], NO_M]), rec("good3", _pair(3))]


def _failed_verify(x):
    assert x.e["failed"].tolist() == [False, True, False, True, True, False] and x.e["off"].tolist() == [0, 2, 2, 4, 4, 4, 6]


def edge_cigar(shape, strand, d, rl=RL):
    """A CIGAR of the shape whose query interval on the strand has qe - qs == d."""
    fwd, s = strand == "+", rl - 1 - d
    cigar = {"SM": ("%dS7M" % s) if fwd else ("30S%dM" % (d + 1)),
             "MS": ("%dM30S" % (d + 1)) if fwd else ("7M%dS" % s),
             "SMS": "20S%dM30S" % (d + 1),
             "SMD": ("%dS7M3D" % s) if fwd else ("30S%dM3D" % (d + 1)),
             "MDS": ("%dM3D30S" % (d + 1)) if fwd else ("7M3D%dS" % s),
             "SMDS": ("20S7M3D%dS" % (s - 20)) if fwd else ("%dS7M3D20S" % (s - 20)),
             "SMI": "%dS7M2I" % s,
             "MIS": "7M2I%dS" % s,
             "SMIS": ("20S7M2I%dS" % (s - 20)) if fwd else ("%dS7M2I20S" % (s - 20))}[shape]
    e = ent("chr3", 7000, strand, cigar)
    assert shape_of(e) == shape and q(e, rl)[1] - q(e, rl)[0] == d
    return e


def _one_base():
    return [rec("one_%s_%s" % (sh, nm), [edge_cigar(sh, st, 1)]) for sh in SHAPES for nm, st in STRANDS]


def _zero_length(shape, strand):
    return lambda: [rec("good", _pair(1)), rec("zero", [edge_cigar(shape, strand, 0)])]


def _one_entry_reads(n):
    def build():
        recs = [rec("r%03d" % k, [at(10 + k % 50, 60 + k % 30, pos=1000 + k, strand="+-"[k % 2], mapq=k % 61)]) for k in range(n)]
        assert sum(len(r["sa"]) for r in recs) == len({r["name"] for r in recs}) == n           # as many groups as SA rows
        return recs
    return build


def _long_read():
    """One read of 300 entries among 3 reads of one entry; its (qs, qe) keys fall with the input order, 20 of them tie."""
    ents, k = [], 0
    for i in range(300):
        k += 0 if i % 15 == 7 else 1
        ents.append(at(800 - 2 * k, 805 - 2 * k, rl=1000, pos=1000 + i, mapq=i % 61))
    keys = [q(e, 1000) for e in ents]
    assert len(set(ents)) == 300 and all(x >= y for x, y in zip(keys, keys[1:])) and sum(x == y for x, y in zip(keys, keys[1:])) == 20
    return [rec("one0", [at(10, 20)]), rec("long", ents, qlen=1000), rec("one1", [at(30, 40)]), rec("one2", [at(50, 60)])]


def _long_read_verify(x):
    pos = x.col("long", 3)
    assert len(pos) == 300 and sum(b == a + 1 for a, b in zip(pos, pos[1:])) == 20          # the tied entries stay in input order


def _many_names(n_names=70_000, n_reads=6_000, seed=7):
    """6 000 reads of 1 to 4 entries among 70 000 names: name ids beyond 16 bits.  A seeded shuffle decides which record carries
    which SA list."""
    rng = np.random.default_rng(seed)
    carriers = rng.permutation(n_names)[:n_reads].tolist()
    sa_of = {}
    for j, i in enumerate(carriers):
        sa_of[i] = [at(int(rng.integers(1, 16)), int(rng.integers(16, 39)), rl=40, pos=int(rng.integers(1, 1 << 27)), strand="+-"[int(rng.integers(2))],
                       rname="chr%d" % int(rng.integers(1, 23)), mapq=int(rng.integers(0, 61)), nm=int(rng.integers(0, 9))) for _ in range(1 + j % 4)]
    assert n_names > 65_536 and sum(i > 65_536 for i in carriers) > 100 and sum(i < 256 for i in carriers) > 5
    return [rec("n%05d" % i, sa_of.get(i), qlen=40) for i in range(n_names)]


def _no_sa():
    return [rec("p%d" % k) for k in range(5)]


def _only_orphans():
    return [supp("o1", _pair(1)), supp("o2", [BAD], flag=256), rec("p")]


# ---- the error rule: the first offending read in the reference's read order decides ------------------------------------------
def _bad(name="x"):
    return rec(name, [BAD], qlen=55)


def _zero(name="z"):
    e = ent("chr1", 500, "+", "54S1M")
    assert q(e, 55) == (54, 54)
    return rec(name, [e], qlen=55)


def _mixed_errors(bad_first, seed):
    def build():
        rng = np.random.default_rng(seed)
        i, j = int(rng.integers(20, 200)), int(rng.integers(256, 300))          # (two thread blocks of the kernel)
        recs = [rec("g%03d" % k, _pair(k)[:1 + k % 2]) for k in range(300)]
        recs[i], recs[j] = (_bad(), _zero()) if bad_first else (_zero(), _bad())
        return recs
    return build


def _error_order():
    """By name id the zero-length read comes first, by its first SA-bearing record the unknown shape does: KeyError."""
    z = _zero()
    return [rec("z", qlen=55), _bad(), supp("z", z["sa"])]


def _error_order_reversed():
    """The other way round: the unknown shape has the lower name id, the zero-length read the earlier SA record."""
    return [rec("x", qlen=55), _zero(), supp("x", [BAD])]


def _error_order_behind_a_good_read():
    """Three reads: SA rows of a good read come first, then the unknown shape, then the zero-length read - which has the lowest
    name id of all.  The ordinal of either report is the read's first SA row, not its place among the name-sorted rows."""
    recs = [rec("z", qlen=55), rec("good", _pair(1)), _bad(), supp("z", _zero()["sa"])]
    sa_names = [r["name"] for r in recs if r["sa"]]
    assert sa_names == ["good", "x", "z"] and [r["name"] for r in recs][0] == "z"
    return recs


CASES = {
    "cigar2pos_vectors": (_cigar2pos_vectors, None), "satags_vectors": (_satags_vectors, None),
    "ties": (_ties, _ties_verify), "dedup": (_dedup, _dedup_verify), "dict_order": (_dict_order, _dict_order_verify),
    "read_length": (_read_length, _read_length_verify), "orphans": (_orphans, _orphans_verify), "failed": (_failed, _failed_verify),
    "one_base": (_one_base, None), "reads255": (_one_entry_reads(255), None), "reads256": (_one_entry_reads(256), None),
    "reads257": (_one_entry_reads(257), None), "long_read": (_long_read, _long_read_verify), "many_names": (_many_names, None),
    "no_sa": (_no_sa, None), "only_orphans": (_only_orphans, None),
}
ERROR_CASES = {
    "bad_zero": (lambda: [_bad(), _zero()], KeyError), "zero_bad": (lambda: [_zero(), _bad()], ZeroDivisionError),
    "mixed_bad_first": (_mixed_errors(True, 11), KeyError), "mixed_zero_first": (_mixed_errors(False, 12), ZeroDivisionError),
    "error_order": (_error_order, KeyError), "error_order_reversed": (_error_order_reversed, ZeroDivisionError),
    "error_order_behind_a_good_read": (_error_order_behind_a_good_read, KeyError),
    "bad_then_no_s": (lambda: [rec("good", _pair(1)), rec("x", [BAD, NO_S])], KeyError),
}
ERROR_CASES.update({"zero_%s_%s" % (sh, nm): (_zero_length(sh, st), ZeroDivisionError) for sh in SHAPES for nm, st in STRANDS})


# ---- from a case to its file, its decoded records and its expectation -----------------------------------------------------------
class _FetchView:
    """What the oracle's fetch() reads, taken from decoded records - with the SA strings as the file holds them."""

    def __init__(self, back, texts):
        g = lambda t: t.cpu().numpy().astype(np.int64)
        self.n, self.chroms = int(back.n), list(back.header_chroms)
        self.tid, self.flag, self.mapq, self.nm, self.name_id = (g(getattr(back, k)) for k in ("tid", "flag", "mapq", "nm", "name_id"))
        self.qlen = np.where(g(back.has_seq) != 0, g(back.qlen), 0)                    # pysam query_length
        self.names = list(back.materialise_names())
        self.sa_str = [texts.get(i) for i in range(self.n)]
        mapped = self.tid[:int(np.count_nonzero(self.tid >= 0))]
        assert not (mapped < 0).any() and not (np.diff(mapped) < 0).any(), "records must be sorted by contig, unplaced ones last"


class Expect:
    """The expectation of a case by read name (for the checks that a case is what it is named after)."""

    def __init__(self, e, names):
        self.e, self.names = e, names
        self.reads = [names[i] for i in e["name"]]

    def _span(self, name):
        r = self.reads.index(name)
        return int(self.e["off"][r]), int(self.e["off"][r + 1])

    def n_rows(self, name):
        a, b = self._span(name)
        return b - a

    def col(self, name, c):
        a, b = self._span(name)
        return self.e["cols"][c, a:b].tolist()

    def qe(self, name):
        return self.col(name, 1)

    def ra(self, name):
        return self.col(name, 3)

    def read_length(self, name):
        return int(self.e["read_length"][self.names.index(name)])


class Case:
    def __init__(self, name, recs, tmp_dir):
        from coral_amd.global_names import chr_idx
        placed = [r for r in recs if r["tid"] >= 0] + [rec(FILLER)]
        recs = placed + [r for r in recs if r["tid"] < 0]
        assert [r["tid"] >= 0 for r in recs] == [True] * len(placed) + [False] * (len(recs) - len(placed)), "unplaced records end the file"
        alns, self.texts = [], {}
        for i, r in enumerate(recs):
            unmapped = bool(r["flag"] & 4)
            alns.append(dict(tid=r["tid"], pos=100 + 10 * i if r["tid"] >= 0 else -1, flag=r["flag"], name=r["name"], qlen=r["qlen"],
                             mapq=0 if unmapped else 60, cigar=[] if unmapped else [(M, r["qlen"])]))
            if r["sa"] is not None:
                self.texts[i] = ";".join(r["sa"]) + ";"
        self.name, self.recs = name, recs
        self.path = os.path.join(str(tmp_dir), name + ".bam")
        written = synth.records_from_alignments(alns)
        written.sa_text = self.texts
        bam.write_bam(written, self.path, fast_seq=True)
        self.rec = bam.decode_bam(self.path, n_threads=2)
        assert self.rec.n == len(recs) and self.rec.flag.tolist() == [r["flag"] for r in recs]
        assert np.diff(self.rec.sa_off.numpy()).tolist() == [len(r["sa"] or ()) for r in recs]          # one token row per entry
        h = _FetchView(self.rec, self.texts)
        assert any(h.sa_str[i] is None and h.tid[i] >= 0 and h.mapq[i] == 60 and h.qlen[i] > 0 for i in range(h.n))
        self.names = h.names
        chr_rank = np.array([chr_idx.get(c, -1) for c in h.chroms], dtype=np.int32)
        try:
            self.expect = dict(zip(("cols", "off", "name", "failed", "read_length", "pairs"), oracle_sa_table(h, chr_rank)))
            self.raises = None
        except (KeyError, ZeroDivisionError) as exc:
            self.expect, self.raises = None, type(exc)


_loaded = {}


def load(name, tmp_dir):
    """The case ``name``, built, written and modelled once per process."""
    if name not in _loaded:
        build = (CASES.get(name) or ERROR_CASES[name])[0]
        _loaded[name] = Case(name, build(), tmp_dir)
    return _loaded[name]
