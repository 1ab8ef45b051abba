"""BAI index built during the BAM decode (bam.build_index), its reader and region query (bam.read_index, bam.region_spans), and the
region-restricted decode behind bam.window_coverage(index=...) and bam.load_bam(regions=...).

The index bytes are compared with an INDEPENDENT restatement in this module: the BAM is walked with zlib + struct, BGZF block
by BGZF block, by tests/bamfile.py, so every record's virtual offset comes from block boundaries found there, and the rules of
SAMv1 §5 are applied to them here without either decoder.  Region decodes are compared with the whole-file decode, filtered here."""
import os
import struct

import numpy as np
import pytest

from coral_amd import _lib, bam, plot_coverage, synth
from tests.bamfile import D, EQ, I, M, N, S, X, oracle_coverage, read_bam, read_bam_bgzf
from tests.decode_support import (RECORD_FIELDS as FIELDS, coverage_odd_records as odd_records, coverage_windows as make_windows, cpu,  # noqa: F401
                                  host_window_coverage as host_coverage, plot_case as _plot_case, with_qual)

PSEUDO = 37450
NO_COOR_TID = 25                        # one behind the last contig while the records are merged and sorted


def reg2bin(beg, end):
    end -= 1
    for shift, off in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return off + (beg >> shift)
    return 0


# ---- the restatement --------------------------------------------------------------------------------------------------------
def walk_bam(path):
    """(ref lengths, records [dict(tid, pos, end, flag, voff)] in file order, virtual offset behind the last record): the records
    of tests/bamfile.py, read BGZF block by BGZF block, with the end of SAMv1 section 5 (a placed read covers at least one base)."""
    parsed = read_bam_bgzf(path)
    recs = []
    for r in parsed.recs:
        ops = r["ops"]
        rlen = 0 if (r["flag"] & 4) or len(ops) == 0 else int((ops >> 4)[np.isin(ops & 15, (M, D, N, EQ, X))].sum())
        recs.append(dict(tid=r["tid"], pos=r["pos"], end=r["pos"] + max(rlen, 1), flag=r["flag"], voff=r["voff"]))
    return parsed.lens, recs, parsed.end_voff


def restated_index(path):
    """The BAI bytes by the rules of the issue: chunks = maximal runs of file-consecutive records with one (tid, bin), from the
    first record's start to the start of the record behind the last; bins ascending, pseudo-bin last; linear index = smallest
    offset per overlapped 16 kb window, holes filled from the left, leading holes 0; n_no_coor."""
    lens, recs, end_voff = walk_bam(path)
    ends = [r["voff"] for r in recs[1:]] + [end_voff]
    per = [dict(bins={}, lin={}, mapped=0, unmapped=0, lo=None, hi=None) for _ in lens]
    no_coor, prev = 0, None
    for r, e in zip(recs, ends):
        if r["tid"] < 0:
            no_coor += 1
            prev = None
            continue
        c = per[r["tid"]]
        beg, end = max(r["pos"], 0), r["end"]
        key = (r["tid"], reg2bin(beg, end))
        chunks = c["bins"].setdefault(key[1], [])
        if key == prev:
            chunks[-1][1] = e
        else:
            chunks.append([r["voff"], e])
        prev = key
        c["unmapped" if r["flag"] & 4 else "mapped"] += 1
        c["lo"] = r["voff"] if c["lo"] is None else c["lo"]
        c["hi"] = e
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            c["lin"][w] = min(c["lin"].get(w, r["voff"]), r["voff"])
    out = [b"BAI\x01", struct.pack("<i", len(lens))]
    for c in per:
        if not c["bins"]:
            out.append(struct.pack("<ii", 0, 0))
            continue
        out.append(struct.pack("<i", len(c["bins"]) + 1))
        for b in sorted(c["bins"]):
            out.append(struct.pack("<Ii", b, len(c["bins"][b])) + b"".join(struct.pack("<QQ", *ch) for ch in c["bins"][b]))
        out.append(struct.pack("<IiQQQQ", PSEUDO, 2, c["lo"], c["hi"], c["mapped"], c["unmapped"]))
        n_intv = max(c["lin"]) + 1
        vals, last = [], 0
        for w in range(n_intv):
            last = c["lin"].get(w, last)
            vals.append(last)
        out.append(struct.pack("<i", n_intv) + struct.pack("<%dQ" % n_intv, *vals))
    out.append(struct.pack("<Q", no_coor))
    return b"".join(out)


# ---- test data ---------------------------------------------------------------------------------------------------------------
def make_records(n=450):
    big = [(S, 100)] + [(M, 7000), (I, 3), (D, 5)] * 142 + [(M, 6000)]            # 1 Mb: bins of levels 0..2, 62 windows
    extra = synth.records_from_alignments([
        dict(tid=7, pos=1_000_000, cigar=big, name="megabase"),
        dict(tid=7, pos=1_300_000, cigar=[(M, 400)], name="twin1"),
        dict(tid=7, pos=1_300_000, cigar=[(M, 90_000)], name="twin2"),             # same start, another bin
        dict(tid=7, pos=1_300_000, cigar=[(M, 300)], name="twin3"),
        dict(tid=NO_COOR_TID, pos=0, cigar=[], flag=4, name="nc1", qlen=50),
        dict(tid=NO_COOR_TID, pos=0, cigar=[], flag=4, name="nc2", qlen=70),
        dict(tid=NO_COOR_TID, pos=0, cigar=[], flag=4, name="nc1", qlen=30),
    ])
    base = synth.merge_sorted(synth.generate(synth.scaled_config("tiny", n), "cpu"), odd_records())
    base.header_chroms.append("sentinel")
    extra.header_chroms.append("sentinel")
    rec = synth.merge_sorted(base, extra)
    rec.header_chroms.pop()
    nc = rec.tid == NO_COOR_TID
    assert int(nc.sum()) == 3 and bool(nc[-3:].all())
    rec.tid[nc], rec.pos[nc], rec.end[nc] = -1, -1, 0
    return rec


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("bai")
    rec = make_records()
    small = str(d / "small_blocks.bam")
    bam.write_bam(rec, small, seed=9, with_qual=with_qual, block_size=1500, empty_block_every=5, fast_seq=True)
    plain = str(d / "plain.bam")
    bam.write_bam(rec, plain, seed=9, with_qual=with_qual, fast_seq=True)
    whole = bam.decode_bam(small, n_threads=2)
    assert whole.n == rec.n
    return dict(dir=d, rec=rec, small=small, plain=plain, whole=whole, walked=walk_bam(small), blocks=bam.LAST_DECODE["blocks"])


def index_bytes(path, device, **kw):
    out = bam.build_index(path, path + ".test.bai", device=device, **kw)
    with open(out, "rb") as fp:
        data = fp.read()
    os.remove(out)
    return data


# ---- index content -----------------------------------------------------------------------------------------------------------
def test_fixture_holds_the_planted_shapes(case):
    lens, recs, _ = case["walked"]
    assert len(recs) == case["rec"].n and sum(r["tid"] < 0 for r in recs) == 3 and recs[-1]["tid"] < 0
    assert any(r["end"] - r["pos"] >= 1_000_000 for r in recs) and any(r["flag"] & 4 and r["tid"] >= 0 for r in recs)
    assert not any(r["tid"] == 2 for r in recs)                                   # chr3: a contig without records
    assert case["blocks"] > 3000 and len({r["voff"] >> 16 for r in recs}) > 300     # thousands of blocks to skip
    assert sum(a["tid"] == b["tid"] and a["pos"] == b["pos"] for a, b in zip(recs, recs[1:])) >= 2


def test_host_index_equals_restatement(case, cpu):
    for path in (case["small"], case["plain"]):
        want = restated_index(path)
        assert index_bytes(path, "cpu", n_threads=3) == want
        assert index_bytes(path, "cpu", n_threads=1) == want


@pytest.mark.parametrize("world", [2, 3, 5])
def test_host_partial_indexes_merge_into_the_single_decode(case, cpu, world):
    assert index_bytes(case["small"], "cpu", world=world, n_threads=2) == restated_index(case["small"])


def check_spec_properties(path, data_path):
    idx = bam.read_index(path)
    lens, recs, end_voff = walk_bam(data_path)
    ends = [r["voff"] for r in recs[1:]] + [end_voff]
    for t in range(idx.n_ref):
        for b, ch in idx.bins[t].items():                                         # file order, disjoint
            assert (ch[:, 0] < ch[:, 1]).all() and (ch[1:, 0] >= ch[:-1, 1]).all(), (t, b)
    for r, e in zip(recs, ends):
        if r["tid"] < 0:
            continue
        ch = idx.bins[r["tid"]][reg2bin(max(r["pos"], 0), r["end"])]
        assert int(((ch[:, 0] <= r["voff"]) & (ch[:, 1] >= e)).sum()) == 1       # inside exactly one chunk of its own bin
        lin = idx.linear[r["tid"]]
        for w in range(max(r["pos"], 0) >> 14, ((r["end"] - 1) >> 14) + 1):
            assert w < len(lin) and int(lin[w]) <= r["voff"]
    for t in range(idx.n_ref):
        mine = [r for r in recs if r["tid"] == t]
        if not mine:
            assert idx.meta[t] is None and not idx.bins[t] and len(idx.linear[t]) == 0
        else:
            assert idx.meta[t][2:] == (sum(not r["flag"] & 4 for r in mine), sum(bool(r["flag"] & 4) for r in mine))
            assert idx.meta[t][0] == mine[0]["voff"]
    assert idx.n_no_coor == sum(r["tid"] < 0 for r in recs)


def test_host_index_spec_properties(case, cpu):
    out = bam.build_index(case["small"], str(case["dir"] / "props.bai"), device="cpu")
    check_spec_properties(out, case["small"])


def swap_two_records(rec):
    """The same records with two neighbours on one contig in the wrong order."""
    a = rec.to("cpu")
    pos = a.pos.clone()
    k = next(i for i in range(10, a.n - 1) if a.tid[i] == a.tid[i + 1] and a.pos[i] + 5 < a.pos[i + 1])
    pos[k], pos[k + 1] = a.pos[k + 1], a.pos[k]
    end = a.end + (pos - a.pos)
    return synth.Records(**{**a.__dict__, "pos": pos, "end": end})


def test_unsorted_file_fails_and_leaves_no_index(case, cpu, tmp_path):
    path = str(tmp_path / "unsorted.bam")
    bam.write_bam(swap_two_records(synth.generate(synth.scaled_config("tiny", 120), "cpu")), path, seed=2, fast_seq=True, block_size=3000)
    with pytest.raises(_lib.CoralHipError, match="coordinate order"):
        bam.build_index(path, device="cpu")
    assert os.listdir(str(tmp_path)) == ["unsorted.bam"]


# ---- reader and query --------------------------------------------------------------------------------------------------------
def bai(contigs, n_no_coor=None):
    """Hand-assembled BAI bytes: contigs = [({bin: [(beg, end), ...]}, [linear offsets])]."""
    out = [b"BAI\x01", struct.pack("<i", len(contigs))]
    for bins, lin in contigs:
        out.append(struct.pack("<i", len(bins)))
        for b, chunks in bins.items():
            out.append(struct.pack("<Ii", b, len(chunks)) + b"".join(struct.pack("<QQ", *c) for c in chunks))
        out.append(struct.pack("<i", len(lin)) + struct.pack("<%dQ" % len(lin), *lin))
    if n_no_coor is not None:
        out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


def V(block, off=0):
    return (block << 16) | off


def test_reader_accepts_what_other_writers_produce(tmp_path):
    # contig 0: the only chunk for a level-5 region sits in the parent (level-4) bin 585, as htslib folds sparse bins; pre-merged
    # chunks in bin 4683; no pseudo-bin; a linear index of 3 windows on a long contig.  contig 1: no bins at all.
    p = str(tmp_path / "hand.bai")
    with open(p, "wb") as fp:
        fp.write(bai([({585: [(V(100), V(900, 7))], 4683: [(V(2000), V(5000))]}, [V(100), V(100), V(2000)]), ({}, [])]))
    idx = bam.read_index(p)
    assert idx.n_ref == 2 and idx.n_no_coor is None and idx.meta == [None, None] and len(idx.linear[0]) == 3
    assert bam.region_spans(idx, [(0, 10, 20)]).tolist() == [[V(100), V(900, 7)]]             # found in the parent bin
    assert bam.region_spans(idx, [(0, 2 * 16384 + 5, 2 * 16384 + 9)]).tolist() == [[V(2000), V(5000)]]      # 585 ends before ioffset[2]
    assert bam.region_spans(idx, [(0, 40 * 16384, 41 * 16384)]).tolist() == []               # beyond the short linear index: its last entry
    assert bam.region_spans(idx, [(1, 0, 1000)]).tolist() == [] and bam.region_spans(idx, [(0, 5, 5)]).tolist() == []
    # the union over regions: overlapping chunk lists become one span, spans that share a block are joined
    both = bam.region_spans(idx, [(0, 10, 20), (0, 16384, 16390), (0, 2 * 16384 + 5, 2 * 16384 + 9), (0, 12, 30)])
    assert both.tolist() == [[V(100), V(900, 7)], [V(2000), V(5000)]]
    with open(p, "wb") as fp:        # with the pseudo-bin and n_no_coor; chunks that touch / share a block
        fp.write(bai([({4681: [(V(10), V(20, 5))], 4682: [(V(20, 9), V(30))], PSEUDO: [(V(10), V(30)), (7, 2)]}, [V(10), V(20, 9)])], 11))
    idx = bam.read_index(p)
    assert idx.n_no_coor == 11 and idx.meta[0] == (V(10), V(30), 7, 2) and PSEUDO not in idx.bins[0]
    assert bam.region_spans(idx, [(0, 0, 16384), (0, 16384, 16385)]).tolist() == [[V(10), V(30)]]
    with pytest.raises(ValueError):
        bam.region_spans(idx, [(1, 0, 5)])


def test_reader_rejects_broken_files(case, cpu, tmp_path):
    good = bai([({4681: [(V(10), V(20))], PSEUDO: [(V(10), V(20)), (1, 0)]}, [V(10)])], 0)
    for k, data in enumerate([good[:-3], good[:30], good[:9], b"BAM\x01" + good[4:], b"", good + b"\0"]):
        p = str(tmp_path / ("bad%d.bai" % k))
        with open(p, "wb") as fp:
            fp.write(data)
        with pytest.raises(_lib.CoralHipError):
            bam.read_index(p)
    p = str(tmp_path / "one_contig.bai")             # a valid index of another file: n_ref differs from the BAM header's
    with open(p, "wb") as fp:
        fp.write(good)
    with pytest.raises(_lib.CoralHipError):
        bam.window_coverage(case["small"], [("chr8", 0, 100)], device="cpu", index=p)
    with pytest.raises(_lib.CoralHipError):
        bam.window_coverage(case["small"], [("chr8", 0, 100)], device="cpu", index=str(tmp_path / "missing.bai"))
    with pytest.raises(_lib.CoralHipError):
        bam.load_bam(case["small"], "cpu", regions=[("chr8", 0, 100)], index=p)


# ---- completeness of the query -----------------------------------------------------------------------------------------------
def comparable(rec, ids=None):
    """Every field tests/test_bam_io.py compares, of the records `ids` (all), in a form that does not depend on numbering."""
    ids = np.arange(rec.n) if ids is None else np.asarray(ids, dtype=np.int64)
    g = lambda k: getattr(rec, k).cpu().numpy()
    out = {k: g(k)[ids].tolist() for k in FIELDS if k not in ("cigar_off", "cigar", "sa_off", "sa", "sa_nm", "nonacgt_rec", "nonacgt_pos", "name_id")}
    co, so, cig, sa, sa_nm = g("cigar_off"), g("sa_off"), g("cigar"), g("sa"), g("sa_nm")
    out["cigar"] = [cig[co[i]:co[i + 1]].tolist() for i in ids]
    out["sa"] = [(sa[so[i]:so[i + 1]].tolist(), sa_nm[so[i]:so[i + 1]].tolist()) for i in ids]
    where = {int(i): k for k, i in enumerate(ids)}
    out["nonacgt"] = sorted((where[int(r)], int(p)) for r, p in zip(g("nonacgt_rec"), g("nonacgt_pos")) if int(r) in where)
    names = rec.materialise_names() if not hasattr(rec.names, "take") else rec.names
    out["names"] = [names[int(k)] for k in g("name_id")[ids]]
    return out


def query_regions(case):
    rec = case["rec"]
    rng = np.random.default_rng(17)
    tid, pos, end = (getattr(rec, k).numpy() for k in ("tid", "pos", "end"))
    chroms, out = rec.header_chroms, []
    placed = np.nonzero(tid >= 0)[0]
    for k in rng.choice(placed, 24):                                              # random, where the reads are
        a = max(int(pos[k]) + int(rng.integers(-400, 400)), 0)
        out.append((chroms[tid[k]], a, a + int(rng.choice([1, 60, 900, 20_000, 300_000]))))
    for k in rng.choice(placed, 6):                                               # exactly on a record's pos / end
        out += [(chroms[tid[k]], int(pos[k]), int(pos[k]) + 1), (chroms[tid[k]], max(int(pos[k]) - 10, 0), int(pos[k])),
                (chroms[tid[k]], int(end[k]), int(end[k]) + 10), (chroms[tid[k]], int(end[k]) - 1, int(end[k]))]
    out += [("chr8", 1_400_000, 1_400_050), ("chr8", 1_999_000, 2_050_000), ("chr8", 1_300_000, 1_300_001)]      # inside the 1 Mb read
    out += [("chr3", 0, 1_000_000), ("chr3", 5_000, 5_001)]                        # the contig without records
    out += [("chr8", 90_000_000, 90_000_100), ("chr1", 0, 10), ("chr8", 500, 500), ("chrM", 16_100, 16_100)]     # empty
    return out


def check_region_decode(case, device, regions_list):
    whole = case["whole"]
    tid, pos, end = (getattr(whole, k).numpy() for k in ("tid", "pos", "end"))
    chroms = whole.header_chroms
    hits = 0
    for regions in regions_list:
        keep = np.zeros(whole.n, dtype=bool)
        for c, a, b in regions:
            keep |= (tid == chroms.index(c)) & (pos < b) & (end > a)
        got = bam.load_bam(case["small"], device, regions=regions, n_threads=2)
        assert got.n == int(keep.sum()), regions
        assert comparable(got) == comparable(whole, np.nonzero(keep)[0]), regions
        first_seen = {}
        assert got.name_id.tolist() == [first_seen.setdefault(s, len(first_seen)) for s in comparable(got)["names"]] and got.n_names == len(first_seen)
        assert got.header_chroms == whole.header_chroms and got.header_lens == whole.header_lens
        if keep.any() and keep.sum() < whole.n // 2:
            assert bam.LAST_DECODE["blocks"] > 0
        hits += int(keep.any())
    return hits


def test_host_region_decode_is_complete(case, cpu):
    bam.build_index(case["small"], device="cpu")
    regions = query_regions(case)
    hits = check_region_decode(case, "cpu", [[r] for r in regions])
    assert 30 < hits < len(regions)
    check_region_decode(case, "cpu", [regions[:9], regions[20:34] + regions[:3], regions])     # several (overlapping) regions in one call
    with pytest.raises(ValueError):
        bam.load_bam(case["small"], "cpu", regions=[("chrNope", 0, 5)])
    with pytest.raises(ValueError):
        bam.load_bam(case["small"], "cpu", regions=[("chr8", 0, 5)], world=2)
    with pytest.raises(ValueError):
        bam.load_bam(case["small"], "cpu", regions=[("chr8", 0, 5)], index=False)


def test_record_past_the_contig_end_is_still_found(cpu, tmp_path):
    """A record that reaches more than a window past its contig's header length: the linear index has the header's windows, the
    windows behind are folded into the last one, and every region the record overlaps still finds it."""
    rec = synth.records_from_alignments([dict(tid=24, pos=100, cigar=[(M, 300)], name="a"), dict(tid=24, pos=16_000, cigar=[(M, 40_000)], name="b"),
                                         dict(tid=24, pos=16_400, cigar=[(M, 50)], name="c")])
    path = str(tmp_path / "past.bam")
    bam.write_bam(rec, path, seed=1, fast_seq=True, block_size=2000)
    idx = bam.read_index(bam.build_index(path, device="cpu"))
    assert len(idx.linear[24]) == (rec.header_lens[24] >> 14) + 1 == 2
    whole = bam.decode_bam(path)
    for region in [("chrM", 40_000, 40_010), ("chrM", 16_390, 16_395), ("chrM", 0, 60_000), ("chrM", 33_000, 33_001)]:
        keep = (whole.pos.numpy() < region[2]) & (whole.end.numpy() > region[1])
        got = bam.load_bam(path, "cpu", regions=[region])
        assert comparable(got) == comparable(whole, np.nonzero(keep)[0]) and got.n >= 1


def test_host_span_straddling_two_blocks(case, cpu):
    straddle_check(case, "cpu")


def straddle_check(case, device):
    """A span whose first record starts in the last bytes of a block (not even its length field fits): the records of the
    span are those of the whole-file decode."""
    _, recs, end_voff = case["walked"]
    raw = open(case["small"], "rb").read()
    isize = lambda voff: struct.unpack_from("<I", raw, (voff >> 16) + struct.unpack_from("<H", raw, (voff >> 16) + 16)[0] + 1 - 4)[0]
    cand = [i for i, r in enumerate(recs[:-4]) if 0 < isize(r["voff"]) - (r["voff"] & 0xffff) < 4]
    assert cand, "no record starts in the last three bytes of a block in this file"
    for i in cand[:3]:
        j = min(i + 7, len(recs) - 1)
        spans = np.array([[recs[i]["voff"], recs[j]["voff"]]], dtype=np.uint64)
        got = bam._decode(case["small"], device, n_threads=2, spans=spans).records
        assert comparable(got) == comparable(case["whole"], np.arange(i, j))


# ---- window coverage through the index ---------------------------------------------------------------------------------------
def coverage_checks(case, device, thresholds=(0, 7, 20), **kw):
    path = case["small"]
    bam.build_index(path, device=device)
    windows = make_windows(case["rec"])
    parsed = read_bam(path)
    parsed = (parsed.refs, parsed.recs)
    for thr in thresholds:
        for cb in ("nofilter", "all"):
            plain = bam.window_coverage(path, windows, thr, cb, device=device, index=False, **kw)
            assert bam.LAST_DECODE["index"] is None
            assert np.array_equal(plain, oracle_coverage(parsed, windows, thr, cb))
            got = bam.window_coverage(path, windows, thr, cb, device=device, **kw)
            assert bam.LAST_DECODE["index"] == path + ".bai"
            assert np.array_equal(got, plain), (thr, cb)
    # one contig's first tenth: fewer blocks are read than the whole file has
    lens = case["rec"].header_lens
    tenth = [("chr8", k * 150, k * 150 + 150) for k in range(0, lens[7] // 10 // 150, 97)]
    a = bam.window_coverage(path, tenth, 7, "all", device=device, index=False, **kw)
    all_blocks = bam.LAST_DECODE["blocks"]
    b = bam.window_coverage(path, tenth, 7, "all", device=device, index=bam.read_index(path + ".bai"), **kw)
    assert np.array_equal(a, b) and a.sum() > 0 and 0 < bam.LAST_DECODE["blocks"] < all_blocks
    # more than 20 spans in one call
    rec = case["rec"]
    picks = np.nonzero(rec.tid.numpy() >= 0)[0][::max(rec.n // 40, 1)]
    narrow = [(rec.header_chroms[int(rec.tid[k])], int(rec.pos[k]) + 10, int(rec.pos[k]) + 40) for k in picks]
    a = bam.window_coverage(path, narrow, 0, "nofilter", device=device, index=False, **kw)
    b = bam.window_coverage(path, narrow, 0, "nofilter", device=device, **kw)
    assert np.array_equal(a, b) and bam.LAST_DECODE["spans"] > 20
    # the spans are disjoint pieces of the file and nothing behind a span's end is read unless its last record goes on there: the
    # blocks read stay below the file's (the header, the 1 Mb read and the records without coordinates lie in no span)
    assert 0 < bam.LAST_DECODE["blocks"] < all_blocks


def test_host_window_coverage_through_the_index(case, cpu):
    coverage_checks(case, "cpu", n_threads=2)


@pytest.mark.parametrize("name", ["tiny_region", "tiny_edge_region", "ultra"])
def test_host_plot_goldens_through_the_index(name, golden_dir, tmp_path, cpu):
    gold, rec, graph, want = _plot_case(golden_dir, name, tmp_path)
    path = str(tmp_path / "r.bam")
    bam.write_bam_native(rec, path, seed=4, n_threads=4)
    assert bam.build_index(path, device="cpu") == path + ".bai"
    bounds = plot_coverage.parse_region(gold["region"])
    got = plot_coverage.coverage_track_bam(path, plot_coverage.parse_graph_intervals(graph), bounds, device="cpu")
    assert got == want and bam.LAST_DECODE["index"] == path + ".bai"
    assert plot_coverage.coverage_track_bam(path, plot_coverage.parse_graph_intervals(graph), bounds, device="cpu", index=False) == want
    golden_windows_every_threshold(path, want, "cpu")


def golden_windows_every_threshold(path, want, device):
    """The plot's windows at thresholds 0, 7, 20 and both callbacks: through the index as without it (0 / nofilter: the golden)."""
    windows = [(c, a, b) for c, a, b, _ in want]
    for thr in (0, 7, 20):
        for cb in ("nofilter", "all"):
            plain = bam.window_coverage(path, windows, thr, cb, device=device, index=False)
            assert bam.LAST_DECODE["index"] is None
            got = bam.window_coverage(path, windows, thr, cb, device=device)
            assert bam.LAST_DECODE["index"] == path + ".bai" and np.array_equal(got, plain), (thr, cb)
            if (thr, cb) == (0, "nofilter"):
                assert got.tolist() == [t for *_, t in want]


def test_stale_or_invalid_index_falls_back_and_explicit_ones_raise(case, cpu, tmp_path):
    rec = synth.generate(synth.scaled_config("tiny", 150), "cpu")
    path = str(tmp_path / "s.bam")
    bam.write_bam(rec, path, seed=1, fast_seq=True, block_size=4000)
    w = [("chr8", 150_000, 151_000), ("chr1", 0, 5_000_000)]
    want = host_coverage(path, w, 0, "nofilter", index=False)
    bam.build_index(path, device="cpu")
    assert np.array_equal(host_coverage(path, w, 0, "nofilter"), want) and bam.LAST_DECODE["index"] == path + ".bai"
    os.utime(path + ".bai", (1, 1))                               # the BAM was rewritten after it was indexed
    assert np.array_equal(host_coverage(path, w, 0, "nofilter"), want)
    assert bam.LAST_DECODE["index"] is None and "older" in bam.LAST_DECODE["index_skipped"]
    with open(path + ".bai", "wb") as fp:                         # not a BAI at all (and new)
        fp.write(b"garbage")
    assert np.array_equal(host_coverage(path, w, 0, "nofilter"), want) and bam.LAST_DECODE["index"] is None
    with pytest.raises(_lib.CoralHipError):
        host_coverage(path, w, 0, "nofilter", index=path + ".bai")
    with pytest.raises(_lib.CoralHipError):
        host_coverage(path, w, 0, "nofilter", index=str(tmp_path / "nope.bai"))
    os.remove(path + ".bai")
    good = bam.build_index(path, str(tmp_path / "elsewhere.bai"), device="cpu")
    with pytest.raises(ValueError):
        host_coverage(path, w, 0, "nofilter", index=good, world=2)
    parts = [host_coverage(path, w, 0, "nofilter", rank=r, world=2) for r in range(2)]       # the default never shards a region decode
    assert np.array_equal(parts[0] + parts[1], want)


def test_both_region_decodes_choose_the_same_index(case, cpu, tmp_path):
    """window_coverage (the coverage request, neighbouring segments joined) and extract_records (the reads request, segments as they
    are) share one rule for the index of a region decode and leave the same account of it in LAST_DECODE."""
    import shutil
    path, regions = str(tmp_path / "p.bam"), [("chr8", 1_300_000, 1_300_500)]
    shutil.copyfile(case["plain"], path)

    def both(**kw):
        left = []
        for call in (bam.window_coverage, bam.extract_records):
            call(path, regions, device="cpu", **kw)
            left.append((bam.LAST_DECODE["index"], bam.LAST_DECODE.get("index_skipped"), bam.LAST_DECODE.get("spans")))
        assert left[0] == left[1], (kw, left)
        return left[0]
    assert both() == (None, None, None)                                           # no index beside the file
    bam.build_index(path, device="cpu")
    used = both()
    assert used[:2] == (path + ".bai", None) and used[2] >= 1                     # an index beside the file
    assert both(index=False) == (None, None, None)
    assert both(world=2) == (None, None, None)                                    # the default one is not looked for
    os.utime(path + ".bai", (1, 1))                                               # an index older than the file
    skipped = both()
    assert skipped[0] is None and "older" in skipped[1] and skipped[2] is None
    assert both(index=False) == (None, None, None) and both(world=2) == (None, None, None)
    for call in (bam.window_coverage, bam.extract_records):                       # a given index does not go with a sharded decode
        with pytest.raises(ValueError, match="not sharded"):
            call(path, regions, device="cpu", index=path + ".bai", world=2)


def test_cli_index_subcommand(case, cpu, tmp_path, capsys):
    from coral_amd import CoRAL
    out = CoRAL.main(["index", "--lr_bam", case["plain"], "--index", str(tmp_path / "cli.bai"), "--device", "cpu"])
    assert out == str(tmp_path / "cli.bai") and open(out, "rb").read() == restated_index(case["plain"])
    assert "Wrote" in capsys.readouterr().out


# ---- GPU twins ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_index_equals_host_and_restatement(case):
    want = restated_index(case["small"])
    assert index_bytes(case["small"], "cuda:0") == want                           # one batch
    assert index_bytes(case["small"], "cuda:0", batch_bytes=1 << 20) == want      # records and runs straddle the batches
    assert bam.LAST_DECODE["batches"] > 2
    with open(bam.build_index(case["small"], str(case["dir"] / "host.bai"), device="cpu"), "rb") as fp:
        assert fp.read() == want                                                  # ... and the host pipeline's bytes
    assert index_bytes(case["plain"], "cuda:0") == restated_index(case["plain"])
    for world in (2, 3, 5):
        assert index_bytes(case["small"], "cuda:0", world=world) == want, world


@pytest.mark.gpu
def test_gpu_index_spec_properties_and_unsorted(case, tmp_path):
    out = bam.build_index(case["small"], str(tmp_path / "props.bai"), device="cuda:0", batch_bytes=1 << 20)
    check_spec_properties(out, case["small"])
    path = str(tmp_path / "unsorted.bam")
    bam.write_bam(swap_two_records(synth.generate(synth.scaled_config("tiny", 120), "cpu")), path, seed=2, fast_seq=True, block_size=3000)
    with pytest.raises(_lib.CoralHipError, match="coordinate order"):
        bam.build_index(path, device="cuda:0")
    assert not os.path.exists(path + ".bai")


@pytest.mark.gpu
def test_gpu_region_decode_is_complete(case):
    bam.build_index(case["small"], device="cuda:0")
    regions = query_regions(case)
    check_region_decode(case, "cuda:0", [[r] for r in regions] + [regions[:9], regions])
    straddle_check(case, "cuda:0")


@pytest.mark.gpu
def test_gpu_window_coverage_through_the_index(case):
    coverage_checks(case, "cuda:0")
    coverage_checks(case, "cuda:0", thresholds=(7,), batch_bytes=1 << 20)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny_region", "tiny_edge_region", "ultra"])
def test_gpu_coverage_table_on_an_indexed_bam(name, golden_dir, tmp_path, capsys):
    from coral_amd import CoRAL
    gold, rec, graph, want = _plot_case(golden_dir, name, tmp_path)
    path = str(tmp_path / "r.bam")
    bam.write_bam_native(rec, path, seed=4, n_threads=4)
    assert CoRAL.main(["index", "--lr_bam", path]) == path + ".bai"                # the CLI, on the GPU
    with open(path + ".bai", "rb") as fp:
        assert fp.read() == restated_index(path)
    table = plot_coverage.CoverageTable.from_bam(path, graph, gold["region"], min_mapq=0, device="cuda:0")
    assert bam.LAST_DECODE["index"] == path + ".bai" and bam.LAST_DECODE["where"] == "gpu"
    for c, a, b, tot in want:
        assert sum(sum(x) for x in table.count_coverage(c, a, b, quality_threshold=0, read_callback="nofilter")) == tot
    golden_windows_every_threshold(path, want, "cuda:0")
