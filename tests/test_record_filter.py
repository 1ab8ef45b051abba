"""The record filter of the BAM decode (bam.RecordFilter, keep_* of a coral_bam_request_t): every result of a filtered decode equals
the result of the same request on a BAM file that holds only the kept records, in the same order - on both pipelines, for small
batches, byte ranges and a batch whose records are all dropped.  The oracles are the unfiltered decode masked in numpy
(select_records) and a second file written from the kept records.  Everything is exact equality."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from coral_amd import CoRAL, _lib, bam, synth
from tests.bamfile import D, EQ, I, M, N, S, X, read_bam
from tests.decode_support import (CORAL_ERR_ARG, CORAL_OK, DEVICE, PIPELINES, _pipeline_by_device, assert_same_qc,  # noqa: F401
                                  assert_same_records as assert_same, concat_records as concat, gpu_open_only)

CHROMS, LENGTHS = ["ctgA", "ctgB", "ctgC"], [400_000, 300_000, 350_000]
BLOCK = 1500                                   # payload bytes per BGZF block: nearly every record straddles blocks
BATCH = 1 << 20                                # the smallest batch the GPU pipeline cuts (whatever smaller value is asked for)
N_REC = 320
RF = bam.RecordFilter
ALL_FOUR = RF(20, 100, 0x1, 0x400)
FILTERS = {
    "mapq": RF(min_mapq=20), "length": RF(min_seq_length=100), "require": RF(require_flags=0x1), "exclude": RF(exclude_flags=0x400),
    "all_four": ALL_FOUR, "keeps_nothing": RF(min_mapq=255, require_flags=0x8000), "keeps_everything": RF(0, 0, 0, 0x8000),
}


def mask_of(rec, f):
    """The rule, in numpy, on the columns of an unfiltered decode."""
    flag, mapq = rec.flag.numpy(), rec.mapq.numpy()
    l_seq = rec.has_seq.numpy() * rec.qlen.numpy()
    return (mapq >= f.min_mapq) & (l_seq >= f.min_seq_length) & ((flag & f.require_flags) == f.require_flags) & ((flag & f.exclude_flags) == 0)


# ---- test data -----------------------------------------------------------------------------------------------------------------
def cigar_of(i, n_ops, aligned):
    """n_ops ops (1 .. about 200) with about `aligned` aligned bases: M runs with small I / D / = / X ops between, clips around."""
    if n_ops == 1:
        return [(M, aligned)]
    ops = [(S, 3 + i % 5)]
    per = max(1, aligned // max(1, n_ops // 2))
    cycle = [(M, per), (I, 1 + i % 3), (EQ, per), (D, 2), (X, 1), (M, per), (N, 5)]
    while len(ops) < n_ops - 1:
        ops.append(cycle[(len(ops) - 1) % len(cycle)])
    return ops + [(M, 7)]


def klass_cycle(i):
    return i % 8


def alignment(i, klass, tid, pos, big=0):
    """Record i.  klass 0-3: passes ALL_FOUR; 4: only its mapq fails; 5: only its length fails (short SEQ, or none at all);
    6: only the required flag is missing; 7: only the excluded flag is set."""
    n_ops = 1 if big else (1, 2, 5, 17, 64, 65, 130, 201)[(i // 8 + i) % 8]
    aligned = big or (6000 + 531 * (i % 9))
    a = dict(tid=tid, pos=pos, cigar=cigar_of(i, n_ops, aligned), name="read%d" % i, nm=i % 11, flag=0x1 | (0x10 if i % 3 == 0 else 0),
             mapq=(60, 20, 25, 255)[i % 4])
    if klass == 1:
        a["flag"] |= 0x800
    if klass == 4:
        a["mapq"] = (19, 0)[(i // 8) % 2]
    if klass == 5:
        if (i // 8) % 2:
            a["has_seq"] = 0
        else:
            a["cigar"] = [(S, 4), (M, 90), (S, 5)]          # l_seq 99
    if klass == 6:
        a["flag"] &= ~0x1
    if klass == 7:
        a["flag"] |= 0x400
    if i % 16 == 1:
        a["name"] = "read%d" % (i - 1)                      # two kept records of one read
    if i % 16 == 8:
        a["name"] = "read%d" % (i - 4)                      # a read whose first record is dropped (klass 4) and whose second is kept
    if i % 5 == 0:
        a["sa"] = [(i % 3, 500 + i, i & 1, 10 + i % 7, 40 + i, (0, 3, -4)[i % 3], 5, 30, 2), (2, 9 + i, 0, 0, 77, 0, 12, 3, 1)][:1 + i % 2]
    if tid == 2 and i % 4 in (0, 2) and klass != 5:
        first = next(ln for op, ln in a["cigar"] if op != S)      # (the first op behind the soft clip is an M)
        a["nonacgt"] = [pos] + ([pos + 8] if first > 9 else [])      # an aligned N at the record's first and (for a longer M) 9th base
    return a


def build_records(n, klass, big_at=()):
    alns = []
    for i in range(n):
        tid = i * 3 // n
        alns.append(alignment(i, klass(i), tid, 1000 + 211 * (i - tid * n // 3), big=200_000 if i in big_at else 0))
    rec = synth.records_from_alignments(alns)
    rec.header_chroms, rec.header_lens = list(CHROMS), list(LENGTHS)
    return rec


def quality(rec):
    """i -> QUAL bytes of record i of `rec` (none for every 7th): a function of the record alone, not of its place in a file."""
    names, name_id, pos = rec.materialise_names(), rec.name_id.numpy(), rec.pos.numpy()
    l_seq = (rec.has_seq * rec.qlen).numpy()

    def q(i):
        key = int(names[name_id[i]][4:]) * 1_000_003 + int(pos[i])
        if key % 7 == 0:
            return b"\xff" * int(l_seq[i])
        return np.random.default_rng(key).integers(0, 45, int(l_seq[i]), dtype=np.uint8).tobytes()
    return q


def stream_layout(path):
    """(start, end) of every record in the file's uncompressed stream."""
    return [(r["start"], r["start"] + r["size"]) for r in read_bam(path).recs]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("record_filter")
    rec = build_records(N_REC, klass_cycle)
    a = str(d / "A.bam")
    bam.write_bam(rec, a, seed=5, block_size=BLOCK, qual=quality(rec))
    whole = bam.decode_bam(a, n_threads=2)
    mask = mask_of(whole, ALL_FOUR)
    kept = bam.select_records(rec, mask)
    b = str(d / "B.bam")
    bam.write_bam(kept, b, seed=5, block_size=BLOCK, qual=quality(kept))
    return dict(dir=d, rec=rec, A=a, B=b, whole=whole, mask=mask)


def test_the_file_is_what_the_tests_need(case):
    whole = case["whole"]
    assert_same(case["rec"], whole)
    masks = {k: mask_of(whole, f) for k, f in FILTERS.items()}
    alone = {k: ~masks[k] for k in ("mapq", "length", "require", "exclude")}
    for k, dropped in alone.items():                         # each of the four tests alone decides some records
        others = np.logical_and.reduce([masks[o] for o in alone if o != k])
        assert (dropped & others).sum() >= 10, k
    assert 0 < masks["all_four"].sum() < whole.n and masks["keeps_nothing"].sum() == 0 and masks["keeps_everything"].all()
    assert ((whole.has_seq.numpy() == 0) & ~masks["length"]).sum() > 0
    n_cigar = whole.n_cigar.numpy()
    assert n_cigar.min() == 1 and n_cigar.max() >= 200 and len(set(whole.tid.tolist())) == 3
    na = whole.nonacgt_rec.numpy()
    assert masks["all_four"][na].any() and (~masks["all_four"][na]).any()
    name_id, m = whole.name_id.numpy(), masks["all_four"]
    first_seen = {}
    for i, k in enumerate(name_id.tolist()):
        first_seen.setdefault(k, i)
    assert any(m[i] and not m[first_seen[k]] for i, k in enumerate(name_id.tolist()))      # a kept record of a read first seen in a dropped one
    layout = stream_layout(case["A"])
    assert len(layout) == whole.n and layout[-1][1] > 2 * BATCH                             # three batches or more
    assert sum(s // BLOCK != (e - 1) // BLOCK for s, e in layout) > whole.n // 2            # records straddle BGZF blocks


# ---- 1. the records ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FILTERS))
@pytest.mark.parametrize("pipe", PIPELINES)
def test_records_equal_the_masked_decode(case, pipe, name):
    f = FILTERS[name]
    whole = bam.load_bam(case["A"], DEVICE[pipe], n_threads=2)
    want = bam.select_records(whole, mask_of(whole, f))
    got = bam.load_bam(case["A"], DEVICE[pipe], n_threads=2, record_filter=f)
    assert_same(want, got)
    assert_same(want, bam.load_bam(case["A"], DEVICE[pipe], n_threads=3, record_filter=tuple(f)))      # a plain 4-tuple serves as well
    if pipe == "gpu":
        assert bam.LAST_DECODE["where"] == "gpu"
        small = bam.decode_bam_gpu(case["A"], "cuda:0", batch_bytes=1 << 16, record_filter=f)
        assert bam.LAST_DECODE["batches"] >= 3
        assert_same(want, small)


@pytest.mark.parametrize("pipe", PIPELINES)
def test_regions_with_a_filter(case, pipe):
    """The filter in the span decode, the region mask on the host afterwards."""
    bam.build_index(case["A"], device="cpu")
    regions = [("ctgA", 5000, 9000), ("ctgC", 2000, 4000)]
    whole = bam.load_bam(case["A"], DEVICE[pipe], regions=regions)
    got = bam.load_bam(case["A"], DEVICE[pipe], regions=regions, record_filter=ALL_FOUR)
    assert 0 < got.n < whole.n
    assert_same(bam.select_records(whole, mask_of(whole, ALL_FOUR)), got)


# ---- 2. the file of the kept records -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", PIPELINES)
def test_results_equal_those_of_the_file_of_kept_records(case, pipe):
    dev = DEVICE[pipe]
    assert_same(bam.load_bam(case["B"], dev), bam.load_bam(case["A"], dev, record_filter=ALL_FOUR))
    for params in ((1000, 0, 0x704, True), (7, 25, 0x10, False)):
        got, want = bam.binned_depth(case["A"], *params, device=dev, record_filter=ALL_FOUR), bam.binned_depth(case["B"], *params, device=dev)
        plain = bam.binned_depth(case["A"], *params, device=dev)
        assert np.array_equal(got.bin_off, want.bin_off) and np.array_equal(got.all_bases, want.all_bases) and np.array_equal(got.all_reads, want.all_reads)
        assert 0 < got.all_bases.sum() < plain.all_bases.sum()                              # the depth's own rules apply on top of the filter
    got, want, plain = bam.read_qc(case["A"], device=dev, record_filter=ALL_FOUR), bam.read_qc(case["B"], device=dev), bam.read_qc(case["A"], device=dev)
    assert_same_qc(got, want)
    assert got.n_records == int(case["mask"].sum()) < plain.n_records and 0 < got.n_no_qual < got.n_reads
    windows = [(c, a, min(a + 5000, 90_000)) for c in CHROMS[:2] for a in range(0, 90_000, 5000)] + [("ctgA", 1000, 60_000)]
    for thr, cb in ((0, "nofilter"), (10, "nofilter"), (30, "all")):
        got = bam.window_coverage(case["A"], windows, thr, cb, device=dev, index=False, record_filter=ALL_FOUR)
        want = bam.window_coverage(case["B"], windows, thr, cb, device=dev, index=False)
        assert np.array_equal(got, want) and 0 < got.sum() < bam.window_coverage(case["A"], windows, thr, cb, device=dev, index=False).sum()
    if pipe == "gpu":                                        # and with small batches
        got = bam._decode(case["A"], dev, batch_bytes=1 << 16, qc=True, depth=(1000, 0, 0x704, 1), records=False, record_filter=ALL_FOUR)
        assert bam.LAST_DECODE["batches"] >= 3
        want = bam.binned_depth(case["B"], device=dev)
        assert np.array_equal(got.depth[1], want.all_bases) and np.array_equal(got.depth[2], want.all_reads)
        assert_same_qc(got.qc, bam.read_qc(case["B"], device=dev))


# ---- 3. pileup -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", PIPELINES)
def test_pileup_splits_by_flag_and_sums_to_window_coverage(case, pipe):
    dev = DEVICE[pipe]
    regions = [("ctgA", 0, 40_000), ("ctgB", 500, 30_000), ("ctgC", 0, 20_000)]
    for thr in (0, 12):
        both = bam.pileup(case["A"], regions, thr, "nofilter", device=dev, index=False)
        fwd = bam.pileup(case["A"], regions, thr, "nofilter", device=dev, index=False, record_filter=RF(exclude_flags=0x10))
        rev = bam.pileup(case["A"], regions, thr, "nofilter", device=dev, index=False, record_filter=RF(require_flags=0x10))
        assert fwd.table.sum() > 0 and rev.table.sum() > 0
        assert np.array_equal(fwd.table.astype(np.int64) + rev.table, both.table)
        for f, p in ((RF(exclude_flags=0x10), fwd), (RF(require_flags=0x10), rev)):
            cov = bam.window_coverage(case["A"], regions, thr, "nofilter", device=dev, index=False, record_filter=f)
            assert cov.tolist() == [int(p.depth(*r).sum()) for r in regions]


# ---- 4. a batch whose records are all dropped ----------------------------------------------------------------------------------
N_RUN, RUN_LO, RUN_HI = 430, 92, 389           # records RUN_LO < i < RUN_HI fail the filter (mapq); RUN_LO and RUN_HI are large and kept


def klass_run(i):
    return 4 if RUN_LO < i < RUN_HI else (0, 1, 2, 3)[i % 4]


@pytest.fixture(scope="module")
def run_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("record_filter_run")
    rec = build_records(N_RUN, klass_run, big_at=(RUN_LO, RUN_HI))
    path = str(d / "run.bam")
    bam.write_bam(rec, path, seed=7, block_size=BLOCK)
    return dict(rec=rec, path=path)


def batch_of_record(path):
    """Per record the batch it is parsed in: the one that holds its last byte (batches are whole BGZF blocks, at most BATCH bytes)."""
    per_batch = (BATCH // BLOCK) * BLOCK
    return [(e - 1) // per_batch for _, e in stream_layout(path)], [s // per_batch for s, _ in stream_layout(path)]


def test_the_run_file_has_batches_without_a_kept_record(run_case):
    f = RF(min_mapq=20)
    mask = mask_of(run_case["rec"], f)
    done_in, starts_in = batch_of_record(run_case["path"])
    batches = set(done_in)
    with_kept = {b for b, m in zip(done_in, mask) if m}
    empty = sorted(batches - with_kept)
    assert len(empty) >= 2 and empty == list(range(empty[0], empty[-1] + 1))
    # a kept record straddles a batch boundary into the run, another one out of it
    assert mask[RUN_LO] and starts_in[RUN_LO] < done_in[RUN_LO] == empty[0] - 1
    assert mask[RUN_HI] and starts_in[RUN_HI] == empty[-1] and done_in[RUN_HI] == empty[-1] + 1


@pytest.mark.gpu
def test_a_batch_whose_records_are_all_dropped(run_case):
    f = RF(min_mapq=20)
    whole = bam.decode_bam_gpu(run_case["path"], "cuda:0", batch_bytes=1 << 16)
    assert_same(run_case["rec"], whole)
    mask = mask_of(whole, f)
    want = bam.select_records(whole, mask)
    got = bam.decode_bam_gpu(run_case["path"], "cuda:0", batch_bytes=1 << 16, record_filter=f)
    done_in, _ = batch_of_record(run_case["path"])
    assert bam.LAST_DECODE["batches"] >= len(set(done_in)) > len({b for b, m in zip(done_in, mask) if m}) + 1
    assert_same(want, got)
    assert_same(want, bam.decode_bam(run_case["path"], n_threads=2, record_filter=f))
    res = bam._decode(run_case["path"], "cuda:0", batch_bytes=1 << 16, qc=True, depth=(1000, 0, 0, 1), coverage=(np.array([[0], [0], [200_000]], dtype=np.int32), 0, 0),
                      record_filter=f)
    host = bam._decode(run_case["path"], "cpu", qc=True, depth=(1000, 0, 0, 1), coverage=(np.array([[0], [0], [200_000]], dtype=np.int32), 0, 0), record_filter=f)
    assert_same(want, res.records)
    assert_same_qc(res.qc, host.qc)
    assert res.counts.tolist() == host.counts.tolist() and res.counts[0] > 0 and all(np.array_equal(x, y) for x, y in zip(res.depth, host.depth))


# ---- 5. byte ranges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", PIPELINES)
def test_byte_ranges_with_a_filter(case, pipe):
    dev = DEVICE[pipe]
    kw = dict(batch_bytes=1 << 16) if pipe == "gpu" else {}
    decode = lambda **k: bam._decode(case["A"], dev, n_threads=2, depth=(1000, 0, 0x704, 1), record_filter=ALL_FOUR, **kw, **k)
    whole = decode()
    parts = [decode(rank=r, world=3) for r in range(3)]
    assert sum(p.records.n > 0 for p in parts) >= 2 and sum(p.records.n for p in parts) == whole.records.n == int(case["mask"].sum())
    got, want = concat([p.records for p in parts]), concat([whole.records])
    assert set(got) == set(want)
    for k, v in want.items():
        assert list(got[k]) == list(v) if k == "names" else np.array_equal(got[k], v), k
    for t in (1, 2):
        assert np.array_equal(sum(p.depth[t] for p in parts), whole.depth[t]) and whole.depth[t].sum() > 0
    assert_same(bam.load_bam(case["A"], dev, rank=1, world=3, record_filter=ALL_FOUR), parts[1].records)


# ---- 6. a malformed tag in a dropped record --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bad_tag_case(tmp_path_factory):
    """A tag of an unknown type ('Q') in front of NM in three records that fail min_mapq = 20."""
    d = tmp_path_factory.mktemp("record_filter_bad_tag")
    rec = build_records(48, klass_cycle)
    bad = [i for i in range(48) if klass_cycle(i) == 4][1:4]
    path, clean = str(d / "bad_tag.bam"), str(d / "clean.bam")
    bam.write_bam(rec, path, seed=3, block_size=BLOCK, aux=lambda i: (b"XXQ\x01\x02\x03\x04" if i in bad else b"", b""))
    bam.write_bam(rec, clean, seed=3, block_size=BLOCK)
    return dict(path=path, clean=clean, bad=bad, rec=rec)


def test_malformed_tag_in_a_dropped_record_host(bad_tag_case):
    f = RF(min_mapq=20)
    mask = mask_of(bad_tag_case["rec"], f)
    assert not mask[bad_tag_case["bad"]].any()
    with pytest.raises(_lib.CoralHipError, match="unknown tag type") as e:                   # unfiltered: a format error, as before
        bam.decode_bam(bad_tag_case["path"], n_threads=2)
    assert "(-4)" in str(e.value)                                                         # CORAL_ERR_FORMAT
    with pytest.raises(_lib.CoralHipError, match="unknown tag type"):                       # ... and when the filter keeps such a record
        bam.decode_bam(bad_tag_case["path"], n_threads=2, record_filter=RF(min_seq_length=100))
    got = bam.decode_bam(bad_tag_case["path"], n_threads=2, record_filter=f)
    assert_same(bam.select_records(bam.decode_bam(bad_tag_case["clean"]), mask), got)


@pytest.mark.gpu
def test_malformed_tag_in_a_dropped_record_gpu(bad_tag_case):
    """The GPU pipeline never walks the tags of the dropped records: the filtered decode succeeds and equals the host pipeline's.
    (The unfiltered decode of this file is asserted on the host pipeline only: no existing decoder test feeds a malformed tag to
    the GPU pipeline, and this file adds none.)"""
    f = RF(min_mapq=20)
    got = bam.decode_bam_gpu(bad_tag_case["path"], "cuda:0", record_filter=f)
    assert bam.LAST_DECODE["where"] == "gpu"
    assert_same(bam.decode_bam(bad_tag_case["path"], n_threads=2, record_filter=f), got)
    assert got.n == int(mask_of(bad_tag_case["rec"], f).sum()) > 0


# ---- 7. argument rules, equal on both pipelines --------------------------------------------------------------------------------
BAD_REQUESTS = {
    "min_mapq < 0": (dict(keep=(-1, 0, 0, 0)), "keep_min_mapq"),
    "min_mapq > 255": (dict(keep=(256, 0, 0, 0)), "keep_min_mapq"),
    "min_seq_length < 0": (dict(keep=(0, -1, 0, 0)), "keep_min_seq_length"),
    "min_seq_length > 2^29": (dict(keep=(0, (1 << 29) + 1, 0, 0)), "keep_min_seq_length"),
    "require_flags < 0": (dict(keep=(0, 0, -1, 0)), "keep_require_flags"),
    "require_flags > 0xffff": (dict(keep=(0, 0, 0x10000, 0)), "keep_require_flags"),
    "exclude_flags < 0": (dict(keep=(0, 0, 0, -1)), "keep_exclude_flags"),
    "exclude_flags > 0xffff": (dict(keep=(0, 0, 0, 0x10000)), "keep_exclude_flags"),
    "with an index request": (dict(keep=(20, 0, 0, 0), index=True), "record filter does not go with an index request"),
}


def test_struct_ends_with_the_four_fields():
    names = [f[0] for f in _lib.coral_bam_request_t._fields_]
    assert names[-4:] == ["keep_min_mapq", "keep_min_seq_length", "keep_require_flags", "keep_exclude_flags"]
    req = _lib.bam_request(keep=RF(3, 4, 5, 6))
    assert (req.keep_min_mapq, req.keep_min_seq_length, req.keep_require_flags, req.keep_exclude_flags) == (3, 4, 5, 6)
    zero = _lib.bam_request()
    assert (zero.keep_min_mapq, zero.keep_min_seq_length, zero.keep_require_flags, zero.keep_exclude_flags) == (0, 0, 0, 0)


def test_host_refuses_bad_filters(case):
    L = _lib.lib()
    for name, (kw, word) in BAD_REQUESTS.items():
        req, h = _lib.bam_request(**kw), C.c_void_p()
        assert L.coral_bam_decode_request(case["A"].encode(), 1, C.byref(req), C.byref(h)) == CORAL_ERR_ARG and h.value is None, name
        assert word in L.coral_bam_last_error().decode(), name
    for keep in ((255, 1 << 29, 0xffff, 0xffff), (0, 0, 0, 0)):                              # the ends of the ranges are legal
        req, h = _lib.bam_request(keep=keep, qc=True, depth=(1000, 0, 0, 1), coverage=(np.zeros((3, 0), dtype=np.int32), 0, 0), per_base=True), C.c_void_p()
        assert L.coral_bam_decode_request(case["A"].encode(), 2, C.byref(req), C.byref(h)) == CORAL_OK, keep
        L.coral_bam_decode_close(h)
    req, h = _lib.bam_request(keep=(0, 0, 0, 0), index=True), C.c_void_p()                  # not active: goes with an index
    assert L.coral_bam_decode_request(case["A"].encode(), 2, C.byref(req), C.byref(h)) == CORAL_OK
    L.coral_bam_decode_close(h)


@pytest.mark.gpu
def test_gpu_refuses_the_same_filters(case):
    L = _lib.lib()
    torch.cuda.set_device(torch.device("cuda:0"))
    for name, (kw, word) in BAD_REQUESTS.items():
        rc, h, ws_bytes, message = gpu_open_only(case["A"], **kw)
        assert rc == CORAL_ERR_ARG and h is None and ws_bytes == 0, name
        assert word in message, name
    sizes = {}
    for key, keep in (("none", None), ("zero", (0, 0, 0, 0)), ("active", (20, 0, 0, 0))):   # open only: no GPU work
        rc, _, sizes[key], _ = gpu_open_only(case["A"], keep=keep)
        assert rc == CORAL_OK
    assert sizes["none"] == sizes["zero"] < sizes["active"]                                   # the second array of record starts


@pytest.mark.parametrize("kw", [dict(min_mapq=-1), dict(min_mapq=256), dict(min_seq_length=-1), dict(min_seq_length=(1 << 29) + 1),
                                dict(require_flags=-1), dict(require_flags=0x10000), dict(exclude_flags=-1), dict(exclude_flags=0x10000),
                                dict(min_mapq="20"), dict(min_seq_length=2.5), dict(exclude_flags=True)])
def test_record_filter_refuses_bad_values(kw):
    with pytest.raises(ValueError):
        RF(**kw)


def test_record_filter_object():
    f = RF(255, 1 << 29, 0xffff, 0xffff)
    assert f.active and tuple(f) == (255, 1 << 29, 0xffff, 0xffff) and f.min_seq_length == 1 << 29
    assert not RF().active and RF() == (0, 0, 0, 0) and RF(min_seq_length=1).active
    with pytest.raises(ValueError):
        bam.decode_bam("/no/such/file.bam", record_filter=(0, 0, 0, 0x10000))                 # checked before anything is opened
    with pytest.raises(TypeError):
        bam.build_index("/no/such/file.bam", record_filter=RF(1))                            # the index takes no filter
    with pytest.raises(TypeError):
        bam.index_partial("/no/such/file.bam", record_filter=RF(1))


# ---- 8. the command line ---------------------------------------------------------------------------------------------------------
FLAGS = ["--filter_min_mapq", "20", "--filter_min_length", "0x64", "--filter_require_flags", "1", "--filter_exclude_flags", "0x400"]


def test_parser_takes_the_filter_flags():
    parse = CoRAL.build_parser().parse_args
    a = parse(["depth", "--lr_bam", "x.bam", "--output", "o"] + FLAGS)
    assert bam.record_filter_from_args(a) == ALL_FOUR
    for argv in (["qc", "--lr_bam", "x", "--output_dir", "o"], ["pileup", "--lr_bam", "x", "--region", "c:1-2", "--output", "o"],
                 ["hsr", "--lr_bam", "x", "--cycles", "c", "--cn_seg", "s", "--output_prefix", "o", "--normal_cov", "1"],
                 ["reconstruct", "--lr_bam", "x", "--cnv_seed", "s", "--cn_seg", "c", "--output_prefix", "o"]):
        assert bam.record_filter_from_args(parse(argv + FLAGS)) == ALL_FOUR and not bam.record_filter_from_args(parse(argv)).active
    with pytest.raises(SystemExit):
        parse(["index", "--lr_bam", "x.bam"] + FLAGS[:2])

    class Old:                                               # an argument object from before the flags
        lr_bam = "x.bam"
    assert not bam.record_filter_from_args(Old()).active


@pytest.mark.parametrize("pipe", PIPELINES)
def test_cli_depth_and_qc_write_what_the_api_gives(case, pipe, tmp_path):
    out = str(tmp_path / "bins.cnn")
    assert CoRAL.main(["depth", "--lr_bam", case["A"], "--output", out, "--device", DEVICE[pipe], "--bin_size", "500"] + FLAGS) == out
    want = str(tmp_path / "want.cnn")
    bam.binned_depth(case["A"], 500, device=DEVICE[pipe], record_filter=ALL_FOUR).write(want)
    other = str(tmp_path / "file_b.cnn")
    bam.binned_depth(case["B"], 500, device=DEVICE[pipe]).write(other)
    assert open(out).read() == open(want).read() == open(other).read()
    CoRAL.main(["qc", "--lr_bam", case["A"], "--output_dir", str(tmp_path / "qc"), "--device", DEVICE[pipe], "--no_plots"] + FLAGS)
    qc = bam.read_qc(case["A"], device=DEVICE[pipe], record_filter=ALL_FOUR)
    assert open(tmp_path / "qc" / "quality_control_summary.tsv").read() == qc.summary_text()
    with open(tmp_path / "qc" / "read_qc.json") as fp:
        got = json.load(fp)
    assert got["counters"] == qc.counters and got["counters"]["n_records"] == int(case["mask"].sum()) and got["base_quality_hist"] == qc.base_quality_hist.tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("decode", ["cpu", "gpu"])
def test_cli_reconstruct_on_the_filtered_file(decode, tmp_path, monkeypatch):
    """`reconstruct` on a file with the flags writes the graph files it writes on the file of the kept records without them."""
    monkeypatch.setenv("CORAL_BAM_DECODE", decode)
    cfg = synth.named_config("tiny")
    rec = synth.generate(cfg, "cpu")
    mapq = rec.mapq.clone()
    mapq[torch.arange(rec.n) % 9 == 4] = 3                   # every 9th record fails --filter_min_mapq 20
    rec.mapq = mapq
    f = RF(min_mapq=20)
    mask = mask_of(rec, f)
    assert 0 < mask.sum() < rec.n
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    bam.write_bam_native(rec, a, seed=cfg.seed, n_threads=2)
    bam.write_bam_native(bam.select_records(rec, mask), b, seed=cfg.seed, n_threads=2)
    cn, seeds = str(tmp_path / "cn.bed"), str(tmp_path / "seeds.bed")
    synth.write_cn_bed(cfg, cn)
    synth.write_seed_bed(cfg, seeds)
    outs = {}
    for key, path, flags in (("a", a, ["--filter_min_mapq", "20"]), ("b", b, [])):
        os.makedirs(tmp_path / key)
        prefix = str(tmp_path / key / "out")
        CoRAL.main(["reconstruct", "--lr_bam", path, "--cnv_seed", seeds, "--cn_seg", cn, "--output_prefix", prefix, "--skip_cycle_decomp",
                    "--log_fn", str(tmp_path / (key + ".log"))] + flags)
        outs[key] = {n: open(tmp_path / key / n).read() for n in sorted(os.listdir(tmp_path / key))}
    assert outs["a"] and set(outs["a"]) == set(outs["b"]) and any(n.endswith("_graph.txt") for n in outs["a"])
    assert outs["a"] == outs["b"]
