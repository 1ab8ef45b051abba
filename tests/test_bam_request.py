"""The request of a BAM decode (coral_bam_request_t): one struct says what a decode of either pipeline is asked for - a byte
range or spans, and the window coverage, the BAI index and the read QC that ride along.  Both pipelines parse it with the same
code (coral_bam_common.h: parse_request), so they accept and refuse the same requests, and what rides along is the same whether it
is asked for alone or together."""
import ctypes as C
import os

import numpy as np
import pytest

from coral_amd import _lib, bam
from tests.decode_support import (CORAL_ERR_ARG, CORAL_OK, DEVICE, PIPELINES, assert_qc_equals_restatement as assert_equal,
                                  assert_same_qc as assert_same, assert_same_records, gpu_decode_started, gpu_open_only, read_qc_case)

WINDOWS = [("chr8", 149_000, 152_000), ("chr8", 150_000, 150_100), ("chr8", 0, 1 << 28)]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return read_qc_case(tmp_path_factory.mktemp("bam_request"))


def segments(case):
    return bam.coverage_segments(WINDOWS, case["rec"].header_chroms)[0]


def assert_same_index(a, b):
    assert set(a) == set(b)
    for k, v in b.items():
        assert np.array_equal(a[k], v), k


# ---- host pipeline -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_threads", [1, 2])
def test_host_three_requests_at_once(case, n_threads):
    segs = segments(case)
    decode = lambda **kw: bam._decode(case["path"], "cpu", n_threads=n_threads, **kw)
    alone_cov = decode(coverage=(segs, 20, 0), records=False).counts
    alone_idx = decode(index=True, records=False).index
    alone_qc = decode(qc=True, records=False).qc
    got = decode(coverage=(segs, 20, 0), index=True, qc=True)
    assert alone_cov.sum() > 0 and np.array_equal(got.counts, alone_cov)
    assert_same_index(got.index, alone_idx)
    assert_same(got.qc, alone_qc)
    assert_equal(got.qc, case["want"])
    assert_same_records(got.records, bam.decode_bam(case["path"], n_threads=n_threads))


def bad_requests(case):
    """name -> (arguments of _lib.bam_request, a word of the message)"""
    V = lambda block, off=0: (block << 16) | off
    size = os.path.getsize(case["path"])
    assert size > 4000
    segs = segments(case)
    assert segs.shape[1] >= 2
    return {
        "rank >= world": (dict(rank=2, world=2), "rank"),
        "spans out of order": (dict(spans=[[V(3000), V(4000)], [V(1000), V(2000)]]), "sorted"),
        "overlapping spans": (dict(spans=[[V(1000), V(3000)], [V(2000), V(4000)]]), "disjoint"),
        "an empty span": (dict(spans=[[V(1000, 7), V(1000, 7)]]), "non-empty"),
        "a span beyond the file": (dict(spans=[[V(size + 5), V(size + 9)]]), "outside the file"),
        "unsorted segments": (dict(coverage=(segs[:, ::-1], 20, 0)), "sorted"),
        "quality threshold above 255": (dict(coverage=(segs, 256, 0)), "threshold"),
        "quality threshold below 0": (dict(coverage=(segs, -1, 0)), "threshold"),
        "index request with spans": (dict(spans=[[V(1000), V(2000)]], index=True), "span decode"),
        "read-QC request with spans": (dict(spans=[[V(1000), V(2000)]], qc=True), "span decode"),
    }


def test_host_refuses_bad_requests(case):
    L = _lib.lib()
    for name, (kw, word) in bad_requests(case).items():
        req, h = _lib.bam_request(**kw), C.c_void_p()
        rc = L.coral_bam_decode_request(case["path"].encode(), 1, C.byref(req), C.byref(h))
        assert rc == CORAL_ERR_ARG and h.value is None, name
        assert word in L.coral_bam_last_error().decode(), name


# ---- every request that may ride together, in one decode ----------------------------------------------------------------------
PILE_WINDOWS = [("chr8", 149_000, 152_000), ("chr8", 150_000, 150_100), ("chr8", 440_000, 451_000)]      # (the last: the 300 kb read's end)
DEPTH = (1000, 0, 0x704, 1)
SORTED_RECORDS = (0, None, None, 2, 1)                           # every record's own bytes, in coordinate order


def maximal_sets(case):
    """The two largest sets of requests one decode accepts -> (name -> each request's own arguments, records wanted).  The reads
    request does not ride with the index, counts and pileup are the two forms of the one coverage request."""
    chroms = case["rec"].header_chroms
    pile_segs = bam.coverage_segments(PILE_WINDOWS, chroms)[0]
    return [(dict(counts=dict(coverage=(segments(case), 20, 0)), qc=dict(qc=True), depth=dict(depth=DEPTH), index=dict(index=True)), True),
            (dict(reads=dict(reads=SORTED_RECORDS), pileup=dict(coverage=(pile_segs, 20, 0), per_base=True), qc=dict(qc=True),
                  depth=dict(depth=DEPTH)), False)]


def assert_same_result(got, want, name, what):
    if name in ("counts", "pileup"):
        assert want.counts.sum() > 0 and np.array_equal(got.counts, want.counts), what
    if name == "pileup":
        assert got.pileup.dtype == want.pileup.dtype and np.array_equal(got.pileup, want.pileup), what
    if name == "qc":
        assert_same(got.qc, want.qc, what)
    if name == "index":
        assert_same_index(got.index, want.index)
    if name in ("depth", "reads"):
        a, b = getattr(got, name), getattr(want, name)
        assert len(a) == len(b) and len(b[-1]) > 0, what
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x, y), what
    if name == "records":
        assert_same_records(got.records, want.records)


@pytest.fixture(scope="module")
def host_alone(case):
    """Every request of the two sets decoded alone on the host pipeline, once."""
    out = {"records": bam._decode(case["path"], "cpu", n_threads=2)}
    for requests, _ in maximal_sets(case):
        for name, kw in requests.items():
            if name not in out:
                out[name] = bam._decode(case["path"], "cpu", n_threads=2, records=False, **kw)
    return out


@pytest.mark.parametrize("pipe", PIPELINES)
def test_maximal_request_sets_equal_each_request_alone(case, host_alone, pipe):
    """What rides along shares the per-record scratch of the parse; a result must not depend on what else rides.  Each of the two
    maximal sets in one decode: every result bit-equal to that request decoded alone on the same pipeline, and to the host's."""
    for batch in ((0, 1 << 20) if pipe == "gpu" else (0,)):
        decode = lambda **kw: bam._decode(case["path"], DEVICE[pipe], n_threads=2, batch_bytes=batch, **kw)
        alone = dict(host_alone) if pipe == "host" else {"records": decode()}
        for requests, records in maximal_sets(case):
            together = decode(records=records, **{k: v for kw in requests.values() for k, v in kw.items()})
            if pipe == "gpu":
                assert bam.LAST_DECODE["where"] == "gpu" and (batch == 0 or bam.LAST_DECODE["batches"] >= 3)
            for name, kw in list(requests.items()) + ([("records", {})] if records else []):
                if name not in alone:
                    alone[name] = decode(records=False, **kw)
                what = "%s, batch_bytes %d, with %s" % (name, batch, "+".join(requests))
                assert_same_result(together, alone[name], name, what)
                assert_same_result(together, host_alone[name], name, what + " (host)")
            assert (together.records is None) == (not records)


# ---- GPU pipeline --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_refuses_the_same_requests(case):
    L = _lib.lib()
    for name, (kw, word) in bad_requests(case).items():
        rc, h, ws_bytes, message = gpu_open_only(case["path"], **kw)
        assert rc == CORAL_ERR_ARG and h is None and ws_bytes == 0, name
        assert word in message, name


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [0, 1 << 20])
def test_gpu_coverage_from_the_workspace_equals_host(case, batch):
    segs = segments(case)
    S = segs.shape[1]
    want = bam._decode(case["path"], "cpu", coverage=(segs, 20, 0), records=False).counts
    bam.decode_bam_gpu(case["path"], "cuda:0", batch_bytes=batch)
    plain_bytes = bam.LAST_DECODE["workspace_bytes"]
    got = bam._decode(case["path"], "cuda:0", batch_bytes=batch, coverage=(segs, 20, 0), records=False)
    assert want.sum() > 0 and got.counts.dtype == np.int64 and np.array_equal(got.counts, want)
    assert bam.LAST_DECODE["where"] == "gpu" and (batch == 0 or bam.LAST_DECODE["batches"] >= 3)
    up256 = lambda n: (n + 255) & ~255
    assert bam.LAST_DECODE["workspace_bytes"] == plain_bytes + up256(3 * S * 4) + up256(S * 8)      # segments and counters live there
    if batch == 0:                                               # an empty table: an empty result, nothing more in the workspace
        none = bam._decode(case["path"], "cuda:0", coverage=(np.zeros((3, 0), dtype=np.int32), 20, 0), records=False)
        assert none.counts.dtype == np.int64 and none.counts.shape == (0,) and none.records is None
        assert bam.LAST_DECODE["workspace_bytes"] == plain_bytes


@pytest.mark.gpu
def test_gpu_finish_before_the_last_batch_is_refused(case):
    """A state check, on a decode that then goes on to its end: the refusals change nothing."""
    L = _lib.lib()
    segs = segments(case)
    want = bam._decode(case["path"], "cpu", coverage=(segs, 20, 0), records=False).counts
    with gpu_decode_started(case["path"], 2, 1 << 20, coverage=(segs, 20, 0)) as d:
        h, stream = d.h, d.stream

        def refused():
            return L.coral_bamgpu_finish(h, stream) == CORAL_ERR_ARG and "not finished" in L.coral_bam_last_error().decode()
        assert refused()                                         # no batch has been parsed
        while d.next() is not None:
            assert refused()                                     # a batch is between next and emit
            d.emit()
        assert d.batches >= 3
        dh, counts = d.finish(), np.zeros(segs.shape[1], dtype=np.int64)
        assert L.coral_bam_coverage_result(dh, len(counts), counts.ctypes.data) == CORAL_OK
        assert np.array_equal(counts, want)
