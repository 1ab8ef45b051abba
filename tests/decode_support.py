"""What the BAM test modules share to drive the product: the pipeline selection, the record and QC comparisons, the GPU decode
driven through the C ABI, and the test data that more than one module decodes.  (The plain-Python reader the expectations come
from is tests/bamfile.py, which imports nothing from here or from coral_amd.)"""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

from coral_amd import _lib, bam, synth
from coral_amd.decode_session import DecodeSession, open_handle
from tests.bamfile import D, EQ, H, I, M, N, S, X, read_bam, restate_read_qc

PIPELINES = ["host", pytest.param("gpu", marks=pytest.mark.gpu)]
DEVICE = {"host": "cpu", "gpu": "cuda:0"}
CORAL_OK, CORAL_ERR_ARG = 0, -1
RECORD_FIELDS = ("tid", "pos", "end", "flag", "mapq", "qlen", "has_seq", "nm", "name_id", "n_cigar", "cigar_off", "cigar",
                 "sa_off", "sa", "sa_nm", "nonacgt_rec", "nonacgt_pos")


# ---- pipeline selection --------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _pipeline_by_device(monkeypatch):
    """The device alone chooses the pipeline.  Autouse in every module that imports it by name."""
    monkeypatch.delenv("CORAL_BAM_DECODE", raising=False)


@contextlib.contextmanager
def host_pipeline():
    """The host pipeline, whatever the device."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("CORAL_BAM_DECODE", "cpu")
        yield


@pytest.fixture()
def cpu():
    with host_pipeline():
        yield


# ---- comparisons ---------------------------------------------------------------------------------------------------------------
def assert_same_records(a, b):
    assert a.n == b.n
    for k in RECORD_FIELDS:
        x, y = getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()
        assert x.shape == y.shape and np.array_equal(x, y), k
    assert a.n_names == b.n_names and a.materialise_names() == b.materialise_names()
    assert a.header_chroms == b.header_chroms and a.header_lens == b.header_lens


def concat_records(parts):
    """Records of consecutive byte ranges put together again (read-name ids are local to a range: compare by name)."""
    out = {}
    for k in RECORD_FIELDS:
        if k not in ("cigar_off", "sa_off", "nonacgt_rec", "name_id"):
            out[k] = np.concatenate([getattr(p, k).cpu().numpy() for p in parts])
    out["n_cigar_padded"] = np.concatenate([np.diff(p.cigar_off.cpu().numpy()) for p in parts])
    out["sa_count"] = np.concatenate([np.diff(p.sa_off.cpu().numpy()) for p in parts])
    base, na = 0, []
    for p in parts:
        na.append(p.nonacgt_rec.cpu().numpy() + base)
        base += p.n
    out["nonacgt_rec"] = np.concatenate(na)
    out["names"] = [p.names[i] for p in parts for i in p.name_id.tolist()]
    return out


def assert_same_qc(a, b, what=""):
    for k in ("length", "qual_sum", "mapq", "flag", "base_quality_hist"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), (what, k)
    assert a.counters == b.counters, what


def assert_qc_equals_restatement(got, want, what=""):
    """A bam.ReadQC against bamfile.restate_read_qc of the same file."""
    for k in ("length", "qual_sum", "mapq", "flag"):
        a = getattr(got, k)
        assert a.dtype == want[k].dtype and np.array_equal(a, want[k]), (what, k)
    assert got.base_quality_hist.dtype == np.int64 and np.array_equal(got.base_quality_hist, want["hist"]), what
    assert got.counters == want["counters"], what
    for k, v in want["counters"].items():
        assert getattr(got, k) == v


# ---- the GPU decode through the C ABI ------------------------------------------------------------------------------------------
def _ok(L, step, rc):
    assert rc == CORAL_OK, "%s: %d, %s" % (step, rc, L.coral_bam_last_error().decode())


def gpu_open_only(path, n_threads=1, batch_bytes=0, sink=None, **request):
    """decode_session.open_handle alone (no GPU work) -> (rc, handle, ws_bytes, message); a handle that was granted is closed."""
    L, req = _lib.lib(), _lib.bam_request(**request)
    rc, h, ws_bytes = open_handle(L, path, n_threads, batch_bytes, req, sink)
    message = L.coral_bam_last_error().decode()
    if h.value is not None:
        L.coral_bamgpu_close(h)
    return rc, h.value, ws_bytes, message


@contextlib.contextmanager
def gpu_decode_started(path, n_threads=2, batch_bytes=0, sink=None, **request):
    """A GPU decode opened and started, closed on every way out: yields the DecodeSession (L, h, stream, dev, ws_bytes, pieces;
    its rules are the class's), on which the caller steps next() / emit()."""
    with DecodeSession(path, _lib.bam_request(**request), device="cuda:0", n_threads=n_threads, batch_bytes=batch_bytes, sink=sink) as d:
        d.start()
        yield d


@contextlib.contextmanager
def gpu_decode(path, n_threads=2, batch_bytes=0, sink=None, **request):
    """A whole GPU decode: every batch parsed and emitted, finished; yields what gpu_decode_started yields, with dh (the host
    handle that the coral_bam_*_result calls take) and batches."""
    with gpu_decode_started(path, n_threads, batch_bytes, sink, **request) as d:
        d.run()
        d.finish()
        yield d


# ---- the inflate kernel alone (tests/test_bam_gpu.py, tests/test_inflate_streams_gpu.py) --------------------------------------
def inflate_on_gpu(pairs, pad=0):
    """One coral_bgzf_inflate launch over all streams (stream k starts `pad + k % 4` bytes after the previous one: every
    alignment of input and output occurs)."""
    L = _lib.lib()
    comp, desc, o_in, o_out = bytearray(), [], 0, 0
    for k, (c, d) in enumerate(pairs):
        gap = pad + (k % 4)
        comp += b"\xaa" * gap
        o_in += gap
        o_out += k % 3
        desc.append((o_in, len(c), o_out, len(d)))
        comp += c
        o_in += len(c)
        o_out += len(d)
    comp += bytes(4096)
    dev = "cuda:0"
    t_comp = torch.frombuffer(bytearray(comp), dtype=torch.uint8).to(dev)
    t_desc = torch.tensor(desc, dtype=torch.int64).to(torch.int32).contiguous().to(dev)      # (values < 2^31)
    t_out = torch.full((o_out + 64,), 0x55, dtype=torch.uint8, device=dev)
    t_status = torch.full((len(pairs),), -1, dtype=torch.int32, device=dev)
    rc = L.coral_bgzf_inflate(t_comp.data_ptr(), t_desc.data_ptr(), len(pairs), t_out.data_ptr(), t_status.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.coral_bam_last_error()
    torch.cuda.synchronize()
    return t_out.cpu().numpy().tobytes(), t_status.cpu().tolist(), desc


# ---- test data of tests/test_bam_io.py, decoded again by test_bam_gpu.py -------------------------------------------------------
def odd_io_records():
    big = [(M, 3), (I, 1)] * 33000 + [(M, 5)]            # 66001 ops -> CG tag path
    return synth.records_from_alignments([
        dict(tid=0, pos=100, cigar=[(S, 5), (M, 50), (D, 700), (M, 20), (I, 3), (M, 10)], name="a", nm=7,
             sa=[(7, 1000, 1, 10, 2000, -30, 55, 60, 12), (11, 5, 0, 0, 300, 4, 9000, 3, 0)], nonacgt=[101, 860]),
        dict(tid=0, pos=120, cigar=[(H, 9), (EQ, 10), (X, 2), (N, 900), (M, 30), (H, 7)], name="b", flag=2064, mapq=0),
        dict(tid=0, pos=130, cigar=[], flag=4, name="c", qlen=40),
        dict(tid=0, pos=180, cigar=[(M, 200)], has_seq=0, flag=256, name="a"),
        dict(tid=3, pos=7, cigar=big, name="long"),
        dict(tid=24, pos=16000, cigar=[(M, 500)], name="mito"),
    ])


# ---- test data of tests/test_window_coverage.py, indexed again by test_bam_index.py --------------------------------------------
def coverage_odd_records():
    """Hand-written records: the flags the 'all' callback drops, no SEQ, N bases, an unmapped read with a CIGAR, a CIGAR of
    more than 65 535 ops (CG tag), soft / hard clips, =, X, D, N."""
    big = [(M, 3), (I, 1), (D, 2)] * 22000 + [(M, 5)]            # 66001 ops -> CG tag
    return synth.records_from_alignments([
        dict(tid=7, pos=150_000, cigar=[(S, 5), (M, 50), (D, 70), (M, 20), (I, 3), (M, 10)], name="a", nonacgt=[150_001, 150_140]),
        dict(tid=7, pos=150_010, cigar=[(H, 9), (EQ, 10), (X, 2), (N, 90), (M, 30), (H, 7)], name="b", flag=0x10),
        dict(tid=7, pos=150_020, cigar=[(M, 60)], flag=4, name="c"),
        dict(tid=7, pos=150_030, cigar=[(M, 200)], has_seq=0, flag=256, name="a"),
        dict(tid=7, pos=150_040, cigar=[(M, 120)], flag=256, name="d"),
        dict(tid=7, pos=150_050, cigar=[(M, 80), (I, 4), (M, 40)], flag=0x400, name="e", nonacgt=[150_060]),
        dict(tid=7, pos=150_060, cigar=[(S, 3), (M, 90)], flag=0x200, name="f"),
        dict(tid=7, pos=150_070, cigar=big, name="long"),
        dict(tid=7, pos=400_000, cigar=[(M, 500)], flag=0x800, name="g"),
        dict(tid=24, pos=16000, cigar=[(M, 500)], name="mito"),
    ])


def coverage_windows(rec, seed=3):
    """Random windows where the reads are (overlapping ones included), the plot's own window shape, windows at both ends of
    chr8 and chrM, a window on a contig without reads, empty windows."""
    rng = np.random.default_rng(seed)
    tid, pos, end = (getattr(rec, k).numpy() for k in ("tid", "pos", "end"))
    chroms, lens = rec.header_chroms, rec.header_lens
    out = []
    for k in rng.choice(rec.n, 60):
        a = int(pos[k]) + int(rng.integers(-300, 300))
        out.append((chroms[tid[k]], max(a, 0), max(a, 0) + int(rng.choice([1, 37, 150, 1000, 25_000]))))
    out += [("chr8", 150_000 + 150 * k, 150_000 + 150 * (k + 1)) for k in range(8)]
    out += [("chr8", 150_000, 151_000), ("chr8", 150_100, 150_250), ("chr8", 150_100, 150_250)]     # overlapping, repeated
    out += [("chr8", 0, 1000), ("chr8", lens[7] - 1000, lens[7]), ("chrM", 0, 10), ("chrM", lens[24] - 5, lens[24])]
    out += [("chr3", 1000, 500_000), ("chr8", 150_090, 150_090), ("chrM", 16_100, 16_100)]
    assert chroms[7] == "chr8" and chroms[24] == "chrM"
    return out


def with_qual(i):
    return i % 3 != 1                 # QUAL on two records in three, absent (0xff) on the rest


def host_window_coverage(path, windows, thr, cb, **kw):
    with host_pipeline():
        return bam.window_coverage(path, windows, thr, cb, device="cpu", **kw)


def plot_case(golden_dir, name, tmp_path):
    with open(os.path.join(golden_dir, "plotcov_%s.json" % name)) as fp:
        gold = json.load(fp)
    _, rec = synth.dataset(gold["config"], "cpu")
    with open(os.path.join(golden_dir, "e2e_%s.json" % gold["config"])) as fp:
        text = json.load(fp)["files"][gold["graph_file"]]
    graph = str(tmp_path / "g_graph.txt")
    with open(graph, "w") as fp:
        fp.write(text)
    want = [(c, a + k * w, a + k * w + w, tot) for c, a, w, totals in gold["tracks"] for k, tot in enumerate(totals)]
    return gold, rec, graph, want


# ---- the file of tests/test_read_qc.py, decoded with further requests by test_bam_request.py -----------------------------------
LONG_READ = 300_000
EDGE_QUAL = bytes([0, 93, 200, 254])


def read_qc_odd_records():
    big = [(M, 3), (I, 1), (D, 2)] * 22000 + [(M, 5)]            # 66001 ops -> CG tag; the record's own n_cigar_op is 2
    alns = [
        dict(tid=7, pos=150_000, cigar=[(S, 5), (M, 50), (D, 70), (M, 30)], name="edgeq"),
        dict(tid=7, pos=150_005, cigar=[(M, 120)], flag=0x100, name="secondary"),
        dict(tid=7, pos=150_010, cigar=[(H, 50), (M, 100), (H, 30)], flag=0x800, name="supp_hard"),
        dict(tid=7, pos=150_015, cigar=[(M, 60)], flag=4, name="unmapped", mapq=0),
        dict(tid=7, pos=150_020, cigar=[(M, 200)], has_seq=0, name="noseq"),
        dict(tid=7, pos=150_025, cigar=[(M, 90)], name="withq_a", mapq=13),
        dict(tid=7, pos=150_026, cigar=[(M, 333)], name="noqual"),
        dict(tid=7, pos=150_027, cigar=[(M, 91)], name="withq_b"),
    ]
    alns += [dict(tid=7, pos=150_030 + k, cigar=[(M, ln)], name="len%d" % ln, mapq=20 + k) for k, ln in enumerate((1, 15, 16, 17, 65))]
    alns += [dict(tid=7, pos=150_070, cigar=big, name="longcigar"),
             dict(tid=7, pos=150_080, cigar=[(S, 100), (M, LONG_READ - 100)], name="huge"),
             dict(tid=7, pos=150_090, cigar=[(H, 10), (M, 77)], name="hard_primary")]
    return synth.records_from_alignments(alns)


def read_qc_writer_options(rec):
    names = rec.materialise_names()
    name_of = lambda i: names[int(rec.name_id[i])]
    qlen = rec.qlen.numpy()

    def qual(i):
        nm, n = name_of(i), int(qlen[i])
        if nm == "edgeq":
            return (EDGE_QUAL * (n // 4 + 1))[:n]
        if nm.startswith("len"):
            return bytes((7 * k + 3) % 94 for k in range(n))
        if nm == "huge":
            k = np.arange(n, dtype=np.int64)
            return ((k * k + 11 * k + 5) % 95).astype(np.uint8).tobytes()
        return None
    with_qual = lambda i: name_of(i) != "noqual" and (i % 4 != 2 or name_of(i).startswith("withq"))
    return dict(qual=qual, with_qual=with_qual)


def read_qc_case(d):
    """The files in directory d, the records read back from the bytes and the restated statistics."""
    rec = synth.merge_sorted(synth.generate(synth.scaled_config("tiny", 500), "cpu"), read_qc_odd_records())
    opts = read_qc_writer_options(rec)
    path, small = str(d / "mixed.bam"), str(d / "mixed_small_blocks.bam")
    bam.write_bam(rec, path, seed=5, fast_seq=True, **opts)
    bam.write_bam(rec, small, seed=5, fast_seq=True, block_size=1500, empty_block_every=5, **opts)
    parsed = read_bam(path)
    assert len(parsed.recs) == rec.n
    none = str(d / "no_reads.bam")
    bam.write_bam(synth.records_from_alignments([dict(tid=7, pos=100, cigar=[(M, 50)], flag=0x100, name="s"),
                                                 dict(tid=7, pos=200, cigar=[(M, 50)], has_seq=0, name="p"),
                                                 dict(tid=7, pos=300, cigar=[(H, 5), (M, 50)], flag=0x800, name="t")]), none, with_qual=True)
    return dict(rec=rec, path=path, small=small, none=none, recs=parsed.recs, want=restate_read_qc(parsed.recs), inflated_bytes=parsed.n_bytes)
