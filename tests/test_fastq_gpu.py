"""The FASTQ session on the GPU (k_fastq_* of coral_amd/csrc/coral_fastq.hip) against the host backend (coral_fastq_host.h), exactly:
rows, histogram, counters, kept flags, the output's bytes, return code and offset on the shared cases of tests/fastq_cases.py -
which tests/test_fastq_core.py holds against the plain-Python restatement - fed at the smallest staging size, and on texts built
at the edges of the kernels' launch geometry as coral_fastq_geometry reports it; `fastq.read_qc` and the two modes on both devices,
and the FASTQ that the decoder's `fastq` mode writes against `bam.read_qc` of the BAM it came from."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from coral_amd import CoRAL, _lib, bam, fastq, synth
from tests import fastq_cases as fc

pytestmark = pytest.mark.gpu
GPU = "cuda:0"
GUARD = 64                           # counters behind the histogram that must stay untouched
WS_GUARD = 4096                      # bytes behind the workspace that must stay untouched
ONE_PIECE = 1 << 20


def geometry():
    g = (C.c_int32 * 8)()
    assert _lib.lib().coral_fastq_geometry(g) == 0
    return dict(zip(("bytes_per_thread", "threads", "lanes", "records_per_piece", "min_staging", "load_bytes", "walk_threads"), g))


def device_session(pieces, thresholds, staging):
    kept = {}

    def setup(stage):
        L = _lib.lib()
        ws_bytes = int(L.coral_fastq_workspace_bytes(stage))
        assert ws_bytes > 0
        hist = torch.zeros(256 + GUARD, dtype=torch.int64, device=GPU)
        ws = torch.full((ws_bytes + WS_GUARD,), 0xA5, dtype=torch.uint8, device=GPU)
        torch.cuda.synchronize()
        kept.update(hist=hist, ws=ws, ws_bytes=ws_bytes)
        return hist, ws, ws_bytes, torch.cuda.current_stream(GPU).cuda_stream, lambda: hist.cpu().numpy()

    out = fc.run_session(pieces, thresholds, device=0, staging=staging, stream_setup=setup)
    torch.cuda.synchronize()
    assert not bool(kept["hist"][256:].any()), "a counter behind the histogram was written"
    assert bool((kept["ws"][kept["ws_bytes"]:] == 0xA5).all()), "a byte behind the workspace was written"
    return out


@functools.lru_cache(maxsize=None)
def host_session(data, thresholds=fc.NO_THRESHOLDS):
    return fc.run_session([data], thresholds)


def check(data, staging, thresholds=fc.NO_THRESHOLDS, pieces=None):
    want = host_session(data, thresholds)
    got = device_session([data] if pieces is None else pieces, thresholds, staging)
    fc.assert_same(got, want, (staging, thresholds))
    return got


@pytest.mark.parametrize("name", sorted(fc.cases()))
def test_device_equals_host_on_the_cases(name):
    g = geometry()
    assert g["min_staging"] == 16
    data = fc.cases()[name]
    assert host_session(data)["rc"] == 0
    for staging in (g["min_staging"], g["min_staging"] + 1, ONE_PIECE):
        check(data, staging)
    if name in ("crlf", "many_short_reads", "empty_sequence_at_the_end"):
        check(data, 17, (2, 40, 4000))
        check(data, ONE_PIECE, (2, 40, 4000))


def test_refusals_on_the_device():
    g = geometry()
    front = fc.cases()["unix"]
    for name, (data, offset) in fc.refused().items():
        for text, at in ((data, offset), (front + data, len(front) + offset)):
            for staging in (g["min_staging"], ONE_PIECE):
                got = device_session([text], fc.NO_THRESHOLDS, staging)
                assert (got["rc"], got["offset"]) == (fc.FORMAT, at), (name, staging, got)
    L = _lib.lib()
    t = torch.zeros(256, dtype=torch.int64, device=GPU)
    h = C.c_void_p()
    for staging, ws_bytes in ((15, 1 << 20), ((1 << 30) + 1, 1 << 20), (4096, 256)):
        assert L.coral_fastq_open(0, 0, 0, 0, -1, staging, t.data_ptr(), t.data_ptr(), ws_bytes, None, C.byref(h)) == -1 and not h.value
    assert L.coral_fastq_open(0, 5, 4, 0, -1, 4096, t.data_ptr(), t.data_ptr(), 1 << 20, None, C.byref(h)) == -1 and not h.value
    assert L.coral_fastq_workspace_bytes(15) < 0 and L.coral_fastq_workspace_bytes((1 << 30) + 1) < 0


def aligned_record(rng, at, n, off, load):
    """A record of n bases appended at stream offset ``at`` whose sequence and quality lines both start ``off`` bytes behind a
    load boundary."""
    pad = lambda pos, least: (off - (pos + least)) % load         # filler so that the line behind a line of `least` bytes starts right
    name = b"@" + b"n" * pad(at, 2) + b"\n"
    seq = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, n)]) + b"\n"
    plus = b"+" + b"p" * pad(at + len(name) + len(seq), 2) + b"\n"
    qual = bytes(rng.randint(33, 127, n).astype(np.uint8)) + b"\n"
    assert (at + len(name)) % load == off and (at + len(name) + len(seq) + len(plus)) % load == off
    return name + seq + plus + qual


@pytest.mark.parametrize("span", ("thread", "wave", "workgroup"))
def test_lines_of_a_threads_a_waves_and_a_workgroups_bytes(span):
    g = geometry()
    rng = np.random.RandomState(41)
    width = g["bytes_per_thread"] * {"thread": 1, "wave": g["lanes"], "workgroup": g["threads"]}[span]
    data = b""
    for off in (0, 1):
        for n in (width - 1, width, width + 1):
            data += aligned_record(rng, len(data), n, off, g["load_bytes"])
    got = check(data, ONE_PIECE)
    assert got["length"] == [width - 1, width, width + 1] * 2
    check(data, 3 * width + 16)
    check(data, width, (width, width, 0))


def test_piece_boundaries_in_every_phase_and_inside_cr_lf():
    rng = np.random.RandomState(42)
    data = b"".join(fc.random_record(rng, b"r%d" % k, 20 + k, b"\r\n") for k in range(6)) + b"@e\r\n\r\n+\r\n\r\n" + fc.random_record(rng, b"last", 9, b"\r\n")
    lines = data.split(b"\n")
    by_line = [l + b"\n" for l in lines[:-1]]                      # a piece boundary at the start of every line: all four phases
    assert b"".join(by_line) == data and len(by_line) % 4 == 0
    check(data, ONE_PIECE, pieces=by_line)
    check(data, ONE_PIECE, (22, 24, 0), pieces=by_line)
    at_cr = [p + b"\r" for p in data.split(b"\r")[:-1]] + [data.split(b"\r")[-1]]      # and between every '\r' and its '\n'
    assert b"".join(at_cr) == data and all(p.startswith(b"\n") for p in at_cr[1:])
    check(data, ONE_PIECE, pieces=at_cr)
    check(data, ONE_PIECE, (0, 23, 3000), pieces=at_cr)
    for phase in range(4):                                        # one boundary alone, at the start of a line of each phase
        cut_at = len(b"".join(by_line[:8 + phase]))
        check(data, ONE_PIECE, pieces=[data[:cut_at], data[cut_at:]])


def test_a_line_longer_than_three_pieces():
    rng = np.random.RandomState(43)
    data = fc.random_record(rng, b"a", 30) + fc.random_record(rng, b"long name " + b"x" * 700, 1000) + fc.random_record(rng, b"b", 5)
    for staging in (64, 256, 300):
        assert check(data, staging)["length"] == [30, 1000, 5]
    check(data, 256, (31, 0, 0))


def test_hundreds_of_records_within_one_waves_bytes_and_the_row_tables_size():
    g = geometry()
    rng = np.random.RandomState(44)
    wave = g["bytes_per_thread"] * g["lanes"]
    many = 3 * g["records_per_piece"] + 37
    data = b"".join(fc.random_record(rng, b"", k % 3) for k in range(many))                  # 7 to 11 bytes a record
    assert data[:wave].count(b"@\n") > 300 and len(data) < ONE_PIECE
    got = check(data, ONE_PIECE)                                  # one fed piece: it is cut at the table's size
    assert got["records"] == many and got["length"] == [k % 3 for k in range(many) if k % 3]
    check(data, ONE_PIECE, (2, 0, 4000))
    check(data, 2000)
    for n in (g["records_per_piece"] - 1, g["records_per_piece"], g["records_per_piece"] + 1):
        data = b"".join(fc.record(b"h%d" % k, b"AC", b"I#") for k in range(n))
        assert check(data, ONE_PIECE)["records"] == n
        assert check(data[:-1], ONE_PIECE)["records"] == n      # the last record closed by the end of the stream


def test_read_qc_and_the_modes_on_both_devices(tmp_path, capsys):
    rng = np.random.RandomState(45)
    data = b"".join(fc.random_record(rng, b"read%d ch=%d" % (k, k % 7), int(n), lo=34, hi=80) for k, n in enumerate(rng.randint(0, 3000, 400)))
    path = str(tmp_path / "reads.fastq")
    with open(path, "wb") as fp:
        fp.write(data)
    want = fc.run_session([data], (500, 2500, 2300))
    res = {}
    for pipe, device in (("gpu", GPU), ("cpu", "cpu")):
        out = str(tmp_path / (pipe + ".fastq"))
        qc = fastq.read_qc(path, device=device, chunk_bytes=100_000, min_length=500, max_length=2500, min_mean_quality=23.0, output=out)
        res[pipe] = (qc.length.tolist(), qc.qual_sum.tolist(), qc.kept.tolist(), qc.base_quality_hist.tolist(), qc.counters, qc.n_kept, qc.kept_bases, open(out, "rb").read())
        assert res[pipe][:4] == (want["length"], want["qual_sum"], want["kept"], want["hist"]) and res[pipe][7] == want["output"]
        assert 0 < qc.n_kept < qc.n_records and fastq.LAST_FASTQ_QC["upload"] >= 0
    assert res["gpu"] == res["cpu"]
    modes = {}
    for pipe, device in (("gpu", GPU), ("cpu", "cpu")):
        d, out = str(tmp_path / ("qc_" + pipe)), str(tmp_path / ("kept_" + pipe + ".fastq"))
        CoRAL.main(["qc", "--fastq", path, "--output_dir", d, "--device", device, "--no_plots", "--chunk_bytes", "70000"])
        capsys.readouterr()
        assert CoRAL.main(["filter", "--fastq", path, "--output", out, "--min_length", "500", "--max_length", "2500", "--min_mean_quality", "23", "--device", device,
                           "--chunk_bytes", "70000"]) == out
        printed = capsys.readouterr().out.replace("kept_" + pipe, "kept_x")
        modes[pipe] = (open(os.path.join(d, "quality_control_summary.tsv"), "rb").read(), open(os.path.join(d, "read_qc.json"), "rb").read(), open(out, "rb").read(), printed)
    assert modes["gpu"] == modes["cpu"] and modes["gpu"][2] == want["output"]
    assert "records: 400\n" in modes["gpu"][3] and "kept_records: %d\n" % want["n_kept"] in modes["gpu"][3]
    assert json.loads(modes["gpu"][1])["counters"]["n_records"] == 400


def test_the_decoders_fastq_read_back_equals_the_bams_read_qc(tmp_path):
    M = 0
    rng = np.random.RandomState(46)
    lens = [int(n) for n in rng.randint(1, 900, 60)] + [5000]
    quals = [rng.randint(0, 94, n).astype(np.uint8) for n in lens]
    rec = synth.records_from_alignments([dict(tid=0, pos=100 + 50 * k, cigar=[(M, n)], flag=16 if k % 3 == 1 else 0, name="read%d" % k) for k, n in enumerate(lens)])
    path, fq = str(tmp_path / "reads.bam"), str(tmp_path / "reads.fastq")
    bam.write_bam(rec, path, seed=3, qual=lambda i: quals[i].tobytes())
    assert CoRAL.main(["fastq", "--lr_bam", path, "--output", fq, "--device", GPU]) == fq
    from_bam = bam.read_qc(path, device=GPU)
    from_fastq = fastq.read_qc(fq, device=GPU, chunk_bytes=10_000)
    assert from_bam.n_reads == from_fastq.n_reads == len(lens) and from_fastq.n_no_seq == 0
    assert sorted(zip(from_fastq.length.tolist(), from_fastq.qual_sum.tolist())) == sorted(zip(from_bam.length.tolist(), from_bam.qual_sum.tolist()))
    assert from_fastq.length.tolist() == lens and from_fastq.qual_sum.tolist() == [int(q.sum()) for q in quals]      # (the decoder writes the reads in file order)
    assert from_fastq.base_quality_hist.tolist() == from_bam.base_quality_hist.tolist()
    assert from_fastq.summary_text() == from_bam.summary_text()
