"""The copy-number segmenter's host backend (coral_cn_segment_host: coral_amd/csrc/coral_cn_host.h over coral_cn_core.h) against
the plain-Python restatement of the rule in tests/cnv_cases.py, on the shared case table; the fixed-point log2 and the FDR cut on
their own; the stand-alone program under AddressSanitizer and UBSan; the Python surface's argument errors and the .cns it writes.
The device build of the same core is compared with the host's, rows and all, in tests/test_cnv_gpu.py."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from coral_amd import _lib, bam, cnv
from tests import cnv_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "cnv_host.cpp")


@pytest.fixture(scope="module")
def table():
    return cc.cases()


@pytest.fixture(scope="module")
def restated(table):
    """name -> (rows, counts, margins) of the restatement, computed once."""
    out = {}
    for name, case in table.items():
        margins = []
        rows, counts = cc.restate(case, margins)
        out[name] = (rows, counts, margins)
    return out


def host_segments(case):
    return cnv.segment_depth(case.depth(bam), None if case.ref is None else case.depth(bam, "ref"), case.levels, case.q, case.centre_contigs, device="cpu")


def test_log2_q16_is_the_stated_algorithm():
    L = _lib.lib()
    xs = [1, 2, 3, 1 << 62] + [(1 << k) + d for k in range(2, 63) for d in (-1, 1)]
    for x in xs:
        assert L.coral_cn_log2_q16(x) == cc.log2_q16(x), x
    assert [L.coral_cn_log2_q16(x) for x in (1, 2, 1 << 62)] == [0, 1 << 16, 62 << 16]
    # truncation, never rounding up: within 2^-16 * 17 below the real log2 (each of the 16 squarings truncates once)
    for x in (3, 5, 7, 1000, 30011, (1 << 40) + 12345, (1 << 62) - 1):
        got = L.coral_cn_log2_q16(x) / 65536.0
        assert got <= math.log2(x) + 1e-12 and math.log2(x) - got < 2.0 ** -16 * 2, x


def test_every_case_keeps_the_margin_at_the_cut(restated):
    """No p_i within relative 1e-6 of its line: math.erfc against std::erfc cannot flip a case.  No case is exempt."""
    assert sum(len(m) for _r, _c, m in restated.values()) > 200
    for name, (_rows, _counts, margins) in restated.items():
        assert all(m > cc.MARGIN for m in margins), (name, min(margins))


def test_the_table_covers_what_it_is_meant_to(restated):
    bp = {name: counts["breakpoints"] for name, (_r, counts, _m) in restated.items()}
    assert bp["one_step"] == 2 and bp["boundary_step"] == 0 and bp["sigma_zero"] >= 2 and bp["nothing_kept"] == 0 and bp["loose_q"] >= 6
    assert restated["nothing_kept"][0] == [] and len(restated["one_kept_bin"][0]) == 1
    assert [r[:4] for r in restated["boundary_step"][0]] == [(0, 0, 15000, 300), (1, 0, 14000, 280)]
    assert restated["centre_on_chr2"][1]["centre"] > 4 * restated["boundary_step"][1]["centre"]
    assert restated["reference"][0] != restated["one_step"][0]


def test_host_backend_equals_the_restatement_on_the_case_table(table, restated):
    for name, case in table.items():
        rows, counts, _m = restated[name]
        seg = host_segments(case)
        assert {k: seg.counts[k] for k in counts} == counts, name
        assert cc.rows_of(seg) == rows, name
        assert seg.counts["rows"] == len(rows) == len(seg)


def test_fdr_cut_is_the_restated_one():
    L = _lib.lib()
    rng = np.random.RandomState(5)
    for trial in range(40):
        M = int(rng.randint(1, 60))
        mags = np.sort(rng.randint(1, 4000000, M).astype(np.int64))[::-1].copy()
        h, sigma, q = 1 << int(rng.randint(1, 6)), float(rng.randint(1000, 200000)), float(rng.choice([1e-4, 1e-2, 0.2]))
        margins = []
        want = cc.fdr_cut(mags.tolist(), h, sigma, q, margins)
        if min(margins) <= cc.MARGIN:
            continue
        assert L.coral_cn_fdr_cut(mags.ctypes.data, M, h, sigma, q) == want, (trial, mags, h, sigma, q)
    one = np.array([7], dtype=np.int64)
    assert L.coral_cn_fdr_cut(one.ctypes.data, 1, 2, 0.0, 1e-4) == 1 and L.coral_cn_fdr_cut(one.ctypes.data, 0, 2, 1.0, 1e-4) == cc.NO_CUT
    assert L.coral_cn_fdr_cut(one.ctypes.data, 1, 2, 1e9, 1e-4) == cc.NO_CUT


def test_sanitizer_run_of_the_stand_alone_program(tmp_path, table):
    """The case table through the stand-alone program (its own main) under AddressSanitizer and UBSan, on the CPU: every array
    is an allocation of exactly its size.  Its answers are the library's."""
    exe, cases_bin, results_bin = str(tmp_path / "cnv_host"), str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    with open(cases_bin, "wb") as fp:
        for case in table.values():
            fp.write(case.pack())
    run = subprocess.run([exe, cases_bin, results_bin], capture_output=True, text=True)
    assert run.returncode == 0 and "cnv_host: %d cases" % len(table) in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    with open(results_bin, "rb") as fp:
        raw = fp.read()
    at = 0
    for name, case in table.items():
        counts = struct.unpack_from("<5q", raw, at)
        n = counts[0]
        at += 40
        contig = np.frombuffer(raw, dtype="<i4", count=n, offset=at)
        at += 4 * n
        cols = [np.frombuffer(raw, dtype="<i8", count=n, offset=at + 8 * n * k) for k in range(5)]
        at += 40 * n
        seg = host_segments(case)
        assert list(counts) == [seg.counts[k] for k in ("rows", "kept", "centre", "ref_centre", "breakpoints")], name
        assert list(zip(contig.tolist(), *(c.tolist() for c in cols))) == cc.rows_of(seg), name
    assert at == len(raw)


def test_argument_errors_come_before_any_work(table):
    d = table["one_step"].depth(bam)
    for kw in ({"levels": 0}, {"levels": 21}, {"levels": 2.5}, {"levels": True}, {"fdr_q": 0.0}, {"fdr_q": 1.0}, {"fdr_q": -1e-4}, {"fdr_q": "x"},
               {"centre_contigs": ["chr9"]}):
        with pytest.raises(ValueError):
            cnv.segment_depth(d, device="no such device", **kw)
    other = table["boundary_step"].depth(bam)
    with pytest.raises(ValueError, match="other bins"):
        cnv.segment_depth(d, reference=other, device="no such device")
    finer = bam.BinnedDepth(["chr1"], [600 * 100], 50, 0, 0x704, True, [0, 1200], np.ones(1200, dtype=np.int64), np.zeros(1200, dtype=np.int64))
    with pytest.raises(ValueError, match="other bins"):
        cnv.segment_depth(d, reference=finer, device="no such device")
    with pytest.raises(ValueError):
        cnv.call_copy_number("/no/such.bam", levels=0)


def test_more_rows_than_the_first_row_capacity():
    """A square wave of 4 bins a level without noise (sigma 0: every step is a breakpoint) makes 5 000 rows, more than the 4 096
    the first call makes room for: the second call, with the capacity the first one named, returns them all."""
    bases = np.where((np.arange(20000) // 4) % 2 == 0, 1000, 2000).astype(np.int64)
    seg = cnv.segment_depth(cc.Case(["chr1"], [20000 * 100], 100, bases).depth(bam), device="cpu")
    assert len(seg) == 5000 and seg.probes.tolist() == [4] * 5000 and seg.counts["breakpoints"] == 4999
    assert seg.start.tolist() == list(range(0, 2000000, 400)) and seg.end.tolist() == list(range(400, 2000001, 400))
    assert set(seg.sum_bases.tolist()) == {4000, 8000}


def test_the_segments_as_a_cns_file(tmp_path, table):
    seg = host_segments(table["one_step"])
    assert len(seg) == 3 and seg.chrom == ["chr1"] * 3 and seg.probes.tolist() == [200, 60, 340]
    assert np.allclose(seg.cn(), 2.0 * 2.0 ** seg.log2) and abs(seg.cn()[1] - 6.0) < 0.2 and abs(seg.cn()[0] - 2.0) < 0.1
    assert np.array_equal(seg.log2, seg.sum_s / (seg.probes * 65536.0)) and np.array_equal(seg.depth, seg.sum_bases / (seg.probes * 100.0))
    path = seg.write(str(tmp_path / "x.cns"))
    with open(path) as fp:
        lines = fp.read().split("\n")
    assert lines[0] == "chromosome\tstart\tend\tgene\tlog2\tdepth\tprobes\tweight" and lines[-1] == "" and len(lines) == 5
    for line, row in zip(lines[1:], seg.rows()):
        s = line.split("\t")
        assert (s[0], int(s[1]), int(s[2]), s[3], float(s[4]), float(s[5]), int(s[6]), int(s[7])) == (row[0], row[1], row[2], "-", row[3], row[4], row[5], row[5])
    assert bam.segment_depth is cnv.segment_depth and bam.find_seeds is cnv.find_seeds


def test_binned_depth_read_gives_the_table_back(tmp_path, table):
    for name in ("short_last_bin_and_tiny_contigs", "one_step", "one_kept_bin"):
        d = table[name].depth(bam)
        back = bam.BinnedDepth.read(d.write(str(tmp_path / (name + ".cnn"))))
        keep = [k for k, l in enumerate(d.lengths) if l > 0]                 # (a contig without bins is not in the file)
        assert back.chroms == [d.chroms[k] for k in keep] and back.lengths == [d.lengths[k] for k in keep] and back.bin_size == d.bin_size
        assert np.array_equal(back.all_bases, d.all_bases) and np.array_equal(back.all_reads, d.all_reads)
    with open(str(tmp_path / "bad.cnn"), "w") as fp:
        fp.write("chrom\tpos\n")
    with pytest.raises(ValueError):
        bam.BinnedDepth.read(str(tmp_path / "bad.cnn"))
