"""The host backend of the reference's per-bin composition (coral_comp_open with device -1: coral_amd/csrc/coral_comp_host.h over
coral_comp_core.h) against the plain-Python restatement of the rule in tests/comp_cases.py, on the shared cases; the independence
of the result from where the text is cut; the refusals; the Python layer (``Composition``); the stand-alone program under
AddressSanitizer and UBSan.  The device build of the same core is compared with the host's in tests/test_comp_gpu.py."""
import ctypes as C
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from coral_amd import _lib, bam, composition
from tests import comp_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "comp_host.cpp")


@pytest.fixture(scope="module")
def table():
    return cc.cases()


def test_the_cases_cover_what_they_are_meant_to(table):
    r = lambda name, b: cc.restate(table[name][0], b)
    assert r("crlf", 30)[:2] == (["one", "two"], [130, 45]) and b"\r\n" in table["crlf"][0]
    assert sum(r("lowercase_runs", 8)[4]) == 8 * 6 + 4 * 7 and sum(r("lowercase_runs", 8)[2]) == 10 + 12 + 16
    assert r("n_runs", 10)[2][:4] == [0, 0, 0, 0] and r("n_runs", 10)[3][:4] == [0, 0, 0, 0] and r("n_runs", 10)[4][8] == 10
    names, lengths, gc, at, masked = r("iupac_and_star", 1000)
    assert lengths == [36 + 4] and gc == [2 + 2] and at == [2 + 2 + 1] and masked == [15 + 1 + 1]
    assert r("shorter_than_a_bin", 16)[1] == [3, 64] and len(r("shorter_than_a_bin", 16)[2]) == 1 + 4
    assert r("ends_on_a_bin_edge", 16)[1] == [64, 17] and len(r("ends_on_a_bin_edge", 16)[2]) == 4 + 2 and len(r("ends_on_a_bin_edge", 64)[2]) == 2
    assert r("empty_contig_between", 10)[:2] == (["a", "empty", "b", "e2", "c"], [20, 0, 21, 0, 2])
    assert r("header_as_last_line", 3)[:2] == (["a", "last"], [8, 0]) and not table["header_as_last_line"][0].endswith(b"\n")
    assert r("no_trailing_newline", 4)[1] == [13]
    assert r("names_with_descriptions", 2)[:2] == (["chr1", "chr2", "chr3|a=b", "chr4"], [4, 5, 2, 0])
    assert len(r("bin_size_one", 1)[2]) == 37 + 5 and max(r("bin_size_one", 1)[2]) == 1
    assert r("bin_larger_than_the_file", 100000)[1] == [50, 9] and len(r("bin_larger_than_the_file", (1 << 31) - 1)[2]) == 2
    assert r("gt_inside_a_line", 4)[:2] == (["a>b"], [8])


def test_host_backend_equals_the_restatement_on_the_cases(table):
    for name, (data, bin_sizes) in table.items():
        for b in bin_sizes:
            want = cc.expected(data, b)
            assert cc.run_session([data], b, want[1][2] + 3) == want, (name, b)
            assert cc.run_session([data], b, max(want[1][2], 1)) == want, (name, b, "exact capacity")


def test_the_result_does_not_depend_on_where_the_text_is_cut(table):
    """Each case cut in two at every byte offset, and fed one byte a call."""
    for name, (data, bin_sizes) in table.items():
        b = bin_sizes[0]
        want = cc.expected(data, b)
        for cut in range(len(data) + 1):
            assert cc.run_session([data[:cut], data[cut:]], b, want[1][2] + 1) == want, (name, cut)
        assert cc.run_session([data[i:i + 1] for i in range(len(data))], b, want[1][2] + 1) == want, name
        assert cc.run_session([data[i:i + 7] for i in range(0, len(data), 7)], b, want[1][2] + 1) == want, name


def test_refusals():
    L = _lib.lib()
    fmt, cap, arg = -4, -3, -1
    for text in (b"ACGT\n>a\nACGT\n", b"\n\nA>a\n", b" \n>a\nAC\n", b"\r>a\nAC\n", b"N"):                # a sequence byte in front of the first header
        assert cc.run_session([text], 10, 8)[0] == fmt, text
        assert cc.run_session([text[:1], text[1:]], 10, 8)[0] == fmt, text
        assert "in front of the first header" in L.coral_bam_last_error().decode()
    for text in (b">\nACGT\n", b"> desc\nAC\n", b">a\nAC\n>\tx\nAC\n", b">a\nAC\n>", b">a\nAC\n>\r\n"):          # a header without a name
        assert cc.run_session([text], 10, 8)[0] == fmt, text
        assert "without a name" in L.coral_bam_last_error().decode()
    data = cc.cases()["empty_contig_between"][0]
    want = cc.expected(data, 5)
    need = want[1][2]
    rc, stats = cc.run_session([data], 5, need - 1)[:2]                                                  # one bin short: the need is reported
    assert rc == cap and stats[:7] == want[1][:7] and stats[2] == need == 4 + 5 + 1
    assert cc.run_session([data], 5, need) == want
    g = np.zeros(4, dtype=np.uint32)
    h = C.c_void_p()
    for bad in (0, -1, 1 << 31, 1 << 40):
        assert L.coral_comp_open(bad, -1, g.ctypes.data, g.ctypes.data, g.ctypes.data, 4, 0, None, 0, None, C.byref(h)) == arg and not h.value
    assert L.coral_comp_open((1 << 31) - 1, -1, g.ctypes.data, g.ctypes.data, g.ctypes.data, 4, 0, None, 0, None, C.byref(h)) == 0
    L.coral_comp_close(h)
    for bad_cap in (0, -5, (1 << 28) + 1):
        assert L.coral_comp_open(10, -1, g.ctypes.data, g.ctypes.data, g.ctypes.data, bad_cap, 0, None, 0, None, C.byref(h)) == arg
    assert L.coral_comp_open(10, -1, None, g.ctypes.data, g.ctypes.data, 4, 0, None, 0, None, C.byref(h)) == arg
    for kw in ({"bin_size": 0}, {"bin_size": 1 << 31}, {"bin_size": 2.5}, {"bin_size": True}, {"chunk_bytes": 15}, {"chunk_bytes": 64.0}):
        with pytest.raises(ValueError):
            composition.reference_composition("/no/such/file.fa", device="no such device", **kw)
    with pytest.raises(_lib.CoralHipError, match="in front of the first header"):
        composition.reference_composition(io.BytesIO(b"ACGT\n"), 10, device="cpu")


def host_composition(data, bin_size, **kw):
    return composition.reference_composition(io.BytesIO(data), bin_size, device="cpu", **kw)


def test_reference_composition_on_the_host(table, tmp_path):
    for name, (data, bin_sizes) in table.items():
        for b in bin_sizes:
            want = cc.expected(data, b)
            for chunk in (16, 17, 64 << 20):
                got = host_composition(data, b, chunk_bytes=chunk)
                assert (got.chroms, got.lengths, got.gc.tolist(), got.at.tolist(), got.masked.tolist()) == tuple(want[2:]), (name, b, chunk)
                assert got.gc.dtype == np.uint32 and got.bin_size == b and got.n_bins == want[1][2] and got.totals["positions"] == want[1][1]
    # a first capacity that is too small: the count is repeated once with what it asked for
    data = table["bin_size_one"][0]
    got = host_composition(data, 1, _capacity=5)
    assert got.gc.tolist() == cc.restate(data, 1)[2] and composition.LAST_COMPOSITION["attempts"] == 2
    assert host_composition(data, 1).n_bins == 42 and composition.LAST_COMPOSITION["attempts"] == 1
    # from a path, plain and gzipped
    import gzip
    plain, packed = str(tmp_path / "ref.fa"), str(tmp_path / "ref.fa.gz")
    with open(plain, "wb") as fp:
        fp.write(table["crlf"][0])
    with gzip.open(packed, "wb") as fp:
        fp.write(table["crlf"][0])
    want = cc.restate(table["crlf"][0], 7)
    for path in (plain, packed):
        got = composition.reference_composition(path, 7, device="cpu")
        assert (got.chroms, got.lengths, got.gc.tolist(), got.at.tolist(), got.masked.tolist()) == want


def test_fractions_and_the_written_table(table, tmp_path):
    data = b">a desc\nGGCCATatNN\nNNNNNNNNNN\nacg\n>none\n>b\nGC\n"
    comp = host_composition(data, 10)
    assert comp.chroms == ["a", "none", "b"] and comp.lengths == [23, 0, 2] and comp.bin_off.tolist() == [0, 3, 3, 4]
    assert comp.gc.tolist() == [4, 0, 2, 2] and comp.at.tolist() == [4, 0, 1, 0] and comp.masked.tolist() == [2, 0, 3, 0]
    gcf = comp.gc_fraction()
    assert gcf[0] == 0.5 and np.isnan(gcf[1]) and gcf[2] == 2 / 3 and gcf[3] == 1.0
    assert comp.masked_fraction().tolist() == [0.2, 0.0, 1.0, 0.0] and comp.bin_lengths().tolist() == [10, 10, 3, 2]
    assert comp.genome_gc() == 8 / 13
    path = str(tmp_path / "bins.tsv")
    assert comp.write(path) == path
    lines = open(path).read().split("\n")
    assert lines[:5] == ["#bin_size\t10", "#contig\ta\t23", "#contig\tnone\t0", "#contig\tb\t2", "chromosome\tstart\tend\tgene\tgc\trmask\tgc_bases\tat_bases\tmasked_bases"]
    assert lines[5] == "a\t0\t10\t-\t0.5\t0.2\t4\t4\t2" and lines[6] == "a\t10\t20\t-\tnan\t0.0\t0\t0\t0" and lines[7] == "a\t20\t23\t-\t%r\t1.0\t2\t1\t3" % (2 / 3)
    assert lines[8] == "b\t0\t2\t-\t1.0\t0.0\t2\t0\t0" and lines[9:] == [""]
    for name, (text, bin_sizes) in table.items():
        for b in bin_sizes:
            comp = host_composition(text, b)
            back = composition.Composition.read(comp.write(path))
            assert (back.chroms, back.lengths, back.bin_size) == (comp.chroms, comp.lengths, comp.bin_size), (name, b)
            assert np.array_equal(back.bin_off, comp.bin_off) and all(np.array_equal(x, y) and x.dtype == np.uint32 for x, y in ((back.gc, comp.gc), (back.at, comp.at), (back.masked, comp.masked)))
    with open(path, "w") as fp:
        fp.write("#bin_size\t10\nchromosome\tstart\tend\n")
    with pytest.raises(ValueError):
        composition.Composition.read(path)
    with open(path, "w") as fp:
        fp.write("#bin_size\t10\n#contig\ta\t12\n" + "\t".join(composition.COLUMNS) + "\na\t0\t10\t-\t0.5\t0.0\t1\t1\t0\na\t10\t13\t-\t0.5\t0.0\t1\t1\t0\n")
    with pytest.raises(ValueError):
        composition.Composition.read(path)


def depth_of(chroms, lengths, bin_size):
    n = sum((l + bin_size - 1) // bin_size for l in lengths)
    off = np.concatenate([[0], np.cumsum([(l + bin_size - 1) // bin_size for l in lengths])])
    return bam.BinnedDepth(chroms, lengths, bin_size, 0, 0, False, off, np.arange(n), np.zeros(n))


def test_for_depth_matches_contigs_by_name():
    data = b">a\n" + b"ACGTN" * 5 + b"\n>extra\nGGGG\n>b\n" + b"ggcc" * 3 + b"\n>c\nT\n"
    comp = host_composition(data, 10)
    gc, at, masked = comp.for_depth(depth_of(["c", "a"], [1, 25], 10))
    assert gc.tolist() == [0, 4, 4, 2] and at.tolist() == [1, 4, 4, 2] and masked.tolist() == [0, 0, 0, 0] and gc.dtype == np.uint32
    gc, at, masked = comp.for_depth(depth_of(["a", "extra", "b", "c"], [25, 4, 12, 1], 10))
    assert gc.tolist() == comp.gc.tolist() and masked.tolist() == [0, 0, 0, 0, 10, 2, 0]
    assert all(len(x) == 0 for x in comp.for_depth(depth_of([], [], 10)))
    with pytest.raises(ValueError, match="not in the FASTA"):
        comp.for_depth(depth_of(["a", "chrM"], [25, 100], 10))
    with pytest.raises(ValueError, match="25 positions in the FASTA and 26"):
        comp.for_depth(depth_of(["a"], [26], 10))
    with pytest.raises(ValueError, match="bins of 10 positions"):
        comp.for_depth(depth_of(["a"], [25], 5))


def test_duplicate_names_are_refused():
    with pytest.raises(ValueError, match="'a' stands in the FASTA more than once"):
        host_composition(b">a x\nACGT\n>b\nAC\n>a y\nGG\n", 10)


def test_sanitizer_run_of_the_stand_alone_program(tmp_path, table):
    """The cases through the stand-alone program (its own main) under AddressSanitizer and UBSan, on the CPU: whole and in pieces
    of 1, 7, 16 and 17 bytes, each piece an allocation of exactly its size, the host backend and scan_piece (the host's share of
    the device path) against each other.  Its answers are the restatement's."""
    exe, cases_bin, results_bin = str(tmp_path / "comp_host"), str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    runs = [(name, b) for name, (_data, bin_sizes) in table.items() for b in bin_sizes]
    rng = np.random.RandomState(5)
    big = b"".join(b">c%d some text\n" % k + cc.wrap(cc.random_sequence(rng, int(n)), 61) for k, n in enumerate((0, 30000, 1, 4999, 5000, 5001, 70000)))
    with open(cases_bin, "wb") as fp:
        for name, b in runs:
            fp.write(struct.pack("<qq", b, len(table[name][0])) + table[name][0])
        fp.write(struct.pack("<qq", 5000, len(big)) + big)
    run = subprocess.run([exe, cases_bin, results_bin], capture_output=True, text=True)
    assert run.returncode == 0 and "comp_host: %d cases" % (len(runs) + 1) in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    raw = open(results_bin, "rb").read()
    at = 0
    for data, b in [(table[name][0], b) for name, b in runs] + [(big, 5000)]:
        names, lengths, gc, at_, masked = cc.restate(data, b)
        n_contigs, n_bins = struct.unpack_from("<qq", raw, at)
        at += 16
        assert (n_contigs, n_bins) == (len(lengths), len(gc))
        assert np.frombuffer(raw, dtype="<i8", count=n_contigs, offset=at).tolist() == lengths
        at += 8 * n_contigs
        for want in (gc, at_, masked):
            assert np.frombuffer(raw, dtype="<u4", count=n_bins, offset=at).tolist() == want
            at += 4 * n_bins
        (nb,) = struct.unpack_from("<q", raw, at)
        assert raw[at + 8:at + 8 + nb].decode("latin-1") == "".join(n + "\n" for n in names)
        at += 8 + nb
    assert at == len(raw)
