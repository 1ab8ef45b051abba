"""The k-mer counter's host backend (coral_kmer_open with device -1: coral_amd/csrc/coral_kmer_host.h over coral_kmer_core.h) against
the plain-Python restatement of the rule in tests/kmer_cases.py, on the shared case table; the independence of the result from
the pieces the text is fed in; the threshold rule on hand-made histograms; the file ``write`` makes; the argument errors; the
refusal at 2^32 bases; the stand-alone program under AddressSanitizer and UBSan.  The device build of the same core is compared
with the host's in tests/test_kmer_gpu.py."""
import ctypes as C
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from coral_amd import _lib, kmers
from tests import kmer_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "kmer_host.cpp")


@pytest.fixture(scope="module")
def table():
    return kc.cases()


def host_count(data, k, canonical=True, chunk_bytes=64 << 20):
    return kmers.count_kmers(io.BytesIO(data), k, canonical, device="cpu", chunk_bytes=chunk_bytes)


def test_the_table_covers_what_it_is_meant_to(table):
    runs, headers = kc.parse(table["lengths_around_k"])
    assert sorted(len(r) for r in runs) == [1, 2, 3, 4, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17] and headers == 16
    assert kc.parse(table["empty_sequences_and_last_header"])[1] == 6 and table["empty_sequences_and_last_header"].endswith(b"header")
    assert kc.parse(table["gt_in_header_and_sequence"])[1] == 1
    assert kc.restate(table["poly_a"], 8, True)[0] == {0: 99993} and kc.restate(table["poly_a"], 8, False)[0] == {0: 99993}
    assert len(kc.restate(table["tandem_ac"], 8, True)[0]) == 2 and len(kc.restate(table["tandem_ac"], 8, False)[0]) == 2
    assert len(kc.restate(table["tandem_acg"], 8, True)[0]) == 3 and len(kc.restate(table["tandem_acg"], 8, False)[0]) == 3
    pal = kc.restate(b">p\nACGTACGT\n", 4, True)[0]                  # ACGT, CGTA, GTAC, TACG, ACGT: ACGT and GTAC are palindromes, TACG counts under CGTA
    assert pal == {kc.kmer_int(b"ACGT"): 2, kc.kmer_int(b"CGTA"): 2, kc.kmer_int(b"GTAC"): 1}
    assert kc.parse(table["random_megabase"])[1] == 40 and kc.restate(table["random_megabase"], 12, True)[1]["n_bases"] == 1_000_000 - 300
    assert max(v for v, _n in kc.restate(table["random_megabase"], 12, True)[2]) >= 30


@pytest.mark.parametrize("k", kc.KS)
def test_host_backend_equals_the_restatement_on_the_case_table(table, k):
    for canonical in (True, False):
        for name, data in table.items():
            counts, stats, hist = kc.restate(data, k, canonical)
            got = kc.results_of(host_count(data, k, canonical))
            assert got[1] == stats, (name, k, canonical)
            assert got[2] == hist, (name, k, canonical)
            assert got[0] == counts, (name, k, canonical)


def test_even_k_palindromes_count_once_per_occurrence(table):
    """ACGT repeated, at k = 4: ACGT and GTAC are their own reverse complements, CGTA and TACG are each other's."""
    data = table["palindromes"]
    for k in (4, 6):
        for canonical in (True, False):
            counts, stats, hist = kc.restate(data, k, canonical)
            assert kc.results_of(host_count(data, k, canonical)) == (counts, stats, hist), (k, canonical)
    counts = kc.restate(data, 4, True)[0]
    acgt, gtac, cgta = kc.kmer_int(b"ACGT"), kc.kmer_int(b"GTAC"), kc.kmer_int(b"CGTA")
    assert (counts[acgt], counts[gtac], counts[cgta]) == (300, 299, 299 + 299) and kc.kmer_int(b"TACG") not in counts
    assert sum(counts.values()) == kc.restate(data, 4, False)[1]["total"] == 1197 + 9 + 3      # (AATT GGCC TTAA are one run of 12 bases: line ends are no breaks)


def test_the_result_does_not_depend_on_the_pieces(table):
    """Each case whole, in pieces of 16, 17, 4 096 and 4 097 bytes (count_kmers' chunk_bytes) and one byte a feed (the C ABI): the
    long header is longer than the small pieces, and the CR LF pairs of the CRLF case fall on both sides of a cut."""
    assert b"\r\n" in table["crlf"] and any(table["crlf"][at - 1:at + 1] == b"\r\n" for at in range(17, len(table["crlf"]), 17))
    assert len(table["long_header"].split(b"\n")[0]) > 4097
    for name, data in table.items():
        for k, canonical in ((8, True), (3, False)):
            want = kc.feed_in_pieces(data, k, canonical, 0)
            assert want[0] == kc.restate(data, k, canonical)[0], name
            for piece in (16, 17, 4096, 4097):
                if len(data) > 200_000 and piece < 4096:
                    continue
                assert kc.results_of(host_count(data, k, canonical, chunk_bytes=piece)) == want, (name, k, piece)
            if len(data) <= 200_000:
                assert kc.feed_in_pieces(data, k, canonical, 1) == want, (name, k)
    big = table["random_megabase"]
    assert kc.feed_in_pieces(big, 11, True, 1) == kc.feed_in_pieces(big, 11, True, 0) == kc.feed_in_pieces(big, 11, True, 17)


def test_threshold_rule_on_hand_made_histograms():
    values, nums = [1, 2, 5, 9, 70000], [9000, 900, 90, 9, 1]          # 10 000 distinct k-mers
    t = lambda p: kmers.threshold_of(values, nums, p)
    assert t("0") == 0 and t(0) == 0 and t("0.0") == 0
    assert t("1") == 70000 and t("1.0") == 70000 and t(1) == 70000
    assert t("0.5") == 1 and t(0.5) == 1
    assert t("0.9") == 1                                             # need = 9 000: reached exactly by the count 1
    assert t("0.9001") == 2                                          # need = 9 001
    assert t("0.99") == 2 and t("0.9901") == 5 and t("0.999") == 5 and t("0.9991") == 9
    assert t("0.9998") == 9 and t(0.9998) == 9 and t("0.9999") == 9 and t("0.99991") == 70000      # need 9 998, 9 999, 10 000 (ceil of 9 999.1)
    assert t(".5") == 1 and t("1.") == 70000
    # need falls between two count values: 3 distinct k-mers, p = 0.5 -> need = 2 -> the second smallest
    assert kmers.threshold_of([4, 10, 11], [1, 1, 1], "0.5") == 10 and kmers.threshold_of([4, 10, 11], [1, 1, 1], "0.34") == 10
    assert kmers.threshold_of([4, 10, 11], [1, 1, 1], "0.33") == 4 and kmers.threshold_of([], [], "0.9998") == 0
    for p in ("0", "1", "0.5", "0.9", "0.9001", "0.9998", "0.99991", "0.34"):
        assert t(p) == kc.threshold(list(zip(values, nums)), p)
    # no floating point: a fraction that no double holds exactly, on counts beyond 2^53
    assert kmers.threshold_of([1, 2], [10 ** 17, 1], "0.99999999999999999") == 1 and kmers.threshold_of([1, 2], [10 ** 17, 1], "0.999999999999999999") == 2


def test_threshold_of_a_count(table):
    kcount = host_count(table["random_megabase"], 11)
    hist = kc.restate(table["random_megabase"], 11, True)[2]
    for p in ("0.9998", "0.5", "0", "1", "0.99"):
        assert kcount.threshold(p) == kc.threshold(hist, p)
    assert kcount.threshold("0.9998") == kcount.threshold(0.9998) and kcount.threshold("1") == kcount.max_count == hist[-1][0]


def test_write_the_exact_text_of_a_small_case(tmp_path):
    data = b">s\nACGTACGTTTTTTTTT\nAATTAATT\n"
    counts = kc.restate(data, 4, True)[0]
    kcount = host_count(data, 4)
    path = str(tmp_path / "k4.txt")
    assert kcount.write(path, greater_than=0) == len(counts) and open(path, "rb").read() == kc.expected_lines(counts, 4, 0)
    # the 24 bases are one sequence (a line end is no break): 21 windows; nine T in a row are six TTTT, counted under AAAA
    assert open(path, "rb").read() == b"AAAA\t6\nAAAC\t1\nAACG\t1\nAATT\t2\nACGT\t2\nATTA\t3\nCGTA\t2\nGTAC\t1\nTAAA\t1\nTTAA\t2\n"
    assert kcount.write(path, greater_than=1) == 6 and open(path, "rb").read() == b"AAAA\t6\nAATT\t2\nACGT\t2\nATTA\t3\nCGTA\t2\nTTAA\t2\n"
    # both strands: the palindromes AATT, ACGT and TTAA are written once
    n = kcount.write(path, greater_than=1, both_strands=True)
    assert open(path, "rb").read() == b"AAAA\t6\nTTTT\t6\nAATT\t2\nACGT\t2\nATTA\t3\nTAAT\t3\nCGTA\t2\nTACG\t2\nTTAA\t2\n" and n == 9
    assert open(path, "rb").read() == kc.expected_lines(counts, 4, 1, both_strands=True)
    # the default is distinct = "0.9998"; p = 1 selects nothing, p = 0 everything
    assert kcount.write(path) == kcount.write(path, distinct="0.9998") and kcount.write(path, distinct="1") == 0 and open(path, "rb").read() == b""
    assert kcount.write(path, distinct="0") == len(counts)
    assert kcount.count("AAAA") == 6 and kcount.count("tttt") == 6 and kcount.count(b"ACGT") == 2 and kcount.counts(["CCCC", "TAAT", "AATT"]).tolist() == [0, 3, 2]
    forward = host_count(data, 4, canonical=False)
    assert forward.count("AAAA") == 0 and forward.count("TTTT") == 6 and forward.write(path, greater_than=5) == 1 and open(path, "rb").read() == b"TTTT\t6\n"


def test_written_k_mers_rise(tmp_path, table):
    kcount = host_count(table["random_megabase"], 8)
    path = str(tmp_path / "k8.txt")
    n = kcount.write(path, greater_than=20)
    lines = open(path, "rb").read().split(b"\n")[:-1]
    words = [ln.split(b"\t")[0] for ln in lines]
    assert n == len(lines) > 1000 and words == sorted(words) and len(set(words)) == len(words) and all(int(ln.split(b"\t")[1]) > 20 for ln in lines)
    kmers_, counts_ = kcount.select(20)
    assert len(kmers_) == n and np.all(np.diff(kmers_.astype(np.int64)) > 0) and counts_.dtype == np.uint32 and kmers_.dtype == np.uint64
    assert open(path, "rb").read() == kc.expected_lines(kc.restate(table["random_megabase"], 8, True)[0], 8, 20)


def test_more_selected_k_mers_than_the_first_capacity(table):
    kcount = host_count(table["random_megabase"], 11)
    counts = kc.restate(table["random_megabase"], 11, True)[0]
    got_k, got_c = kcount.select(0)
    assert len(got_k) == len(counts) > kmers._FIRST_SELECT and dict(zip(got_k.tolist(), got_c.tolist())) == counts


def test_argument_errors_come_before_any_work(tmp_path):
    missing = str(tmp_path / "no_such.fa")
    for kw in ({"k": 0}, {"k": 17}, {"k": 2.5}, {"k": True}, {"chunk_bytes": 15}, {"chunk_bytes": 0}, {"chunk_bytes": 64.0}):
        with pytest.raises(ValueError):
            kmers.count_kmers(missing, device="no such device", **kw)
    for kw in ({"distinct": "1.5"}, {"distinct": "-0.1"}, {"distinct": "abc"}, {"distinct": "1e-3"}, {"distinct": 1e-5}, {"distinct": ""}, {"distinct": "0.5.1"},
               {"distinct": "0.9998", "greater_than": 3}, {"greater_than": -1}, {"greater_than": 2.5}, {"k": 0}, {"chunk_bytes": 8}):
        with pytest.raises(ValueError):
            kmers.repetitive_kmers(missing, str(tmp_path / "never.txt"), device="no such device", **kw)
    assert not os.path.exists(str(tmp_path / "never.txt"))
    kcount = host_count(b">s\nACGTACGT\n", 4)
    for bad in ("ACG", "ACGTA", "ACGN", "AC-T", 5):
        with pytest.raises(ValueError):
            kcount.count(bad)
    with pytest.raises(ValueError):
        kcount.write(str(tmp_path / "never.txt"), distinct="0.5", greater_than=1)
    with pytest.raises(ValueError):
        kcount.write(str(tmp_path / "never.txt"), distinct="2")
    assert not os.path.exists(str(tmp_path / "never.txt"))


def test_a_stream_of_two_to_the_32_bases_is_refused():
    """The base counter is started 10 bases below the limit (coral_kmer_open's bases_before): 9 more bases pass, the tenth is refused."""
    near = (1 << 32) - 10
    ok = kmers.count_kmers(io.BytesIO(b">s\nACGTACGTA\n"), 4, device="cpu", _bases_before=near)
    assert ok.n_bases == (1 << 32) - 1 and ok.total == 6
    with pytest.raises(_lib.CoralHipError, match="2\\^32 bases"):
        kmers.count_kmers(io.BytesIO(b">s\nACGTACGTAC\n"), 4, device="cpu", _bases_before=near)
    # and it stays refused: through the C ABI, the feed after the refused one and finish fail too
    L = _lib.lib()
    table_ = np.zeros(256, dtype=np.uint32)
    h = C.c_void_p()
    assert L.coral_kmer_open(4, 1, -1, table_.ctypes.data, 0, None, 0, None, near, C.byref(h)) == 0
    assert L.coral_kmer_feed(h, b"ACGTACGTA", 9) == 0 and L.coral_kmer_feed(h, b"NNNN\n", 5) == 0 and L.coral_kmer_feed(h, b"A", 1) == -3
    assert L.coral_kmer_feed(h, b"N", 1) == -3 and L.coral_kmer_finish(h, (C.c_int64 * 8)(), None) == -3
    L.coral_kmer_close(h)
    assert L.coral_kmer_open(4, 1, -1, table_.ctypes.data, 0, None, 0, None, 1 << 32, C.byref(h)) == -1
    assert L.coral_kmer_table_bytes(15) == 4 << 30 and L.coral_kmer_table_bytes(16) == 16 << 30 and L.coral_kmer_table_bytes(17) < 0 and L.coral_kmer_table_bytes(0) < 0


def test_sanitizer_run_of_the_stand_alone_program(tmp_path, table):
    """Cases of the table through the stand-alone program (its own main) under AddressSanitizer and UBSan, on the CPU: whole and in
    pieces of 1, 7, 16, 17, 4 096 and 4 097 bytes, each piece an allocation of exactly its size.  Its answers are the library's."""
    exe, cases_bin, results_bin = str(tmp_path / "kmer_host"), str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    runs = [(name, k, canonical) for name in table if name != "random_megabase" for k, canonical in ((1, True), (4, False), (8, True))]
    runs.append(("random_megabase", 9, True))
    with open(cases_bin, "wb") as fp:
        for name, k, canonical in runs:
            fp.write(struct.pack("<iiq", k, int(canonical), len(table[name])) + table[name])
    run = subprocess.run([exe, cases_bin, results_bin], capture_output=True, text=True)
    assert run.returncode == 0 and "kmer_host: %d cases" % len(runs) in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    with open(results_bin, "rb") as fp:
        raw = fp.read()
    at = 0
    for name, k, canonical in runs:
        head = struct.unpack_from("<5q", raw, at)
        n = head[3]
        at += 40
        idx = np.frombuffer(raw, dtype="<u8", count=n, offset=at)
        at += 8 * n
        cnt = np.frombuffer(raw, dtype="<u4", count=n, offset=at)
        at += 4 * n
        want = kc.feed_in_pieces(table[name], k, canonical, 0)
        assert dict(zip(idx.tolist(), cnt.tolist())) == want[0] and list(head[:4]) == list(want[1].values()), (name, k)
        assert head[4] == (max(want[0].values()) if want[0] else 0), (name, k)
    assert at == len(raw)
