"""The k-mer counter on the GPU (k_kmer_* of coral_amd/csrc/coral_kmer.hip) against the host backend (coral_kmer_host.h), exactly:
table entries, statistics, histogram and selections on the shared case table of tests/kmer_cases.py - which
tests/test_kmer_core.py holds against the plain-Python restatement -, at the 4 GiB and 16 GiB tables of k = 15 and 16, in pieces
of awkward sizes, at the edges of the count kernel's launch geometry, with a histogram tail, with more selected rows than the
first capacity, and one run of the `kmers` mode on both devices."""
import ctypes as C
import functools
import io

import numpy as np
import pytest

from coral_amd import CoRAL, _lib, kmers
from tests import kmer_cases as kc

pytestmark = pytest.mark.gpu
GPU = "cuda:0"
WHOLE = 2 << 20                      # a piece that holds every case of the table


@functools.lru_cache(maxsize=None)
def host_results(name_or_data, k, canonical):
    """The host backend's answers, computed once: (non-zero entries as sorted arrays, stats, histogram, selections at two
    thresholds)."""
    data = kc.cases()[name_or_data] if isinstance(name_or_data, str) else name_or_data
    return summary(kmers.count_kmers(io.BytesIO(data), k, canonical, device="cpu"))


def summary(kcount):
    values, nums = kcount.histogram()
    t_mid = kcount.threshold("0.5")
    entries = kcount.select(0)
    picked = kcount.select(t_mid)
    out = (entries[0].tolist(), entries[1].tolist(), dict(n_sequences=kcount.n_sequences, n_bases=kcount.n_bases, total=kcount.total, distinct=kcount.distinct,
                                                          max_count=kcount.max_count), values.tolist(), nums.tolist(), t_mid, picked[0].tolist(), picked[1].tolist())
    kcount.close()
    return out


def device_results(data, k, canonical=True, chunk_bytes=WHOLE):
    return summary(kmers.count_kmers(io.BytesIO(data), k, canonical, device=GPU, chunk_bytes=chunk_bytes))


def geometry():
    g = (C.c_int32 * 8)()
    assert _lib.lib().coral_kmer_geometry(g) == 0
    return dict(zip(("symbols_per_thread", "count_threads", "table_tile", "table_threads", "carried", "scatter_bytes", "lds_bins", "listed_from"), g))


@pytest.mark.parametrize("k", (1, 3, 8, 11))
def test_device_equals_host_on_the_case_table(k):
    for name, data in kc.cases().items():
        for canonical in (True, False):
            assert device_results(data, k, canonical) == host_results(name, k, canonical), (name, k, canonical)
    # the whole table's 4^k entries, not only what select returns
    data = kc.cases()["random_megabase"]
    dev, host = kmers.count_kmers(io.BytesIO(data), k, device=GPU, chunk_bytes=WHOLE), kmers.count_kmers(io.BytesIO(data), k, device="cpu")
    assert np.array_equal(dev.table(), host.table()) and dev.table().dtype == np.uint32 and len(dev.table()) == 4 ** k
    words = ["ACGTTGCAGGA"[:k], "A" * k, "T" * k, "GATTACAGATT"[:k]]
    assert dev.counts(words).tolist() == host.counts(words).tolist() and dev.count("A" * k) == dev.count("T" * k) > 0


def test_even_k_palindromes_on_the_device():
    data = kc.cases()["palindromes"]
    for k in (4, 6):
        for canonical in (True, False):
            assert device_results(data, k, canonical) == host_results("palindromes", k, canonical), (k, canonical)
    got = device_results(data, 4)
    assert dict(zip(got[0], got[1])) == kc.restate(data, 4, True)[0]


@pytest.mark.parametrize("name", ("random_megabase", "poly_a"))
def test_the_four_gib_table_of_k_15(name):
    data = kc.cases()[name]
    got = device_results(data, 15)
    assert got == host_results(name, 15, True)
    assert got[2]["total"] == kc.restate(data, 15, True)[1]["total"] and got[2]["distinct"] == kc.restate(data, 15, True)[1]["distinct"]


def test_the_sixteen_gib_table_of_k_16():
    data = b">ten_kb\n" + kc.wrap(kc.random_bases(np.random.RandomState(16), 10_000), 60)
    got = device_results(data, 16)
    assert got == host_results(data, 16, True)
    counts = kc.restate(data, 16, True)[0]
    assert dict(zip(got[0], got[1])) == counts and got[2]["total"] == 10_000 - 15 and max(got[0]) > 1 << 31


@pytest.mark.parametrize("chunk_bytes", (16, 17, 4097, WHOLE))
def test_the_result_does_not_depend_on_the_pieces(chunk_bytes):
    data = kc.cases()["random_megabase"]
    assert device_results(data, 8, True, chunk_bytes) == host_results("random_megabase", 8, True)
    if chunk_bytes > 17:
        assert device_results(data, 11, False, chunk_bytes) == host_results("random_megabase", 11, False)
        for name in ("long_header", "crlf", "empty_sequences_and_last_header", "gt_in_header_and_sequence"):
            assert device_results(kc.cases()[name], 3, True, chunk_bytes) == host_results(name, 3, True), name
    else:                             # a header longer than the piece, CR LF pairs across the cuts
        for name in ("long_header", "crlf", "empty_sequences_and_last_header", "gt_in_header_and_sequence", "n_runs"):
            assert device_results(kc.cases()[name], 3, True, chunk_bytes) == host_results(name, 3, True), name


@pytest.mark.parametrize("where", ("last_of_a_run", "first_of_the_next"))
def test_sequences_at_the_count_kernels_tile_edges(where):
    """One sequence each of tile - 1, tile, tile + 1 and 2 tile + 1 bases, tile = the symbols of one workgroup of k_kmer_count; no
    header and no line ends, so a byte's offset is its symbol's.  A break stands as the last symbol of a thread's run, or as the first
    of the next thread's: in the first workgroup's first and last threads and, where the sequence reaches it, in the second's."""
    g = geometry()
    spt, tile = g["symbols_per_thread"], g["symbols_per_thread"] * g["count_threads"]
    assert spt >= 16 and tile % spt == 0 and g["carried"] >= 15
    rng = np.random.RandomState(3)
    for n in (tile - 1, tile, tile + 1, 2 * tile + 1):
        seq = bytearray(kc.random_bases(rng, n))
        firsts = [spt, 2 * spt, tile - spt, tile, tile + spt, 2 * tile]
        for f in firsts:
            at = f - 1 if where == "last_of_a_run" else f
            if at < n:
                seq[at] = ord("N")
        data = bytes(seq)
        for k in (8, 15 if n == tile + 1 else 11):
            got = device_results(data, k)
            assert got == host_results(data, k, True), (n, k)
            assert got[2]["n_bases"] == n - data.count(b"N") and got[2]["n_sequences"] == 0
        # and the same symbols arriving in two pieces: the second piece's first thread warms up on the carried symbols
        assert device_results(data, 11, True, chunk_bytes=tile - 5) == host_results(data, 11, True), n


def test_a_histogram_whose_tail_is_used():
    """At k = 2 the ten canonical 2-mers of a megabase have counts around 62 500 (the four palindromes: binned) and 125 000 (the
    six others: above 65 535, so listed, not binned)."""
    g = geometry()
    got = device_results(kc.cases()["random_megabase"], 2)
    assert got == host_results("random_megabase", 2, True)
    assert g["listed_from"] == 65536 and sum(got[4]) == got[2]["distinct"] == 10
    assert sum(n for v, n in zip(got[3], got[4]) if v >= 65536) == 6 and sum(n for v, n in zip(got[3], got[4]) if g["lds_bins"] <= v < 65536) == 4
    # a count at the last binned value, one at the first listed one and one in the LDS bins' last and first-outside values
    parts = [b"A" * (65535 + 1), b"C" * (65536 + 1), b"AC" * ((g["lds_bins"] - 1 + 1) // 2) + b"A", b"AG" * (g["lds_bins"] // 2) + b"A"]
    data = b"".join(b">p%d\n" % i + p + b"\n" for i, p in enumerate(parts))
    got = device_results(data, 2, False)
    assert got == host_results(data, 2, False)
    assert 65535 in got[3] and 65536 in got[3]


def test_more_selected_k_mers_than_the_first_capacity():
    data = kc.cases()["random_megabase"]
    dev, host = kmers.count_kmers(io.BytesIO(data), 11, device=GPU, chunk_bytes=WHOLE), kmers.count_kmers(io.BytesIO(data), 11, device="cpu")
    got, want = dev.select(0), host.select(0)
    assert len(want[0]) > kmers._FIRST_SELECT and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.all(np.diff(got[0].astype(np.int64)) > 0)
    # the C ABI: the first call names the rows, nothing is written behind the capacity it was given
    import torch
    L = _lib.lib()
    kd, cd = torch.full((1001,), -1, dtype=torch.int64, device=GPU), torch.full((1001,), -1, dtype=torch.int32, device=GPU)
    n = C.c_int64(0)
    torch.cuda.synchronize()
    assert L.coral_kmer_select(dev._handle, 0, 1000, kd.data_ptr(), cd.data_ptr(), C.byref(n)) == -3 and n.value == len(want[0])
    assert np.array_equal(kd[:1000].cpu().numpy().view(np.uint64), want[0][:1000]) and int(kd[1000]) == -1 and int(cd[1000]) == -1
    assert L.coral_kmer_select(dev._handle, 0, 0, None, None, C.byref(n)) == -3 and n.value == len(want[0])


def test_a_session_closed_with_pieces_in_flight():
    """Through the C ABI: a device session at staging 16 is fed five pieces in one call - both staging buffers are retired and used
    again - and closed without coral_kmer_finish.  Close has to wait for what is in flight; a count of the same text afterwards
    equals the host backend's."""
    import torch
    L = _lib.lib()
    data = b">one\nACGTTGCAGGATTACAGATTACACGT\n>two\nGGGATCCNNACGTACGTTTGACCATGCAGGCTAAT\nACGTAG\n"
    assert len(data) == 80
    table = torch.zeros(4 ** 3, dtype=torch.int32, device=GPU)
    ws_bytes = L.coral_kmer_workspace_bytes(3, 16)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=GPU)
    stream = torch.cuda.current_stream(GPU)
    stream.synchronize()
    handle = C.c_void_p()
    assert L.coral_kmer_open(3, 1, 0, table.data_ptr(), 16, ws.data_ptr(), ws_bytes, stream.cuda_stream, 0, C.byref(handle)) == 0
    assert L.coral_kmer_feed(handle, data, len(data)) == 0
    L.coral_kmer_close(handle)
    assert device_results(data, 3, True, 16) == host_results(data, 3, True)
    assert host_results(data, 3, True)[2]["n_sequences"] == 2


def test_kmers_mode_on_both_devices(tmp_path, capsys):
    fasta = str(tmp_path / "ref.fa")
    with open(fasta, "wb") as fp:
        fp.write(kc.cases()["random_megabase"])
    out = {}
    for pipe, device in (("gpu", GPU), ("cpu", "cpu")):
        txt, hist = str(tmp_path / (pipe + ".txt")), str(tmp_path / (pipe + ".hist"))
        assert CoRAL.main(["kmers", "--ref", fasta, "--output", txt, "--k", "11", "--histogram", hist, "--device", device, "--chunk_bytes", "300000"]) == txt
        out[pipe] = (open(txt, "rb").read(), open(hist, "rb").read(), capsys.readouterr().out.replace(pipe + ".", "x."))
    assert out["gpu"] == out["cpu"]
    counts, stats, hist = kc.restate(kc.cases()["random_megabase"], 11, True)
    t = kc.threshold(hist, "0.9998")
    assert out["gpu"][0] == kc.expected_lines(counts, 11, t) and len(out["gpu"][0]) > 0
    assert "n_bases: %d\n" % stats["n_bases"] in out["gpu"][2] and "threshold: %d\n" % t in out["gpu"][2]
