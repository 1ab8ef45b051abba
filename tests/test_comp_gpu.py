"""The reference's per-bin composition on the GPU (k_comp_* of coral_amd/csrc/coral_comp.hip) against the host backend
(coral_comp_host.h), exactly: contigs, names, statistics and the three tables on the shared cases of tests/comp_cases.py - which
tests/test_comp_core.py holds against the plain-Python restatement - fed at the smallest staging size, and on texts built at the
edges of the kernels' launch geometry as coral_comp_geometry reports it; one run of the `composition` mode on both devices."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from coral_amd import CoRAL, _lib, composition
from tests import comp_cases as cc

pytestmark = pytest.mark.gpu
GPU = "cuda:0"
GUARD = 8                            # bins behind the capacity that must stay untouched


def geometry():
    g = (C.c_int32 * 8)()
    assert _lib.lib().coral_comp_geometry(g) == 0
    return dict(zip(("bytes_per_thread", "count_threads", "lanes", "headers_per_piece", "walk_threads", "min_staging", "load_bytes"), g))


def device_session(data, bin_size, capacity, staging):
    kept = {}

    def setup(cap, stage):
        L = _lib.lib()
        ws_bytes = int(L.coral_comp_workspace_bytes(stage))
        assert ws_bytes > 0
        tables = torch.zeros((3, cap + GUARD), dtype=torch.int32, device=GPU)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=GPU)
        torch.cuda.synchronize()
        kept["tables"] = tables
        return tables, ws, ws_bytes, torch.cuda.current_stream(GPU).cuda_stream, lambda: tables.cpu().numpy().view(np.uint32)

    out = cc.run_session([data], bin_size, capacity, device=0, staging=staging, stream_setup=setup)
    torch.cuda.synchronize()
    assert not bool(kept["tables"][:, capacity:].any()), "a counter behind the capacity was written"
    return out


@functools.lru_cache(maxsize=None)
def host_session(data, bin_size):
    bins = cc.run_session([data], bin_size, 1)[1][2]
    return cc.run_session([data], bin_size, max(bins, 1))


def check(data, bin_size, staging):
    want = host_session(data, bin_size)
    assert want[0] == 0
    got = device_session(data, bin_size, max(want[1][2], 1), staging)
    assert got[:4] == want[:4], (bin_size, staging, got[:2], want[:2])
    for k in (4, 5, 6):
        assert got[k] == want[k], (bin_size, staging, ("gc", "at", "masked")[k - 4], [i for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b][:10])
    return got


def one_line(rng, name, n):
    """A contig on one line, so that a position's byte offset is its coordinate plus the header's length."""
    return b">" + name + b"\n" + cc.random_sequence(rng, n) + b"\n"


def test_device_equals_host_on_the_cases_at_the_smallest_staging_size():
    g = geometry()
    assert g["min_staging"] == 16
    for name, (data, bin_sizes) in cc.cases().items():
        for b in bin_sizes:
            check(data, b, g["min_staging"])
            check(data, b, 17)
    for name in ("crlf", "empty_contig_between", "iupac_and_star"):
        check(cc.cases()[name][0], cc.cases()[name][1][0], 1 << 20)             # and each in one piece


def test_refusals_on_the_device():
    for text in (b"ACGT\n>a\nACGT\n", b"\n\nA>a\n", b">a\nAC\n>\nAC\n", b">a\nAC\n>"):
        assert device_session(text, 10, 8, 16)[0] == -4, text
        assert device_session(text, 10, 8, 4096)[0] == -4, text
    data = cc.cases()["empty_contig_between"][0]
    want = host_session(data, 5)
    rc, stats = device_session(data, 5, want[1][2] - 1, 16)[:2]                  # one bin short: the need is reported, nothing written behind
    assert rc == -3 and stats[:7] == want[1][:7]
    L = _lib.lib()
    t = torch.zeros(16, dtype=torch.int32, device=GPU)
    h = C.c_void_p()
    for staging, ws_bytes in ((15, 1 << 20), ((1 << 30) + 1, 1 << 20), (4096, 256)):
        assert L.coral_comp_open(10, 0, t.data_ptr(), t.data_ptr(), t.data_ptr(), 16, staging, t.data_ptr(), ws_bytes, None, C.byref(h)) == -1 and not h.value
    assert L.coral_comp_workspace_bytes(15) < 0 and L.coral_comp_workspace_bytes((1 << 30) + 1) < 0


def test_bins_and_contigs_across_piece_boundaries():
    g = geometry()
    rng = np.random.RandomState(21)
    tile = g["bytes_per_thread"] * g["count_threads"]
    # a bin that straddles a piece boundary: pieces of 5 000 bytes, bins of 3 000 positions, lines of 60
    data = b">straddle x\n" + cc.wrap(cc.random_sequence(rng, 40_000), 60) + b">second\n" + cc.wrap(cc.random_sequence(rng, 7_001), 60)
    got = check(data, 3000, 5000)
    assert got[3] == [40_000, 7_001]
    # a contig that spans three pieces of one workgroup's bytes each, and one of exactly two
    data = one_line(rng, b"three", 2 * tile + 100) + one_line(rng, b"next", 333) + one_line(rng, b"two", 2 * tile - 6)
    for b in (1000, 4096, 1 << 20):
        check(data, b, tile)
    check(data, 1000, tile + 1)
    check(data, 1000, tile - 1)


def test_more_headers_than_a_piece_or_a_wave_holds():
    g = geometry()
    rng = np.random.RandomState(22)
    many = 2 * g["headers_per_piece"] + 37
    # contigs of 0..6 positions: up to a dozen header lines within one thread's bytes, hundreds within a wave's
    data = b"".join(b">c%d\n" % k + cc.random_sequence(rng, k % 7) + (b"\n" if k % 7 else b"") for k in range(many))
    assert len(data) < 1 << 18
    got = check(data, 4, 1 << 18)                                              # one fed piece: it is cut at the table's size
    assert got[1][0] == many and got[3] == [k % 7 for k in range(many)]
    check(data, 1, 1 << 18)
    check(data, 4, 2000)                                                       # more than a wave's lanes of headers a piece, fewer than the table
    assert g["lanes"] < data[:2000].count(b">") < g["headers_per_piece"]
    # exactly the table's size, one more and one less in one piece
    for n in (g["headers_per_piece"] - 1, g["headers_per_piece"], g["headers_per_piece"] + 1):
        data = b"".join(b">h%d\nAC\n" % k for k in range(n))
        assert check(data, 2, 1 << 16)[1][0] == n


@pytest.mark.parametrize("span", ("thread", "wave"))
def test_bin_sizes_around_a_threads_and_a_waves_span(span):
    g = geometry()
    rng = np.random.RandomState(23)
    width = g["bytes_per_thread"] * (g["lanes"] if span == "wave" else 1)
    # the header is one load long, so that positions start on a thread's first byte; a second contig starts off every edge
    head = b">" + b"p" * (g["load_bytes"] - 2) + b"\n"
    assert len(head) == g["load_bytes"]
    data = head + cc.random_sequence(rng, 5 * width * 4 + 3) + b"\n>q\n" + cc.random_sequence(rng, 3 * width + 1)
    for b in (width - 1, width, width + 1):
        check(data, b, 1 << 20)
        check(data, b, 3 * width + 16)
    long_head = b">" + b"p" * (g["bytes_per_thread"] - 2) + b"\n"
    check(long_head + data[len(head):], width, 1 << 20)


def test_every_byte_its_own_bin_and_a_piece_that_is_all_header():
    g = geometry()
    rng = np.random.RandomState(24)
    data = b">a\n" + cc.wrap(cc.random_sequence(rng, 70_000), 70) + b">b\n" + cc.wrap(cc.random_sequence(rng, 3_000), 70)
    got = check(data, 1, 1 << 16)
    assert got[1][2] == 73_000 and max(got[4]) == 1
    # a header line longer than three pieces; the pieces in its middle are all header
    data = b">a\nACGT\n>long " + b"x" * 300 + b" > more\nGGCC\nA\n>" + b"n" * 200 + b"\nTT"
    for staging in (16, 64, 100):
        assert check(data, 3, staging)[2] == ["a", "long", "n" * 200]


def test_reference_composition_and_the_mode_on_both_devices(tmp_path, capsys):
    rng = np.random.RandomState(25)
    data = b"".join(b">chr%d desc\n" % k + cc.wrap(cc.random_sequence(rng, n), 60) for k, n in enumerate((150_000, 0, 99_999, 1_000, 1)))
    fasta = str(tmp_path / "ref.fa")
    with open(fasta, "wb") as fp:
        fp.write(data)
    dev, host = composition.reference_composition(fasta, 1000, device=GPU, chunk_bytes=100_000), composition.reference_composition(fasta, 1000, device="cpu")
    assert dev.chroms == host.chroms == ["chr%d" % k for k in range(5)] and dev.lengths == host.lengths and dev.totals == host.totals
    assert all(np.array_equal(x, y) for x, y in ((dev.gc, host.gc), (dev.at, host.at), (dev.masked, host.masked)))
    assert composition.LAST_COMPOSITION["attempts"] == 1
    small = composition.reference_composition(fasta, 10, device=GPU, _capacity=100)                  # too few bins at first: repeated once
    assert small.n_bins == 15_000 + 10_000 + 100 + 1 and int(small.gc.sum()) == int(host.gc.sum())
    out = {}
    for pipe, device in (("gpu", GPU), ("cpu", "cpu")):
        path = str(tmp_path / (pipe + ".tsv"))
        assert CoRAL.main(["composition", "--ref", fasta, "--bin_size", "500", "--output", path, "--device", device, "--chunk_bytes", "70000"]) == path
        out[pipe] = (open(path, "rb").read(), capsys.readouterr().out.replace(pipe + ".", "x."))
    assert out["gpu"] == out["cpu"] and "positions: 251000\n" in out["gpu"][1] and "bins: 503\n" in out["gpu"][1]
