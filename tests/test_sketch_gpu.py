"""The minimizer sketch on the GPU (k_sketch_* of coral_amd/csrc/coral_sketch.hip) against the host backend (coral_sketch_host.h),
exactly: the minimizers of the shared case table of tests/sketch_cases.py - which tests/test_sketch_core.py holds against the
plain-Python restatement -, in pieces of awkward sizes, with contig ends, contig starts, N runs, ties and short contigs at the edges
of the sketch kernel's tiles, with more minimizers than the first capacity, with weights, and the sorted index with its lookup and
anchors."""
import ctypes as C
import functools
import io

import numpy as np
import pytest

from coral_amd import _lib, minimizers
from tests import kmer_cases, sketch_cases as SC

pytestmark = pytest.mark.gpu
GPU = "cuda:0"
WHOLE = 2 << 20                      # a piece that holds every text here


@functools.lru_cache(maxsize=None)
def host_rows(data: bytes, k, w, weights=None):
    """The host backend's index rows, computed once; None for a refused text."""
    try:
        return SC.index_rows(minimizers.sketch_reference(io.BytesIO(data), k, w, weights, device="cpu", chunk_bytes=WHOLE))
    except _lib.CoralHipError:
        return None


def device_index(data: bytes, k, w, weights=None, chunk_bytes=WHOLE, **kw):
    return minimizers.sketch_reference(io.BytesIO(data), k, w, weights, device=GPU, chunk_bytes=chunk_bytes, **kw)


def geometry():
    g = (C.c_int32 * 8)()
    assert _lib.lib().coral_sketch_geometry(g) == 0
    return dict(tile=g[0], carry=g[1])


@pytest.mark.parametrize("k,w", SC.KW)
def test_device_equals_host_on_the_case_table(k, w):
    for name, data in sorted(SC.cases().items()):
        want = host_rows(data, k, w)
        if want is None:
            with pytest.raises(_lib.CoralHipError):
                device_index(data, k, w)
            continue
        idx = device_index(data, k, w)
        host = minimizers.sketch_reference(io.BytesIO(data), k, w, device="cpu")
        assert SC.index_rows(idx) == want, name
        assert (idx.contig_names, idx.contig_lengths, idx.positions) == (host.contig_names, host.contig_lengths, host.positions), name


@pytest.mark.parametrize("piece", (16, 17, 4097, WHOLE))
def test_result_does_not_depend_on_the_pieces(piece):
    data = SC.six_records()
    idx = device_index(data, 15, 50, chunk_bytes=piece)
    assert SC.index_rows(idx) == host_rows(data, 15, 50) and len(idx.contig_names) == 6


def edge_texts(k, w):
    """Texts that put a contig end, a contig start, an N run, a run of ties and a contig with fewer than w k-mers at a tile's last
    position, at the next tile's first and one past it.  Fed whole, the symbol of the first header line stands at buffer index
    `carry`, contig a's base i at carry + 1 + i, and a second header line takes one index."""
    g = geometry()
    rng = np.random.RandomState(21)
    rb = kmer_cases.random_bases
    out = {}
    for at in (g["tile"] - 1, g["tile"], g["tile"] + 1, 2 * g["tile"] - 1, 2 * g["tile"]):
        i = at - g["carry"] - 1                                      # contig a's base at buffer index `at`
        tail = rb(rng, 700)
        out["contig_end", at] = b">a\n" + rb(rng, i + 1) + b"\n>b\n" + tail + b"\n"
        out["contig_start", at] = b">a\n" + rb(rng, i - 1) + b"\n>b\n" + tail + b"\n"
        for n in (3, w, w + 1):
            out["n_run_%d_starts" % n, at] = b">a\n" + rb(rng, i) + b"N" * n + tail + b"\n"
            out["n_run_%d_ends" % n, at] = b">a\n" + rb(rng, i - n + 1) + b"N" * n + tail + b"\n"
        out["ties_start", at] = b">a\n" + rb(rng, i) + b"A" * (2 * w + k) + tail + b"\n"
        out["ties_end", at] = b">a\n" + rb(rng, i - (2 * w + k) + 1) + b"A" * (2 * w + k) + tail + b"\n"
        out["ties_across", at] = b">a\n" + rb(rng, i - w) + b"AC" * (w + k) + tail + b"\n"
        short = max(k + w - 3, 0)                                    # w - 2 k-mers: the clipped single window (w = 1: no base at all)
        out["short_contig_ends", at] = b">a\n" + rb(rng, i - short - 1) + b"\n>s\n" + rb(rng, short) + b"\n>b\n" + tail + b"\n"
        out["short_contig_starts", at] = b">a\n" + rb(rng, i - 1) + b"\n>s\n" + rb(rng, short) + b"\n>b\n" + tail + b"\n"
        out["short_contig_across", at] = b">a\n" + rb(rng, i - 1 - short // 2) + b"\n>s\n" + rb(rng, short) + b"\n>b\n" + tail + b"\n"
    return out


@pytest.mark.parametrize("k,w", ((15, 50), (11, 5), (3, 256), (16, 256), (1, 1)))
def test_contig_ends_starts_n_runs_and_ties_at_the_tile_edges(k, w):
    for (what, at), data in edge_texts(k, w).items():
        want = host_rows(data, k, w)
        assert want is not None
        assert SC.index_rows(device_index(data, k, w)) == want, (what, at)
        assert SC.index_rows(device_index(data, k, w, chunk_bytes=1031)) == want, (what, at, "pieces")      # the same text at other buffer indices


def test_more_minimizers_than_the_first_capacity():
    data = kmer_cases.cases()["poly_a"]                              # 100 kb of A: density 1
    idx = device_index(data, 15, 50, _capacity=1000)
    assert minimizers.LAST_SKETCH["attempts"] == 2
    assert idx.n == 100_000 - 15 + 1 and SC.index_rows(idx) == host_rows(data, 15, 50)
    with pytest.raises(_lib.CoralHipError):
        class OneWay(io.RawIOBase):
            def __init__(self, b):
                self._fp = io.BytesIO(b)

            def readable(self):
                return True

            def readinto(self, b):
                return self._fp.readinto(b)
        minimizers.sketch_reference(OneWay(data), 15, 50, device=GPU, _capacity=1000)


def test_weights_on_the_device_at_k11():
    from coral_amd import kmers
    data = kmer_cases.random_megabase()[:300_000]
    kc = kmers.count_kmers(io.BytesIO(data), 11, device="cpu")
    listed = tuple(kc.select(3)[0].tolist())
    kc.close()
    assert len(listed) > 100
    want = host_rows(data, 11, 5, listed)
    assert want != host_rows(data, 11, 5)
    idx = device_index(data, 11, 5, listed)
    assert idx.weighted and SC.index_rows(idx) == want
    assert SC.index_rows(device_index(data, 11, 5, listed, chunk_bytes=50_001)) == want


def test_weights_on_the_device_at_k15_with_the_128_mib_bitmap():
    data = b">t\n" + kmer_cases.wrap(b"ACGGTCA" * 300, 60) + SC.six_records()
    tandem = [(b"ACGGTCA" * 4)[i:i + 15] for i in range(7)]
    assert _lib.lib().coral_sketch_bitmap_bytes(15) == 128 << 20
    want = host_rows(data, 15, 50, tuple(t.decode() for t in tandem))
    assert want != host_rows(data, 15, 50)
    assert SC.index_rows(device_index(data, 15, 50, [t.decode() for t in tandem])) == want


@pytest.fixture(scope="module")
def megabase():
    data = kmer_cases.random_megabase()
    host = minimizers.sketch_reference(io.BytesIO(data), 15, 50, device="cpu")
    dev = device_index(data, 15, 50, chunk_bytes=300_007)
    return data, host, dev


def test_device_sort_equals_the_host_index(megabase):
    _data, host, dev = megabase
    assert dev.n == host.n > 30_000
    assert all(np.array_equal(a, b) for a, b in zip(dev.arrays(), host.arrays()))
    keys = dev.arrays()[0]
    assert np.all(keys[1:] >= keys[:-1]) and (dev.contig_names, dev.contig_lengths) == (host.contig_names, host.contig_lengths)


def test_lookup_and_anchors_equal_the_host_backends(megabase, tmp_path):
    data, host, dev = megabase
    keys = host.arrays()[0]
    uniq, counts = np.unique(keys, return_counts=True)
    planted = uniq[counts >= 20]                                     # the 3 kb element stands 30 times
    assert len(planted) > 20
    rng = np.random.RandomState(4)
    query_keys = np.concatenate([uniq[:500], uniq[-500:], planted, rng.randint(0, 1 << 31, 500).astype(np.uint64), [0, (1 << 31) - 1]]).astype(np.uint64)
    for a, b in zip(dev.lookup(query_keys), host.lookup(query_keys)):
        assert np.array_equal(a, b)
    # reads: one that lies in a copy of the planted element, others from anywhere
    first = int(host.lookup(planted[:1])[0][0])
    contig, pos = int(host.arrays()[1][first]), int(host.arrays()[2][first])
    records = [b"".join(rec.split(b"\n")[1:]) for rec in data.split(b">")[1:]]
    lo = max(0, min(pos - 500, len(records[contig]) - 2000))
    reads = [records[contig][lo:lo + 2000], records[3][100:2100], kmer_cases.revcomp(records[5][1000:3000].replace(b"N", b"A")), records[7][:1500]]
    on_dev = minimizers.sketch_sequences(reads, 15, 50, device=GPU)
    on_host = minimizers.sketch_sequences(reads, 15, 50, device="cpu")
    assert all(np.array_equal(a, b) for a, b in zip(on_dev, on_host)) and len(on_dev[0]) > 100
    biggest = int(host.lookup(on_host[3])[1].max())
    assert biggest >= 20
    kept = None
    for max_occ in (10, 1000):
        got, want = dev.anchors(on_dev, max_occ=max_occ), host.anchors(on_host, max_occ=max_occ)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        kept = len(got[0]) if kept is None else kept
        assert len(got[0]) >= kept
    assert len(dev.anchors(on_dev, max_occ=1000)[0]) >= kept + biggest      # max_occ = 10 dropped the planted element, 1000 keeps it
    # a saved index, loaded onto the device, answers alike
    loaded = minimizers.MinimizerIndex.load(dev.save(str(tmp_path / "mega.cmi.npz")), device=GPU)
    assert all(np.array_equal(a, b) for a, b in zip(loaded.anchors(on_dev, max_occ=1000), host.anchors(on_host, max_occ=1000)))


def test_anchor_property_on_the_device():
    fasta, reads = SC.anchor_setup()
    k, w = 15, 50
    idx = device_index(fasta, k, w)
    sketch = minimizers.sketch_sequences([r[3] for r in reads], k, w, device=GPU)
    max_occ = int(np.unique(idx.arrays()[0], return_counts=True)[1].max())
    assert SC.check_anchor_property(idx, reads, k, sketch, max_occ) > 50 * 40


def test_a_session_closed_with_pieces_in_flight():
    """Through the C ABI: a device session at staging 16 is fed five pieces in one call - both staging buffers are retired and used
    again - and closed without coral_sketch_finish.  Close has to wait for what is in flight; a sketch of the same text afterwards
    equals the host backend's."""
    import torch
    L = _lib.lib()
    data = b">one\nACGTTGCAGGATTACAGATTACACGT\n>two\nGGGATCCNNACGTACGTTTGACCATGCAGGCTAAT\nACGTAG\n"
    assert len(data) == 80
    keys, values = torch.zeros(64, dtype=torch.int64, device=GPU), torch.zeros(64, dtype=torch.int64, device=GPU)
    ws_bytes = L.coral_sketch_workspace_bytes(16)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=GPU)
    stream = torch.cuda.current_stream(GPU)
    stream.synchronize()
    handle = C.c_void_p()
    assert L.coral_sketch_open(3, 4, 0, None, keys.data_ptr(), values.data_ptr(), 64, 16, ws.data_ptr(), ws_bytes, stream.cuda_stream, C.byref(handle)) == 0
    assert L.coral_sketch_feed(handle, data, len(data)) == 0
    L.coral_sketch_close(handle)
    assert SC.index_rows(device_index(data, 3, 4, chunk_bytes=16)) == host_rows(data, 3, 4)
    assert len(host_rows(data, 3, 4)) > 10
