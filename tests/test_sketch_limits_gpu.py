"""The sketch kernels (k_sketch_* of coral_amd/csrc/coral_sketch.hip) at the bounds their code is sized for, device against host
backend, exactly: k = 16 and the pair (16, 256) that fills the carry and the LDS arrays, capacities at every edge of the write pass
(row, workgroup, tile, the running total across pieces) with guard entries behind the arrays and guard bytes behind the workspace,
pieces with more header lines than one holds so that the contig table is filled as far as it ever is, and the index kernels (sort,
lookup, anchors) on synthetic arrays through the C ABI with NumPy as the reference: more queries than one trip of the capped grid
takes, capacities inside a key's run of entries, n around the radix sort's tiles.  The host backend is held against the plain-Python
restatement on the same texts by tests/test_sketch_core.py.  All geometry comes from coral_sketch_geometry."""
import ctypes as C
import functools
import io

import numpy as np
import pytest
import torch

from coral_amd import _lib, minimizers
from tests import kmer_cases, sketch_cases as SC

pytestmark = pytest.mark.gpu
GPU = "cuda:0"
ROOM = 1 << 13                       # a capacity that holds every sketch of the small texts here
# grid_of in coral_sketch.hip caps k_sketch_lookup and k_sketch_anchor_write at 4096 workgroups, and both are launched with 256
# threads: one trip of the grid-stride loop takes 4096 * 256 queries, so this many make some threads take a second one
MANY_QUERIES = 4096 * 256 + 257


@functools.lru_cache(maxsize=None)
def on_host(data: bytes, k, w, piece=0, capacity=ROOM):
    """The host backend's session, computed once; never a refusal here."""
    out = SC.feed_in_pieces(data, k, w, piece, capacity)
    assert out is not None and out[0] in (0, -3)
    return out


def assert_same_session(got, want, what):
    """rc, the counts (contigs, positions, minimizers, written ones), rows, names and lengths of two sessions."""
    assert want is not None and got[0] == want[0], what
    assert got[1][:4] == want[1][:4], what
    assert got[2] == want[2], what
    assert (got[3], got[4]) == (want[3], want[4]), what


# ---- a. the limits of k and w ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,w", SC.EDGE_KW)
def test_the_limits_of_k_and_w(k, w):
    data = SC.limits_text()
    want = on_host(data, k, w)
    assert want[0] == 0 and len(want[2]) > 0 and want[1][1] == 6000
    for piece in (0, 16, 17, 1031):
        assert_same_session(SC.feed_in_pieces(data, k, w, piece, ROOM, device=GPU), want, piece)


def test_weights_at_k16_with_the_512_mib_bitmap():
    """One upload of 4^16 bits.  The listed k-mers take a row out of the sketch and make the windows inside the AC tandem
    repetitive as a whole, so that keys with bit 32 go through the tile kernel's LDS arrays and into the output."""
    data, k, w, listed = SC.k16_weights_case()
    bitmap = SC.bitmap_of(listed, k)
    assert bitmap.nbytes == _lib.lib().coral_sketch_bitmap_bytes(16) == 512 << 20
    want = SC.feed_in_pieces(data, k, w, 0, ROOM, bitmap=bitmap)
    assert want[0] == 0 and want[2] != on_host(data, k, w)[2]
    SC.assert_bit_32_marks_the_listed(data, want[2], listed)
    got = SC.feed_in_pieces(data, k, w, 0, ROOM, bitmap=bitmap, device=GPU)
    assert_same_session(got, want, "weighted")
    SC.assert_bit_32_marks_the_listed(data, got[2], listed)


# ---- b. capacity ----------------------------------------------------------------------------------------------------------------
def capacity_runs(data, k, w, capacities, piece):
    full = on_host(data, k, w, piece, 1 << 16)
    assert full[0] == 0
    n = len(full[2])
    for cap in sorted(set(c for c in capacities if c >= 0)):
        want = on_host(data, k, w, piece, cap)
        assert want[0] == (-3 if cap < n else 0) and want[2] == full[2][:cap]      # the header's contract, on the host
        got = SC.feed_in_pieces(data, k, w, piece, cap, device=GPU)                # (the guards are asserted inside)
        assert (got[0], got[1][2], got[1][3]) == (want[0], n, min(cap, n)), cap
        assert got[1][:4] == want[1][:4], cap
        assert got[2] == full[2][:cap], cap


@pytest.mark.parametrize("piece", (0, 1031))
def test_capacities_at_the_edges_of_the_write_pass(piece):
    """poly-A at (5, 4): density 1, so output rank r is contig position r, which stands at buffer index carry + 1 + r when the
    text is fed whole.  The cut falls into the first row of a tile, at a wave's and a workgroup's end, at a tile's end (the next
    tile's `first` is the capacity: it writes nothing) and at the text's end; in pieces it falls into a later piece, where the
    total of the pieces before is added."""
    tile, carry, block = SC.geometry()[:3]
    data = SC.poly_a_6200()
    n = 6196
    assert len(on_host(data, 5, 4, 0, 1 << 16)[2]) == n > 2 * tile
    edges = [tile - carry - 1, 2 * tile - carry - 1]                 # the ranks of the first positions of the second and the third tile
    caps = [0, 1, 63, 64, 65, block - 1, block, block + 1, n - 1, n, n + 1] + [e + d for e in edges for d in (-1, 0, 1)]
    capacity_runs(data, 5, 4, caps, piece)


@pytest.mark.parametrize("piece", (0, 1031))
def test_capacities_at_a_tile_edge_at_the_usual_density(piece):
    """six_records() at (15, 50), about 2 / (w + 1) of the positions: the capacities are the number of minimizers in front of
    buffer index `tile`, that number - 1 and + 1, and the count in front of a tile that has none, where there is one."""
    tile, carry = SC.geometry()[:2]
    data = SC.six_records()
    _rc, _stats, rows, _names, lengths = on_host(data, 15, 50, 0, 1 << 16)
    first = np.concatenate([[0], np.cumsum(np.array(lengths) + 1)])[:-1] + carry + 1      # the buffer index of every contig's position 0, fed whole
    at = np.array([first[c] + p for _key, c, p, _s in rows])
    per_tile = np.bincount(at // tile)
    assert len(per_tile) > 2 and per_tile[0] > 1
    caps = [int(per_tile[0]) + d for d in (-1, 0, 1)]
    caps += [int(per_tile[:t].sum()) for t in range(1, len(per_tile)) if per_tile[t] == 0]
    capacity_runs(data, 15, 50, caps, piece)


# ---- c. the contig table --------------------------------------------------------------------------------------------------------
def header_texts():
    return dict(many_headers=SC.many_headers_text(SC.geometry()), one_base_contigs=SC.one_base_contigs())


def test_the_many_headers_text_fills_the_contig_table():
    """A piece's table holds the carried contig starts - at most one in front of the carry and one a carried symbol - and its own,
    at most max_bound: 1 + carry + max_bound entries, when the carry is all contig starts and the piece has max_bound header
    lines.  Fed whole, the text's first piece is max_bound empty contigs, more than the carry holds, and its second max_bound
    header lines again."""
    _tile, carry, _block, _items, max_bound, table_cap = SC.geometry()[:6]
    assert 1 + carry + max_bound <= table_cap
    lines = header_texts()["many_headers"].split(b"\n")
    assert max_bound > carry and all(line == b">x" for line in lines[:2 * max_bound])
    assert lines[2 * max_bound - carry - 1:2 * max_bound] == [b">x"] * (carry + 1)      # a run of more than `carry` empty contigs in front of max_bound header lines, twice over


@pytest.mark.parametrize("k,w", SC.MANY_HEADERS_KW)
@pytest.mark.parametrize("text", ("many_headers", "one_base_contigs"))
def test_more_header_lines_than_a_piece_holds(text, k, w):
    data = header_texts()[text]
    max_bound = SC.geometry()[4]
    want = on_host(data, k, w)
    assert want[0] == 0 and want[1][0] == len(want[3]) > 2 * max_bound
    for piece in (0, 16, 3073):                                      # whole: cut at every max_bound header lines
        assert_same_session(SC.feed_in_pieces(data, k, w, piece, ROOM, device=GPU), want, piece)
    idx = minimizers.sketch_reference(io.BytesIO(data), k, w, device=GPU)
    host = minimizers.sketch_reference(io.BytesIO(data), k, w, device="cpu")
    assert SC.index_rows(idx) == SC.index_rows(host) == SC.sorted_rows(want[2])
    assert (idx.contig_names, idx.contig_lengths, idx.positions) == (host.contig_names, host.contig_lengths, host.positions) == (want[3], want[4], want[1][1])


def test_sketch_sequences_of_more_reads_than_a_piece_holds():
    rng = np.random.RandomState(34)
    reads = [kmer_cases.random_bases(rng, int(n)) for n in rng.randint(0, 81, 3000)]
    assert len(reads) > 2 * SC.geometry()[4]
    got = minimizers.sketch_sequences(reads, 15, 50, device=GPU)
    want = minimizers.sketch_sequences(reads, 15, 50, device="cpu")
    assert want is not None and len(want[0]) > 2000 and len(set(want[0].tolist())) > 2000
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))


# ---- d. the index on synthetic arrays -------------------------------------------------------------------------------------------
def up(a):
    """A numpy array -> a device tensor of the same bytes."""
    a = np.ascontiguousarray(a)
    signed = {8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize]
    return torch.from_numpy(a.view(signed).copy()).to(GPU)


def into_guarded(a):
    """A numpy array of 8-byte entries -> a device array of them with SENTINEL guard entries behind."""
    t = SC.guarded(len(a), GPU)
    t[:len(a)] = up(a)
    return t


def down(t, n):
    return t[:n].cpu().numpy().view(np.uint64)


def stream_of():
    torch.cuda.set_device(GPU)
    s = torch.cuda.current_stream(GPU)
    s.synchronize()
    return s


def synthetic_pairs(rng, k, n):
    """n keys below 2^(2k + 1) out of at most n / 8 distinct values, half of those with the repetitive bit 2k, and values 0 .. n - 1."""
    n_distinct = max(1, min(n // 8, 2 << 2 * k))
    pool = rng.randint(0, 1 << 2 * k, n_distinct, dtype=np.uint64) | ((np.arange(n_distinct, dtype=np.uint64) & np.uint64(1)) << np.uint64(2 * k))
    return pool[rng.randint(0, n_distinct, n)], np.arange(n, dtype=np.uint64)


@pytest.mark.parametrize("k", (1, 8, 15, 16))
def test_sort_is_the_stable_sort_of_numpy(k):
    L = _lib.lib()
    rng = np.random.RandomState(40 + k)
    for n in (0, 1, 2, 255, 256, 257, 100_003):
        keys, values = synthetic_pairs(rng, k, n)
        order = np.argsort(keys, kind="stable")
        if n > 2:
            assert len(np.unique(keys)) <= n // 8 and (keys >> np.uint64(2 * k)).max() == 1 and (keys >> np.uint64(2 * k)).min() == 0
        hk, hv = keys.copy(), values.copy()
        assert L.coral_sketch_sort(-1, hk.ctypes.data, hv.ctypes.data, n, k, None, 0, None) == 0
        assert np.array_equal(hk, keys[order]) and np.array_equal(hv, values[order]), n
        dk, dv = into_guarded(keys), into_guarded(values)
        ws_bytes = int(L.coral_sketch_sort_workspace_bytes(n))
        ws = SC.guarded_workspace(ws_bytes, GPU)
        stream = stream_of()
        assert L.coral_sketch_sort(0, dk.data_ptr(), dv.data_ptr(), n, k, ws.data_ptr(), ws_bytes, stream.cuda_stream) == 0
        assert np.array_equal(down(dk, n), keys[order]), n
        assert np.array_equal(down(dv, n), values[order]), n          # ties in their first order
        SC.assert_untouched(dk, n, n)
        SC.assert_untouched(dv, n, n)
        SC.assert_workspace_guard(ws, ws_bytes, n)


def sorted_keys_with_duplicates(rng, n):
    return np.sort(rng.randint(0, 1 << 33, max(1, n // 3), dtype=np.uint64)[rng.randint(0, max(1, n // 3), n)]) if n else np.zeros(0, dtype=np.uint64)


@pytest.mark.parametrize("n", (0, 1, 1000))
def test_lookup_of_more_queries_than_one_trip_of_the_grid(n):
    L = _lib.lib()
    rng = np.random.RandomState(50 + n)
    keys = sorted_keys_with_duplicates(rng, n)
    nq = MANY_QUERIES
    query = rng.randint(0, 1 << 33, nq, dtype=np.uint64)                        # absent ones, nearly all
    if n:
        present = rng.rand(nq) < 0.5
        query[present] = keys[rng.randint(0, n, int(present.sum()))]
        assert len(np.unique(keys)) < n or n == 1
    query[[0, 1, nq - 2, nq - 1]] = np.array([0, 0xFFFFFFFFFFFFFFFF, 0, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    want_first = np.searchsorted(keys, query, side="left").astype(np.int64)
    want_count = np.searchsorted(keys, query, side="right").astype(np.int64) - want_first
    assert (want_count[4096 * 256:] > 0).any() == (n > 0)            # the second trip finds entries too
    hf, hc = np.full(nq, -7, dtype=np.int64), np.full(nq, -7, dtype=np.int64)
    assert L.coral_sketch_lookup(-1, keys.ctypes.data if n else None, n, query.ctypes.data, nq, hf.ctypes.data, hc.ctypes.data, None) == 0
    assert np.array_equal(hf, want_first) and np.array_equal(hc, want_count)
    dkeys, dq = up(keys) if n else None, up(query)
    first, count = SC.guarded(nq, GPU), SC.guarded(nq, GPU)
    stream = stream_of()
    assert L.coral_sketch_lookup(0, dkeys.data_ptr() if n else None, n, dq.data_ptr(), nq, first.data_ptr(), count.data_ptr(), stream.cuda_stream) == 0
    assert np.array_equal(down(first, nq).view(np.int64), want_first)
    assert np.array_equal(down(count, nq).view(np.int64), want_count)
    SC.assert_untouched(first, nq)
    SC.assert_untouched(count, nq)


@functools.lru_cache(maxsize=None)
def anchor_index():
    """1 000 sorted entries: 390 keys with 1 entry, 100 with 2, 10 with 20 and 10 with 21; values of distinct (contig, pos) and
    either strand."""
    rng = np.random.RandomState(60)
    counts = rng.permutation([1] * 390 + [2] * 100 + [20] * 10 + [21] * 10)
    uniq = np.sort(rng.choice(1 << 20, len(counts), replace=False).astype(np.uint64)) << np.uint64(11)
    keys = np.repeat(uniq, counts)
    values = (rng.randint(0, 50, 1000).astype(np.uint64) << np.uint64(32)) | (rng.choice(1 << 20, 1000, replace=False).astype(np.uint64) << np.uint64(1)) | rng.randint(0, 2, 1000).astype(np.uint64)
    assert len(keys) == 1000
    return keys, values, uniq


def anchor_queries(rng, nq, uniq, present):
    """nq query minimizers, a share `present` of them (and the last 257) with keys of the index, the others with absent ones."""
    qkey = rng.randint(0, 1 << 33, nq, dtype=np.uint64) | np.uint64(1)       # (odd: the index's keys are multiples of 2048)
    hit = rng.rand(nq) < present
    hit[-257:] = True
    qkey[hit] = uniq[rng.randint(0, len(uniq), int(hit.sum()))]
    return rng.randint(0, 1 << 20, nq).astype(np.uint32), rng.randint(0, 1 << 16, nq).astype(np.uint32), rng.randint(0, 2, nq).astype(np.uint8), qkey


def expand_plainly(keys, values, queries, max_occ):
    """The anchors by the header's words: query order, then index order; the entry's value with its strand bit ^ the query's."""
    query, qpos, qstrand, qkey = queries
    first = np.searchsorted(keys, qkey, side="left")
    count = np.searchsorted(keys, qkey, side="right") - first
    a_query, a_ref = [], []
    for i in np.flatnonzero((count > 0) & (count <= max_occ)).tolist():
        for e in range(int(first[i]), int(first[i] + count[i])):
            a_query.append(int(query[i]) << 32 | int(qpos[i]))
            a_ref.append(int(values[e]) ^ int(qstrand[i]))
    emitted = np.where(count <= max_occ, count, 0)
    return np.array(a_query, dtype=np.uint64), np.array(a_ref, dtype=np.uint64), emitted


def anchors_on_both(keys, values, queries, max_occ, capacity, want_q, want_r):
    """coral_sketch_anchors on the host and on the device at one capacity, both against the plain expansion."""
    L = _lib.lib()
    query, qpos, qstrand, qkey = queries
    nq, n, total = len(qkey), len(keys), len(want_q)
    written, want_rc = min(capacity, total), 0 if capacity >= total else -3
    what = (max_occ, capacity, total)
    hq, hr, hn = np.full(capacity + 1, SC.SENTINEL, dtype=np.uint64), np.full(capacity + 1, SC.SENTINEL, dtype=np.uint64), C.c_int64(-1)
    assert L.coral_sketch_anchors(-1, keys.ctypes.data, values.ctypes.data, n, query.ctypes.data, qpos.ctypes.data, qstrand.ctypes.data, qkey.ctypes.data, nq, max_occ, capacity,
                                  hq.ctypes.data if capacity else None, hr.ctypes.data if capacity else None, None, 0, None, C.byref(hn)) == want_rc, what
    assert hn.value == total and np.array_equal(hq[:written], want_q[:written]) and np.array_equal(hr[:written], want_r[:written]), what
    assert (hq[written:] == SC.SENTINEL).all() and (hr[written:] == SC.SENTINEL).all(), what
    dev = [up(a) for a in (keys, values, query, qpos, qstrand, qkey)]
    aq, ar, dn = SC.guarded(capacity, GPU), SC.guarded(capacity, GPU), C.c_int64(-1)
    ws_bytes = int(L.coral_sketch_anchors_workspace_bytes(nq))
    ws = SC.guarded_workspace(ws_bytes, GPU)
    stream = stream_of()
    rc = L.coral_sketch_anchors(0, dev[0].data_ptr(), dev[1].data_ptr(), n, dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(), dev[5].data_ptr(), nq, max_occ, capacity,
                                aq.data_ptr() if capacity else None, ar.data_ptr() if capacity else None, ws.data_ptr(), ws_bytes, stream.cuda_stream, C.byref(dn))
    assert (rc, dn.value) == (want_rc, total), what
    assert np.array_equal(down(aq, written), want_q[:written]), what
    assert np.array_equal(down(ar, written), want_r[:written]), what
    SC.assert_untouched(aq, written, what)                           # nothing behind the written ones, the guard included
    SC.assert_untouched(ar, written, what)
    SC.assert_workspace_guard(ws, ws_bytes, what)


@pytest.mark.parametrize("max_occ", (0, 1, 20, 21))
def test_anchors_at_max_occ_and_at_capacities_inside_a_run(max_occ):
    """A key with exactly max_occ entries is kept, one with max_occ + 1 is dropped; capacities: all anchors, one fewer, a cut
    inside one key's run of entries, none."""
    keys, values, uniq = anchor_index()
    queries = anchor_queries(np.random.RandomState(61), 700, uniq, 0.5)
    want_q, want_r, emitted = expand_plainly(keys, values, queries, max_occ)
    total = len(want_q)
    assert total == int(emitted.sum()) and (total > 0) == (max_occ > 0)
    assert sorted(set(emitted.tolist())) == [c for c in (0, 1, 2, 20, 21) if c <= max_occ]      # every count up to max_occ is there, none above
    capacities = {total, total - 1, 0}
    runs = np.flatnonzero(emitted >= 2)
    if len(runs):
        i = runs[len(runs) // 2]
        capacities.add(int(emitted[:i].sum() + emitted[i] // 2))
    else:
        assert max_occ < 2
    for capacity in sorted(c for c in capacities if c >= 0):
        anchors_on_both(keys, values, queries, max_occ, capacity, want_q, want_r)


def test_anchors_of_more_queries_than_one_trip_of_the_grid():
    keys, values, uniq = anchor_index()
    queries = anchor_queries(np.random.RandomState(62), MANY_QUERIES, uniq, 0.01)
    want_q, want_r, emitted = expand_plainly(keys, values, queries, 20)
    total = len(want_q)
    assert emitted[4096 * 256:].sum() > 0 and total > 10_000          # the second trip writes anchors too
    anchors_on_both(keys, values, queries, 20, total, want_q, want_r)
    anchors_on_both(keys, values, queries, 20, total - 1, want_q, want_r)


def test_anchors_in_an_empty_index():
    """No entries and no arrays: no anchors on the host and on the device, whatever max_occ, and nothing written."""
    queries = anchor_queries(np.random.RandomState(63), 1000, anchor_index()[2], 0.5)
    L = _lib.lib()
    dq = [up(a) for a in queries]
    ws_bytes = int(L.coral_sketch_anchors_workspace_bytes(1000))
    for max_occ in (0, 5):
        hq, hr, hn = np.full(16, SC.SENTINEL, dtype=np.uint64), np.full(16, SC.SENTINEL, dtype=np.uint64), C.c_int64(-1)
        assert L.coral_sketch_anchors(-1, None, None, 0, queries[0].ctypes.data, queries[1].ctypes.data, queries[2].ctypes.data, queries[3].ctypes.data, 1000, max_occ, 16, hq.ctypes.data,
                                      hr.ctypes.data, None, 0, None, C.byref(hn)) == 0
        assert hn.value == 0 and (hq == SC.SENTINEL).all() and (hr == SC.SENTINEL).all()
        aq, ar, dn = SC.guarded(16, GPU), SC.guarded(16, GPU), C.c_int64(-1)
        ws = SC.guarded_workspace(ws_bytes, GPU)
        stream = stream_of()
        assert L.coral_sketch_anchors(0, None, None, 0, dq[0].data_ptr(), dq[1].data_ptr(), dq[2].data_ptr(), dq[3].data_ptr(), 1000, max_occ, 16, aq.data_ptr(), ar.data_ptr(), ws.data_ptr(),
                                      ws_bytes, stream.cuda_stream, C.byref(dn)) == 0
        assert dn.value == 0
        SC.assert_untouched(aq, 0, max_occ)
        SC.assert_untouched(ar, 0, max_occ)
        SC.assert_workspace_guard(ws, ws_bytes, max_occ)
