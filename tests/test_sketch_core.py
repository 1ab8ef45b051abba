"""The minimizer sketch on the CPU: coral_sketch_core.h through the host backend (coral_sketch_host.h, coral_sketch.cpp) against the
brute-force restatement of tests/sketch_cases.py - at the limits of k and w and with more header lines than a device piece holds
too -, the sorted index with its lookup and anchors, the weights, the capacities around the number of minimizers, the capacity
retry and the saved file.  Every result is integers: every comparison is exact."""
import io

import numpy as np
import pytest

from coral_amd import _lib, minimizers
from tests import kmer_cases, sketch_cases as SC


def host_index(data: bytes, k, w, weights=None, chunk_bytes=1 << 20, **kw):
    return minimizers.sketch_reference(io.BytesIO(data), k, w, weights, device="cpu", chunk_bytes=chunk_bytes, **kw)


# ---- the rule -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,inputs,expected", [(4, (0, 1, 255, 0x67), (67, 134, 0, 56)),
                                               (15, (0, 1, 4 ** 15 - 1, 0x1234567), (1072721685, 932509926, 140824814, 94922518)),
                                               (16, (0, 1), (4290886808, 3079993582))])
def test_hash64_known_values(k, inputs, expected):
    assert tuple(minimizers.hash64(x, k) for x in inputs) == expected
    assert tuple(SC.hash64(x, k) for x in inputs) == expected


def test_hash64_is_a_permutation_at_k4():
    assert sorted(minimizers.hash64(x, 4) for x in range(256)) == list(range(256))


def test_native_hash_equals_python_through_single_kmer_contigs():
    """A contig of exactly k bases is one window of one k-mer: its key is the native hash64 of its canonical form."""
    rng = np.random.RandomState(3)
    for k in (4, 15, 16):
        seqs = [kmer_cases.random_bases(rng, k) for _ in range(40)]
        q, pos, strand, key = minimizers.sketch_sequences(seqs, k, 7, device="cpu")
        for i, p, s, v in zip(q.tolist(), pos.tolist(), strand.tolist(), key.tolist()):
            fwd, rev = kmer_cases.kmer_int(seqs[i]), kmer_cases.kmer_int(kmer_cases.revcomp(seqs[i]))
            assert (p, s, v) == (0, int(rev < fwd), minimizers.hash64(min(fwd, rev), k))
        assert sorted(q.tolist()) == [i for i, s in enumerate(seqs) if s != kmer_cases.revcomp(s)]


def test_known_answer():
    assert SC.minimizers_of(SC.KNOWN_TEXT, 5, 4) == SC.KNOWN_ANSWER
    rc, stats, rows, names, lengths = SC.feed_in_pieces(b">known\n" + SC.KNOWN_TEXT + b"\n", 5, 4, 0, 64)
    assert rc == 0 and names == ["known"] and lengths == [len(SC.KNOWN_TEXT)]
    assert [(p, s, key) for key, _c, p, s in rows] == SC.KNOWN_ANSWER
    assert rows[2][0] == rows[3][0] and (rows[2][3], rows[3][3]) == (1, 0)       # positions 8 and 9: reverse complements, a tie


@pytest.mark.parametrize("k,w", SC.KW)
@pytest.mark.parametrize("name", sorted(SC.cases()))
def test_host_backend_equals_the_restatement(name, k, w):
    data = SC.cases()[name]
    want = SC.restate(data, k, w)
    rc, stats, rows, names, lengths = SC.feed_in_pieces(data, k, w, 0, 1 << 16)
    if want == SC.REFUSED:
        assert rc == -4                                              # CORAL_ERR_FORMAT, as the composition session
        return
    assert rc == 0
    assert (names, lengths) == (want[0], want[1])
    assert rows == want[2]
    assert stats[:4] == [len(want[0]), sum(want[1]), len(want[2]), len(want[2])]


@pytest.mark.parametrize("k,w", SC.EDGE_KW)
def test_host_backend_equals_the_restatement_at_the_limits_of_k_and_w(k, w):
    """k = 16 (the mask is 2^32 - 1, the repetitive bit is bit 32), k = 1 and 2 (every second 2-mer can be a palindrome), w = 1 and
    w = 256, and the pair (16, 256) that the device's carry and LDS arrays are sized for."""
    texts = [SC.limits_text()] + ([SC.cases()["contigs_around_k_and_w"]] if (k, w) == (16, 256) else [])
    for data in texts:
        names, lengths, want = SC.restate(data, k, w)
        assert len(want) > 0
        for piece in (0, 17):
            rc, stats, rows, got_names, got_lengths = SC.feed_in_pieces(data, k, w, piece, 1 << 13)
            assert rc == 0 and (got_names, got_lengths) == (names, lengths)
            assert rows == want
            assert stats[:4] == [len(names), sum(lengths), len(want), len(want)]
    if (k, w) == (16, 1):                                            # every valid position is chosen: keys that need all 32 bits
        assert max(key for key, *_ in SC.restate(SC.limits_text(), k, w)[2]) >= 1 << 31


@pytest.mark.parametrize("k,w", SC.MANY_HEADERS_KW)
@pytest.mark.parametrize("text", ("many_headers", "one_base_contigs"))
def test_more_header_lines_than_a_device_piece_holds(text, k, w):
    g = SC.geometry()
    data = SC.many_headers_text(g) if text == "many_headers" else SC.one_base_contigs()
    names, lengths, want = SC.restate(data, k, w)
    if text == "many_headers":
        assert (len(names), sum(lengths)) == (4 * g[4] + 1406, 308)
        assert len(want) == {(3, 4): 131, (16, 256): 1, (1, 1): 308}[k, w]      # recorded from the restatement: pins the text's generator
    else:
        assert (len(names), sum(lengths)) == (3000, 3000) and len(want) == (3000 if k == 1 else 0)      # a minimizer a contig, or no k-mer at all
    for piece in (0, 16, 3073):
        rc, stats, rows, got_names, got_lengths = SC.feed_in_pieces(data, k, w, piece, 1 << 12)
        assert rc == 0 and (got_names, got_lengths) == (names, lengths)
        assert rows == want
        assert stats[:4] == [len(names), sum(lengths), len(want), len(want)]


def test_expected_densities_of_the_table():
    """poly-A: every k-mer position; AC tandem: its two k-mers alternate, so every second position (every one at w = 1); ACGT
    tandem at k = 8, w = 1: the k-mers at even positions are their own reverse complements and invalid, the odd ones are chosen."""
    cases = SC.cases()
    assert len(SC.restate(cases["poly_a"], 5, 4)[2]) == 3000 - 5 + 1
    assert len(SC.restate(cases["tandem_ac"], 5, 4)[2]) == (3000 - 5 + 1) // 2
    assert [p for _key, _c, p, _s in SC.restate(b">pal\n" + b"ACGT" * 200 + b"\n", 8, 1)[2]] == list(range(1, 800 - 8 + 1, 2))
    assert len(SC.restate(cases["tandem_ac"], 8, 1)[2]) == 3000 - 8 + 1


@pytest.mark.parametrize("piece", (16, 17, 4097, 0))
def test_result_does_not_depend_on_the_pieces(piece):
    data = SC.six_records()
    whole = SC.feed_in_pieces(data, 15, 50, 0, 1 << 16)
    assert whole[0] == 0 and len(whole[2]) > 500 and len(whole[3]) == 6
    assert SC.feed_in_pieces(data, 15, 50, piece, 1 << 16) == whole
    assert whole[2] == SC.restate(data, 15, 50)[2]


def test_python_pieces_and_host_blocks():
    """chunk_bytes of sketch_reference, and a contig longer than the host backend's block of undecided keys."""
    rng = np.random.RandomState(5)
    data = b">long\n" + kmer_cases.wrap(kmer_cases.random_bases(rng, 150_000), 60) + b">short\nACGTTGCAGGATCCA\n"
    a, b = host_index(data, 11, 5, chunk_bytes=4097), host_index(data, 11, 5)
    assert SC.index_rows(a) == SC.index_rows(b) == SC.sorted_rows(SC.restate(data, 11, 5)[2])
    assert a.contig_names == ["long", "short"] and a.contig_lengths == [150_000, 15] and a.positions == 150_015


# ---- weights ------------------------------------------------------------------------------------------------------------------------
def test_a_repetitive_kmer_loses_to_any_other():
    k, w = 5, 4
    data = b">known\n" + SC.KNOWN_TEXT + b"\n"
    plain = SC.restate(data, k, w)[2]
    smallest = min(plain)                                            # (key, contig, pos, strand) of the smallest key
    seq = SC.KNOWN_TEXT[smallest[2]:smallest[2] + k]
    rep = frozenset([SC.canonical(seq)])
    want = SC.restate(data, k, w, rep)[2]
    assert want != plain and all(key < 4 ** k for key, *_ in want)   # the repetitive k-mer is chosen nowhere: every window has another
    for weights in ([seq.decode()], [seq.lower()], [kmer_cases.revcomp(seq)], [SC.canonical(seq)]):
        assert SC.index_rows(host_index(data, k, w, weights)) == SC.sorted_rows(want)
    assert host_index(data, k, w, [seq]).weighted and not host_index(data, k, w).weighted


def test_an_all_repetitive_window_still_yields_its_minimum():
    k, w = 5, 4
    data = b">a\n" + b"A" * 40 + b"\n>b\n" + SC.KNOWN_TEXT + b"\n"
    rows = SC.index_rows(host_index(data, k, w, ["AAAAA"]))
    want = SC.restate(data, k, w, frozenset([0]))[2]
    assert rows == SC.sorted_rows(want)
    poly = [r for r in rows if r[1] == 0]
    assert len(poly) == 36 and all(key == (minimizers.hash64(0, k) | 1 << 2 * k) for key, *_ in poly)


def test_a_repetitive_kmer_at_k16_carries_bit_32():
    """The widest key: at k = 16 the repetitive bit is bit 32 and the bitmap has 4^16 bits (512 MiB)."""
    data, k, w, listed = SC.k16_weights_case()
    plain, want = SC.restate(data, k, w)[2], SC.restate(data, k, w, listed)[2]
    assert want != plain and not any(key >> 32 for key, *_ in plain)
    SC.assert_bit_32_marks_the_listed(data, want, listed)            # the windows inside the AC tandem: all repetitive, their minimum is chosen
    assert _lib.lib().coral_sketch_bitmap_bytes(16) == 512 << 20
    rc, stats, rows, _names, _lengths = SC.feed_in_pieces(data, k, w, 0, 1 << 13, bitmap=SC.bitmap_of(listed, k))
    assert rc == 0 and rows == want
    SC.assert_bit_32_marks_the_listed(data, rows, listed)


def test_the_bitmap_is_built_from_a_kmers_file(tmp_path):
    from coral_amd import kmers
    k = 8
    data = kmer_cases.cases()["tandem_acg"][:4000] + b"\n>r\n" + kmer_cases.random_bases(np.random.RandomState(2), 3000) + b"\n"
    for both in (False, True):
        path = str(tmp_path / ("rep_%d.txt" % both))
        kc = kmers.count_kmers(io.BytesIO(data), k, device="cpu")
        assert kc.write(path, greater_than=5, both_strands=both) > 0
        listed, _counts = kc.select(5)
        kc.close()
        assert np.array_equal(minimizers.weights_bitmap(path, k), SC.bitmap_of(listed.tolist(), k))
        want = SC.restate(data, k, 5, frozenset(listed.tolist()))[2]
        assert SC.index_rows(host_index(data, k, 5, path)) == SC.sorted_rows(want)
    assert want != SC.restate(data, k, 5)[2]


def test_weights_of_another_length_are_refused():
    with pytest.raises(ValueError):
        host_index(b">a\nACGTACGTAC\n", 5, 4, ["ACGTAC"])
    with pytest.raises(ValueError):
        minimizers.weights_bitmap([4 ** 5], 5)


# ---- capacity -----------------------------------------------------------------------------------------------------------------------
def test_capacity_overflow_reports_the_needed_size_and_the_retry_succeeds():
    data = SC.cases()["poly_a"]
    want = SC.restate(data, 5, 4)[2]
    rc, stats, rows, _names, _lengths = SC.feed_in_pieces(data, 5, 4, 0, 100)
    assert rc == -3 and stats[2] == len(want) and stats[3] == 100 and rows == want[:100]      # CORAL_ERR_CAPACITY; nothing behind the capacity
    idx = host_index(data, 5, 4, _capacity=100)
    assert minimizers.LAST_SKETCH["attempts"] == 2 and SC.index_rows(idx) == SC.sorted_rows(want)


@pytest.mark.parametrize("piece", (0, 1031))
def test_capacities_around_the_number_of_minimizers(piece):
    """CORAL_ERR_CAPACITY below n and success from n on, stats[2] = n, stats[3] = the written ones, and they are the first ones."""
    data = SC.poly_a_6200()
    want = SC.restate(data, 5, 4)[2]
    n = len(want)
    assert n == 6196 and [r[2] for r in want] == list(range(n))
    for cap in (0, 1, 64, n - 1, n, n + 1):
        rc, stats, rows, _names, _lengths = SC.feed_in_pieces(data, 5, 4, piece, cap)
        assert rc == (-3 if cap < n else 0), cap
        assert (stats[2], stats[3]) == (n, min(cap, n)), cap
        assert rows == want[:cap], cap


def test_a_stream_that_cannot_be_started_over_raises():
    class OneWay(io.RawIOBase):
        def __init__(self, data):
            self._fp = io.BytesIO(data)

        def readable(self):
            return True

        def readinto(self, b):
            return self._fp.readinto(b)

    with pytest.raises(_lib.CoralHipError):
        minimizers.sketch_reference(OneWay(SC.cases()["poly_a"]), 5, 4, device="cpu", _capacity=100)


# ---- the index ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mega_index():
    data = b">t\n" + b"ACGGTCA" * 60 + b"\n" + SC.six_records()
    return data, host_index(data, 8, 5)


def test_index_is_sorted_with_ties_in_contig_position_order(mega_index):
    data, idx = mega_index
    rows = SC.index_rows(idx)
    assert rows == SC.sorted_rows(SC.restate(data, 8, 5)[2])
    keys = [r[0] for r in rows]
    assert keys == sorted(keys) and len(set(keys)) < len(keys)
    assert idx.n == len(rows) and idx.k == 8 and idx.w == 5 and len(idx.contig_names) == 7


def test_lookup(mega_index):
    _data, idx = mega_index
    keys = idx.arrays()[0]
    uniq, first_of, counts = np.unique(keys, return_index=True, return_counts=True)
    assert counts.max() > 1                                          # the tandem: a key with several entries
    absent = np.setdiff1d(np.arange(int(uniq[0]), int(uniq[0]) + 4000, dtype=np.uint64), uniq)[:50]
    query = np.concatenate([uniq, absent, [uniq[0], uniq[-1], 0, (1 << 17) - 1]]).astype(np.uint64)
    first, count = idx.lookup(query)
    want_first = np.searchsorted(keys, query, side="left")
    want_count = np.searchsorted(keys, query, side="right") - want_first
    assert np.array_equal(first, want_first) and np.array_equal(count, want_count)
    assert np.array_equal(count[:len(uniq)], counts) and np.array_equal(first[:len(uniq)], first_of) and not count[len(uniq):len(uniq) + len(absent)].any()
    assert idx.lookup(np.zeros(0, dtype=np.uint64))[0].shape == (0,)


def test_anchors_follow_query_then_index_order_and_max_occ(mega_index):
    _data, idx = mega_index
    keys, contigs, positions, strands = idx.arrays()
    uniq, counts = np.unique(keys, return_counts=True)
    many, one = uniq[np.argmax(counts)], uniq[np.argmin(counts)]
    queries = (np.array([7, 7, 9], dtype=np.uint32), np.array([5, 11, 0], dtype=np.uint32), np.array([1, 0, 0], dtype=np.uint8), np.array([many, one, many], dtype=np.uint64))

    def expected(max_occ):
        out = []
        for q, p, s, key in zip(*(a.tolist() for a in queries)):
            at = np.flatnonzero(keys == key)
            if len(at) <= max_occ:
                out += [(q, p, int(contigs[i]), int(positions[i]), s ^ int(strands[i])) for i in at]
        return out

    for max_occ in (int(counts.max()), int(counts.max()) - 1, 0):
        got = idx.anchors(queries, max_occ=max_occ)
        assert list(zip(*(a.tolist() for a in got))) == expected(max_occ)
    assert len(idx.anchors(queries, max_occ=int(counts.max()) - 1)[0]) == int(counts.min())
    with pytest.raises(ValueError):
        idx.anchors(queries, max_occ=-1)


def test_anchor_property_on_the_host_backend():
    fasta, reads = SC.anchor_setup()
    k, w = 15, 50
    idx = host_index(fasta, k, w)
    sketch = minimizers.sketch_sequences([r[3] for r in reads], k, w, device="cpu")
    max_occ = int(np.unique(idx.arrays()[0], return_counts=True)[1].max())
    assert SC.check_anchor_property(idx, reads, k, sketch, max_occ) > 50 * 40


def test_sketch_sequences_equals_the_restatement_per_sequence():
    seqs = [b"ACGTTGCAGGATCCAAGTCTAGGCATTACAGATTACA", b"", b"ACG", b"acgtnnACGTTGCAGGATCCAAGtctagg", b"ACGTTGCAGGATCCAAGTCTAGGCATTACAGATTACA"[::-1]]
    q, pos, strand, key = minimizers.sketch_sequences(seqs, 5, 4, device="cpu")
    want = [(i, p, s, v) for i, seq in enumerate(seqs) for p, s, v in SC.minimizers_of(seq, 5, 4)]
    assert list(zip(q.tolist(), pos.tolist(), strand.tolist(), key.tolist())) == want
    assert minimizers.sketch_sequences([], 5, 4, device="cpu")[0].shape == (0,)
    with pytest.raises(ValueError):
        minimizers.sketch_sequences([b"ACGT\nACGT"], 5, 4, device="cpu")


def test_save_load_round_trip(tmp_path, mega_index):
    _data, idx = mega_index
    path = idx.save(str(tmp_path / "ref.cmi.npz"))
    with np.load(path) as z:
        assert sorted(z.files) == ["keys", "lengths", "meta", "name_off", "names", "values"] and z["meta"].tolist() == [1, 8, 5, 0]
    back = minimizers.MinimizerIndex.load(path)
    assert (back.k, back.w, back.weighted, back.n, back.contig_names, back.contig_lengths) == (idx.k, idx.w, idx.weighted, idx.n, idx.contig_names, idx.contig_lengths)
    assert all(np.array_equal(a, b) for a, b in zip(back.arrays(), idx.arrays()))
    q = idx.arrays()[0][:20]
    assert all(np.array_equal(a, b) for a, b in zip(back.lookup(q), idx.lookup(q)))
    back.close()
    with pytest.raises(ValueError):
        back.arrays()


# ---- arguments ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(k=0), dict(k=17), dict(k=True), dict(k=15.0), dict(w=0), dict(w=257), dict(w="50"), dict(chunk_bytes=15), dict(chunk_bytes=None)])
def test_argument_errors_come_before_any_work(kw):
    args = dict(k=15, w=50, chunk_bytes=1 << 20)
    args.update(kw)
    with pytest.raises(ValueError):
        minimizers.sketch_reference("/nonexistent/ref.fa", device="cpu", **args)
    if "chunk_bytes" not in kw:
        with pytest.raises(ValueError):
            minimizers.sketch_sequences([b"ACGT"], args["k"], args["w"], device="cpu")


def test_native_argument_errors():
    import ctypes as C
    L = _lib.lib()
    h = C.c_void_p()
    out = np.zeros(4, dtype=np.uint64)
    for k, w in ((0, 5), (17, 5), (5, 0), (5, 257)):
        assert L.coral_sketch_open(k, w, -1, None, out.ctypes.data, out.ctypes.data, 4, 0, None, 0, None, C.byref(h)) == -1
    assert L.coral_sketch_open(5, 4, -1, None, None, None, 4, 0, None, 0, None, C.byref(h)) == -1
    assert L.coral_sketch_bitmap_bytes(15) == 128 << 20 and L.coral_sketch_bitmap_bytes(1) == 4 and L.coral_sketch_bitmap_bytes(17) == -1
    assert L.coral_sketch_workspace_bytes(15) == -1
