"""The DEFLATE compressor core of the GPU BGZF writer (coral_amd/csrc/coral_deflate_core.h) compiled for the HOST
(tests/native/deflate_host.cpp: the same logic, lanes as loops) against Python's zlib and gzip: every member's fields, its stream
inflated, the block type chosen, the distance limit, the RFC 1951 corner cases of the code construction, and the compressed size
against zlib level 1.  The device build of the same code is compared byte for byte with this one in
tests/test_bgzf_deflate_gpu.py."""
import ctypes as C
import gzip
import heapq
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import deflate_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "deflate_host.cpp")
TOK_MATCH = 1 << 31
# compressed size against zlib level 1 on the same bytes (profiles/bgzf_deflate.md: the measured ratios, rounded up to 0.05)
RATIO_BAM, RATIO_ACGT = 1.00, 1.00              # measured 0.9883 and 0.9665


def host_deflate_library(directory):
    so = os.path.join(str(directory), "libdeflate_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC], check=True)
    L = C.CDLL(so)
    L.coral_test_deflate.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]

    def run(data):
        """(member, tokens uint32) of one block"""
        slot = np.zeros(65536, dtype=np.uint8)
        tok, n_tok = np.zeros(max(len(data), 1), dtype=np.uint32), C.c_uint32(0)
        n = L.coral_test_deflate(bytes(data), len(data), slot.ctypes.data, tok.ctypes.data, C.byref(n_tok))
        assert 26 <= n <= len(data) + 31 and not slot[n:].any(), "a member has its length, the rest of the slot stays zero"
        return slot[:n].tobytes(), tok[:n_tok.value].copy()
    run.library = L
    return run


@pytest.fixture(scope="module")
def deflate(tmp_path_factory):
    return host_deflate_library(tmp_path_factory.mktemp("deflate"))


@pytest.fixture(scope="module")
def done(deflate):
    """name -> (data, member, tokens, BTYPE) of every case, each member checked on the way."""
    res = {}
    for name, data in dc.cases():
        member, tok = deflate(data)
        res[name] = (data, member, tok, dc.check_member(member, data))
    return res


def matches(tok):
    """(lengths, distances) of the match tokens"""
    m = tok[(tok & TOK_MATCH) != 0]
    return ((m >> 16) & 0xff).astype(np.int64) + 3, (m & 0x7fff).astype(np.int64) + 1


def replay(tok):
    out = bytearray()
    for t in tok.tolist():
        if t & TOK_MATCH:
            length, dist = ((t >> 16) & 0xff) + 3, (t & 0x7fff) + 1
            assert dist <= len(out)
            for _ in range(length):
                out.append(out[-dist])
        else:
            out.append(t)
    return bytes(out)


def test_every_case_is_a_valid_member(done):
    """(the fixture checked CRC, ISIZE, BSIZE, zlib and gzip on every member)  The tokens of pass 1 restate the block, with lengths
    3..258 and distances 1..32768; a member is deterministic."""
    for name, (data, member, tok, btype) in done.items():
        assert btype in (0, 2), name
        lens, dists = matches(tok)
        assert replay(tok) == data, name
        if len(lens):
            assert 3 <= lens.min() and lens.max() <= 258 and 1 <= dists.min() and dists.max() <= 32768, name
    assert done["len_0"][1][18:-8] == b"\x01\x00\x00\xff\xff" and len(done["len_0"][1]) == 31


def test_members_in_a_row_are_a_gzip_file(done):
    names = ["len_0", "len_1", "len_65", "urandom", "one_byte", "acgt", "len_0", "fibonacci"]
    assert gzip.decompress(b"".join(done[n][1] for n in names) + dc.EOF_BLOCK) == b"".join(done[n][0] for n in names)


def test_block_type_is_chosen_per_block(done):
    data, member, tok, btype = done["urandom"]
    assert btype == 0 and len(member) == len(data) + 31 and member[18:23] == b"\x01\x00\xff\xff\x00" and member[23:-8] == data
    for name in ("len_1", "len_2", "len_3", "len_4", "len_63"):          # the dynamic header alone is longer than these
        assert done[name][3] == 0, name
    for name in ("largest_text", "one_byte", "acgt", "period_2", "period_65", "fibonacci", "no_distance_code", "one_distance_code"):
        assert done[name][3] == 2 and len(done[name][1]) < len(done[name][0]) + 31, name


def test_runs_and_short_periods_compress(done):
    data, member, tok, _ = done["one_byte"]
    lens, dists = matches(tok)
    assert (dists == 1).all() and lens.max() == 258 and len(tok) <= 2 + len(data) // 258 + 1 and len(member) < 400
    for p in (2, 3, 64, 65):
        data, member, tok, _ = done["period_%d" % p]
        lens, dists = matches(tok)
        assert len(member) < 600 and set(dists.tolist()) <= {1, p, 2 * p, 3 * p, 4 * p} | set(range(p, 5000, p)), p
        assert lens.sum() > 4500, p


def test_the_window_ends_at_32768(done):
    data, member, tok, _ = done["motif_at_32768"]
    lens, dists = matches(tok)
    assert dists.max() == 32768 and lens[dists == 32768].sum() >= 290
    for d in (32769, 40000):
        data, member, tok, _ = done["motif_at_%d" % d]
        lens, dists = matches(tok)
        assert dists.max() <= 32768 and not ((dists > 1) & (lens > 16)).any()      # the second motif is written as literals


def test_no_distance_code_and_one_distance_code(done):
    data, member, tok, btype = done["no_distance_code"]
    assert btype == 2 and len(matches(tok)[0]) == 0
    hlit, hdist, ll, d = dc.dynamic_header(member[18:-8])
    assert hdist == 1 and d == [0] and dc.kraft(ll) == 1.0
    data, member, tok, btype = done["one_distance_code"]
    lens, dists = matches(tok)
    assert btype == 2 and len(lens) == 199 and set(dists.tolist()) == {1}
    hlit, hdist, ll, d = dc.dynamic_header(member[18:-8])
    assert hdist == 1 and d == [1] and dc.kraft(ll) == 1.0                # one bit, not zero


def huffman(freq):
    """(depth, cost in bits) of the unlimited Huffman code of the non-zero frequencies"""
    heap = [(f, 0, 0) for f in freq if f]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1, a[2] + b[2] + a[0] + b[0]))
    return heap[0][1], heap[0][2]


def test_code_lengths_are_limited_to_15_bits(deflate, done):
    """The block of 46 367 bytes with Fibonacci frequencies inflates (the fixture), and its header is trimmed and complete.  Its
    matches take most of the frequent bytes out of the literal histogram, so the limit itself is pinned on the code construction
    alone, given the Fibonacci histogram as it stands: the unlimited tree is 21 deep."""
    data, member, tok, btype = done["fibonacci"]
    hlit, hdist, ll, d = dc.dynamic_header(member[18:-8])
    assert btype == 2 and dc.kraft(ll) == 1.0 and all(ll[s] for s in range(22)) and ll[256] and max(ll) <= 15
    assert hlit == max(s for s, l in enumerate(ll) if l) + 1 and hdist == max(s for s, l in enumerate(d) if l) + 1
    L = deflate.library
    L.coral_test_code_lengths.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]

    def lengths(freq):
        f = np.ascontiguousarray(freq, dtype=np.uint32)
        lens, codes = np.zeros(len(f), dtype=np.uint8), np.zeros(len(f), dtype=np.uint16)
        assert L.coral_test_code_lengths(f.ctypes.data, len(f), lens.ctypes.data, codes.ctypes.data) == 0
        seen = set()
        for s in np.nonzero(lens)[0]:                              # prefix-free: the codes as written, first bit first
            text = "{:016b}".format(int(codes[s]))[::-1][:int(lens[s])]
            seen.add(text)
        assert len(seen) == int((lens != 0).sum()) and not any(a != b and b.startswith(a) for a in seen for b in seen)
        return lens.astype(np.int64)

    lens = lengths(dc.FIB)
    assert huffman(dc.FIB)[0] == 21 and lens.max() == 15 and dc.kraft(lens.tolist()) == 1.0
    assert all(lens[a] >= lens[b] for a in range(22) for b in range(22) if dc.FIB[a] < dc.FIB[b])
    rng = np.random.default_rng(5)
    for n_sym, top in ((286, 4), (286, 60000), (30, 1000), (2, 5), (19, 1 << 20)):
        freq = rng.integers(0, top, n_sym)
        freq[0] = max(freq[0], 1)
        freq[n_sym - 1] = max(freq[n_sym - 1], 1)
        lens = lengths(freq)
        depth, cost = huffman(freq.tolist())
        assert ((lens != 0) == (freq != 0)).all() and lens.max() <= 15 and dc.kraft(lens.tolist()) == 1.0
        assert (lens * freq).sum() >= cost and (depth > 15 or (lens * freq).sum() == cost), (n_sym, top)
    one = np.zeros(30, dtype=np.uint32)
    one[7] = 9
    assert lengths(one).tolist() == [0] * 7 + [1] + [0] * 22 and lengths(np.zeros(30, dtype=np.uint32)).sum() == 0


def test_matches_at_the_end_of_the_block(done):
    data, member, tok, _ = done["match_ends_on_last_byte"]
    lens, dists = matches(tok)
    assert tok[-1] & TOK_MATCH and lens[-1] == 100 and dists[-1] == 400
    data, member, tok, _ = done["candidate_runs_past_end"]
    lens, dists = matches(tok)
    assert tok[-1] & TOK_MATCH and lens[-1] == 50 and dists[-1] == 400


def test_sanitizer_run_of_the_stand_alone_program(tmp_path, done):
    """The same cases through the stand-alone program (its own main) under AddressSanitizer and UBSan, on the CPU: the input and
    the token array are allocations of exactly their size.  Its members are the library's."""
    exe, cases_bin, members_bin = str(tmp_path / "deflate_host"), str(tmp_path / "cases.bin"), str(tmp_path / "members.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DDEFLATE_HOST_MAIN",
                    SRC, "-o", exe], check=True)
    with open(cases_bin, "wb") as fp:
        for data, _m, _t, _b in done.values():
            fp.write(struct.pack("<I", len(data)) + data)
    run = subprocess.run([exe, cases_bin, members_bin], capture_output=True, text=True)
    assert run.returncode == 0 and "deflate_host: %d cases" % len(done) in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    with open(members_bin, "rb") as fp:
        raw = fp.read()
    at = 0
    for name, (_d, member, _t, _b) in done.items():
        n = struct.unpack_from("<I", raw, at)[0]
        assert raw[at + 4:at + 4 + n] == member, name
        at += 4 + n
    assert at == len(raw)


def zlib1(data):
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    return len(co.compress(data) + co.flush())


def sizes(deflate, data):
    """(bytes of our DEFLATE streams, bytes of zlib level 1's) over the 0xff00-byte blocks of data"""
    ours = theirs = 0
    for at in range(0, len(data), dc.BLOCK_MAX):
        block = data[at:at + dc.BLOCK_MAX]
        member, _ = deflate(block)
        assert dc.check_member(member, block) == 2
        ours += len(member) - 26
        theirs += zlib1(block)
    return ours, theirs


def test_size_against_zlib_level_1(deflate, tmp_path):
    """What the host writer uses today.  The bytes are deterministic: the margin above the measured ratio is room for later
    tuning, not for noise."""
    for what, data, bound in (("bam records", dc.bam_payload(tmp_path), RATIO_BAM), ("acgt", dc.acgt_payload(), RATIO_ACGT)):
        ours, theirs = sizes(deflate, data)
        print("%s: %d bytes -> %d, zlib level 1 %d, ratio %.4f" % (what, len(data), ours, theirs, ours / theirs))
        assert ours <= theirs * bound, (what, ours, theirs)
