"""The inflate kernel (k_bgzf_inflate, coral_amd/csrc/coral_bamgpu.hip: Inflater on the device backend, with the hand-written
DevWaveT::fast in front of the general loop) on the hand-built streams of tests/deflate_streams.py — dynamic headers no compressor
writes, chosen symbols on codes longer than the look-up tables, far distances out of global memory, stored blocks at every bit
phase — and the same blocks through the whole decode (CRC kernel, record parser) as members of a BAM file.  The host build of the
core runs the very same lists in tests/test_inflate_core.py.

Single-line mutants of coral_inflate_core.h that every stream of streams() passes (host build, temporary copies of the header)
and that these lists catch in tests/test_inflate_core.py:
  1. read_dynamic_header, repeat branch: `prev = val;` -> `prev = prev;`
       test_core_decodes_hand_built_streams (cl_16_after_zero_runs)
  2. read_dynamic_header: `i + rep > total` -> also refuses a repeat that crosses hlit
       test_core_decodes_hand_built_streams (cl_16_across_boundary, cl_17_across_boundary, cl_18_across_boundary)
  3. codes_vector, long-code branch: `bits((x >> 5) & 7u)` -> `& 3u`
       test_core_decodes_hand_built_streams (lengths_behind_table, lengths_and_distances_behind_table)

Two refusals the lists brought in: a stored block cut inside the bytes that the bit buffer had read ahead (Inflater::run now
checks the end of the input to the bit, input_overrun), and, on the device only, a last match one byte longer than the block's
declared size (DevWaveT::match cut it to what fits, and the block ended at exactly its size).
"""
import struct
import zlib

import pytest

from coral_amd import bam, synth
from tests import deflate_streams as ds
from tests.bamfile import bgzf_blocks
from tests.decode_support import DEVICE, PIPELINES, assert_same_records, inflate_on_gpu


@pytest.fixture(scope="module")
def valid():
    return [(c["name"], c["comp"], c["text"]) for c in ds.dynamic_streams()] + [r for r in ds.incomplete_streams() if r[0].endswith("accepted")]


def _exact(pairs, out, status, desc, names):
    """Every status 0, every output its text, every byte between the outputs as it was."""
    assert [n for n, st in zip(names, status) if st != 0] == []
    prev_end = 0
    for name, (_, d), (_, _, o, n) in zip(names, pairs, desc):
        assert out[o:o + n] == d, name
        assert out[prev_end:o] == b"\x55" * (o - prev_end), name
        prev_end = o + n
    assert out[prev_end:] == b"\x55" * (len(out) - prev_end)


@pytest.mark.gpu
def test_kernel_decodes_hand_built_streams(valid):
    """Two launches; a 3-byte stream of one byte in front of the second one and a gap of 3 + k % 4 move every stream to another
    byte phase of the input window (stream_off) and every output to another place in its first 256-byte line (a0)."""
    names = [n for n, _, _ in valid]
    pairs = [(c, t) for _, c, t in valid]
    w = ds.Deflate()
    w.fixed([("L", 0x33)], True)
    first = w.done()
    assert (len(first[0]), len(first[1])) == (3, 1)
    out, status, desc0 = inflate_on_gpu(pairs)
    _exact(pairs, out, status, desc0, names)
    out, status, desc1 = inflate_on_gpu([first] + pairs, pad=3)
    _exact([first] + pairs, out, status, desc1, ["first"] + names)
    for (i0, _, o0, _), (i1, _, o1, _) in zip(desc0, desc1[1:]):
        assert i0 & 3 != i1 & 3 and o0 & 255 != o1 & 255


@pytest.mark.gpu
def test_kernel_rejects_hand_built_streams(valid):
    """Every refused stream between two valid ones: its status is not 0, its neighbours are exact, and nothing outside its own
    output range was written."""
    rejected = ds.rejected_streams()
    pairs, kinds = [], []
    for k, (name, comp, size) in enumerate(rejected):
        pairs += [(valid[k % len(valid)][1], valid[k % len(valid)][2]), (comp, bytes(size))]
        kinds += [None, name]
    pairs.append((valid[-1][1], valid[-1][2]))
    kinds.append(None)
    out, status, desc = inflate_on_gpu(pairs, pad=1)
    want = bytearray(b"\x55" * len(out))
    for kind, (_, d), (_, _, o, n) in zip(kinds, pairs, desc):
        want[o:o + n] = d if kind is None else out[o:o + n]
    assert [k for k, st in zip(kinds, status) if k is not None and st == 0] == []
    assert [i for i, (k, st) in enumerate(zip(kinds, status)) if k is None and st != 0] == []
    assert out == bytes(want)


# ---- the crafted blocks as members of a BAM file -------------------------------------------------------------------------------
def _greedy(data, at=0, end=None):
    """Tokens of data[at:end] from a plain greedy matcher: the latest earlier place with the same three bytes, extended."""
    end = len(data) if end is None else end
    last, toks, i = {}, [], at
    for j in range(max(0, at - 32768), at):
        last[data[j:j + 3]] = j
    while i < end:
        key = data[i:i + 3]
        j = last.get(key, -1)
        n = 0
        if j >= 0 and i - j <= 32768 and i + 3 <= end:
            while n < 258 and i + n < end and data[j + n] == data[i + n]: n += 1
        if n >= 3:
            toks.append(("M", n, i - j))
        else:
            toks.append(("L", data[i]))
            n = 1
        for k in range(i, i + n):
            last[data[k:k + 3]] = k
        i += n
    return toks


def _all_codes_of_15_bits(data):
    """The seven most frequent bytes at 1..7 bits; 250 other symbols and six length symbols (a complete code) at 15."""
    order = sorted(range(256), key=lambda s: (-data.count(s), s))
    lens = [15] * 263
    for k, s in enumerate(order[:7]): lens[s] = k + 1
    assert ds.kraft(lens) == 32768
    return lens


def _recode(data, style):
    w, lits = ds.Deflate(), [("L", b) for b in data]
    if style == 0:
        w.stored(data, True)
    elif style == 1:
        w.dynamic(lits, True)
    elif style == 2:
        w.dynamic(lits, True, ll_lens=_all_codes_of_15_bits(data), d_lens=[0])
        assert max(w.blocks[0]["ll_lens"]) == 15
    elif style == 3:
        w.fixed(_greedy(data, 0, len(data) // 2), False)
        w.dynamic(_greedy(data, len(data) // 2), True)
    else:
        w.dynamic(_greedy(data), True)
    comp, text = w.done()
    assert text == data
    return comp


def _member(comp, data):
    total = 18 + len(comp) + 8
    assert total <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", total - 1) + comp + struct.pack("<II", zlib.crc32(data), len(data)))


@pytest.fixture(scope="module")
def recoded_bam(tmp_path_factory):
    d = tmp_path_factory.mktemp("recoded")
    rec = synth.generate(synth.scaled_config("tiny", 200), "cpu")
    plain, crafted = str(d / "plain.bam"), str(d / "crafted.bam")
    bam.write_bam(rec, plain, seed=3, block_size=12000)
    with open(plain, "rb") as fp:
        raw = fp.read()
    blocks = list(bgzf_blocks(raw))
    ends = [b[0] for b in blocks[1:]] + [len(raw)]
    out, styles = bytearray(), 0
    for (at, _, isize), end in zip(blocks, ends):
        data = zlib.decompress(raw[at:end], 31)
        if isize:
            out += _member(_recode(data, styles % 5), data)
            styles += 1
        else:
            out += raw[at:end]
    assert styles >= 10                                   # every style at least twice
    with open(crafted, "wb") as fp:
        fp.write(out)
    return plain, crafted


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_decode_of_recoded_blocks(pipeline, recoded_bam):
    """Stored, literal-only, 15-bit-code, mixed fixed / dynamic and greedy-match members with their own CRC-32: the same records
    as the file they were taken from."""
    plain, crafted = recoded_bam
    decode = bam.decode_bam if pipeline == "host" else lambda p: bam.decode_bam_gpu(p, DEVICE[pipeline])
    assert_same_records(decode(crafted), decode(plain))
