"""Native BAM decoder (host entry points of the C ABI) round trip against the pure-Python writer, plus an independent
pure-Python read of the same file through the gzip module (BGZF is multi-member gzip)."""
import gzip

import numpy as np
import pytest
import torch

from coral_amd import bam, synth
from tests.bamfile import pairs, read_bam
from tests.decode_support import assert_same_records as assert_same, concat_records as _concat, odd_io_records as _odd


def test_roundtrip_synthetic_tiny(tmp_path):
    rec = synth.generate(synth.scaled_config("tiny", 600), "cpu")
    p = str(tmp_path / "t.bam")
    bam.write_bam(rec, p, seed=11)
    back = bam.decode_bam(p, n_threads=3)
    assert_same(rec, back)
    assert int((rec.sa_off[1:] - rec.sa_off[:-1] > 0).sum()) > 0 and rec.nonacgt_pos.numel() > 0


def test_roundtrip_odd_records_and_long_cigar(tmp_path):
    rec = _odd()
    p = str(tmp_path / "odd.bam")
    bam.write_bam(rec, p)
    back = bam.decode_bam(p, n_threads=2)
    assert_same(rec, back)
    assert int(back.n_cigar.max()) == 66001


def test_file_is_standard_bam(tmp_path):
    """Independent check of the writer: gzip module + struct parsing of header and first record."""
    rec = _odd()
    p = str(tmp_path / "odd.bam")
    bam.write_bam(rec, p)
    parsed = read_bam(p)
    n_ref, r = len(parsed.refs), parsed.recs[0]
    assert n_ref == 25
    tid, pos, mapq, n_cig, flag, l_seq = (r[k] for k in ("tid", "pos", "mapq", "n_cig", "flag", "l_seq"))
    assert (tid, pos, mapq, n_cig, flag, l_seq) == (0, 100, 60, 6, 0, 88)
    assert r["name"] == "a"
    assert pairs(r["ops"]) == [(4, 5), (0, 50), (2, 700), (0, 20), (1, 3), (0, 10)]
    flat = r["codes"].tolist()
    assert flat[5 + 1] == 15 and all(c in (1, 2, 4, 8, 15) for c in flat)      # the N planted at ref 101 = query offset 6
    assert ("SA", "Z", "chr8,1000,-,10S2000M30D55S,60,12;chr12,5,+,300M4I9000S,3,0;") in r["tags"]


def test_decoder_rejects_garbage(tmp_path):
    from coral_amd import _lib
    p = tmp_path / "bad.bam"
    p.write_bytes(b"this is not a bam file at all, not even gzip")
    with pytest.raises(_lib.CoralHipError):
        bam.decode_bam(str(p))
    with pytest.raises(_lib.CoralHipError):
        bam.decode_bam(str(tmp_path / "missing.bam"))


def test_sa_shapes_tokenised(tmp_path):
    """SA CIGARs outside [S]M[I|D][S]: no S / no M -> zero clips or zero M (the read fails as a whole later,
    cigar_parsing.py:248-253); containing S and M but another shape -> leading clip = -2 (KeyError in the reference,
    cigar_parsing.py:255)."""
    M, S = 0, 4
    rec = synth.records_from_alignments([dict(tid=0, pos=10, cigar=[(S, 5), (M, 50)], name="x")])
    rec.sa_text = {0: "chr1,500,+,7S40M,60,1;chr2,9,-,47M,3,2;chr3,8,+,7H40M,1,0;chr4,7,-,1S2M3S4M,0,5;chrZ,6,+,3S4M2I1S,9,9;"}
    p = str(tmp_path / "s.bam")
    bam.write_bam(rec, p)
    back = bam.decode_bam(p)
    assert back.sa.tolist() == [[0, 500, 0, 7, 40, 0, 0, 60], [1, 9, 1, 0, 0, 0, 0, 3], [2, 8, 0, 0, 0, 0, 0, 1],
                                [3, 7, 1, -2, 2, 0, 3, 0], [-1, 6, 0, 3, 4, 2, 1, 9]]
    assert back.sa_nm.tolist() == [1, 2, 0, 5, 9]


def test_native_writer_roundtrip_and_is_standard_bam(tmp_path):
    """coral_bam_write -> coral_bam_decode gives the records back; the file is multi-member gzip that the gzip module reads,
    with the BAM magic, and the odd records (CG-tag CIGAR, unmapped, no SEQ, non-ACGT bases) survive."""
    for name, rec in (("synthetic", synth.generate(synth.scaled_config("tiny", 1500), "cpu")), ("odd", _odd())):
        p = str(tmp_path / (name + ".bam"))
        bam.write_bam_native(rec, p, seed=5, n_threads=3)
        assert_same(rec, bam.decode_bam(p, n_threads=3))
        raw = gzip.open(p, "rb").read()
        assert raw[:4] == b"BAM\x01"
    assert raw.count(b"SAZ") >= 1


@pytest.mark.parametrize("config,n_reads", [("tiny", 3000), ("ultra", 400)])
def test_byte_ranges_partition_the_file(config, n_reads, tmp_path):
    """Decoding the file as `world` byte ranges (one per GPU process) gives exactly the records of the whole-file decode, in
    order, none dropped, none repeated — for short reads (many records per BGZF block) and for ultra-long ones (records of
    several blocks straddling range boundaries), for any number of ranges and threads."""
    cfg = synth.scaled_config(config, n_reads)
    rec = synth.generate(cfg, "cpu")
    p = str(tmp_path / "x.bam")
    bam.write_bam_native(rec, p, seed=3, n_threads=4)
    whole = _concat([bam.decode_bam(p, n_threads=2)])
    assert len(whole["tid"]) == rec.n
    for world in (2, 3, 5, 8, 13):
        parts = [bam.decode_bam(p, n_threads=1 + (r % 3), rank=r, world=world) for r in range(world)]
        got = _concat(parts)
        assert sum(q.n for q in parts) == rec.n, world
        for k, v in whole.items():
            assert (list(v) == list(got[k])) if k == "names" else np.array_equal(v, got[k]), (world, k)
        assert all(q.header_chroms == rec.header_chroms for q in parts)


def test_decoder_rejects_garbage(tmp_path):
    from coral_amd._lib import CoralHipError
    p = tmp_path / "junk.bam"
    p.write_bytes(b"this is not a BGZF file" * 10)
    with pytest.raises(CoralHipError):
        bam.decode_bam(str(p))
    rec = synth.generate(synth.scaled_config("tiny", 300), "cpu")
    good = tmp_path / "good.bam"
    bam.write_bam_native(rec, str(good))
    data = bytearray(good.read_bytes())
    data[len(data) // 2: len(data) // 2 + 64] = b"\x00" * 64            # corrupt a block in the middle
    bad = tmp_path / "bad.bam"
    bad.write_bytes(bytes(data))
    with pytest.raises(CoralHipError):
        bam.decode_bam(str(bad))
    trunc = tmp_path / "trunc.bam"
    trunc.write_bytes(bytes(good.read_bytes()[:-5000]))
    with pytest.raises(CoralHipError):
        bam.decode_bam(str(trunc))
    # a byte flipped inside a STORED block: the block still inflates, only the trailer's CRC-32 tells
    stored = tmp_path / "stored.bam"
    bam.write_bam_native(rec, str(stored), level=0)
    data = bytearray(stored.read_bytes())
    data[len(data) // 2] ^= 0x40
    flipped = tmp_path / "flipped.bam"
    flipped.write_bytes(bytes(data))
    with pytest.raises(CoralHipError):
        bam.decode_bam(str(flipped))
    assert bam.decode_bam(str(stored)).n == rec.n
