"""The GC correction and the called-base mask of the copy-number segmenter on the GPU (coral_cn_segment_gc_gpu: k_cn_gc_* of
coral_amd/csrc/coral_cngpu.hip) against the host backend (coral_cn_segment_gc_host), exactly - rows, counts, bias and the bins per
stratum - on the cases of tests/comp_cases.py, which tests/test_cnv_gc_core.py holds against the plain-Python restatement, and on
a table large enough for strata, scans and sorts to cross workgroups; without a composition the new entry point against the old;
one run of `cnv --lr_bam --ref` on both devices."""
import numpy as np
import pytest

from coral_amd import CoRAL, bam, cnv, composition, synth
from tests import cnv_cases as cn
from tests import comp_cases as cc
from tests.bamfile import M

pytestmark = pytest.mark.gpu
GPU = "cuda:0"


def test_device_equals_host_on_the_cases():
    for name, t in cc.gc_cases().items():
        assert cc.segment_gc(*t, gpu=GPU) == cc.segment_gc(*t), name


def test_device_equals_host_on_the_biased_table():
    from tests.test_cnv_gc_core import biased_table
    plain, biased, gc, at, strata, step = biased_table(lambda g: g % 3)
    got = cc.segment_gc(biased, gc, at, strata, 1, 500, gpu=GPU)
    assert got == cc.segment_gc(biased, gc, at, strata, 1, 500) and got[1]["breakpoints"] == 1


def test_seventy_thousand_bins_across_24_contigs():
    rng = np.random.RandomState(31)
    chroms = ["chr%d" % k for k in range(1, 23)] + ["chrX", "chrY"]
    n_of = [int(n) for n in rng.randint(1500, 4400, 24)]
    n_of[3], n_of[23] = 1, 700
    lengths = [n * 1000 - (0 if k % 3 else 417) for k, n in enumerate(n_of)]          # every third contig ends in a short bin
    n = sum(n_of)
    assert 65_000 < n < 80_000
    frac = np.clip(0.42 + 0.08 * np.sin(np.arange(n) / 37.0) + rng.normal(0, 0.03, n), 0.05, 0.95)
    called = np.full(n, 1000, dtype=np.int64)
    called[rng.randint(0, n, 900)] = rng.randint(0, 1000, 900)                           # gaps: some below the mask, some empty
    gc = (called * frac).astype(np.uint32)
    at = (called - gc).astype(np.uint32)
    steps = [(a, a + int(w), f) for a, w, f in zip(rng.randint(0, n - 400, 40), rng.randint(3, 400, 40), rng.choice([0.5, 1.5, 2.0, 4.0], 40))]
    bases = (cn.noisy(rng, n, 6000, steps) * (1.0 + 0.5 * np.sin(9.0 * frac))).astype(np.int64)
    bases[rng.randint(0, n, 300)] = 0
    off = np.concatenate([[0], np.cumsum(n_of)])
    bases[off[22]:off[23]] //= 2                                                        # chrX at half the depth: no centring contig
    case = cn.Case(chroms, lengths, 1000, bases)
    for strata, min_bins, permille in ((100, 256, 500), (1000, 64, 900), (7, 1, 0)):
        host = cc.segment_gc(case, gc, at, strata, min_bins, permille)
        assert cc.segment_gc(case, gc, at, strata, min_bins, permille, gpu=GPU) == host, (strata, min_bins, permille)
        assert host[1]["breakpoints"] > 20 and host[1]["kept"] > 60_000 and (host[1]["uncalled"] > 300) == (permille > 0)
    ref = cn.noisy(rng, n, 5000, [(1000, 1300, 0.5)])
    with_ref = cn.Case(chroms, lengths, 1000, bases, ref=ref)
    assert cc.segment_gc(with_ref, gc, at, 100, 256, 500, gpu=GPU) == cc.segment_gc(with_ref, gc, at, 100, 256, 500)


def test_without_a_composition_the_new_entry_point_is_the_old():
    for name, case in cn.cases().items():
        old = cc.segment_gc(case, None, None, 100, 256, 500, gpu=GPU, entry="old")
        new = cc.segment_gc(case, None, None, 100, 256, 500, gpu=GPU)
        assert old == new == cc.segment_gc(case, None, None, 100, 256, 500), name


def test_cnv_mode_with_the_reference_fasta_on_both_devices(tmp_path, capsys):
    """chr1 of 300 kb at 2x in reads of 2 000 bases, 8x over 60 kb; its FASTA has a gap of 20 kb of N."""
    alns = [dict(tid=0, pos=p, cigar=[(M, 2000)], has_seq=0, name="base%d_%d" % (p, k)) for p in range(0, 300_000, 2000) for k in range(2)]
    alns += [dict(tid=0, pos=p, cigar=[(M, 2000)], has_seq=0, name="amp%d_%d" % (p, k)) for p in range(100_000, 160_000, 2000) for k in range(6)]
    alns.sort(key=lambda a: a["pos"])
    rec = synth.records_from_alignments(alns)
    rec.header_chroms, rec.header_lens = ["chr1", "chrM"], [300_000, 16_569]
    path, fasta = str(tmp_path / "tiny.bam"), str(tmp_path / "tiny.fa")
    bam.write_bam(rec, path, seed=3, fast_seq=True)
    rng = np.random.RandomState(8)
    seq = bytearray(cc.random_sequence(rng, 300_000, b"ACGTacgt"))
    seq[200_000:220_000] = b"N" * 20_000
    with open(fasta, "wb") as fp:
        fp.write(b">chrM mito\n" + cc.wrap(cc.random_sequence(rng, 16_569, b"ACGT"), 70) + b">chr1\n" + cc.wrap(bytes(seq), 70))
    out = {}
    for pipe, device in (("gpu", GPU), ("cpu", "cpu")):
        cns = str(tmp_path / (pipe + ".cns"))
        assert CoRAL.main(["cnv", "--lr_bam", path, "--ref", fasta, "--gc_min_bins", "32", "--output", cns, "--device", device]) == cns
        out[pipe] = (open(cns).read(), capsys.readouterr().out.replace(pipe + ".", "x."))
    assert out["gpu"] == out["cpu"] and "20 bins masked as uncalled" in out["gpu"][1]
    rows = [ln.split("\t") for ln in out["gpu"][0].split("\n")[1:-1]]
    assert [(r[0], int(r[1]), int(r[2]), int(r[6])) for r in rows] == [("chr1", 0, 100000, 100), ("chr1", 100000, 160000, 60), ("chr1", 160000, 300000, 120)]
    seg = cnv.call_copy_number(path, device=GPU, composition=composition.reference_composition(fasta, 1000, device=GPU), gc_min_bins=32)
    assert seg.write(str(tmp_path / "api.cns")) and open(str(tmp_path / "api.cns")).read() == out["gpu"][0]
