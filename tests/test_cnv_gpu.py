"""The copy-number segmenter on the GPU (coral_cn_segment_gpu: k_cn_*, k_haar_* of coral_amd/csrc/coral_cngpu.hip) against the host
backend (coral_cn_segment_host), exactly, rows and counts: the shared case table of tests/cnv_cases.py - which
tests/test_cnv_core.py holds against the plain-Python restatement -, the shapes at the launch geometry's edges, and one run of
the `cnv` mode from a BAM file to the .cns and the seed bed."""
import numpy as np
import pytest

from coral_amd import CoRAL, bam, cnv, synth
from tests import cnv_cases as cc
from tests.bamfile import M

pytestmark = pytest.mark.gpu
GPU = "cuda:0"


def table_of(chroms, lengths, bin_size, bases):
    return cc.Case(chroms, lengths, bin_size, bases).depth(bam)


def both(depth, reference=None, **kw):
    host = cnv.segment_depth(depth, reference, device="cpu", **kw)
    dev = cnv.segment_depth(depth, reference, device=GPU, **kw)
    assert dev.counts == host.counts
    assert cc.rows_of(dev) == cc.rows_of(host)
    return host


def jitter(n, level, seed):
    """Poisson depth around ``level``."""
    return np.random.RandomState(seed).poisson(float(level), n).astype(np.int64)


def test_device_equals_host_on_the_case_table():
    for name, case in cc.cases().items():
        ref = None if case.ref is None else case.depth(bam, "ref")
        host = both(case.depth(bam), ref, levels=case.levels, fdr_q=case.q, centre_contigs=case.centre_contigs)
        assert len(host) == host.counts["rows"], name


def test_steps_at_workgroup_and_scan_tile_edges():
    """One contig of 70 001 kept bins; the level changes at k = 255, 256, 257, 1023, 1024 and n - 2."""
    n = 70001
    edges = [0, 255, 256, 257, 1023, 1024, n - 2, n]
    bases = jitter(n, 20000, 11)
    for a, b, times in zip(edges, edges[1:], (1, 2, 3, 1, 4, 2, 3)):
        bases[a:b] *= times
    host = both(table_of(["chr1"], [n * 100], 100, bases))
    starts = set(host.start.tolist())
    assert 1023 * 100 in starts and (n - 2) * 100 in starts and starts & {25500, 25600, 25700} and host.counts["kept"] == n
    assert host.counts["breakpoints"] >= 4


def test_more_contigs_than_a_grid_row_in_front_of_a_large_one():
    """3 000 contigs of 1..5 bins - smaller than every h - and then one of 9 000 bins with two steps."""
    sizes = [1 + (7 * k) % 5 for k in range(3000)]
    big = jitter(9000, 5000, 3)
    big[2000:2600] *= 3
    chroms = ["s%d" % k for k in range(3000)] + ["chr1"]
    bases = np.concatenate([jitter(sum(sizes), 5000 + 2000, 5), big])
    bases[np.arange(0, sum(sizes), 17)] = 0                      # some of the small contigs lose bins, some all of them
    host = both(table_of(chroms, [s * 10 for s in sizes] + [9000 * 10], 10, bases))
    rows = cc.rows_of(host)
    assert [r[1:4] for r in rows if r[0] == 3000] == [(0, 20000, 2000), (20000, 26000, 600), (26000, 90000, 6400)]
    assert len(rows) > 2500 and len({r[0] for r in rows}) > 2500      # (the small contigs that kept a bin)


def test_more_rows_than_the_first_row_capacity():
    """A square wave of 4 bins a level without noise: sigma is 0, every step is a breakpoint - 5 000 rows, more than the 4 096 the
    first call makes room for, so both backends are asked a second time with the capacity the first call named."""
    bases = np.where((np.arange(20000) // 4) % 2 == 0, 1000, 2000).astype(np.int64)
    host = both(table_of(["chr1"], [20000 * 100], 100, bases))
    assert len(host) == 5000 and host.probes.tolist() == [4] * 5000 and host.counts["breakpoints"] == 4999


def test_a_step_at_a_contig_boundary_makes_no_breakpoint():
    bases = np.concatenate([jitter(1500, 1000, 1), jitter(1300, 9000, 2)])
    host = both(table_of(["chr1", "chr2"], [1500 * 50, 1300 * 50], 50, bases))
    assert [r[:4] for r in cc.rows_of(host)] == [(0, 0, 75000, 1500), (1, 0, 65000, 1300)] and host.counts["breakpoints"] == 0
    # and nothing leaks: each contig alone gives the same row, whatever stands beside it
    for c, (a, b) in enumerate(((0, 1500), (1500, 2800))):
        alone = both(table_of(["chr%d" % (c + 1)], [(b - a) * 50], 50, bases[a:b]), centre_contigs=None)
        assert alone.sum_bases.tolist() == [host.sum_bases[c]] and alone.probes.tolist() == [host.probes[c]]


def test_a_reference_table():
    n = 6000
    sample, normal = jitter(n, 8000, 7), jitter(n, 3000, 9)
    sample[1000:1400] *= 2
    sample[3000:3300] = sample[3000:3300] // 2
    normal[3000:3300] = normal[3000:3300] // 2                   # a dip of both: no segment
    normal[[5, 6, 4000]] = [0, 0, 20]
    d, r = table_of(["chr1", "chr2"], [4000 * 100, 2000 * 100], 100, sample), table_of(["chr1", "chr2"], [4000 * 100, 2000 * 100], 100, normal)
    host = both(d, r)
    assert [x[1:4] for x in cc.rows_of(host) if x[0] == 0] == [(0, 100000, 998), (100000, 140000, 400), (140000, 400000, 2600)]
    assert host.counts["ref_centre"] > 0 and host.counts["kept"] == n - 3
    plain = both(d)
    assert plain.counts["breakpoints"] == 4


@pytest.fixture(scope="module")
def amplified(tmp_path_factory):
    """chr1 of 1.2 Mb at 1x in reads of 5 000 bases, 8x over the 300 bins of 1 000 bases from 100 000; the centromere behind it."""
    d = tmp_path_factory.mktemp("cnv_e2e")
    alns = [dict(tid=0, pos=p, cigar=[(M, 5000)], has_seq=0, name="base%d" % p) for p in range(0, 1_200_000, 5000)]
    alns += [dict(tid=0, pos=p, cigar=[(M, 5000)], has_seq=0, name="amp%d_%d" % (p, k)) for p in range(100_000, 400_000, 5000) for k in range(7)]
    alns.sort(key=lambda a: a["pos"])
    rec = synth.records_from_alignments(alns)
    rec.header_chroms, rec.header_lens = ["chr1", "chrM"], [1_200_000, 16_569]
    path = str(d / "amplified.bam")
    bam.write_bam(rec, path, seed=3, fast_seq=True)
    cen = str(d / "centromeres.bed")
    with open(cen, "w") as fp:
        fp.write("chr1\t900000\t950000\tp11.1\tacen\nchr1\t950000\t1000000\tq11\tacen\n")
    return dict(dir=d, bam=path, centromeres=cen)


def test_cnv_mode_from_a_bam_file_to_the_cns_and_the_seeds(amplified):
    d = amplified["dir"]
    out = {}
    for pipe, device in (("gpu", GPU), ("cpu", "cpu")):
        cns, bed = str(d / (pipe + ".cns")), str(d / (pipe + "_CNV_SEEDS.bed"))
        assert CoRAL.main(["cnv", "--lr_bam", amplified["bam"], "--output", cns, "--seeds", bed, "--centromeres", amplified["centromeres"], "--device", device]) == cns
        out[pipe] = (open(cns).read(), open(bed).read())
    assert out["gpu"] == out["cpu"]
    rows = [ln.split("\t") for ln in out["gpu"][0].split("\n")[1:-1]]
    assert [(r[0], int(r[1]), int(r[2]), int(r[6])) for r in rows] == [("chr1", 0, 100000, 100), ("chr1", 100000, 400000, 300), ("chr1", 400000, 1200000, 800)]
    assert [float(r[5]) for r in rows] == [1.0, 8.0, 1.0] and abs(float(rows[1][4]) - 3.0) < 1e-3
    seeds = cnv.find_seeds(str(d / "gpu.cns"), amplified["centromeres"], amplified["bam"])
    assert seeds == [("chr1", 100000, 399999)] and out["gpu"][1] == "chr1\t100000\t399999\n"
    seg = cnv.call_copy_number(amplified["bam"], device=GPU)
    assert seg.write(str(d / "api.cns")) and open(str(d / "api.cns")).read() == out["gpu"][0]
