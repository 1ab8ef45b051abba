"""The GC correction and the called-base mask of the copy-number segmenter on the host (coral_cn_segment_gc_host:
coral_amd/csrc/coral_cn_host.h over coral_cn_core.h) against the plain-Python restatement in tests/comp_cases.py - rows, counts,
bias and the bins per stratum -, two properties of the correction, the old entry points against the new ones without a
composition, and the Python layer's arguments.  The device is compared with the host in tests/test_cnv_gc_gpu.py."""
import numpy as np
import pytest

from coral_amd import _lib, bam, cnv, composition
from tests import cnv_cases as cn
from tests import comp_cases as cc


@pytest.fixture(scope="module")
def table():
    return cc.gc_cases()


def test_the_cases_cover_what_they_are_meant_to(table):
    r = {name: cc.restate_gc(*t) for name, t in table.items()}
    assert r["g4_three_bins"][3] == [1, 0, 1, 0, 1] and r["g4_three_bins"][1]["kept"] == 3
    sb = r["g1000_fifty_bins"][3]
    assert len(sb) == 1001 and sum(sb) == 50 and sum(1 for x in sb if x == 0) > 940 and all(b != 0 for b in (r["g1000_fifty_bins"][2][0], r["g1000_fifty_bins"][2][1000]))
    assert r["one_stratum"][3][41] == 400 and sum(r["one_stratum"][3]) == 400 and len(set(r["one_stratum"][2])) == 1
    assert r["gc_equals_acgt"][3][10] > 200 and r["gc_equals_acgt"][3][5] > 100
    assert len(set(r["min_bins_above_p"][2])) == 1 and sum(r["min_bins_above_p"][3]) == r["min_bins_above_p"][1]["kept"]
    assert min(r["both_signs"][2]) < 0 < max(r["both_signs"][2])
    case, gc, at, G = table["strata_the_pool_lacks"][:4]
    lacking = {int(g) * G // (int(g) + int(a)) for g, a in zip(gc[800:], at[800:])} - {t for t, n in enumerate(r["strata_the_pool_lacks"][3]) if n}
    assert len(lacking) > 10 and any(row[0] == 1 for row in r["strata_the_pool_lacks"][0])
    assert (r["min_called_0"][1]["uncalled"], r["min_called_500"][1]["uncalled"], r["min_called_1000"][1]["uncalled"]) == (3, 23, 24)
    assert r["with_a_reference"][1]["ref_centre"] > 0
    for name in table:
        assert r[name][1]["breakpoints"] >= (0 if name == "g4_three_bins" else 1), name


def test_host_equals_the_restatement(table):
    for name, t in table.items():
        margins = []
        want = cc.restate_gc(*t, margins=margins)
        assert all(m > cn.MARGIN for m in margins), name             # no cut hangs on the last bit of erfc
        got = cc.segment_gc(*t)
        assert got[2] == want[2], name
        assert got[3] == want[3], name
        assert got[1] == want[1], name
        assert got[0] == want[0], name


def biased_table(k_of_stratum, strata=20, n=2400, step=1920, seed=5):
    """One contig with a two-fold step at bin ``step``; the GC fraction runs through eight levels, 60 bins each, again and again,
    so that the depth of a bin - multiplied by 2^k(g) of its stratum g - shows steps of two and four every 60 bins.  Every
    stratum has 300 bins, 60 of them behind the step, which starts a new round of the eight levels: every stratum's median is
    a bin in front of the step and stands at the same quantile of those, as the rule needs it (a stratum that lay mostly behind
    the step would have the step itself taken out as bias, and strata with unequal shares behind it would get medians a
    fraction of the noise apart, which the segmenter finds as steps of their own where the level changes)."""
    rng = np.random.RandomState(seed)
    frac = np.tile(np.repeat(0.27 + 0.05 * np.arange(8), 60), n // 480 + 1)[:n] + rng.uniform(-0.01, 0.01, n)
    gc = np.round(frac * 1000).astype(np.uint32)
    at = (1000 - gc).astype(np.uint32)
    plain = cn.noisy(rng, n, 3000, [(step, n, 2.0)])
    g = gc.astype(np.int64) * strata // 1000
    k = np.array([k_of_stratum(int(x)) for x in g], dtype=np.int64)
    assert plain.min() * 4 > plain.max() * 1 and len(set(k.tolist())) == 3
    return cn.Case(["chr1"], [n * 1000], 1000, plain), cn.Case(["chr1"], [n * 1000], 1000, plain << k), gc, at, strata, step


def test_log2_q16_shifts_exactly():
    L = _lib.lib()
    rng = np.random.RandomState(1)
    for x in [1, 2, 3, (1 << 40) - 1] + [int(v) for v in rng.randint(1, 1 << 40, 300, dtype=np.int64)]:
        for k in range(5):
            assert L.coral_cn_log2_q16(x << k) == L.coral_cn_log2_q16(x) + (k << 16)


def test_a_bias_of_whole_powers_of_two_is_taken_out_exactly():
    plain, biased, gc, at, strata, step = biased_table(lambda g: g % 3)
    a = cc.segment_gc(plain, gc, at, strata, 1, 500)
    b = cc.segment_gc(biased, gc, at, strata, 1, 500)
    assert a[1]["kept"] == b[1]["kept"] == 2400                      # the 1/32 mask keeps every bin in both runs
    assert [r[:5] for r in a[0]] == [r[:5] for r in b[0]] and a[1]["breakpoints"] == b[1]["breakpoints"]
    assert a[3] == b[3] and a[2] != b[2]
    assert cc.restate_gc(biased, gc, at, strata, 1, 500)[0] == b[0]


def test_the_correction_shows():
    plain, biased, gc, at, strata, step = biased_table(lambda g: g % 3)
    depth = biased.depth(bam)
    comp = composition.Composition(["chr1"], [2400 * 1000], 1000, gc, at, np.zeros(2400, dtype=np.uint32))
    without = cnv.segment_depth(depth, device="cpu")
    with_it = cnv.segment_depth(depth, device="cpu", composition=comp, gc_strata=strata, gc_min_bins=1)
    assert without.gc_bias is None and without.counts["breakpoints"] > with_it.counts["breakpoints"]
    assert with_it.counts["breakpoints"] == 1 and with_it.start.tolist() == [0, step * 1000] and with_it.end.tolist() == [step * 1000, 2400 * 1000]
    assert abs(with_it.log2[1] - with_it.log2[0] - 1.0) < 0.01
    assert with_it.gc_bias["strata"] == strata and int(with_it.gc_bias["stratum_bins"].sum()) == 2400 and with_it.gc_bias["bias"].dtype == np.float64
    assert np.array_equal(with_it.gc_bias["bias"] * 65536.0, with_it.gc_bias["bias_q16"]) and with_it.counts["uncalled"] == 0


def test_without_a_composition_the_new_entry_points_are_the_old():
    for name, case in cn.cases().items():
        old = cc.segment_gc(case, None, None, 100, 256, 500, entry="old")
        new = cc.segment_gc(case, None, None, 100, 256, 500)
        assert old[:2] == new[:2] and new[1]["uncalled"] == 0, name
        assert old[0] == cn.restate(case)[0], name
        assert new[2] == [-7] * 101                                   # bias and stratum_bins are not touched


def test_segment_depth_takes_a_composition_by_contig_name(table):
    case, gc, at, G, min_bins, permille = table["strata_the_pool_lacks"]
    depth = case.depth(bam)
    # the FASTA has the contigs in another order and one more
    comp = composition.Composition(["chrX", "chrUn", "chr1"], [300 * 100, 250, 800 * 100], 100, np.concatenate([gc[800:], [1, 2, 3], gc[:800]]),
                                   np.concatenate([at[800:], [1, 2, 3], at[:800]]), np.zeros(1103, dtype=np.uint32))
    seg = cnv.segment_depth(depth, device="cpu", composition=comp, gc_strata=G, gc_min_bins=min_bins, min_called=permille / 1000)
    want = cc.restate_gc(case, gc, at, G, min_bins, permille)
    assert cn.rows_of(seg) == want[0] and seg.gc_bias["bias_q16"].tolist() == want[2] and seg.gc_bias["stratum_bins"].tolist() == want[3]
    assert {k: seg.counts[k] for k in want[1]} == want[1]
    for kw in ({"gc_strata": 0}, {"gc_strata": 1001}, {"gc_strata": 2.5}, {"gc_min_bins": 0}, {"gc_min_bins": True}, {"min_called": -0.1}, {"min_called": 1.5}, {"min_called": "x"}):
        with pytest.raises(ValueError):
            cnv.segment_depth(depth, device="no such device", composition=comp, **kw)
        with pytest.raises(ValueError):
            cnv.call_copy_number("/no/such.bam", device="no such device", **kw)
    with pytest.raises(ValueError, match="bins of 100 positions"):
        cnv.segment_depth(cn.Case(["chr1"], [800 * 50], 50, np.ones(800)).depth(bam), device="no such device", composition=comp)
    with pytest.raises(ValueError, match="not in the FASTA"):
        cnv.segment_depth(cn.Case(["chr9"], [800 * 100], 100, np.ones(800)).depth(bam), device="no such device", composition=comp)
    for bad in ((0, 1, 500), (1001, 1, 500), (4, 0, 500), (4, 1, -1), (4, 1, 1001)):
        with pytest.raises(AssertionError):
            cc.segment_gc(table["g4_three_bins"][0], table["g4_three_bins"][1], table["g4_three_bins"][2], *bad)
