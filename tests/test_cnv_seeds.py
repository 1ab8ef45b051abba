"""cnv.find_seeds / write_seeds against the reference's run_seeding, through tests/golden/cnv_seeds.json (made by
tests/golden/make_cnv_seeds_golden.py from the unmodified reference: per case the input text, the bed it wrote - or the exception
it ended with - and, once, the centromere rows and chromosome sizes it read).  Text for text."""
import json
import os

import pytest

from coral_amd import cnv

HERE = os.path.dirname(os.path.abspath(__file__))
WANTED = ("p_arm", "q_arm", "both_arms_bed", "gap_300001", "gap_300002", "length_99998", "length_99999", "length_100000",
          "long_seed_between_gain_and_1p2_gain", "arm_at_cn4_raises_the_cutoff", "cutoff_splits_a_chain", "dropped_segment_quirk", "no_seed", "no_gain_at_all")


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    with open(os.path.join(HERE, "golden", "cnv_seeds.json")) as fp:
        g = json.load(fp)
    d = tmp_path_factory.mktemp("cnv_seeds")
    g["dir"] = d
    g["centromere_file"] = str(d / "centromeres.bed")
    with open(g["centromere_file"], "w") as fp:
        fp.write("".join("\t".join(row) + "\n" for row in g["centromeres"]))
    g["sizes_file"] = str(d / "chrom.sizes")
    with open(g["sizes_file"], "w") as fp:
        fp.write("".join("%s\t%d\n" % kv for kv in g["chrom_sizes"].items()))
    return g


def seeds_text(golden, name, sizes=None, **kw):
    case = golden["cases"][name]
    src, dst = str(golden["dir"] / (name + case["extension"])), str(golden["dir"] / (name + "_CNV_SEEDS.bed"))
    with open(src, "w") as fp:
        fp.write(case["input"])
    seeds = cnv.find_seeds(src, golden["centromere_file"], golden["chrom_sizes"] if sizes is None else sizes, **kw)
    assert cnv.write_seeds(seeds, dst) == dst
    with open(dst) as fp:
        return fp.read()


def test_the_fixture_holds_the_cases():
    with open(os.path.join(HERE, "golden", "cnv_seeds.json")) as fp:
        g = json.load(fp)
    assert sorted(g["cases"]) == sorted(WANTED) and (g["gain"], g["min_seed_size"], g["max_seg_gap"]) == (6.0, 99999, 300001)
    seeds = {k: c.get("seeds") for k, c in g["cases"].items()}
    assert seeds["gap_300001"].count("\n") == 1 and seeds["gap_300002"] == "" and seeds["length_99998"] == "" and seeds["length_99999"] != ""
    assert "chr5\t10000000" not in seeds["long_seed_between_gain_and_1p2_gain"] and "chr21\t6000000" not in seeds["arm_at_cn4_raises_the_cutoff"]
    assert seeds["no_seed"] == "" and g["cases"]["no_gain_at_all"]["reference_raises"] == "IndexError"
    assert {c["extension"] for c in g["cases"].values()} == {".cns", ".bed"}


@pytest.mark.parametrize("name", [n for n in WANTED if n != "no_gain_at_all"])
def test_find_seeds_writes_the_references_bed(golden, name):
    want = golden["cases"][name]["seeds"]
    assert seeds_text(golden, name, gain=golden["gain"], min_seed_size=golden["min_seed_size"], max_seg_gap=golden["max_seg_gap"]) == want
    assert seeds_text(golden, name, sizes=golden["sizes_file"]) == want          # the defaults are the reference's module constants


def test_where_the_reference_ends_with_an_exception(golden, tmp_path):
    """No segment at or above the gain: IndexError there, no seeds here.  A seed astride the centromere: os.abort() there,
    ValueError naming it here.  Another extension: an undefined name there, ValueError here."""
    assert seeds_text(golden, "no_gain_at_all") == ""
    cen = str(tmp_path / "cen.bed")
    with open(cen, "w") as fp:
        fp.write("chrA\t1000000\t1000010\tp11\tacen\nchrA\t1000010\t1000020\tq11\tacen\n")
    astride = str(tmp_path / "astride.bed")
    with open(astride, "w") as fp:
        fp.write("chrA\t800000\t1000000\t8.0\nchrA\t1000020\t1200000\t8.0\n")
    with pytest.raises(ValueError, match="chrA:800000-1200000"):
        cnv.find_seeds(astride, cen, {"chrA": 3000000})
    other = str(tmp_path / "segments.txt")
    with open(other, "w") as fp:
        fp.write("chrA\t0\t500000\t8.0\n")
    with pytest.raises(ValueError, match="cns or a .bed"):
        cnv.find_seeds(other, cen, {"chrA": 3000000})
    unlisted = str(tmp_path / "unlisted.bed")                    # a contig without centromere rows is skipped (KeyError there)
    with open(unlisted, "w") as fp:
        fp.write("chrUn_1\t0\t500000\t9.0\nchrA\t0\t400000\t8.0\n")
    assert cnv.find_seeds(unlisted, cen, {"chrA": 3000000}) == [("chrA", 0, 399999)]
    with pytest.raises(ValueError, match="no length"):
        cnv.find_seeds(unlisted, cen, {})
