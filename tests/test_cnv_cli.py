"""The `cnv` mode's command line on the host backend (--device cpu): --depth in place of --lr_bam, --reference_cnn, --seeds, and the
argument errors, which come before any work.  The GPU backend's run of the mode is in tests/test_cnv_gpu.py."""
import numpy as np
import pytest

from coral_amd import CoRAL, bam, cnv
from tests import cnv_cases as cc


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cnv_cli")
    table = cc.cases()
    out = dict(dir=d, case=table["one_step"], ref_case=table["reference"])
    out["depth"] = table["one_step"].depth(bam).write(str(d / "sample.cnn"))
    out["normal"] = table["reference"].depth(bam, "ref").write(str(d / "normal.cnn"))
    out["centromeres"] = str(d / "centromeres.bed")
    with open(out["centromeres"], "w") as fp:
        fp.write("chr1\t50000\t51000\tp11\tacen\nchr1\t51000\t52000\tq11\tacen\n")
    return out


def test_depth_table_in_place_of_the_bam_file(files):
    cns = str(files["dir"] / "sample.cns")
    assert CoRAL.main(["cnv", "--depth", files["depth"], "--output", cns, "--device", "cpu"]) == cns
    want = cnv.segment_depth(files["case"].depth(bam), device="cpu")
    assert open(cns).read() == open(want.write(str(files["dir"] / "want.cns"))).read() and len(want) == 3


def test_reference_levels_and_q_reach_the_segmenter(files):
    cns = str(files["dir"] / "with_normal.cns")
    CoRAL.main(["cnv", "--depth", files["depth"], "--reference_cnn", files["normal"], "--levels", "3", "--fdr_q", "0.01", "--output", cns, "--device", "cpu"])
    want = cnv.segment_depth(files["ref_case"].depth(bam), files["ref_case"].depth(bam, "ref"), levels=3, fdr_q=0.01, device="cpu")
    assert open(cns).read() == open(want.write(str(files["dir"] / "want_with_normal.cns"))).read()


def test_seeds_from_the_written_cns(files):
    cns, bed = str(files["dir"] / "seeded.cns"), str(files["dir"] / "seeded_CNV_SEEDS.bed")
    CoRAL.main(["cnv", "--depth", files["depth"], "--output", cns, "--seeds", bed, "--centromeres", files["centromeres"], "--gain", "5", "--min_seed_size", "5000",
                "--max_seg_gap", "1000", "--device", "cpu"])
    sizes = {"chr1": 60000}
    assert open(bed).read() == "".join("%s\t%d\t%d\n" % s for s in cnv.find_seeds(cns, files["centromeres"], sizes, 5.0, 5000, 1000)) == "chr1\t20000\t25999\n"


@pytest.mark.parametrize("argv", [
    ["--levels", "0"], ["--levels", "21"], ["--fdr_q", "0"], ["--fdr_q", "1.5"], ["--seeds", "x.bed"],
    ["--seeds", "x.bed", "--centromeres", "c.bed", "--output", "x.txt"]])
def test_argument_errors_come_before_any_work(files, argv):
    args = ["cnv", "--depth", str(files["dir"] / "does_not_exist.cnn"), "--output", str(files["dir"] / "never.cns"), "--device", "cpu"]
    with pytest.raises(ValueError):
        CoRAL.main(args + argv)


@pytest.mark.parametrize("argv", [[], ["--lr_bam", "x.bam", "--depth", "x.cnn", "--output", "x.cns"], ["--lr_bam", "x.bam"], ["--depth", "x.cnn", "--output", "x.cns", "--levels", "five"]])
def test_the_parser_refuses(argv):
    with pytest.raises(SystemExit):
        CoRAL.main(["cnv"] + argv)


def test_a_reference_with_other_bins_is_refused(files):
    other = bam.BinnedDepth(["chr1"], [60000], 50, 0, 0x704, True, [0, 1200], np.ones(1200, dtype=np.int64), np.zeros(1200, dtype=np.int64)).write(str(files["dir"] / "fine.cnn"))
    with pytest.raises(ValueError, match="other bins"):
        CoRAL.main(["cnv", "--depth", files["depth"], "--reference_cnn", other, "--output", str(files["dir"] / "never.cns"), "--device", "cpu"])
