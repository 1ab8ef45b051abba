"""The `composition` mode's command line on the host backend (--device cpu), `cnv --depth ... --composition ...` and `cnv --depth
... --ref ...`, and the argument refusals, which come before any work.  The GPU backend's runs of both modes are in
tests/test_comp_gpu.py and tests/test_cnv_gc_gpu.py."""
import numpy as np
import pytest

from coral_amd import CoRAL, bam, cnv, composition
from tests import cnv_cases as cn
from tests import comp_cases as cc


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """A genome of two contigs with a gap of N, its FASTA, and a depth table over it with a GC wave and one amplified stretch."""
    d = tmp_path_factory.mktemp("comp_cli")
    rng = np.random.RandomState(14)
    frac = 0.3 + 0.3 * (np.arange(700) // 25 % 4) / 3.0                                     # four GC levels, 25 bins each, again and again
    strong = rng.rand(700_000) < np.repeat(frac, 1000)                                    # every base G/C with its bin's probability
    chr1 = bytearray(np.where(strong, np.frombuffer(b"GC", dtype=np.uint8)[rng.randint(0, 2, 700_000)], np.frombuffer(b"AT", dtype=np.uint8)[rng.randint(0, 2, 700_000)]).tobytes())
    chr1[300_000:330_000] = b"N" * 30_000
    chr2 = cc.random_sequence(rng, 50_250, b"ACGTacgt")
    out = dict(dir=d, fasta=str(d / "ref.fa"))
    with open(out["fasta"], "wb") as fp:
        fp.write(b">chr1 assembled\n" + cc.wrap(bytes(chr1), 80) + b">chr2\n" + cc.wrap(chr2, 80) + b">unplaced\nACGT\n")
    comp = composition.reference_composition(out["fasta"], 1000, device="cpu")
    gcf = np.nan_to_num(comp.gc_fraction()[:700], nan=0.5)
    bases = np.concatenate([(cn.noisy(rng, 700, 4000, [(100, 200, 3.0)]) * (0.85 + 0.3 * gcf)).astype(np.int64), cn.noisy(rng, 51, 4000)])
    out["case"] = cn.Case(["chr1", "chr2"], [700_000, 50_250], 1000, bases)
    out["depth"] = out["case"].depth(bam).write(str(d / "sample.cnn"))
    out["comp"] = comp
    return out


def test_composition_mode_writes_the_table(files, capsys):
    path = str(files["dir"] / "bins.tsv")
    assert CoRAL.main(["composition", "--ref", files["fasta"], "--bin_size", "1000", "--output", path, "--device", "cpu", "--chunk_bytes", "4096"]) == path
    printed = capsys.readouterr().out
    assert "contigs: 3\npositions: 750254\nbins: 752\n" in printed and "gc_fraction: %.6f\n" % files["comp"].genome_gc() in printed
    back = composition.Composition.read(path)
    want = cc.restate(open(files["fasta"], "rb").read(), 1000)
    assert (back.chroms, back.lengths, back.gc.tolist(), back.at.tolist(), back.masked.tolist()) == want and back.bin_size == 1000
    assert back.gc[300:330].tolist() == [0] * 30 and back.at[300:330].tolist() == [0] * 30 and np.isnan(back.gc_fraction()[300:330]).all()


def test_cnv_with_a_written_composition_and_with_the_fasta(files, capsys):
    d = files["dir"]
    table, plain, with_table, with_fasta = (str(d / n) for n in ("bins2.tsv", "plain.cns", "table.cns", "fasta.cns"))
    files["comp"].write(table)
    CoRAL.main(["cnv", "--depth", files["depth"], "--output", plain, "--device", "cpu"])
    capsys.readouterr()
    CoRAL.main(["cnv", "--depth", files["depth"], "--composition", table, "--gc_strata", "50", "--gc_min_bins", "40", "--min_called", "0.9", "--output", with_table, "--device", "cpu"])
    printed = capsys.readouterr().out
    CoRAL.main(["cnv", "--depth", files["depth"], "--ref", files["fasta"], "--gc_strata", "50", "--gc_min_bins", "40", "--min_called", "0.9", "--output", with_fasta, "--device", "cpu"])
    assert open(with_table).read() == open(with_fasta).read() != open(plain).read()
    want = cnv.segment_depth(files["case"].depth(bam), device="cpu", composition=files["comp"], gc_strata=50, gc_min_bins=40, min_called=0.9)
    assert open(with_table).read() == open(want.write(str(d / "want.cns"))).read()
    assert "GC correction: " in printed and "30 bins masked as uncalled" in printed and want.counts["uncalled"] == 30
    # the GC wave is gone: the amplified stretch and the gap are the only edges on chr1
    rows = [r for r in want.rows() if r[0] == "chr1"]
    assert [(r[1], r[2]) for r in rows] == [(0, 100_000), (100_000, 200_000), (200_000, 700_000)]
    assert len(open(plain).read().splitlines()) > len(open(with_table).read().splitlines()) + 10


@pytest.mark.parametrize("argv", [["--gc_strata", "0"], ["--gc_strata", "1001"], ["--gc_min_bins", "0"], ["--min_called", "-0.5"], ["--min_called", "1.01"]])
def test_cnv_argument_errors_come_before_any_work(files, argv):
    args = ["cnv", "--depth", str(files["dir"] / "does_not_exist.cnn"), "--composition", str(files["dir"] / "nor_this.tsv"), "--output", str(files["dir"] / "never.cns"), "--device", "cpu"]
    with pytest.raises(ValueError):
        CoRAL.main(args + argv)


@pytest.mark.parametrize("argv", [["--bin_size", "0"], ["--bin_size", str(1 << 31)], ["--chunk_bytes", "8"]])
def test_composition_argument_errors_come_before_any_work(files, argv):
    with pytest.raises(ValueError):
        CoRAL.main(["composition", "--ref", str(files["dir"] / "does_not_exist.fa"), "--output", str(files["dir"] / "never.tsv"), "--device", "no such device"] + argv)
    assert not (files["dir"] / "never.tsv").exists()


@pytest.mark.parametrize("argv", [["composition"], ["composition", "--ref", "x.fa"], ["composition", "--ref", "x.fa", "--output", "o", "--bin_size", "ten"],
                                  ["cnv", "--depth", "x.cnn", "--output", "x.cns", "--ref", "x.fa", "--composition", "x.tsv"],
                                  ["cnv", "--depth", "x.cnn", "--output", "x.cns", "--gc_strata", "many"]])
def test_the_parser_refuses(argv):
    with pytest.raises(SystemExit):
        CoRAL.main(argv)


def test_a_composition_with_other_bins_is_refused(files):
    other = composition.reference_composition(files["fasta"], 500, device="cpu").write(str(files["dir"] / "fine.tsv"))
    with pytest.raises(ValueError, match="bins of 500 positions"):
        CoRAL.main(["cnv", "--depth", files["depth"], "--composition", other, "--output", str(files["dir"] / "never.cns"), "--device", "cpu"])
    assert not (files["dir"] / "never.cns").exists()
