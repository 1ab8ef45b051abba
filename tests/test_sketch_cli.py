"""The `sketch` mode's command line: on the host backend (--device cpu) a small FASTA file end to end, --weights from the `kmers`
mode's output, the printed summary and the error exits; one GPU case holds --device cuda:0 against --device cpu.  Arrays are
compared, not file bytes: a zip archive carries timestamps."""
import io

import numpy as np
import pytest

from coral_amd import CoRAL, minimizers
from tests import kmer_cases, sketch_cases as SC

K, W = 8, 5


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("sketch_cli")
    data = SC.six_records() + b">repeat\n" + kmer_cases.wrap(b"GATTACA" * 80, 60)
    out = dict(dir=d, data=data, fasta=str(d / "ref.fa"))
    with open(out["fasta"], "wb") as fp:
        fp.write(data)
    return out


def run(files, name, *argv, device="cpu"):
    path = str(files["dir"] / name)
    assert CoRAL.main(["sketch", "--ref", files["fasta"], "--output", path, "--k", str(K), "--w", str(W), "--device", device] + list(argv)) == path
    return minimizers.MinimizerIndex.load(path)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a.arrays(), b.arrays())) and (a.k, a.w, a.weighted, a.contig_names, a.contig_lengths) == (
        b.k, b.w, b.weighted, b.contig_names, b.contig_lengths)


def test_the_mode_end_to_end_and_its_summary(files, capsys):
    want = minimizers.sketch_reference(io.BytesIO(files["data"]), K, W, device="cpu")
    got = run(files, "ref.cmi.npz")
    printed = capsys.readouterr().out
    assert same(got, want) and got.n > 1000
    for text in ("contigs: 7\n", "bases: %d\n" % sum(want.contig_lengths), "minimizers: %d\n" % want.n, "density: %.6f\n" % (want.n / sum(want.contig_lengths)), "seconds: open=", " read=",
                 " sketch=", " sort=", "ref.cmi.npz (%d entries)\n" % want.n):
        assert text in printed, text
    assert same(run(files, "small_pieces.cmi.npz", "--chunk_bytes", "17"), want)
    assert set(minimizers.LAST_SKETCH) >= {"read", "feed", "upload", "symbols", "sketch", "sort", "write", "wall"}


def test_weights_from_the_kmers_mode(files):
    rep = str(files["dir"] / "repetitive.txt")
    assert CoRAL.main(["kmers", "--ref", files["fasta"], "--output", rep, "--k", str(K), "--greater_than", "10", "--device", "cpu"]) == rep
    listed = [line.split(b"\t")[0].decode() for line in open(rep, "rb")]
    assert len(listed) >= 7
    want = minimizers.sketch_reference(io.BytesIO(files["data"]), K, W, listed, device="cpu")
    got = run(files, "weighted.cmi.npz", "--weights", rep)
    assert got.weighted and same(got, want) and not same(got, run(files, "plain.cmi.npz"))
    assert SC.index_rows(got) == SC.sorted_rows(SC.restate(files["data"], K, W, frozenset(SC.canonical(s.encode()) for s in listed))[2])


@pytest.mark.parametrize("argv", [["--k", "0"], ["--k", "17"], ["--w", "0"], ["--w", "257"], ["--chunk_bytes", "15"]])
def test_argument_errors_come_before_any_work(files, argv):
    args = ["sketch", "--ref", str(files["dir"] / "does_not_exist.fa"), "--output", str(files["dir"] / "never.npz"), "--device", "cpu"]
    with pytest.raises(ValueError):
        CoRAL.main(args + argv)


def test_weights_of_another_k_are_refused(files):
    rep = str(files["dir"] / "k6.txt")
    with open(rep, "w") as fp:
        fp.write("ACGTAC\t12\n")
    with pytest.raises(ValueError):
        CoRAL.main(["sketch", "--ref", files["fasta"], "--output", str(files["dir"] / "never.npz"), "--k", str(K), "--weights", rep, "--device", "cpu"])


@pytest.mark.parametrize("argv", [[], ["--ref", "x.fa"], ["--ref", "x.fa", "--output", "x.npz", "--k", "fifteen"], ["--ref", "x.fa", "--output", "x.npz", "--w", "wide"]])
def test_the_parser_refuses(argv):
    with pytest.raises(SystemExit):
        CoRAL.main(["sketch"] + argv)


def test_a_missing_file_is_an_error(files):
    with pytest.raises(OSError):
        CoRAL.main(["sketch", "--ref", str(files["dir"] / "does_not_exist.fa"), "--output", str(files["dir"] / "never.npz"), "--device", "cpu"])


@pytest.mark.gpu
def test_both_devices_write_equal_arrays(files):
    assert same(run(files, "gpu.cmi.npz", device="cuda:0"), run(files, "cpu.cmi.npz"))
    assert same(run(files, "gpu_pieces.cmi.npz", "--chunk_bytes", "4097", device="cuda:0"), run(files, "cpu.cmi.npz"))
