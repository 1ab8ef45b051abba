"""The `kmers` mode's command line on the host backend (--device cpu): a small FASTA file and its .gz end to end, --histogram,
--greater_than, --forward, --both_strands, the printed summary and the error exits.  The GPU backend's run of the mode is in
tests/test_kmer_gpu.py."""
import gzip

import pytest

from coral_amd import CoRAL
from tests import kmer_cases as kc

K = 6


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("kmer_cli")
    table = kc.cases()
    data = table["n_runs"] + table["crlf"] + table["palindromes"] + b">repeat\n" + kc.wrap(b"GATTACA" * 40, 60)
    out = dict(dir=d, data=data, fasta=str(d / "ref.fa"), gz=str(d / "ref.fa.gz"))
    with open(out["fasta"], "wb") as fp:
        fp.write(data)
    with gzip.open(out["gz"], "wb") as fp:
        fp.write(data)
    return out


def run(files, name, *argv, ref="fasta"):
    path = str(files["dir"] / name)
    assert CoRAL.main(["kmers", "--ref", files[ref], "--output", path, "--k", str(K), "--device", "cpu"] + list(argv)) == path
    return open(path, "rb").read()


def test_the_mode_end_to_end_and_its_summary(files, capsys):
    counts, stats, hist = kc.restate(files["data"], K, True)
    assert run(files, "default.txt") == kc.expected_lines(counts, K, kc.threshold(hist, "0.9998"))      # (of fewer than 5 000 distinct k-mers, 0.9998 keeps all)
    capsys.readouterr()
    t = kc.threshold(hist, "0.99")
    text = run(files, "default.txt", "--distinct", "0.99")
    printed = capsys.readouterr().out
    assert text == kc.expected_lines(counts, K, t) and text
    lines = text.count(b"\n")
    for want in ("n_sequences: %d\n" % stats["n_sequences"], "n_bases: %d\n" % stats["n_bases"], "total: %d\n" % stats["total"], "distinct: %d\n" % stats["distinct"],
                 "threshold: %d\n" % t, "default.txt (%d lines)\n" % lines):
        assert want in printed, want
    assert run(files, "gz.txt", "--distinct", "0.99", ref="gz") == text
    assert run(files, "small_pieces.txt", "--distinct", "0.99", "--chunk_bytes", "16") == text


def test_distinct_and_greater_than(files):
    counts, _stats, hist = kc.restate(files["data"], K, True)
    for p in ("0.5", "0.99", "0", "1"):
        assert run(files, "p.txt", "--distinct", p) == kc.expected_lines(counts, K, kc.threshold(hist, p)), p
    assert run(files, "p1.txt", "--distinct", "1") == b""
    for n in (0, 3, 10 ** 6):
        assert run(files, "n.txt", "--greater_than", str(n)) == kc.expected_lines(counts, K, n), n


def test_forward_and_both_strands(files):
    forward = kc.restate(files["data"], K, False)[0]
    canonical = kc.restate(files["data"], K, True)[0]
    assert forward != canonical
    assert run(files, "forward.txt", "--forward", "--greater_than", "2") == kc.expected_lines(forward, K, 2)
    both = run(files, "both.txt", "--both_strands", "--greater_than", "2")
    assert both == kc.expected_lines(canonical, K, 2, both_strands=True) and both.count(b"\n") > run(files, "one.txt", "--greater_than", "2").count(b"\n")


def test_histogram_file(files, capsys):
    hist = kc.restate(files["data"], K, True)[2]
    path = str(files["dir"] / "hist.txt")
    run(files, "with_hist.txt", "--histogram", path)
    assert open(path).read() == "".join("%d\t%d\n" % row for row in hist) and len(hist) > 3
    assert "hist.txt (%d lines)" % len(hist) in capsys.readouterr().out


@pytest.mark.parametrize("argv", [["--k", "0"], ["--k", "17"], ["--distinct", "1.5"], ["--distinct", "x"], ["--distinct", "1e-3"], ["--greater_than", "-1"], ["--chunk_bytes", "15"]])
def test_argument_errors_come_before_any_work(files, argv):
    args = ["kmers", "--ref", str(files["dir"] / "does_not_exist.fa"), "--output", str(files["dir"] / "never.txt"), "--device", "cpu"]
    with pytest.raises(ValueError):
        CoRAL.main(args + argv)


@pytest.mark.parametrize("argv", [[], ["--ref", "x.fa"], ["--ref", "x.fa", "--output", "x.txt", "--distinct", "0.5", "--greater_than", "3"],
                                  ["--ref", "x.fa", "--output", "x.txt", "--k", "fifteen"]])
def test_the_parser_refuses(argv):
    with pytest.raises(SystemExit):
        CoRAL.main(["kmers"] + argv)


def test_a_missing_file_is_an_error(files):
    with pytest.raises(OSError):
        CoRAL.main(["kmers", "--ref", str(files["dir"] / "does_not_exist.fa"), "--output", str(files["dir"] / "never.txt"), "--device", "cpu"])
