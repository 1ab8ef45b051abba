"""The `qc --fastq` and `filter` modes of coral_amd/CoRAL.py on the host backend (`--device cpu`, coral_fastq_* behind
coral_amd/fastq.py): the files of `qc --fastq` against `qc --lr_bam` on a BAM that holds the same reads, the kept reads' bytes
and the printed counters of `filter`, and the argument rules."""
import json
import os

import numpy as np
import pytest

from coral_amd import CoRAL, bam, fastq, synth
from tests import fastq_cases as fc
from tests.bamfile import M, read_bam

SEQ_LETTERS = "=ACMGRSVTWYHKDBN"


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """A BAM of unclipped primary records with qualities, and the FASTQ of the same reads written from the bytes that
    tests/bamfile.py reads back."""
    d = tmp_path_factory.mktemp("fastqcli")
    rng = np.random.RandomState(51)
    lens = [int(n) for n in rng.randint(1, 400, 80)] + [7000]
    quals = [rng.randint(0, 61, n).astype(np.uint8) for n in lens]
    rec = synth.records_from_alignments([dict(tid=0, pos=10 + 20 * k, cigar=[(M, n)], flag=16 if k % 4 == 2 else 0, name="read%d" % k) for k, n in enumerate(lens)])
    path, fq = str(d / "reads.bam"), str(d / "reads.fastq")
    bam.write_bam(rec, path, seed=9, qual=lambda i: quals[i].tobytes())
    recs = read_bam(path).recs
    assert [r["l_seq"] for r in recs] == lens
    text = b"".join(fc.record(r["name"].encode(), "".join(SEQ_LETTERS[c] for c in r["codes"]).encode(), bytes((r["qual"] + 33).astype(np.uint8))) for r in recs)
    with open(fq, "wb") as fp:
        fp.write(text)
    return dict(bam=path, fastq=fq, text=text, lens=lens, quals=quals)


def test_qc_fastq_writes_what_qc_lr_bam_writes(case, tmp_path, capsys):
    d_fq, d_bam = str(tmp_path / "from_fastq"), str(tmp_path / "from_bam")
    wrote = CoRAL.main(["qc", "--fastq", case["fastq"], "--output_dir", d_fq, "--device", "cpu", "--chunk_bytes", "5000"])
    printed = capsys.readouterr().out
    want = {"quality_control_summary.tsv", "read_qc.json"}
    try:
        import matplotlib  # noqa: F401
        want |= {"mean_length_histogram.png", "mean_sequence_quality_histogram.png"}
    except ImportError:
        pass
    assert set(os.listdir(d_fq)) == want and {os.path.basename(w) for w in wrote} == want and all(("Wrote %s" % w) in printed for w in wrote)
    CoRAL.main(["qc", "--lr_bam", case["bam"], "--output_dir", d_bam, "--device", "cpu", "--no_plots"])
    tsv = open(os.path.join(d_fq, "quality_control_summary.tsv"), "rb").read()
    assert tsv == open(os.path.join(d_bam, "quality_control_summary.tsv"), "rb").read() and tsv.startswith(b"\tQ25\tQ50\tQ75\nmean_length\t")
    with open(os.path.join(d_fq, "read_qc.json")) as fp:
        js = json.load(fp)
    with open(os.path.join(d_bam, "read_qc.json")) as fp:
        js_bam = json.load(fp)
    assert js["summary"] == js_bam["summary"] and js["base_quality_hist"] == js_bam["base_quality_hist"]
    n = len(case["lens"])
    assert js["counters"] == dict(n_records=n, n_reads=n, n_secondary=0, n_supplementary=0, n_unmapped=n, n_no_seq=0, n_no_qual=0, total_bases=sum(case["lens"]))


def test_filter_writes_the_kept_reads_and_prints_the_counters(case, tmp_path, capsys):
    out = str(tmp_path / "kept.fastq")
    assert CoRAL.main(["filter", "--fastq", case["fastq"], "--output", out, "--min_length", "100", "--max_length", "300", "--min_mean_quality", "29.5", "--device", "cpu",
                       "--chunk_bytes", "3000"]) == out
    printed = capsys.readouterr().out
    want = fc.expected(case["text"], (100, 300, 2950))
    keep = [100 <= n <= 300 and 100 * int(q.sum()) >= 2950 * n for n, q in zip(case["lens"], case["quals"])]
    assert want["kept"] == [int(k) for k in keep] and 0 < sum(keep) < len(keep)
    assert open(out, "rb").read() == want["output"]
    assert printed == "records: %d\nreads: %d\nbases: %d\nkept_records: %d\nkept_bases: %d\nWrote %s\n" % (
        len(keep), len(keep), sum(case["lens"]), sum(keep), sum(n for n, k in zip(case["lens"], keep) if k), out)
    CoRAL.main(["filter", "--fastq", case["fastq"], "--output", out, "--device", "cpu"])                 # no thresholds: the input byte for byte
    assert open(out, "rb").read() == case["text"]
    assert fastq.LAST_FASTQ_QC["write"] >= 0


def test_argument_rules(case, tmp_path):
    d = str(tmp_path / "o")
    for argv in (["qc", "--fastq", case["fastq"], "--lr_bam", case["bam"], "--output_dir", d, "--device", "cpu"],
                 ["qc", "--output_dir", d, "--device", "cpu"],
                 ["qc", "--fastq", case["fastq"], "--output_dir", d, "--device", "cpu", "--filter_min_mapq", "20"],
                 ["qc", "--fastq", case["fastq"], "--output_dir", d, "--device", "cpu", "--filter_exclude_flags", "0x4"],
                 ["filter", "--output", d],
                 ["filter", "--fastq", case["fastq"]]):
        with pytest.raises(SystemExit) as e:
            CoRAL.main(argv)
        assert e.value.code not in (0, None), argv
        assert not os.path.exists(d)
    with pytest.raises(ValueError):
        CoRAL.main(["filter", "--fastq", case["fastq"], "--output", d, "--min_length", "10", "--max_length", "5", "--device", "cpu"])
    assert not os.path.exists(d)
