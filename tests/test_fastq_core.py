"""The host backend of the FASTQ session (coral_fastq_host.h behind coral_fastq_*, `device="cpu"` of coral_amd/fastq.py) against the
plain-Python restatement of tests/fastq_cases.py: rows, histogram, counters, kept flags, the output's bytes, return code and
offset, whatever the cuts; the filter at its thresholds; the summary against the reference's scripts/report_nanopore_qc.py:38-48
and 70-74 restated with numpy."""
import os

import numpy as np
import pytest

from coral_amd import fastq
from tests import fastq_cases as fc


def feedings(data):
    yield "whole", fc.cut(data, "whole")
    yield "bytes", fc.cut(data, "bytes")
    for seed in (1, 2):
        yield "random%d" % seed, fc.cut(data, "random", seed)


@pytest.mark.parametrize("name", sorted(fc.cases()))
def test_host_backend_equals_the_restatement(name):
    data = fc.cases()[name]
    want = fc.expected(data)
    assert want["rc"] == 0 and want["output"] == data                # no thresholds: the input byte for byte
    for how, pieces in feedings(data):
        fc.assert_same(fc.run_session(pieces), want, (name, how))


def test_the_cases_hold_what_they_are_named_for():
    want = {k: fc.expected(v) for k, v in fc.cases().items()}
    assert want["empty_stream"]["records"] == 0 and want["empty_stream"]["hist"] == [0] * 256
    assert want["one_long_read"]["length"] == [3, 300_000, 2]
    assert want["many_short_reads"]["records"] == 5000 and set(want["many_short_reads"]["length"]) == set(range(1, 7)) and want["many_short_reads"]["no_seq"] > 500
    assert want["empty_sequence_in_the_middle"]["no_seq"] == 1 and want["empty_sequence_at_the_end"]["no_seq"] == 1
    assert want["empty_sequence_at_the_end"]["records"] == want["empty_sequence_at_the_end_with_quality_line"]["records"] == 2
    assert want["quality_extremes"]["qual_sum"] == [0, 5 * 93, 93 + 40] and want["quality_extremes"]["hist"][93] == 6
    assert want["crlf"]["length"] == want["unix"]["length"] == [5, 17, 1, 64, 33]
    assert want["no_trailing_newline"]["length"] == want["no_trailing_newline_crlf"]["length"] == [12, 7]


@pytest.mark.parametrize("name", sorted(fc.refused()))
def test_refusals_with_their_offsets(name):
    data, offset = fc.refused()[name]
    want = fc.expected(data)
    assert (want["rc"], want["offset"]) == (fc.FORMAT, offset)       # the restatement agrees with the literal offset
    for how, pieces in feedings(data):
        got = fc.run_session(pieces)
        assert (got["rc"], got["offset"]) == (fc.FORMAT, offset), (name, how, got)
    # and behind a few good records, so that the offset is the stream's, not the piece's
    front = fc.cases()["unix"]
    for how, pieces in feedings(front + data):
        got = fc.run_session(pieces)
        assert (got["rc"], got["offset"]) == (fc.FORMAT, len(front) + offset), (name, how, got)


def threshold_text():
    """Reads at threshold - 1, at the threshold and at threshold + 1: lengths 9, 10, 11 around a length threshold of 10, and reads
    of 10 bases whose quality sums are 204, 205 and 206 around a mean of 20.50 (100 * 205 == 2050 * 10)."""
    def with_sum(n, total):
        q = [total // n] * n
        for i in range(total - sum(q)):
            q[i] += 1
        assert sum(q) == total
        return bytes(v + 33 for v in q)
    out = b""
    for k, n in enumerate((9, 10, 11)):
        out += fc.record(b"len%d" % n, b"ACGTACGTACG"[:n], with_sum(n, 30 * n))
    for total in (204, 205, 206):
        out += fc.record(b"sum%d" % total, b"ACGTACGTAC", with_sum(10, total), b"\r\n")
    out += b"@none\n\n+\n\n"
    return out


def test_the_filter_at_its_thresholds():
    data = threshold_text()
    names = [b"len9", b"len10", b"len11", b"sum204", b"sum205", b"sum206", b"none"]
    for thresholds, kept in (((0, 0, 0), names),
                             ((10, 0, 0), [b"len10", b"len11", b"sum204", b"sum205", b"sum206"]),
                             ((0, 10, 0), [b"len9", b"len10", b"sum204", b"sum205", b"sum206", b"none"]),
                             ((0, 0, 2050), [b"len9", b"len10", b"len11", b"sum205", b"sum206", b"none"]),
                             ((10, 10, 2050), [b"len10", b"sum205", b"sum206"]),
                             ((11, 0, 3000), [b"len11"]),
                             ((0, 0, 3001), [b"none"])):
        want = fc.expected(data, thresholds)
        assert [r.split()[0][1:] for r in want["output"].split(b"\n") if r.startswith(b"@")] == kept, thresholds      # (no quality line here starts with '@')
        assert want["n_kept"] == len(kept)
        for how, pieces in feedings(data):
            fc.assert_same(fc.run_session(pieces, thresholds), want, (thresholds, how))
    assert fc.expected(data)["output"] == data


def test_the_filter_on_the_cases_does_not_depend_on_the_cuts():
    for name in ("crlf", "no_trailing_newline", "empty_sequence_at_the_end", "many_short_reads", "one_long_read"):
        data = fc.cases()[name]
        for thresholds in ((3, 0, 0), (2, 5, 4000), (0, 0, 4650)):
            want = fc.expected(data, thresholds)
            for how, pieces in (("whole", fc.cut(data, "whole")), ("random", fc.cut(data, "random", 5))):
                fc.assert_same(fc.run_session(pieces, thresholds), want, (name, thresholds, how))
    data = fc.cases()["many_short_reads"]
    assert 0 < fc.expected(data, (2, 5, 4000))["n_kept"] < 5000
    got = fc.run_session([data], (2, 5, 4000), output=False)                     # and without an output: the same rows
    assert got["kept"] == fc.expected(data, (2, 5, 4000))["kept"] and got["output"] == b""


def restated_summary_text(data):
    """The script's lines 38-48 and 70-74 on the same lists, formatted as ``bam.ReadQC.summary_text`` words pandas' ``to_csv``."""
    lengths, quals = fc.quality_lists(data)
    mean_lengths = [n for n in lengths]                                          # len(sequence)
    mean_qualities = [np.mean(np.array(q)) for q in quals]                       # np.mean(quality)
    row = lambda name, values: "\t".join([name] + [repr(float(np.percentile(values, q))) for q in (25, 50, 75)]) + "\n"
    return "\tQ25\tQ50\tQ75\n" + row("mean_length", mean_lengths) + row("mean_sequence_quality", mean_qualities)


def test_the_summary_is_the_scripts(tmp_path):
    for name in ("unix", "crlf", "many_short_reads", "empty_sequence_in_the_middle"):
        data = fc.cases()[name]
        path = str(tmp_path / (name + ".fastq"))
        with open(path, "wb") as fp:
            fp.write(data)
        qc = fastq.read_qc(path, device="cpu", chunk_bytes=4096)
        want = fc.expected(data)
        assert qc.summary_text() == restated_summary_text(data), name
        assert qc.length.tolist() == want["length"] and qc.qual_sum.tolist() == want["qual_sum"] and qc.base_quality_hist.tolist() == want["hist"]
        assert qc.counters == dict(n_records=want["records"], n_reads=want["reads"], n_secondary=0, n_supplementary=0, n_unmapped=want["reads"], n_no_seq=want["no_seq"],
                                   n_no_qual=0, total_bases=want["bases"])
        assert set(qc.mapq.tolist()) <= {255} and set(qc.flag.tolist()) <= {4} and qc.kept.tolist() == want["kept"]
        assert (qc.n_kept, qc.kept_bases) == (want["records"], want["bases"])
        assert fastq.LAST_FASTQ_QC["wall"] > 0 and "write" in fastq.LAST_FASTQ_QC
        with open(path, "rb") as fp:                                             # an open file, and the parts merge as the BAM's do
            again = fastq.read_qc(fp, device="cpu")
        assert again.summary_text() == qc.summary_text()
    from coral_amd import bam
    both = bam.merge_read_qc([qc, qc])
    assert both.n_records == 2 * qc.n_records and both.length.tolist() == 2 * qc.length.tolist()


def test_read_qc_writes_the_kept_records_and_reads_gz(tmp_path):
    import gzip
    data = fc.cases()["many_short_reads"]
    path, gz = str(tmp_path / "in.fastq"), str(tmp_path / "in.fastq.gz")
    with open(path, "wb") as fp:
        fp.write(data)
    with gzip.open(gz, "wb") as fp:
        fp.write(data)
    want = fc.expected(data, (3, 0, 4512))
    for k, src in enumerate((path, gz)):
        out = str(tmp_path / ("out%d.fastq" % k))
        qc = fastq.read_qc(src, device="cpu", chunk_bytes=1000, min_length=3, min_mean_quality=45.12, output=out)
        assert open(out, "rb").read() == want["output"] and qc.kept.tolist() == want["kept"] and (qc.n_kept, qc.kept_bases) == (want["n_kept"], want["kept_bases"])
    with open(str(tmp_path / "out.bin"), "wb") as fp:                            # an open file as the output: written behind what it holds
        fp.write(b"head\n")
        fastq.read_qc(path, device="cpu", output=fp)
    assert open(str(tmp_path / "out.bin"), "rb").read() == b"head\n" + data
    with pytest.raises(Exception, match="byte 11"):
        bad = str(tmp_path / "bad.fastq")
        with open(bad, "wb") as fp:
            fp.write(fc.refused()["blank_line_between_records"][0])
        fastq.read_qc(bad, device="cpu")


def test_argument_errors_come_before_any_work(tmp_path):
    out = str(tmp_path / "never.fastq")
    missing = str(tmp_path / "missing.fastq")                                    # (not opened: the arguments are checked first)
    for kw in (dict(min_length=-1), dict(max_length=-1), dict(min_mean_quality=-0.5), dict(min_length=10, max_length=9), dict(chunk_bytes=fastq.min_staging() - 1),
               dict(min_length=1.5), dict(min_mean_quality=93.5), dict(min_length=1 << 31)):
        with pytest.raises(ValueError):
            fastq.read_qc(missing, device="cpu", output=out, **kw)
        assert not os.path.exists(out)
    assert fastq.min_staging() == 16
