"""Per-read length and base-quality statistics counted during the BAM decode (bam.read_qc, the `qc` mode): both pipelines against
an INDEPENDENT restatement of the reference's scripts/report_nanopore_qc.py: restate_read_qc, which tests/test_bam_request.py
checks against as well and which therefore lives next to the reader in tests/bamfile.py, and restated_summary here.  The BAM is
read with gzip + struct in tests/bamfile.py, and the script's own formulas (len, np.mean of the quality values, np.percentile)
are applied to the primary records with SEQ — one per FASTQ record the file was aligned from.  (The script itself reads the
FASTQ through pysam.FastxFile, which cannot be run here: parity with it is not pinned)"""
import json
import os
import warnings

import numpy as np
import pytest

from coral_amd import bam, synth
from tests.bamfile import M, read_bam as _read_bam, restate_read_qc as restate
from tests.decode_support import (LONG_READ, assert_qc_equals_restatement as assert_equal, assert_same_qc as assert_same, assert_same_records,
                                  read_qc_case)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def read_bam(path):
    """(every record straight from the bytes, the length of the inflated stream)"""
    parsed = _read_bam(path)
    return parsed.recs, parsed.n_bytes


def restated_summary(want):
    ml, mq = want["mean_lengths"], want["mean_qualities"]
    out = {"length_Q%d" % q: float(np.percentile(ml, q)) for q in (25, 50, 75)}
    out.update({"quality_Q%d" % q: float(np.percentile(mq, q)) for q in (25, 50, 75)})
    out["mean_length"], out["mean_quality"] = float(np.mean(ml)), float(np.mean(mq))
    half, run = sum(ml) / 2, 0
    for ln in sorted(ml, reverse=True):                       # N50: the length at which the longest reads hold half the bases
        run += ln
        if run >= half:
            out["n50"] = ln
            break
    out["total_bases"] = sum(ml)
    return out


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return read_qc_case(tmp_path_factory.mktemp("readqc"))


def host(path, **kw):
    return bam.read_qc(path, device="cpu", **kw)


# ---- the restatement sees what was planted ---------------------------------------------------------------------------------------
def test_restatement_reads_the_planted_records(case):
    recs, want = case["recs"], case["want"]
    c = want["counters"]
    assert c["n_secondary"] >= 1 and c["n_supplementary"] >= 1 and c["n_unmapped"] >= 1 and c["n_no_seq"] >= 1
    assert 50 < c["n_no_qual"] < c["n_reads"] - 100 and c["n_reads"] < c["n_records"]
    assert {1, 15, 16, 17, 65, 77, LONG_READ} <= set(want["mean_lengths"])
    assert any(r["n_cig"] == 2 and r["l_seq"] == 88005 for r in recs)                 # the CG-tag record: placeholder CIGAR of 2 ops
    assert all(want["hist"][v] > 0 for v in (0, 93, 200, 254)) and want["hist"][255] == 0
    assert case["inflated_bytes"] > 2 * (1 << 20)                                     # several 1 MiB batches
    i = want["mean_lengths"].index(LONG_READ)
    assert want["qual_sum"][i] > 10_000_000


# ---- host pipeline ---------------------------------------------------------------------------------------------------------------
def test_host_pipeline_matches_the_restatement(case):
    got = host(case["path"], n_threads=3)
    assert_equal(got, case["want"])
    assert bam.LAST_DECODE["blocks"] > 0 and bam.LAST_DECODE["uncompressed_bytes"] > 0


def test_summary_is_bit_equal_to_the_scripts_floats(case):
    got, want = host(case["path"]).summary(), restated_summary(case["want"])
    assert set(got) == set(want)
    for k, v in want.items():
        assert type(got[k]) is type(v) and got[k] == v, k
    assert np.array_equal(host(case["path"]).mean_qualities(), np.array(case["want"]["mean_qualities"]))


def test_write_summary_is_what_pandas_writes(case, tmp_path):
    pd = pytest.importorskip("pandas")
    want = case["want"]
    ml, mq = want["mean_lengths"], want["mean_qualities"]
    frame = pd.DataFrame(columns=['Q25', 'Q50', 'Q75'])                                # the script's lines 70-74
    frame.loc['mean_length'] = [np.percentile(ml, 25), np.percentile(ml, 50), np.percentile(ml, 75)]
    frame.loc['mean_sequence_quality'] = [np.percentile(mq, 25), np.percentile(mq, 50), np.percentile(mq, 75)]
    ref = str(tmp_path / "pandas.tsv")
    frame.to_csv(ref, sep='\t')
    out = host(case["path"]).write_summary(str(tmp_path / "quality_control_summary.tsv"))
    assert open(out, "rb").read() == open(ref, "rb").read()


def test_write_summary_literal(tmp_path):
    qc = bam.ReadQC([10, 20, 30, 40], [100, 400, -1, 1200], [60] * 4, [0, 16, 0, 4], np.zeros(256, dtype=np.int64),
                    dict(n_records=4, n_reads=4, n_secondary=0, n_supplementary=0, n_unmapped=1, n_no_seq=0, n_no_qual=1, total_bases=100))
    out = qc.write_summary(str(tmp_path / "s.tsv"))
    assert open(out, "rb").read() == b"\tQ25\tQ50\tQ75\nmean_length\t17.5\t25.0\t32.5\nmean_sequence_quality\t15.0\t20.0\t25.0\n"
    s = qc.summary()
    assert s["n50"] == 30 and s["total_bases"] == 100 and s["mean_length"] == 25.0 and s["mean_quality"] == 20.0


def test_host_pipeline_ranges_merge_to_the_whole(case):
    whole = host(case["path"], n_threads=2)
    for path in (case["path"], case["small"]):
        parts = [host(path, n_threads=2, rank=r, world=3) for r in range(3)]
        assert sum(p.n_records > 0 for p in parts) >= 2
        assert_same(bam.merge_read_qc(parts), whole, path)
    assert_equal(bam.merge_read_qc([host(case["small"], rank=r, world=3) for r in range(3)]), case["want"])


def test_host_pipeline_small_blocks_and_empty_blocks(case):
    assert_equal(host(case["small"], n_threads=2), case["want"])


def test_qc_command_line(case, tmp_path, capsys):
    from coral_amd import CoRAL
    d = str(tmp_path / "out")
    wrote = CoRAL.main(["qc", "--lr_bam", case["path"], "--output_dir", d, "--device", "cpu"])
    printed = capsys.readouterr().out
    want = {"quality_control_summary.tsv", "read_qc.json"}
    try:
        import matplotlib  # noqa: F401
        want |= {"mean_length_histogram.png", "mean_sequence_quality_histogram.png"}
    except ImportError:
        pass
    assert set(os.listdir(d)) == want and {os.path.basename(w) for w in wrote} == want
    assert all(("Wrote %s" % w) in printed for w in wrote)
    with open(os.path.join(d, "read_qc.json")) as fp:
        js = json.load(fp)
    assert js["counters"] == case["want"]["counters"] and js["base_quality_hist"] == case["want"]["hist"].tolist()
    assert js["summary"] == restated_summary(case["want"])
    assert open(os.path.join(d, "quality_control_summary.tsv")).read() == host(case["path"]).summary_text()
    d2 = str(tmp_path / "out2")
    CoRAL.main(["qc", "--lr_bam", case["path"], "--output_dir", d2, "--device", "cpu", "--no_plots"])
    assert set(os.listdir(d2)) == {"quality_control_summary.tsv", "read_qc.json"}


def test_file_without_reads(case):
    recs, _ = read_bam(case["none"])
    got = host(case["none"])
    assert_equal(got, restate(recs))
    assert len(got.length) == 0 and got.n_reads == 0 and got.n_records == 3 and got.base_quality_hist.sum() == 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(ValueError, match="no read"):
            got.summary()
        with pytest.raises(ValueError, match="no read"):
            got.write_summary(os.devnull)


def test_write_bam_qual_option_checks_the_length(tmp_path):
    rec = synth.records_from_alignments([dict(tid=7, pos=100, cigar=[(M, 50)], name="a")])
    with pytest.raises(ValueError):
        bam.write_bam(rec, str(tmp_path / "x.bam"), qual=lambda i: b"\x01" * 49)


# ---- GPU pipeline ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_pipeline_matches_host_and_restatement(case):
    h = host(case["path"], n_threads=2)
    assert_equal(h, case["want"], "host")
    for path in (case["path"], case["small"]):
        for batch in (0, 1 << 20):                # 1 MiB batches: the 300 000-base read and others straddle them
            got = bam.read_qc(path, device="cuda:0", batch_bytes=batch)
            assert_equal(got, case["want"], (path, batch))
            assert_same(got, h, (path, batch))
            assert bam.LAST_DECODE["where"] == "gpu" and (batch == 0 or bam.LAST_DECODE["batches"] >= 3)
    assert_equal(bam.read_qc(case["none"], device="cuda:0"), restate(read_bam(case["none"])[0]))


@pytest.mark.gpu
def test_gpu_pipeline_ranges_merge_to_the_whole(case):
    for path, batch in ((case["path"], 0), (case["small"], 1 << 20)):
        parts = [bam.read_qc(path, device="cuda:0", rank=r, world=3, batch_bytes=batch) for r in range(3)]
        assert_equal(bam.merge_read_qc(parts), case["want"], path)


@pytest.mark.gpu
def test_gpu_request_leaves_the_records_alone(case):
    plain = bam.decode_bam_gpu(case["small"], "cuda:0", batch_bytes=1 << 20)
    got = bam._decode(case["small"], "cuda:0", batch_bytes=1 << 20, qc=True)
    assert_same_records(got.records, plain)
    assert_equal(got.qc, case["want"])
    assert bam._decode(case["small"], "cuda:0", batch_bytes=1 << 20).qc is None


@pytest.mark.gpu
def test_gpu_three_requests_at_once(case):
    rec = case["rec"]
    windows = [("chr8", 149_000, 152_000), ("chr8", 150_000, 150_100), ("chr8", 0, 1 << 28)]
    segs, first, last = bam.coverage_segments(windows, rec.header_chroms)
    for batch in (0, 1 << 20):
        alone_cov = bam._decode(case["path"], "cuda:0", batch_bytes=batch, coverage=(segs, 20, 0), records=False).counts
        alone_idx = bam._decode(case["path"], "cuda:0", batch_bytes=batch, records=False, index=True).index
        plain = bam.decode_bam_gpu(case["path"], "cuda:0", batch_bytes=batch)
        got_rec, cov, idx, qc = bam._decode(case["path"], "cuda:0", batch_bytes=batch, coverage=(segs, 20, 0), index=True, qc=True)
        assert alone_cov.sum() > 0 and np.array_equal(cov, alone_cov)
        assert set(idx) == set(alone_idx)
        for k, v in alone_idx.items():
            assert np.array_equal(idx[k], v), k
        assert_same_records(got_rec, plain)
        assert_equal(qc, case["want"], batch)
