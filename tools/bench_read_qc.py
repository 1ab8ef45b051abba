"""Cost of the read-QC request on the GPU decode (bam.read_qc: k_bam_qc_plan + k_bam_qc per batch).

Writes a BAM of the 'cfg3_12k' records with real QUAL (the pure-Python writer; the file tools/bench_window_coverage.py uses) and
times, median of `runs`:
  decode    decode_bam_gpu alone (no request: nothing is launched, nothing more allocated)
  qc        read_qc (the same decode with the request riding along, records not materialised)
as wall time and as HIP-event time on the caller's stream, plus the QUAL bytes k_bam_qc reads.  One JSON line.
    python tools/bench_read_qc.py [runs] [--bam PATH] [--peaked-qual] [--kernels-only] [--decode-only] [--stats-csv PATH]
--peaked-qual:  QUAL drawn from eight values, 70 % of the bytes on two of them (what a real basecaller's QUAL looks like to the
                histogram), instead of write_bam's even 0..60: the file that tells the histogram layouts apart.
--kernels-only: one decode with the request and nothing else (the leg to run under rocprofv3 --kernel-trace --stats).
--decode-only:  only the `decode` leg (runs on a checkout without the request: the yardstick for "no request costs nothing").
--stats-csv:    a rocprofv3 kernel_stats CSV of the --kernels-only leg: k_bam_qc's own time goes into the line."""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from coral_amd import bam, synth

ap = argparse.ArgumentParser()
ap.add_argument("runs", nargs="?", type=int, default=7)
ap.add_argument("--bam", default="")
ap.add_argument("--peaked-qual", action="store_true")
ap.add_argument("--kernels-only", action="store_true")
ap.add_argument("--decode-only", action="store_true")
ap.add_argument("--stats-csv", default="")
args = ap.parse_args()

d = tempfile.mkdtemp(prefix="coral_readqc_")
path = args.bam or os.path.join(d, "cfg3_12k_qual.bam")
_, rec = synth.dataset("cfg3_12k", "cpu")
PEAK_VALUES = np.array([40, 38, 30, 22, 14, 8, 4, 50], dtype=np.uint8)
PEAK_WEIGHTS = [0.40, 0.30, 0.10, 0.07, 0.05, 0.04, 0.03, 0.01]
if not os.path.exists(path):
    t0 = time.perf_counter()
    qlen = rec.qlen.cpu().numpy()
    peaked = (lambda i: PEAK_VALUES[np.random.default_rng(i).choice(8, int(qlen[i]), p=PEAK_WEIGHTS)].tobytes()) if args.peaked_qual else None
    bam.write_bam(rec, path, seed=1, with_qual=True, fast_seq=True, qual=peaked)
    print("BAM written: %.1f MB in %.1f s" % (os.path.getsize(path) / 1e6, time.perf_counter() - t0), file=sys.stderr, flush=True)
dev = "cuda:0"

if args.kernels_only:
    qc = bam.read_qc(path, device=dev)
    torch.cuda.synchronize()
    print(json.dumps({"reads": qc.n_reads, "qual_bytes": int(qc.base_quality_hist.sum())}))
    sys.exit(0)


def timed(fn):
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(s)
    out = fn()
    e1.record(s)
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0, e0.elapsed_time(e1) / 1e3


legs = {"decode": lambda: bam.decode_bam_gpu(path, dev)}
if not args.decode_only:
    legs["qc"] = lambda: bam.read_qc(path, device=dev)
res = {k: {"wall_s": [], "event_s": []} for k in legs}
qc = None
timed(legs["decode"])                                   # warm-up: code objects, pinned buffers, caching allocator
for r in range(args.runs):
    for k, fn in legs.items():                          # interleaved, so that drift hits every leg alike
        o, w, e = timed(fn)
        res[k]["wall_s"].append(w)
        res[k]["event_s"].append(e)
        if k == "qc":
            qc = o
        del o

med = {k: {m: round(statistics.median(v[m]), 4) for m in v} for k, v in res.items()}
spread = {k: {m: [round(min(v[m]), 4), round(max(v[m]), 4)] for m in v} for k, v in res.items()}
line = {"tool": "bench_read_qc", "data": "cfg3_12k", "qual": "peaked" if args.peaked_qual else "even 0..60", "records": rec.n, "bam_MB": round(os.path.getsize(path) / 1e6, 1), "runs": args.runs,
        "median": med, "min_max": spread, "all_runs": res}
if qc is not None:
    host = bam.read_qc(path, device="cpu")
    same = all(np.array_equal(getattr(qc, k), getattr(host, k)) for k in ("length", "qual_sum", "mapq", "flag", "base_quality_hist"))
    assert same and qc.counters == host.counters, "the GPU result differs from the host pipeline's"
    line["overhead_vs_decode"] = {m: round(med["qc"][m] / med["decode"][m] - 1, 4) for m in ("wall_s", "event_s")}
    line["reads"], line["qual_bytes_read"] = qc.n_reads, int(qc.base_quality_hist.sum())
    line["inflated_bytes"] = int(bam.LAST_DECODE.get("uncompressed_bytes", 0))
    line["summary"] = qc.summary()
if args.stats_csv:
    with open(args.stats_csv) as fp:
        rows = [r for r in csv.DictReader(fp) if "k_bam_qc" in r.get("Name", "")]
    line["kernel_stats"] = {("k_bam_qc_plan" if "plan" in r["Name"] else "k_bam_qc"): {"calls": int(r["Calls"]), "total_us": round(float(r["TotalDurationNs"]) / 1e3, 1)}
                            for r in rows}
    t = line["kernel_stats"].get("k_bam_qc", {}).get("total_us")
    if t and "qual_bytes_read" in line:
        line["k_bam_qc_GBps"] = round(line["qual_bytes_read"] / t / 1e3, 1)
print(json.dumps(line))
import shutil
shutil.rmtree(d, ignore_errors=True)
