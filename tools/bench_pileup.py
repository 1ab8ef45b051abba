"""Cost of the pileup request on the GPU decode (bam.pileup: k_bam_cov_plan + k_bam_pileup per batch).

Writes a BAM of the 'cfg3_12k' records with real QUAL (the pure-Python writer; the file tools/bench_read_qc.py and
tools/bench_window_coverage.py use), takes the amplified intervals of that data set's graph (tests/golden/e2e_cfg3_12k.json) as
regions and times, median of `runs`:
  decode    decode_bam_gpu alone (no request: nothing is launched, nothing more allocated)
  cov       window_coverage over the same regions (k_bam_cov_count: one 64-bit atomic per work item and segment)
  pileup    pileup of the regions (k_bam_pileup: one 32-bit atomic per counted base)
as wall time and as HIP-event time on the caller's stream, plus the counted bases (= atomics).  One JSON line.
    python tools/bench_pileup.py [runs] [--bam PATH] [--hot] [--kernels-only] [--decode-only] [--stats-csv PATH]
--hot:          instead, a file of `HOT_READS` reads of 10 kb that all cross one region of 300 bases: the ecDNA case, the worst
                case for contention on the table.
--kernels-only: one decode with the pileup request and nothing else (the leg to run under rocprofv3 --kernel-trace --stats).
--decode-only:  only the `decode` leg (runs on a checkout without the request: the yardstick for "no request costs nothing").
--stats-csv:    a rocprofv3 kernel_stats CSV of the --kernels-only leg: the kernels' own times go into the line."""
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

from coral_amd import bam, plot_coverage, synth

HOT_READS, HOT_READ_LEN, HOT_AT, HOT_LEN = 6000, 10_000, 1_000_000, 300

ap = argparse.ArgumentParser()
ap.add_argument("runs", nargs="?", type=int, default=5)
ap.add_argument("--bam", default="")
ap.add_argument("--hot", action="store_true")
ap.add_argument("--kernels-only", action="store_true")
ap.add_argument("--decode-only", action="store_true")
ap.add_argument("--stats-csv", default="")
args = ap.parse_args()

d = tempfile.mkdtemp(prefix="coral_pileup_")
if args.hot:
    path = args.bam or os.path.join(d, "hot_spot_qual.bam")
    starts = HOT_AT + HOT_LEN - HOT_READ_LEN + (np.arange(HOT_READS) * (HOT_READ_LEN - HOT_LEN)) // HOT_READS
    rec = synth.records_from_alignments([dict(tid=7, pos=int(s), cigar=[(0, HOT_READ_LEN)], name="h%d" % k) for k, s in enumerate(starts)])
    regions = [("chr8", HOT_AT, HOT_AT + HOT_LEN)]
else:
    path = args.bam or os.path.join(d, "cfg3_12k_qual.bam")
    _, rec = synth.dataset("cfg3_12k", "cpu")
    with open(os.path.join(ROOT, "tests", "golden", "e2e_cfg3_12k.json")) as fp:
        text = json.load(fp)["files"]["out_amplicon1_graph.txt"]
    graph = os.path.join(d, "g_graph.txt")
    with open(graph, "w") as fp:
        fp.write(text)
    regions = [(c, a, b + 1) for c, ivs in plot_coverage.parse_graph_intervals(graph).items() for a, b in ivs]
if not os.path.exists(path):
    t0 = time.perf_counter()
    bam.write_bam(rec, path, seed=1, with_qual=True, fast_seq=True)
    print("BAM written: %.1f MB in %.1f s" % (os.path.getsize(path) / 1e6, time.perf_counter() - t0), file=sys.stderr, flush=True)
dev = "cuda:0"

if args.kernels_only:
    p = bam.pileup(path, regions, 20, "nofilter", device=dev, index=False)
    torch.cuda.synchronize()
    print(json.dumps({"positions": len(p.table), "atomics": int(p.table.sum(dtype=np.int64)), "batches": bam.LAST_DECODE["batches"]}))
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
    legs["cov"] = lambda: bam.window_coverage(path, regions, 20, "nofilter", device=dev, index=False)
    legs["pileup"] = lambda: bam.pileup(path, regions, 20, "nofilter", device=dev, index=False)
res = {k: {"wall_s": [], "event_s": []} for k in legs}
outs = {}
timed(legs["decode"])                                   # warm-up: code objects, pinned buffers, caching allocator
for r in range(args.runs):
    for k, fn in legs.items():                          # interleaved, so that drift hits every leg alike
        o, w, e = timed(fn)
        res[k]["wall_s"].append(w)
        res[k]["event_s"].append(e)
        if k != "decode":
            outs[k] = o
        del o

med = {k: {m: round(statistics.median(v[m]), 4) for m in v} for k, v in res.items()}
spread = {k: {m: [round(min(v[m]), 4), round(max(v[m]), 4)] for m in v} for k, v in res.items()}
line = {"tool": "bench_pileup", "data": "hot spot: %d reads of %d bases over %d positions" % (HOT_READS, HOT_READ_LEN, HOT_LEN) if args.hot else "cfg3_12k",
        "records": rec.n, "bam_MB": round(os.path.getsize(path) / 1e6, 1), "regions": len(regions), "runs": args.runs, "median": med, "min_max": spread,
        "all_runs": res}
if "pileup" in outs:
    p = outs["pileup"]
    host = bam.pileup(path, regions, 20, "nofilter", device="cpu", index=False)
    assert p.regions == host.regions and np.array_equal(p.table, host.table), "the GPU table differs from the host pipeline's"
    assert [int(p.depth(*r).sum()) for r in regions] == outs["cov"].tolist(), "the table's sums differ from window_coverage"
    line["overhead_vs_decode"] = {k: {m: round(med[k][m] / med["decode"][m] - 1, 4) for m in ("wall_s", "event_s")} for k in ("cov", "pileup")}
    line["positions"], line["atomics"] = len(p.table), int(p.table.sum(dtype=np.int64))
    line["max_depth"] = int(p.table.sum(axis=1).max()) if len(p.table) else 0
if args.stats_csv:
    with open(args.stats_csv) as fp:
        rows = {r["Name"].split("(")[0].split("<")[0]: r for r in csv.DictReader(fp)}
    line["kernel_stats"] = {k: {"calls": int(r["Calls"]), "total_us": round(float(r["TotalDurationNs"]) / 1e3, 1)}
                            for k, r in rows.items() if k in ("k_bam_pileup", "k_bam_cov_plan", "k_bgzf_inflate", "k_bgzf_crc")}
    t = line["kernel_stats"].get("k_bam_pileup", {}).get("total_us")
    if t and "atomics" in line:
        line["k_bam_pileup_Gatomics_per_s"] = round(line["atomics"] / t / 1e3, 2)
print(json.dumps(line))
import shutil
shutil.rmtree(d, ignore_errors=True)
