"""Cost of the window-coverage request on the GPU decode (bam.window_coverage: k_bam_cov_plan + k_bam_cov_count per batch).

Writes a BAM of the 'cfg3_12k' records with real QUAL (the pure-Python writer), takes the amplified intervals of that data
set's graph (tests/golden/e2e_cfg3_12k.json) and the coverage track's windows over them, and times, median of `runs`:
  decode            decode_bam_gpu alone
  cov_t0 / cov_t20  window_coverage at quality threshold 0 and 20 (the same decode with the request riding along)
as wall time and as HIP-event time on the caller's stream, plus the SEQ + QUAL bytes the kernels can touch (records that
overlap a window, 1.5 B per base).  One JSON line.
    python tools/bench_window_coverage.py [runs] [--bam PATH] [--kernels-only]
--kernels-only: one decode with the request at threshold 20 and nothing else (the leg to run under rocprofv3)."""
import argparse
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

ap = argparse.ArgumentParser()
ap.add_argument("runs", nargs="?", type=int, default=5)
ap.add_argument("--bam", default="")
ap.add_argument("--kernels-only", action="store_true")
args = ap.parse_args()

d = tempfile.mkdtemp(prefix="coral_wcov_")
path = args.bam or os.path.join(d, "cfg3_12k_qual.bam")
_, rec = synth.dataset("cfg3_12k", "cpu")
if not os.path.exists(path):
    t0 = time.perf_counter()
    bam.write_bam(rec, path, seed=1, with_qual=True, fast_seq=True)
    print("BAM written: %.1f MB in %.1f s" % (os.path.getsize(path) / 1e6, time.perf_counter() - t0), file=sys.stderr, flush=True)
with open(os.path.join(ROOT, "tests", "golden", "e2e_cfg3_12k.json")) as fp:
    text = json.load(fp)["files"]["out_amplicon1_graph.txt"]
graph = os.path.join(d, "g_graph.txt")
with open(graph, "w") as fp:
    fp.write(text)
intervals = plot_coverage.parse_graph_intervals(graph)
windows = plot_coverage.plot_windows(intervals)
dev = "cuda:0"

if args.kernels_only:
    n = bam.window_coverage(path, windows, 20, "nofilter", device=dev)
    torch.cuda.synchronize()
    print(json.dumps({"windows": len(windows), "bases_t20": int(n.sum())}))
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


legs = {
    "decode": lambda: bam.decode_bam_gpu(path, dev),
    "cov_t0": lambda: bam.window_coverage(path, windows, 0, "nofilter", device=dev),
    "cov_t20": lambda: bam.window_coverage(path, windows, 20, "nofilter", device=dev),
}
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

# bytes the request can touch: SEQ + QUAL of the records with SEQ that overlap a window
tid, pos, end, qlen, hs = (getattr(rec, k).numpy().astype(np.int64) for k in ("tid", "pos", "end", "qlen", "has_seq"))
segs, _, _ = bam.coverage_segments(windows, rec.header_chroms)
hit = np.zeros(rec.n, dtype=bool)
for t, a, b in segs.T.astype(np.int64):
    hit |= (tid == t) & (pos < b) & (end > a)
seq_qual = int((((qlen + 1) // 2 + qlen) * (hs > 0) * hit).sum())
resident = plot_coverage.coverage_track(__import__("coral_amd.records", fromlist=["DeviceRecords"]).DeviceRecords(rec, dev), intervals)
assert [n for *_, n in resident] == outs["cov_t0"].tolist(), "threshold-0 track differs from the resident-records track"

med = {k: {m: round(statistics.median(v[m]), 4) for m in v} for k, v in res.items()}
line = {
    "tool": "bench_window_coverage", "data": "cfg3_12k", "records": rec.n, "bam_MB": round(os.path.getsize(path) / 1e6, 1),
    "windows": len(windows), "segments": int(segs.shape[1]), "runs": args.runs,
    "median": med,
    "overhead_vs_decode": {k: {m: round(med[k][m] / med["decode"][m] - 1, 4) for m in ("wall_s", "event_s")} for k in ("cov_t0", "cov_t20")},
    "seq_qual_bytes_touched": seq_qual, "records_in_windows": int(hit.sum()),
    "bases_t0": int(outs["cov_t0"].sum()), "bases_t20": int(outs["cov_t20"].sum()),
    "all_runs": res,
}
print(json.dumps(line))
import shutil
shutil.rmtree(d, ignore_errors=True)
