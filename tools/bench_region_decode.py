"""Cost of the BAI index request on the GPU decode, and what a region decode through the index saves (bam.build_index,
bam.window_coverage(index=...)).

Writes a BAM of the 'cfg3_12k' records with real QUAL (as tools/bench_window_coverage.py), builds its index, takes the coverage
track's windows of that data set's first amplicon, and times, median of `runs`, as wall time and as HIP-event time:
  decode         decode_bam_gpu alone (no request: the kernels of the decode as before)
  decode_index   the same decode with the index request riding along (bam.index_partial: k_bam_index per batch)
  cov_whole      window_coverage(index=False): the whole file is inflated
  cov_region     window_coverage through the index: only the blocks it names
plus the blocks read by the last two, and whether the index bytes are the same for three batch sizes.  One JSON line.
    python tools/bench_region_decode.py [runs] [--bam PATH] [--kernels-only]
--kernels-only: one decode with the index request and nothing else (the leg to run under rocprofv3)."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from coral_amd import bam, plot_coverage, synth

ap = argparse.ArgumentParser()
ap.add_argument("runs", nargs="?", type=int, default=7)
ap.add_argument("--bam", default="")
ap.add_argument("--kernels-only", action="store_true")
args = ap.parse_args()

d = tempfile.mkdtemp(prefix="coral_region_")
path = args.bam or os.path.join(d, "cfg3_12k_qual.bam")
_, rec = synth.dataset("cfg3_12k", "cpu")
if not os.path.exists(path):
    t0 = time.perf_counter()
    bam.write_bam(rec, path, seed=1, with_qual=True, fast_seq=True)
    print("BAM written: %.1f MB in %.1f s" % (os.path.getsize(path) / 1e6, time.perf_counter() - t0), file=sys.stderr, flush=True)
dev = "cuda:0"

if args.kernels_only:
    p = bam.index_partial(path, dev)
    torch.cuda.synchronize()
    print(json.dumps({"records": p["n_records"], "heads": int(len(p["head_key"]))}))
    sys.exit(0)

with open(os.path.join(ROOT, "tests", "golden", "e2e_cfg3_12k.json")) as fp:
    text = json.load(fp)["files"]["out_amplicon1_graph.txt"]
graph = os.path.join(d, "g_graph.txt")
with open(graph, "w") as fp:
    fp.write(text)
windows = plot_coverage.plot_windows(plot_coverage.parse_graph_intervals(graph))
index_path = os.path.join(d, "bench.bai")


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


def index_file(batch_bytes):
    with open(bam.build_index(path, index_path, device=dev, batch_bytes=batch_bytes), "rb") as fp:
        return fp.read()


sizes = {"default": 0, "64MiB": 64 << 20, "16MiB": 16 << 20}
files = {k: index_file(v) for k, v in sizes.items()}
host_file = None
if os.environ.get("CORAL_BENCH_HOST_INDEX"):                 # the host pipeline's bytes as well (slow on a large file)
    with open(bam.build_index(path, index_path + ".host", device="cpu"), "rb") as fp:
        host_file = fp.read()
index_file(0)
# host share of build_index behind the decode: joining the partial index, the stable sort of the run heads, the file's bytes
part = bam.index_partial(path, dev)
t0 = time.perf_counter()
bam.index_bytes(bam.merge_index_partials([part]), rec.header_lens)
host_write_s = time.perf_counter() - t0
idx = bam.read_index(index_path)
blocks = {}


def leg_cov(index):
    def run():
        out = bam.window_coverage(path, windows, 20, "nofilter", device=dev, index=index)
        blocks["cov_region" if index is not False else "cov_whole"] = bam.LAST_DECODE["blocks"]
        return out
    return run


legs = {
    "decode": lambda: bam.decode_bam_gpu(path, dev),
    "decode_index": lambda: bam.index_partial(path, dev),
    "cov_whole": leg_cov(False),
    "cov_region": leg_cov(idx),
}
res = {k: {"wall_s": [], "event_s": []} for k in legs}
outs = {}
timed(legs["decode"])                                   # warm-up: code objects, pinned buffers, caching allocator
for r in range(args.runs):
    for k, fn in legs.items():                          # interleaved, so that drift hits every leg alike
        o, w, e = timed(fn)
        res[k]["wall_s"].append(w)
        res[k]["event_s"].append(e)
        if k.startswith("cov"):
            outs[k] = o
        del o
assert outs["cov_whole"].tolist() == outs["cov_region"].tolist(), "the region decode counts differ from the whole-file decode's"

med = {k: {m: round(statistics.median(v[m]), 4) for m in v} for k, v in res.items()}
line = {
    "tool": "bench_region_decode", "data": "cfg3_12k", "records": rec.n, "bam_MB": round(os.path.getsize(path) / 1e6, 1),
    "windows": len(windows), "runs": args.runs, "index_bytes": len(files["default"]),
    "index_identical_across_batch_sizes": len(set(files.values())) == 1,
    "run_heads": int(len(part["head_key"])), "host_sort_and_write_s": round(host_write_s, 4),
    "index_identical_to_host_pipeline": None if host_file is None else host_file == files["default"],
    "median": med,
    "index_overhead_vs_decode": {m: round(med["decode_index"][m] / med["decode"][m] - 1, 4) for m in ("wall_s", "event_s")},
    "region_vs_whole": {m: round(med["cov_region"][m] / med["cov_whole"][m], 4) for m in ("wall_s", "event_s")},
    "blocks_whole": blocks["cov_whole"], "blocks_region": blocks["cov_region"],
    "share_of_blocks_read": round(blocks["cov_region"] / max(blocks["cov_whole"], 1), 4),
    "all_runs": res,
}
print(json.dumps(line))
shutil.rmtree(d, ignore_errors=True)
