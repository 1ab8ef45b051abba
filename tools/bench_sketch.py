"""Cost of the minimizer sketch (minimizers.sketch_reference: k_sketch_* of coral_sketch.hip and the radix sort) next to the k-mer
counter's (kmers.count_kmers) on the same file: both sessions stream the same bytes through the same staging, so the counter is the
yardstick.

Runs on the synthetic genome of tools/bench_kmers.py (`python tools/bench_kmers.py 1 --bases N --host_runs 0 --keep FILE` writes
it; none is shipped and none is fetched).  After one warm-up of each, `runs` alternating pairs: count_kmers, then sketch_reference.
Reports the medians of the wall times, the sketch's own stage times (minimizers.LAST_SKETCH: reading the file, the feed calls, and
from HIP events the uploads, symbols + contig table, the sketch kernels; the sort), minimizers per second and the density; with
`--host_runs` the host backend's time on the same file (one thread, O(n w); a reference, not the code under test) and a check
that both give the same arrays.  One JSON line.
    python tools/bench_sketch.py FILE [runs] [--k K] [--w W] [--host_runs N] [--chunk_bytes N]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from coral_amd import kmers, minimizers

ap = argparse.ArgumentParser()
ap.add_argument("fasta")
ap.add_argument("runs", nargs="?", type=int, default=5)
ap.add_argument("--k", type=int, default=15)
ap.add_argument("--w", type=int, default=50)
ap.add_argument("--host_runs", type=int, default=0)
ap.add_argument("--chunk_bytes", type=int, default=64 << 20)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_sketch.py measures on a GPU"
dev = "cuda:0"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def count():
    kc, s = timed(lambda: kmers.count_kmers(args.fasta, args.k, device=dev, chunk_bytes=args.chunk_bytes))
    stage = dict(kmers.LAST_COUNT)
    kc.close()
    return s, stage


def sketch():
    idx, s = timed(lambda: minimizers.sketch_reference(args.fasta, args.k, args.w, device=dev, chunk_bytes=args.chunk_bytes))
    return s, dict(minimizers.LAST_SKETCH), idx


count()                                                              # warm-up: code objects, the page cache, the allocator
sketch()[2].close()
count_wall, count_stage, sketch_wall, sketch_stage, idx = [], [], [], [], None
for run in range(args.runs):
    s, stage = count()
    count_wall.append(s)
    count_stage.append(stage)
    if idx is not None:
        idx.close()
    s, stage, idx = sketch()
    sketch_wall.append(s)
    sketch_stage.append(stage)
    print("bench_sketch: run %d: count %.3f s, sketch %.3f s" % (run, count_wall[-1], s), file=sys.stderr, flush=True)
med = lambda v: round(statistics.median(v), 5)
positions = idx.positions
line = {"tool": "bench_sketch", "runs": args.runs, "k": args.k, "w": args.w, "file_MB": round(os.path.getsize(args.fasta) / 1e6, 1), "chunk_bytes": args.chunk_bytes,
        "contigs": len(idx.contig_names), "positions": positions, "minimizers": idx.n, "density": round(idx.n / positions, 5),
        "sketch_wall_s": med(sketch_wall), "sketch_wall_min_max": [round(min(sketch_wall), 5), round(max(sketch_wall), 5)],
        "sketch_stage_s": {k: med([s[k] for s in sketch_stage]) for k in sketch_stage[0]},
        "count_wall_s": med(count_wall), "count_wall_min_max": [round(min(count_wall), 5), round(max(count_wall), 5)],
        "count_stage_s": {k: med([s[k] for s in count_stage]) for k in count_stage[0]},
        "sketch_over_count": round(statistics.median(sketch_wall) / statistics.median(count_wall), 3),
        "minimizers_per_s": round(idx.n / statistics.median(sketch_wall)), "positions_per_s_of_the_sketch_kernels": round(positions / statistics.median([s["sketch"] for s in sketch_stage]))}
host_wall = []
for _ in range(args.host_runs):
    t1 = time.perf_counter()
    host = minimizers.sketch_reference(args.fasta, args.k, args.w, device="cpu", chunk_bytes=args.chunk_bytes)
    host_wall.append(time.perf_counter() - t1)
    assert all(np.array_equal(a, b) for a, b in zip(host.arrays(), idx.arrays())), "the GPU sketch differs from the host backend's"
    line["equals_host"] = True
if host_wall:
    line.update({"host_wall_s": med(host_wall), "host_over_gpu": round(statistics.median(host_wall) / statistics.median(sketch_wall), 2)})
print(json.dumps(line))
