"""Cost of the copy-number segmenter (cnv.segment_depth: coral_cn_segment_gpu against coral_cn_segment_host) and of the `cnv`
mode end to end.

Builds a binned-depth table of hg38's shape (chr1..chr22, X, Y) at each `--bin_size` (default 1000 and 100: about 3.1 M and 31 M
bins): Poisson depth of 30x from a seed, the centromeres empty, steps of 0.5x .. 8x planted on every contig.  Times, median of
`runs` after one warm-up:
  gpu     segment_depth on cuda:0, wall time around a call that ends in a stream synchronise, and the call's own stage times from
          HIP events (cnv.LAST_SEGMENT: upload, centre + signal + compaction + prefix sums, noise, the levels' peaks and sorts, the
          cuts on the host, unify + rows + download)
  host    segment_depth with device "cpu" on the same box (one thread), `--host_runs` times
and checks that both give the same rows.  Then, on a BAM of `--reads` config-3 reads (0: skipped): bam.binned_depth alone against
cnv.call_copy_number (the decode plus the segmenter) at 1 kb bins.  One JSON line.
    python tools/bench_cnv.py [runs] [--bin_size B ...] [--host_runs N] [--reads N] [--kernels-only]
--kernels-only: one GPU segment_depth per bin size and nothing else (the leg to run under rocprofv3 --kernel-trace --stats)."""
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

from coral_amd import bam, cnv

HG38 = [248956422, 242193529, 198295559, 190214555, 181538259, 170805979, 159345973, 145138636, 138394717, 133797422, 135086622, 133275309, 114364328, 107043718,
        101991189, 90338345, 83257441, 80373285, 58617616, 64444167, 46709983, 50818468, 156040895, 57227415]
CHROMS = ["chr%d" % k for k in range(1, 23)] + ["chrX", "chrY"]
FACTORS = (0.5, 1.5, 2.0, 3.0, 4.0, 8.0)

ap = argparse.ArgumentParser()
ap.add_argument("runs", nargs="?", type=int, default=5)
ap.add_argument("--bin_size", type=int, action="append")
ap.add_argument("--host_runs", type=int, default=1)
ap.add_argument("--reads", type=int, default=200000)
ap.add_argument("--kernels-only", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_cnv.py measures on a GPU"
dev = "cuda:0"


def table(bin_size, seed=7):
    """(BinnedDepth, planted steps) of hg38's shape: 30x, the 3 Mb in the middle of every contig empty, six steps per contig."""
    rng = np.random.default_rng(seed)
    parts, planted = [], 0
    for length in HG38:
        n = -(-length // bin_size)
        mean = np.full(n, 30.0 * bin_size)
        for k, f in enumerate(FACTORS):
            a = (k + 1) * n // 8
            mean[a:a + max(2, 200_000 // bin_size) * (k + 1)] *= f
            planted += 2
        mean[n // 2:n // 2 + 3_000_000 // bin_size] = 0.0
        parts.append(rng.poisson(mean).astype(np.int64))
    bases = np.concatenate(parts)
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return bam.BinnedDepth(CHROMS, HG38, bin_size, 0, 0x704, True, off, bases, np.zeros(len(bases), dtype=np.int64)), planted


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def rows(seg):
    return (seg.contig.tolist(), seg.start.tolist(), seg.end.tolist(), seg.probes.tolist(), seg.sum_s.tolist(), seg.sum_bases.tolist())


line = {"tool": "bench_cnv", "runs": args.runs, "host_runs": args.host_runs, "tables": []}
for bin_size in args.bin_size or [1000, 100]:
    depth, planted = table(bin_size)
    if args.kernels_only:
        seg = cnv.segment_depth(depth, device=dev)
        line["tables"].append({"bin_size": bin_size, "bins": depth.n_bins, "rows": len(seg)})
        continue
    timed(lambda: cnv.segment_depth(depth, device=dev))                       # warm-up: code objects, hipcub's choices, the allocator
    wall, stages = [], []
    for _ in range(args.runs):
        seg, w = timed(lambda: cnv.segment_depth(depth, device=dev))
        wall.append(w)
        stages.append(dict(cnv.LAST_SEGMENT))
    host_wall = []
    for _ in range(args.host_runs):
        t0 = time.perf_counter()
        host = cnv.segment_depth(depth, device="cpu")
        host_wall.append(time.perf_counter() - t0)
    assert rows(host) == rows(seg) and host.counts == seg.counts, "the GPU rows differ from the host backend's"
    med = lambda v: round(statistics.median(v), 5)
    line["tables"].append({
        "bin_size": bin_size, "bins": depth.n_bins, "kept": seg.counts["kept"], "rows": len(seg), "breakpoints": seg.counts["breakpoints"], "planted_steps": planted,
        "equals_host": True, "gpu_wall_s": med(wall), "gpu_wall_min_max": [round(min(wall), 5), round(max(wall), 5)],
        "gpu_stage_s": {k: med([s[k] for s in stages]) for k in stages[0] if k != "workspace_bytes"}, "workspace_MB": round(stages[0]["workspace_bytes"] / 1e6, 1),
        "host_wall_s": med(host_wall), "host_over_gpu": round(statistics.median(host_wall) / statistics.median(wall), 2)})
    del depth, seg

if args.reads and not args.kernels_only:
    from coral_amd import synth
    d = tempfile.mkdtemp(prefix="coral_cnv_")
    path = os.path.join(d, "cfg3_%d.bam" % args.reads)
    rec = synth.generate(synth.scaled_config("cfg3", args.reads), dev, chunk_pieces=200000).to("cpu")
    bam.write_bam_native(rec, path, seed=1, level=1)
    del rec
    legs = {"binned_depth": lambda: bam.binned_depth(path, 1000, device=dev), "call_copy_number": lambda: cnv.call_copy_number(path, 1000, device=dev)}
    res = {k: [] for k in legs}
    timed(legs["call_copy_number"])
    for _ in range(args.runs):
        for k, fn in legs.items():                          # interleaved, so that drift hits both alike
            out, w = timed(fn)
            res[k].append(w)
    line["end_to_end"] = {"reads": args.reads, "bam_MB": round(os.path.getsize(path) / 1e6, 1), "bins": out.counts["kept"], "rows": len(out),
                          "wall_s": {k: round(statistics.median(v), 4) for k, v in res.items()}, "min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in res.items()}}
    import shutil
    shutil.rmtree(d, ignore_errors=True)
print(json.dumps(line))
