"""Cost of the binned-depth request on the GPU decode (bam.binned_depth: k_bam_depth per batch).

Writes a BAM of the 'cfg3_12k' records with real QUAL (the pure-Python writer; the file tools/bench_pileup.py uses) and times,
median of `runs`:
  decode    decode_bam_gpu alone (no request: nothing is launched, nothing more allocated)
  depth     the decode with the binned-depth request at `--bin_size` (default 1000) and the defaults of bam.binned_depth
  cov       window coverage over the same bins at threshold 0 (k_bam_cov_count; the only other way to these numbers)
as wall time and as HIP-event time on the caller's stream.  One JSON line.
    python tools/bench_depth.py [runs] [--bam PATH] [--reads N] [--hot] [--bin_size B] [--kernels-only] [--decode-only] [--stats-csv PATH]
--reads N:      instead, N config-3 reads through the native writer (no QUAL, so no `cov` leg): 2000000 is the full-size file.
--hot:          instead, a file of `HOT_READS` reads of 10 kb that all start in one bin: every read adds to the same few counters.
--kernels-only: one decode with the request and nothing else (the leg to run under rocprofv3 --kernel-trace --stats).
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

from coral_amd import bam, synth

HOT_READS, HOT_READ_LEN, HOT_AT = 60000, 10_000, 1_000_000

ap = argparse.ArgumentParser()
ap.add_argument("runs", nargs="?", type=int, default=7)
ap.add_argument("--bam", default="")
ap.add_argument("--reads", type=int, default=0)
ap.add_argument("--hot", action="store_true")
ap.add_argument("--bin_size", type=int, default=1000)
ap.add_argument("--kernels-only", action="store_true")
ap.add_argument("--decode-only", action="store_true")
ap.add_argument("--stats-csv", default="")
args = ap.parse_args()

d = tempfile.mkdtemp(prefix="coral_depth_")
dev = "cuda:0"
has_qual = False
t0 = time.perf_counter()
if args.hot:
    data, path = "hot spot: %d reads of %d bases starting in one bin" % (HOT_READS, HOT_READ_LEN), args.bam or os.path.join(d, "hot_spot.bam")
    if not os.path.exists(path):
        rec = synth.records_from_alignments([dict(tid=7, pos=HOT_AT + (k * 900) // HOT_READS, cigar=[(0, HOT_READ_LEN)], name="h%d" % k)
                                             for k in range(HOT_READS)])
        bam.write_bam_native(rec, path, seed=1)
elif args.reads:
    data, path = "cfg3, %d reads (native writer, no QUAL)" % args.reads, args.bam or os.path.join(d, "cfg3_%d.bam" % args.reads)
    if not os.path.exists(path):
        rec = synth.generate(synth.scaled_config("cfg3", args.reads), dev, chunk_pieces=200000).to("cpu")
        bam.write_bam_native(rec, path, seed=1, level=1)
        del rec
else:
    data, path, has_qual = "cfg3_12k", args.bam or os.path.join(d, "cfg3_12k_qual.bam"), True
    if not os.path.exists(path):
        _, rec = synth.dataset("cfg3_12k", "cpu")
        bam.write_bam(rec, path, seed=1, with_qual=True, fast_seq=True)
print("BAM ready: %.1f MB in %.1f s" % (os.path.getsize(path) / 1e6, time.perf_counter() - t0), file=sys.stderr, flush=True)
params = bam.depth_parameters(args.bin_size, 0, 0x704, True) if hasattr(bam, "depth_parameters") else None

if args.kernels_only:
    res = bam._decode(path, dev, records=False, depth=params)
    torch.cuda.synchronize()
    print(json.dumps({"bins": int(len(res.depth[1])), "bases": int(res.depth[1].sum()), "reads": int(res.depth[2].sum()), "batches": bam.LAST_DECODE["batches"]}))
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
    legs["depth"] = lambda: bam._decode(path, dev, depth=params)
    if has_qual:
        chroms, lengths = bam.bam_reference_names(path), bam.bam_reference_lengths(path)
        tid = np.concatenate([np.full(-(-l // args.bin_size), t, dtype=np.int64) for t, l in enumerate(lengths)])
        lo = np.concatenate([np.arange(0, l, args.bin_size, dtype=np.int64) for l in lengths])
        hi = np.minimum(lo + args.bin_size, np.asarray(lengths, dtype=np.int64)[tid])
        segs = np.stack([tid, lo, hi]).astype(np.int32)
        legs["cov"] = lambda: bam._decode(path, dev, coverage=(segs, 0, 1))
res = {k: {"wall_s": [], "event_s": []} for k in legs}
outs = {}
timed(legs["decode"])                                   # warm-up: code objects, pinned buffers, caching allocator
for r in range(args.runs):
    for k, fn in legs.items():                          # interleaved, so that drift hits every leg alike
        o, w, e = timed(fn)
        res[k]["wall_s"].append(w)
        res[k]["event_s"].append(e)
        if k != "decode":
            outs[k] = (o.depth, o.counts)
        del o

med = {k: {m: round(statistics.median(v[m]), 4) for m in v} for k, v in res.items()}
spread = {k: {m: [round(min(v[m]), 4), round(max(v[m]), 4)] for m in v} for k, v in res.items()}
line = {"tool": "bench_depth", "data": data, "bam_MB": round(os.path.getsize(path) / 1e6, 1), "bin_size": args.bin_size, "runs": args.runs, "median": med,
        "min_max": spread, "all_runs": res}
if "depth" in outs:
    off, bases, reads = outs["depth"][0]
    if os.path.getsize(path) < 1 << 30:                 # (the host pipeline on the full-size file takes minutes)
        host = bam._decode(path, "cpu", records=False, depth=params).depth
        assert all(np.array_equal(a, b) for a, b in zip(host, (off, bases, reads))), "the GPU tables differ from the host pipeline's"
        line["equals_host"] = True
    line["overhead_vs_decode"] = {k: {m: round(med[k][m] / med["decode"][m] - 1, 4) for m in ("wall_s", "event_s")} for k in outs}
    line["bins"], line["bases"], line["reads"], line["max_bin_bases"] = int(len(bases)), int(bases.sum()), int(reads.sum()), int(bases.max())
    if "cov" in outs:                                   # D ops are the difference: the coverage rule never counts them
        line["cov_bases"] = int(outs["cov"][1].sum())
if args.stats_csv:
    with open(args.stats_csv) as fp:
        rows = {r["Name"].split("(")[0].split("<")[0]: r for r in csv.DictReader(fp)}
    line["kernel_stats"] = {k: {"calls": int(r["Calls"]), "total_us": round(float(r["TotalDurationNs"]) / 1e3, 1)}
                            for k, r in rows.items() if k in ("k_bam_depth", "k_bam_emit", "k_bam_meta", "k_bgzf_inflate", "k_bgzf_crc")}
print(json.dumps(line))
import shutil
shutil.rmtree(d, ignore_errors=True)
