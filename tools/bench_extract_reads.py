"""Cost of the reads request on the GPU decode (bam.extract_reads: k_bam_reads_plan + k_bam_reads_emit per batch; with
--format bam the records request, bam.extract_records: k_bam_reads_plan + k_bam_reads_copy per batch).

Writes a BAM of the 'cfg3_12k' records with real QUAL (the pure-Python writer; the file tools/bench_read_qc.py uses) and times,
median of `runs`:
  decode    decode_bam_gpu alone (no request: nothing is launched, nothing more allocated)
  regions   the same decode with a reads request for the plot regions (the config's amplicon intervals; no index: the whole file)
  all       the same decode with a request for every read (exclude_flags 0x900)
as wall time and as HIP-event time on the caller's stream, plus the text bytes written.  One JSON line.
    python tools/bench_extract_reads.py [runs] [--bam PATH] [--format fastq|bam] [--kernels-only] [--decode-only]
--format bam:   the `regions` and `all` legs ask for the records' own bytes (exclude_flags 0x900, as FASTQ); the line also holds the host wall
                time of RecordBytes.write(level=1) and (level=0) of the `regions` result, and the time of a device-to-device
                hipMemcpyAsync of as many bytes as the `all` leg copied (the yardstick for k_bam_reads_copy's rate).
--kernels-only: one decode with the request for every read and nothing else (the leg to run under rocprofv3 --kernel-trace --stats).
--decode-only:  only the `decode` leg (runs on a checkout without the request: the yardstick for "no request costs nothing")."""
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

from coral_amd import bam, synth

ap = argparse.ArgumentParser()
ap.add_argument("runs", nargs="?", type=int, default=7)
ap.add_argument("--bam", default="")
ap.add_argument("--format", choices=("fastq", "bam"), default="fastq")
ap.add_argument("--kernels-only", action="store_true")
ap.add_argument("--decode-only", action="store_true")
args = ap.parse_args()

d = tempfile.mkdtemp(prefix="coral_reads_")
path = args.bam or os.path.join(d, "cfg3_12k_qual.bam")
cfg, rec = synth.dataset("cfg3_12k", "cpu")
if not os.path.exists(path):
    t0 = time.perf_counter()
    bam.write_bam(rec, path, seed=1, with_qual=True, fast_seq=True)
    print("BAM written: %.1f MB in %.1f s" % (os.path.getsize(path) / 1e6, time.perf_counter() - t0), file=sys.stderr, flush=True)
dev = "cuda:0"
seeds = os.path.join(d, "seeds.bed")
synth.write_seed_bed(cfg, seeds)
with open(seeds) as fp:                                  # the plot regions: the seed intervals widened by 100 kb on either side
    regions = [(r[0], max(int(r[1]) - 100_000, 0), int(r[2]) + 100_000) for r in (ln.split() for ln in fp if ln.strip())]

as_bam = args.format == "bam"
extract = (lambda *a, **kw: bam.extract_records(*a, exclude_flags=0x900, **kw)) if as_bam else bam.extract_reads      # the same records either way
payload = (lambda r: r.data) if as_bam else (lambda r: r.text)

if args.kernels_only:
    got = extract(path, device=dev, index=False)
    torch.cuda.synchronize()
    print(json.dumps({"format": args.format, "reads": got.n, "text_bytes": int(len(payload(got)))}))
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
    legs["regions"] = lambda: extract(path, regions, device=dev, index=False)
    legs["all"] = lambda: extract(path, device=dev, index=False)
res = {k: {"wall_s": [], "event_s": []} for k in legs}
last = {}
timed(legs["decode"])                                   # warm-up: code objects, pinned buffers, caching allocator
for r in range(args.runs):
    for k, fn in legs.items():                          # interleaved, so that drift hits every leg alike
        o, w, e = timed(fn)
        res[k]["wall_s"].append(w)
        res[k]["event_s"].append(e)
        if k != "decode":
            last[k] = o
        del o

med = {k: {m: round(statistics.median(v[m]), 4) for m in v} for k, v in res.items()}
spread = {k: {m: [round(min(v[m]), 4), round(max(v[m]), 4)] for m in v} for k, v in res.items()}
line = {"tool": "bench_extract_reads", "format": args.format, "data": "cfg3_12k", "records": rec.n, "bam_MB": round(os.path.getsize(path) / 1e6, 1), "runs": args.runs,
        "regions": regions, "median": med, "min_max": spread, "all_runs": res}
for k, got in last.items():
    host = extract(path, regions if k == "regions" else None, device="cpu", index=False)
    assert np.array_equal(payload(got), payload(host)) and np.array_equal(got.offsets, host.offsets), "the GPU result differs from the host pipeline's"
    line[k] = {"reads": got.n, "text_bytes": int(len(payload(got))),
               "overhead_vs_decode": {m: round(med[k][m] / med["decode"][m] - 1, 4) for m in ("wall_s", "event_s")}}
if as_bam and "regions" in last:                        # the writer, host only
    line["write_s"] = {}
    for level in (1, 0):
        t = []
        for r in range(3):
            t0 = time.perf_counter()
            last["regions"].write(os.path.join(d, "regions_l%d.bam" % level), level=level)
            t.append(time.perf_counter() - t0)
        line["write_s"]["level%d" % level] = {"median": round(statistics.median(t), 4), "min_max": [round(min(t), 4), round(max(t), 4)],
                                              "file_MB": round(os.path.getsize(os.path.join(d, "regions_l%d.bam" % level)) / 1e6, 2)}
if as_bam and "all" in last:                            # hipMemcpyAsync device to device of the bytes the `all` leg copied
    n = int(len(last["all"].data))
    src, dst = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    src.zero_()
    dst.copy_(src)                                      # (contiguous, same dtype, same device: torch issues hipMemcpyAsync)
    t = [timed(lambda: dst.copy_(src))[2] for _ in range(9)]
    line["memcpy_d2d"] = {"bytes": n, "event_s_median": round(statistics.median(t), 6), "GB_per_s": round(n / statistics.median(t) / 1e9, 1)}
print(json.dumps(line))
import shutil
shutil.rmtree(d, ignore_errors=True)
