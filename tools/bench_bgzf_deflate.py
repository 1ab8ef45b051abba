"""Wall time of the BAM writers: RecordBytes.write(level=1) on the host (coral_bgzf_write: zlib on `--threads` threads) against
RecordBytes.write(device="cuda:0") (coral_bgzf_write_gpu: k_bgzf_deflate + k_bgzf_pack per chunk of 1 024 blocks), and
bam.sort_bam end to end both ways.

The bytes written are the records of the shuffled 'cfg3_12k' file of tools/bench_sort.py (real QUAL; made here when --bam does not
exist, and left there), in file order.  Median and [min, max] of `runs` interleaved runs, the two files' sizes, and a check that
the GPU-written file inflates to the header and the records.  One JSON line.
    python tools/bench_bgzf_deflate.py [runs] [--bam PATH] [--threads N] [--make-only] [--kernels-only] [--host-only]
--make-only:     write the shuffled file and stop (no GPU needed).
--kernels-only:  one write(device=...) and nothing else: the leg to run under rocprofv3 --kernel-trace --stats.
--host-only:     only the host leg (no GPU needed; runs on a checkout without the feature too)."""
import argparse
import gzip
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from coral_amd import bam, synth

ap = argparse.ArgumentParser()
ap.add_argument("runs", nargs="?", type=int, default=7)
ap.add_argument("--bam", default="")
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--make-only", action="store_true")
ap.add_argument("--kernels-only", action="store_true")
ap.add_argument("--host-only", action="store_true")
args = ap.parse_args()

d = tempfile.mkdtemp(prefix="coral_deflate_")
path = args.bam or os.path.join(d, "cfg3_12k_qual_shuffled.bam")
if not os.path.exists(path):
    t0 = time.perf_counter()
    cfg, rec = synth.dataset("cfg3_12k", "cpu")
    ordered = os.path.join(d, "cfg3_12k_qual.bam")
    bam.write_bam(rec, ordered, seed=1, with_qual=True, fast_seq=True)
    src = bam.extract_records(ordered, device="cpu", index=False)
    perm = np.random.default_rng(7).permutation(src.n)
    lens = np.diff(src.offsets)[perm]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    take = np.repeat(src.offsets[:-1][perm] - off[:-1], lens) + np.arange(int(off[-1]), dtype=np.int64)
    bam.RecordBytes(src.data[take], off, src.header).write(path, level=1)
    os.remove(ordered)
    del src, take
    print("shuffled BAM written: %.1f MB in %.1f s" % (os.path.getsize(path) / 1e6, time.perf_counter() - t0), file=sys.stderr, flush=True)
if args.make_only:
    sys.exit(0)

dev = "cuda:0"
src = bam.extract_records(path, device="cpu", index=False)
out_h, out_g = os.path.join(d, "host.bam"), os.path.join(d, "gpu.bam")
if args.kernels_only:
    src.write(out_g, device=dev)
    print(json.dumps({"records": src.n, "bytes": int(len(src.data)), "blocks": (len(src.data) + 0xff00 - 1) // 0xff00 + 1, "file_MB": round(os.path.getsize(out_g) / 1e6, 1)}))
    shutil.rmtree(d, ignore_errors=True)
    sys.exit(0)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


legs = {"write_host": lambda: src.write(out_h, level=1, n_threads=args.threads)}
if not args.host_only:
    legs["write_gpu"] = lambda: src.write(out_g, device=dev)
    legs["write_gpu"]()                                    # warm-up: code objects, the caching allocator
res = {k: [] for k in legs}
for r in range(args.runs):
    for k, fn in legs.items():                             # interleaved, so that drift hits every leg alike
        res[k].append(round(timed(fn), 4))
line = {"tool": "bench_bgzf_deflate", "data": "cfg3_12k shuffled, file order", "records": src.n, "record_MB": round(len(src.data) / 1e6, 1), "runs": args.runs,
        "host_threads": args.threads, "median_s": {k: round(statistics.median(v), 4) for k, v in res.items()},
        "min_max_s": {k: [min(v), max(v)] for k, v in res.items()}, "all_runs_s": res, "file_MB": {"host": round(os.path.getsize(out_h) / 1e6, 1)}}
if not args.host_only:
    line["file_MB"]["gpu"] = round(os.path.getsize(out_g) / 1e6, 1)
    with gzip.open(out_g, "rb") as fp:
        back = fp.read()
    assert back == src.header + src.data.tobytes(), "the GPU-written file does not inflate to the header and the records"
    del back
    sort_legs = {"sort_bam_host_write": lambda: bam.sort_bam(path, out_h, device=dev, n_threads=args.threads),
                 "sort_bam_gpu_write": lambda: bam.sort_bam(path, out_g, device=dev, n_threads=args.threads, write_device=dev)}
    sres = {k: [] for k in sort_legs}
    for r in range(3):
        for k, fn in sort_legs.items():
            sres[k].append(round(timed(fn), 4))
    line["sort_bam"] = {"runs": 3, "median_s": {k: round(statistics.median(v), 4) for k, v in sres.items()}, "min_max_s": {k: [min(v), max(v)] for k, v in sres.items()}}
print(json.dumps(line))
shutil.rmtree(d, ignore_errors=True)
