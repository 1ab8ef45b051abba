"""Cost of the coordinate order on the GPU decode (bam.extract_records(order="coordinate"): k_bam_sort_keys, hipcub's radix
sort, k_bam_sort_permute and k_bam_reads_copy_sorted per batch, coral_bam_records_merge over the batches' runs).

Writes a BAM of the 'cfg3_12k' records with real QUAL whose records are SHUFFLED (a mapper writes in read order; fixed seed: the
file of tools/bench_read_qc.py decoded in file order on the host, permuted, written again with RecordBytes.write) and times,
median of `runs` interleaved runs:
  decode       decode_bam_gpu alone (no request: nothing is launched, nothing more allocated)
  file         the decode with a records request for every record, order="file" (what the parent commit can do)
  coordinate   the same request with order="coordinate": the difference to `file` is the cost of the sort
as wall time and as HIP-event time on the caller's stream.  The line also holds the host wall time of coral_bam_records_merge over
the runs of a `--batch_bytes` decode (runs = batches; with the default batch the file is one run and nothing is merged), as its
share of that decode's wall time, and the wall time of bam.sort_bam (level 1, with the index).  One JSON line.
    python tools/bench_sort.py [runs] [--bam PATH] [--batch_bytes N] [--kernels-only file|coordinate] [--decode-only] [--stream]
--kernels-only: one decode with the request in that order and nothing else (the leg to run under rocprofv3 --kernel-trace
                --stats: k_bam_reads_copy of `file` against k_bam_reads_copy_sorted of `coordinate` on the same bytes).
--decode-only:  only the `decode` leg (runs on a checkout without the feature: the yardstick for "no request costs nothing").
--stream:       the streamed sort (bam.sort_bam_stream) against the in-memory one (bam.sort_bam(write_device=gpu)), both without
                the index, `runs` times each, interleaved, every run in a fresh child process so that its peak resident set
                (VmHWM) is its own: wall time, the two phases, phase 2 split into order / read / inflate / copy / sink,
                spill size against output size, the edge members inflated twice, peak host RSS of both paths; the outputs
                must be equal byte for byte.  --batch_bytes and --stage_bytes are passed on (0: the defaults)."""
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
ap.add_argument("--batch_bytes", type=int, default=64 << 20)
ap.add_argument("--kernels-only", choices=("file", "coordinate"), default=None)
ap.add_argument("--decode-only", action="store_true")
ap.add_argument("--stream", action="store_true")
ap.add_argument("--stream-leg", choices=("memory", "stream"), default=None, help=argparse.SUPPRESS)
ap.add_argument("--stage_bytes", type=int, default=0)
ap.add_argument("--out", default="", help=argparse.SUPPRESS)
args = ap.parse_args()

d = tempfile.mkdtemp(prefix="coral_sort_")
path = args.bam or os.path.join(d, "cfg3_12k_qual_shuffled.bam")
n_records = None
if not os.path.exists(path):
    t0 = time.perf_counter()
    cfg, rec = synth.dataset("cfg3_12k", "cpu")
    ordered = os.path.join(d, "cfg3_12k_qual.bam")
    bam.write_bam(rec, ordered, seed=1, with_qual=True, fast_seq=True)
    src = bam.extract_records(ordered, device="cpu", index=False)           # (file order: this leg exists on the parent commit too)
    perm = np.random.default_rng(7).permutation(src.n)
    lens = np.diff(src.offsets)[perm]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    take = np.repeat(src.offsets[:-1][perm] - off[:-1], lens) + np.arange(int(off[-1]), dtype=np.int64)
    bam.RecordBytes(src.data[take], off, src.header).write(path, level=1)
    os.remove(ordered)
    n_records = int(src.n)
    del src, take
    print("shuffled BAM written: %.1f MB in %.1f s" % (os.path.getsize(path) / 1e6, time.perf_counter() - t0), file=sys.stderr, flush=True)
dev = "cuda:0"

if args.stream_leg:                                     # one run in this (fresh) process: its peak RSS is the leg's own
    def peak_rss_MB():                                  # VmHWM: of this program alone (ru_maxrss would carry the parent's over the exec)
        with open("/proc/self/status") as fp:
            return round(next(int(ln.split()[1]) for ln in fp if ln.startswith("VmHWM:")) / 1024, 1)
    batch = args.batch_bytes if args.batch_bytes != (64 << 20) else 0
    t0 = time.perf_counter()
    if args.stream_leg == "stream":
        st = bam.sort_bam_stream(path, args.out, index=False, device=dev, batch_bytes=batch, stage_bytes=args.stage_bytes)
        extra = dict(bam.LAST_SORT_STREAM, records=st.records, bytes=st.bytes, spill_bytes=st.spill_bytes)
    else:
        bam.sort_bam(path, args.out, index=False, device=dev, write_device=dev, batch_bytes=batch)
        extra = {"batches": bam.LAST_DECODE.get("batches")}
    wall = time.perf_counter() - t0
    print(json.dumps(dict(extra, leg=args.stream_leg, wall_s=round(wall, 4), peak_rss_MB=peak_rss_MB(),
                          file_bytes=os.path.getsize(args.out))))
    os.rmdir(d)
    sys.exit(0)

if args.stream:
    import hashlib
    import subprocess
    runs = {"memory": [], "stream": []}
    digest = {}
    for r in range(args.runs):
        for leg in runs:                                # interleaved; a fresh child each (this process never touches the GPU)
            out = os.path.join(d, leg + ".bam")
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--bam", path, "--stream-leg", leg, "--out", out, "--batch_bytes", str(args.batch_bytes),
                                   "--stage_bytes", str(args.stage_bytes)], capture_output=True, text=True, timeout=900)
            if done.returncode != 0:
                sys.exit("leg %s failed (%d): %s" % (leg, done.returncode, done.stderr[-2000:]))
            runs[leg].append(json.loads(done.stdout.strip().splitlines()[-1]))
            with open(out, "rb") as fp:
                h = hashlib.sha256()
                for piece in iter(lambda: fp.read(1 << 24), b""):
                    h.update(piece)
                digest[leg] = h.hexdigest()
            os.remove(out)
        assert digest["memory"] == digest["stream"], "the streamed sort's file differs from the in-memory sort's"
    med = lambda leg, k: round(statistics.median(x[k] for x in runs[leg]), 4)
    keys = ("phase1_seconds", "phase2_seconds", "order_seconds", "read_seconds", "inflate_wait_seconds", "inflate_gpu_seconds", "copy_gpu_seconds", "sink_seconds")
    last = runs["stream"][-1]
    print(json.dumps({"tool": "bench_sort --stream", "bam_MB": round(os.path.getsize(path) / 1e6, 1), "runs": args.runs, "records": last["records"],
                      "record_bytes": last["bytes"], "output_bytes": last["file_bytes"], "spill_bytes": last["spill_bytes"],
                      "spill_over_output": round(last["spill_bytes"] / last["file_bytes"], 4), "sorted_runs": last["runs"], "steps": last["steps"],
                      "spill_members_inflated": last["spill_members_inflated"], "edge_members_inflated_twice": last["edge_members_inflated_twice"],
                      "workspace_MB": round(last["workspace_bytes"] / 2 ** 20, 1), "merge_workspace_MB": round(last["merge_workspace_bytes"] / 2 ** 20, 1),
                      "median": {"memory": {"wall_s": med("memory", "wall_s"), "peak_rss_MB": med("memory", "peak_rss_MB")},
                                 "stream": dict({"wall_s": med("stream", "wall_s"), "peak_rss_MB": med("stream", "peak_rss_MB")}, **{k: med("stream", k) for k in keys})},
                      "identical_bytes": True, "all_runs": runs}))
    import shutil
    shutil.rmtree(d, ignore_errors=True)
    sys.exit(0)

if args.decode_only:
    extract = None
else:
    extract = lambda order, **kw: bam.extract_records(path, device=dev, index=False, order=order, **kw)

if args.kernels_only:
    got = extract(args.kernels_only)
    torch.cuda.synchronize()
    print(json.dumps({"order": args.kernels_only, "records": got.n, "bytes": int(len(got.data)), "batches": bam.LAST_DECODE.get("batches")}))
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
    legs["file"] = lambda: extract("file")
    legs["coordinate"] = lambda: extract("coordinate")
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
line = {"tool": "bench_sort", "data": "cfg3_12k shuffled", "records": n_records, "bam_MB": round(os.path.getsize(path) / 1e6, 1), "runs": args.runs,
        "median": med, "min_max": spread, "all_runs": res}
if not args.decode_only:
    got = last["coordinate"]
    host = bam.extract_records(path, device="cpu", index=False, order="coordinate")
    assert np.array_equal(got.data, host.data) and np.array_equal(got.offsets, host.offsets), "the GPU result differs from the host pipeline's"
    assert len(got.data) == len(last["file"].data) and got.n == last["file"].n
    line["coordinate"] = {"records": got.n, "bytes": int(len(got.data)),
                          "sort_cost_vs_file": {m: round(med["coordinate"][m] / med["file"][m] - 1, 4) for m in ("wall_s", "event_s")},
                          "overhead_vs_decode": {m: round(med["coordinate"][m] / med["decode"][m] - 1, 4) for m in ("wall_s", "event_s")}}
    # the host merge: the sorted results of the batches of a small-batch decode are its runs; here the same runs are made from
    # `world` sorted byte ranges and merged through the same native call, timed on its own
    t = []
    for r in range(3):
        t0 = time.perf_counter()
        many = extract("coordinate", batch_bytes=args.batch_bytes)
        t.append(time.perf_counter() - t0)
    batches = int(bam.LAST_DECODE.get("batches", 0))
    assert np.array_equal(many.data, got.data)
    world = max(batches, 2)
    parts = [bam.extract_records(path, device="cpu", index=False, order="coordinate", rank=k, world=world) for k in range(world)]
    m = []
    for r in range(3):
        t0 = time.perf_counter()
        whole = bam.merge_sorted_record_bytes(parts)
        m.append(time.perf_counter() - t0)
    assert np.array_equal(whole.data, got.data)
    line["merge"] = {"batch_bytes": args.batch_bytes, "batches": batches, "decode_wall_s_median": round(statistics.median(t), 4), "runs_merged": world,
                     "merge_wall_s_median": round(statistics.median(m), 4), "share_of_wall": round(statistics.median(m) / statistics.median(t), 4)}
    t0 = time.perf_counter()
    out = bam.sort_bam(path, os.path.join(d, "sorted.bam"), device=dev)
    line["sort_bam_s"] = {"wall_s": round(time.perf_counter() - t0, 4), "file_MB": round(os.path.getsize(out) / 1e6, 1)}
print(json.dumps(line))
import shutil
shutil.rmtree(d, ignore_errors=True)
