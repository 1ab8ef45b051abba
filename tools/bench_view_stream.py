"""The streamed `view` against the in-memory one: bam.view_bam (each batch's records deflated in HBM and written while the decode
runs) and bam.extract_records(...).write(device=gpu) (the records to the host, then back through coral_bgzf_write_gpu - what the
parent commit can do) on the same file with the reference workflow's filter, --filter_min_mapq 25 --filter_min_length 1001
(the reference's scripts/align_nanopore_reads.sh:42-44).

A third leg, `decode`, is the same decode with no records request at all (bam.decode_bam_gpu with the filter): what the stream
leg takes longer than that is what its copy, deflate and write kernels and its file writes add in wall time, and set against the
in-memory leg's writer (its wall time less its decode) says how much of the compression is hidden behind the decode.

Each leg runs in a fresh child process of its own - peak RSS is a process's high-water mark -: one warm run that is not counted,
then `runs` timed ones.  Per leg: wall time (median, min, max), waited_for_gpu_seconds of the decode (bam.LAST_DECODE), the
output's size, and the child's peak RSS.  The two outputs are compared byte for byte.  One JSON line.
    python tools/bench_view_stream.py [BAM] [--runs N] [--batch_bytes N] [--chunk_blocks N] [--min_mapq Q] [--min_length L]
Without a path: the 'cfg3_12k' records with real QUAL (the file of tools/bench_read_qc.py), written once."""
import argparse
import json
import os
import resource
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("bam", nargs="?", default="")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--batch_bytes", type=int, default=0)
ap.add_argument("--chunk_blocks", type=int, default=0)
ap.add_argument("--min_mapq", type=int, default=25)
ap.add_argument("--min_length", type=int, default=1001)
ap.add_argument("--device", default="cuda:0")
ap.add_argument("--leg", choices=("stream", "memory", "decode"), default=None)       # (the child's side)
ap.add_argument("--out", default="")
args = ap.parse_args()


def leg():
    import torch
    from coral_amd import bam
    flt = bam.RecordFilter(min_mapq=args.min_mapq, min_seq_length=args.min_length)

    def stream():
        return bam.view_bam(args.bam, args.out, record_filter=flt, device=args.device, batch_bytes=args.batch_bytes, chunk_blocks=args.chunk_blocks).records

    def memory():
        rec = bam.extract_records(args.bam, device=args.device, index=False, record_filter=flt, batch_bytes=args.batch_bytes)
        rec.write(args.out, device=args.device)
        return rec.n

    def decode():
        return bam.decode_bam_gpu(args.bam, args.device, batch_bytes=args.batch_bytes, record_filter=flt).n
    fn = {"stream": stream, "memory": memory, "decode": decode}[args.leg]
    fn()                                                  # warm: code objects, pinned buffers, the caching allocator, the page cache
    torch.cuda.synchronize()
    rss_warm = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    wall, waited, decode = [], [], []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        n = fn()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        waited.append(float(bam.LAST_DECODE["waited_for_gpu_seconds"]))
        decode.append(float(bam.LAST_DECODE["seconds"]))
    print(json.dumps({"leg": args.leg, "records": int(n), "batches": int(bam.LAST_DECODE["batches"]), "file_bytes": os.path.getsize(args.out) if args.leg != "decode" else 0,
                      "wall_s": wall, "waited_for_gpu_s": waited, "decode_s": decode, "peak_rss_MB_after_warm_run": round(rss_warm / 1024, 1),
                      "peak_rss_MB": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024, 1)}))


if args.leg:
    leg()
    sys.exit(0)

d = tempfile.mkdtemp(prefix="coral_view_stream_")
path = args.bam or os.path.join(d, "cfg3_12k_qual.bam")
if not os.path.exists(path):
    from coral_amd import bam, synth
    t0 = time.perf_counter()
    cfg, rec = synth.dataset("cfg3_12k", "cpu")
    bam.write_bam(rec, path, seed=1, with_qual=True, fast_seq=True)
    print("BAM written: %.1f MB in %.1f s" % (os.path.getsize(path) / 1e6, time.perf_counter() - t0), file=sys.stderr, flush=True)
    del rec

line = {"tool": "bench_view_stream", "bam_MB": round(os.path.getsize(path) / 1e6, 1), "runs": args.runs, "batch_bytes": args.batch_bytes,
        "chunk_blocks": args.chunk_blocks, "filter": {"min_mapq": args.min_mapq, "min_length": args.min_length}, "legs": {}}
outs = {}
for name in ("stream", "memory", "decode"):
    outs[name] = os.path.join(d, name + ".bam")
    cmd = [sys.executable, os.path.abspath(__file__), path, "--leg", name, "--out", outs[name], "--runs", str(args.runs), "--batch_bytes", str(args.batch_bytes),
           "--chunk_blocks", str(args.chunk_blocks), "--min_mapq", str(args.min_mapq), "--min_length", str(args.min_length), "--device", args.device]
    got = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=600)       # (a fresh child: its peak RSS is this leg's alone)
    r = json.loads(got.stdout.decode().strip().splitlines()[-1])
    for k in ("wall_s", "waited_for_gpu_s", "decode_s"):
        v = r.pop(k)
        r[k] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "all": [round(x, 4) for x in v]}
    line["legs"][name] = r
with open(outs["stream"], "rb") as a, open(outs["memory"], "rb") as b:
    line["byte_identical"] = a.read() == b.read()
s, m = line["legs"]["stream"], line["legs"]["memory"]
dec = line["legs"]["decode"]["wall_s"]["median"]
added, writer = s["wall_s"]["median"] - dec, m["wall_s"]["median"] - m["decode_s"]["median"]
line["stream_vs_memory"] = {"wall": round(s["wall_s"]["median"] / m["wall_s"]["median"], 4), "peak_rss_MB_saved": round(m["peak_rss_MB"] - s["peak_rss_MB"], 1),
                            "stream_added_to_decode_s": round(added, 4), "memory_writer_s": round(writer, 4),
                            "hidden_share_of_the_writer": round(1 - added / writer, 4) if writer > 0 else None}
print(json.dumps(line))
import shutil
shutil.rmtree(d, ignore_errors=True)
