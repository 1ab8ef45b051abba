"""Cost of the read QC on the FASTQ itself (fastq.read_qc: k_fastq_* of coral_fastq.hip against the host backend) beside
composition.reference_composition on a FASTA of the same size in the same process - the rate at which the machine streams text to
the device.

Generates both files under the temporary directory (none is shipped and none is fetched): `--bytes` (default 1 GB) of seeded
FASTQ, reads of 15 to 25 kb with qualities 2 .. 50, and a FASTA of the same size in 24 records of 60-column lines.  Times, after
one warm-up of each, `runs` alternating pairs:
  fastq_qc      fastq.read_qc on cuda:0 without thresholds and without an output: wall time and the call's own stage times
                (fastq.LAST_FASTQ_QC: reading the file, the feed calls, and from HIP events the uploads, scan + walk, accumulate)
  composition   reference_composition on cuda:0 on the FASTA: wall time and its stage times
  filter        fastq.read_qc with thresholds that keep about half the reads and an output file, `runs` times: wall time and
                the write stage
  plain read    the pieces of each file read and dropped, three times: what `read` costs without a session
  host          fastq.read_qc with device "cpu" (one thread; a reference, not the code under test), once; rows, histogram and
                counters must equal the GPU's
One JSON line.
    python tools/bench_fastq_qc.py [runs] [--bytes N] [--chunk_bytes N] [--no_host]"""
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

from coral_amd import composition, fasta_stream, fastq

ap = argparse.ArgumentParser()
ap.add_argument("runs", nargs="?", type=int, default=5)
ap.add_argument("--bytes", type=int, default=1_000_000_000)
ap.add_argument("--chunk_bytes", type=int, default=64 << 20)
ap.add_argument("--no_host", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_fastq_qc.py measures on a GPU"
dev = "cuda:0"
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def write_fastq(path, n_bytes, seed=17):
    rng = np.random.default_rng(seed)
    written, k = 0, 0
    with open(path, "wb", buffering=32 << 20) as fp:                      # (large writes, as the FASTA's: the page cache serves both alike)
        while written < n_bytes:
            n = int(rng.integers(15_000, 25_001))
            level = int(rng.integers(8, 40))                              # the read's own quality level
            qual = np.clip(rng.integers(level - 6, level + 7, n), 2, 50).astype(np.uint8) + 33
            rec = b"@read%d runid=bench ch=%d\n" % (k, k % 512) + ACGT[rng.integers(0, 4, n, dtype=np.uint8)].tobytes() + b"\n+\n" + qual.tobytes() + b"\n"
            fp.write(rec)
            written += len(rec)
            k += 1
            if k % 5000 == 0:
                print("bench_fastq_qc: %d reads written" % k, file=sys.stderr, flush=True)
    return k


def write_fasta(path, n_bytes, seed=18):
    rng = np.random.default_rng(seed)
    per = n_bytes // 24 // 61 * 60
    with open(path, "wb") as fp:
        for r in range(24):
            fp.write(b">chr%d synthetic\n" % (r + 1))
            lines = np.empty((per // 60, 61), dtype=np.uint8)
            lines[:, :60] = ACGT[rng.integers(0, 4, per, dtype=np.uint8)].reshape(-1, 60)
            lines[:, 60] = ord("\n")
            lines.tofile(fp)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


med = lambda v: round(statistics.median(v), 5)
span = lambda v: [round(min(v), 5), round(max(v), 5)]
d = tempfile.mkdtemp(prefix="coral_fastq_")
fq, fa, kept_path = os.path.join(d, "reads.fastq"), os.path.join(d, "genome.fa"), os.path.join(d, "kept.fastq")
t0 = time.perf_counter()
n_reads = write_fastq(fq, args.bytes)
write_fasta(fa, os.path.getsize(fq))
line = {"tool": "bench_fastq_qc", "runs": args.runs, "reads": n_reads, "fastq_MB": round(os.path.getsize(fq) / 1e6, 1), "fasta_MB": round(os.path.getsize(fa) / 1e6, 1),
        "chunk_bytes": args.chunk_bytes, "generate_s": round(time.perf_counter() - t0, 1)}

qc_gpu = lambda: fastq.read_qc(fq, device=dev, chunk_bytes=args.chunk_bytes)
comp_gpu = lambda: composition.reference_composition(fa, 1000, device=dev, chunk_bytes=args.chunk_bytes)
filter_gpu = lambda: fastq.read_qc(fq, device=dev, chunk_bytes=args.chunk_bytes, min_length=18_000, min_mean_quality=15.0, output=kept_path)

timed(qc_gpu)                                                             # warm-up: code objects, the page cache, the allocator
timed(comp_gpu)
qc_wall, comp_wall, qc_stages, comp_stages = [], [], [], []
for run in range(args.runs):
    qc, w = timed(qc_gpu)
    qc_wall.append(w)
    qc_stages.append(dict(fastq.LAST_FASTQ_QC))
    _, w2 = timed(comp_gpu)
    comp_wall.append(w2)
    comp_stages.append(dict(composition.LAST_COMPOSITION))
    print("bench_fastq_qc: pair %d: fastq_qc %.3f s, composition %.3f s" % (run, w, w2), file=sys.stderr, flush=True)
size = os.path.getsize(fq)
line.update({"records": qc.n_records, "bases": qc.total_bases, "fastq_qc_wall_s": med(qc_wall), "fastq_qc_wall_min_max": span(qc_wall), "fastq_qc_walls": [round(w, 4) for w in qc_wall],
             "fastq_qc_stage_s": {k: med([s[k] for s in qc_stages]) for k in qc_stages[0]}, "fastq_qc_GB_per_s": round(size / statistics.median(qc_wall) / 1e9, 2),
             "composition_wall_s": med(comp_wall), "composition_wall_min_max": span(comp_wall), "composition_walls": [round(w, 4) for w in comp_wall],
             "composition_stage_s": {k: med([s[k] for s in comp_stages]) for k in comp_stages[0]},
             "fastq_qc_over_composition": round(statistics.median(qc_wall) / statistics.median(comp_wall), 3)})
cs = line["composition_stage_s"]
line["composition_other_s"] = round(cs["wall"] - cs["read"] - cs["feed"] - cs["finish_wait"] - cs["download"], 5)      # its workspace, pinned buffers and session
line["kernels_below_uploads"] = bool(line["fastq_qc_stage_s"]["scan_walk"] + line["fastq_qc_stage_s"]["accumulate"] < line["fastq_qc_stage_s"]["upload"])
line["pairs_within_compositions_range"] = [bool(w <= max(comp_wall)) for w in qc_wall]


def plain_read(path):
    """The file's pieces read and dropped: what `read` costs without a session."""
    it, spent = fasta_stream.pieces(path, args.chunk_bytes)
    for _ in it:
        pass
    return spent[0]


line["plain_read_s"] = {"fastq": med([plain_read(fq) for _ in range(3)]), "fasta": med([plain_read(fa) for _ in range(3)])}
timed(filter_gpu)
flt_wall, flt_stages = [], []
for run in range(args.runs):
    flt, w = timed(filter_gpu)
    flt_wall.append(w)
    flt_stages.append(dict(fastq.LAST_FASTQ_QC))
line.update({"filter_wall_s": med(flt_wall), "filter_wall_min_max": span(flt_wall), "filter_stage_s": {k: med([s[k] for s in flt_stages]) for k in flt_stages[0]},
             "filter_kept_records": flt.n_kept, "filter_kept_MB": round(os.path.getsize(kept_path) / 1e6, 1)})
if not args.no_host:
    t1 = time.perf_counter()
    host = fastq.read_qc(fq, device="cpu", chunk_bytes=args.chunk_bytes)
    line["host_wall_s"] = round(time.perf_counter() - t1, 3)
    line["host_stage_s"] = {k: round(v, 4) for k, v in fastq.LAST_FASTQ_QC.items()}
    assert host.counters == qc.counters and all(np.array_equal(a, b) for a, b in ((host.length, qc.length), (host.qual_sum, qc.qual_sum), (host.base_quality_hist, qc.base_quality_hist)))
    line["equals_host"] = True
    line["host_over_gpu"] = round(line["host_wall_s"] / statistics.median(qc_wall), 2)
for p in (fq, fa, kept_path):
    os.remove(p)
os.rmdir(d)
print(json.dumps(line))
