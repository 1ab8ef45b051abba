"""Cost of the k-mer counter (kmers.count_kmers: k_kmer_* of coral_kmer.hip against the host backend) and of the `kmers` mode's two
steps, count and write, at k = 15.

Generates a synthetic genome under the temporary directory (none is shipped and none is fetched): `--bases` (default 1 Gb) seeded
random bases in 24 records of 60-column lines, 5 % of them planted repeats - tandem repeats of 2..60-base units, copies of a few
interspersed elements of 300 b..6 kb, homopolymer runs - and N blocks.  Times, median of `runs` after one warm-up:
  gpu     count_kmers on cuda:0, wall time, and the call's own stage times (kmers.LAST_COUNT: reading the file, the feed calls,
          and from HIP events the uploads, classify + compact, the count kernel, the statistics pass), then threshold, select, write
  host    count_kmers with device "cpu" on the same file (one thread; a reference, not the code under test), `--host_runs` times
and checks that both give the same statistics, histogram and selected k-mers.  One JSON line.
    python tools/bench_kmers.py [runs] [--bases N] [--k K] [--host_runs N] [--chunk_bytes N] [--keep FILE]"""
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

from coral_amd import kmers

ap = argparse.ArgumentParser()
ap.add_argument("runs", nargs="?", type=int, default=5)
ap.add_argument("--bases", type=int, default=1_000_000_000)
ap.add_argument("--k", type=int, default=15)
ap.add_argument("--host_runs", type=int, default=1)
ap.add_argument("--chunk_bytes", type=int, default=64 << 20)
ap.add_argument("--keep", help="write the genome here and leave it")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_kmers.py measures on a GPU"
dev = "cuda:0"
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def write_genome(path, n_bases, seed=15):
    rng = np.random.default_rng(seed)
    elements = [ACGT[rng.integers(0, 4, int(n))] for n in (300, 1200, 6000)]
    per = n_bases // 24
    planted = 0
    with open(path, "wb") as fp:
        for r in range(24):
            seq = ACGT[rng.integers(0, 4, per, dtype=np.uint8)]
            budget, at = per // 20, 0                               # 5 % of the record
            while budget > 0:
                kind = int(rng.integers(0, 4))
                at = int(rng.integers(0, per - 20000))
                if kind == 0:                                        # tandem repeat
                    unit = ACGT[rng.integers(0, 4, int(rng.integers(2, 61)))]
                    piece = np.tile(unit, int(rng.integers(5, 200)))[:10000]
                elif kind == 1:                                      # interspersed element
                    piece = elements[int(rng.integers(0, 3))]
                elif kind == 2:                                      # homopolymer
                    piece = np.full(int(rng.integers(10, 80)), ACGT[int(rng.integers(0, 4))], dtype=np.uint8)
                else:                                                # N block
                    piece = np.full(int(rng.integers(1, 5000)), ord("N"), dtype=np.uint8)
                seq[at:at + len(piece)] = piece
                budget -= len(piece)
                planted += len(piece)
            fp.write(b">chr%d synthetic\n" % (r + 1))
            whole = per // 60 * 60
            lines = np.empty((whole // 60, 61), dtype=np.uint8)
            lines[:, :60] = seq[:whole].reshape(-1, 60)
            lines[:, 60] = ord("\n")
            lines.tofile(fp)
            if per > whole:
                fp.write(seq[whole:].tobytes() + b"\n")
            print("bench_kmers: record %d of 24 written" % (r + 1), file=sys.stderr, flush=True)
    return planted


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def answers(kc, t):
    values, nums = kc.histogram()
    sel = kc.select(t)
    return (kc.n_sequences, kc.n_bases, kc.total, kc.distinct, kc.max_count, values.tolist(), nums.tolist(), sel[0].tolist(), sel[1].tolist())


d = tempfile.mkdtemp(prefix="coral_kmers_")
fasta = args.keep or os.path.join(d, "genome.fa")
t0 = time.perf_counter()
planted = write_genome(fasta, args.bases)
line = {"tool": "bench_kmers", "runs": args.runs, "k": args.k, "bases": args.bases, "planted_bases": planted, "file_MB": round(os.path.getsize(fasta) / 1e6, 1),
        "chunk_bytes": args.chunk_bytes, "generate_s": round(time.perf_counter() - t0, 1)}
out_txt = os.path.join(d, "repetitive.txt")

kc, _ = timed(lambda: kmers.count_kmers(fasta, args.k, device=dev, chunk_bytes=args.chunk_bytes))      # warm-up: code objects, the page cache, the allocator
kc.close()
del kc
wall, stages = [], []
for run in range(args.runs):
    kc, w = timed(lambda: kmers.count_kmers(fasta, args.k, device=dev, chunk_bytes=args.chunk_bytes))
    wall.append(w)
    stage = dict(kmers.LAST_COUNT)
    t1 = time.perf_counter()
    t = kc.threshold("0.9998")
    stage["threshold"] = time.perf_counter() - t1
    lines = kc.write(out_txt, greater_than=t)
    stage["select"], stage["write"] = kmers.LAST_COUNT["select"], kmers.LAST_COUNT["write"]
    stages.append(stage)
    gpu_answers = answers(kc, t) if run == args.runs - 1 else None
    stats = dict(n_sequences=kc.n_sequences, n_bases=kc.n_bases, total=kc.total, distinct=kc.distinct, max_count=kc.max_count, threshold=t, lines=lines)
    kc.close()
    del kc
    print("bench_kmers: gpu run %d: %.3f s" % (run, w), file=sys.stderr, flush=True)
med = lambda v: round(statistics.median(v), 5)
count_s = statistics.median([s["count"] for s in stages])
line.update(stats)
line.update({"gpu_wall_s": med(wall), "gpu_wall_min_max": [round(min(wall), 5), round(max(wall), 5)],
             "gpu_stage_s": {k: med([s[k] for s in stages]) for k in stages[0]},
             "gpu_stage_min_max": {k: [round(min(s[k] for s in stages), 5), round(max(s[k] for s in stages), 5)] for k in ("upload", "classify_compact", "count", "statistics")},
             "count_G_kmers_per_s": round(stats["total"] / count_s / 1e9, 2), "guide_scattered_f32_G_adds_per_s": 20.0})
host_wall = []
for _ in range(args.host_runs):
    t1 = time.perf_counter()
    hc = kmers.count_kmers(fasta, args.k, device="cpu", chunk_bytes=args.chunk_bytes)
    host_wall.append(time.perf_counter() - t1)
    line["host_stage_s"] = {k: round(v, 4) for k, v in kmers.LAST_COUNT.items()}
    assert answers(hc, stats["threshold"]) == gpu_answers, "the GPU count differs from the host backend's"
    line["equals_host"] = True
    hc.close()
    del hc
if host_wall:
    line.update({"host_wall_s": med(host_wall), "host_over_gpu": round(statistics.median(host_wall) / statistics.median(wall), 2)})
if not args.keep:
    os.remove(fasta)
if os.path.exists(out_txt):
    os.remove(out_txt)
os.rmdir(d)
print(json.dumps(line))
