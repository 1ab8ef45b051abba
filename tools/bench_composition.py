"""Cost of the reference's per-bin composition (composition.reference_composition: k_comp_* of coral_comp.hip against the host
backend) beside kmers.count_kmers on the same file - the rate at which the machine streams a FASTA to the device -, and of
cnv.segment_depth with and without a composition.

Generates a synthetic genome under the temporary directory as tools/bench_kmers.py does (none is shipped and none is fetched):
`--bases` (default 1 Gb) seeded random bases in 24 records of 60-column lines, 5 % of them planted repeats (lower case, as a
soft-masked assembly has them) and N blocks.  Times, after one warm-up of each, `runs` alternating pairs:
  composition   reference_composition on cuda:0: wall time and the call's own stage times (composition.LAST_COMPOSITION: reading
                the file, the feed calls, and from HIP events the uploads, ordinals + contigs, the count kernel)
  kmers         count_kmers(k = 15) on cuda:0 on the same file: wall time
  host          reference_composition with device "cpu" (one thread; a reference, not the code under test), once; the tables
                must equal the GPU's
  segment       cnv.segment_depth on `--bins` (default 3.1 M) bins of synthetic depth with a GC wave, with and without the
                composition, alternating: the total and the `gc` stage of cnv.LAST_SEGMENT
One JSON line.
    python tools/bench_composition.py [runs] [--bases N] [--bin_size N] [--bins N] [--chunk_bytes N] [--no_kmers] [--no_host]"""
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

from coral_amd import bam, cnv, composition, kmers

ap = argparse.ArgumentParser()
ap.add_argument("runs", nargs="?", type=int, default=5)
ap.add_argument("--bases", type=int, default=1_000_000_000)
ap.add_argument("--bin_size", type=int, default=1000)
ap.add_argument("--bins", type=int, default=3_100_000)
ap.add_argument("--chunk_bytes", type=int, default=64 << 20)
ap.add_argument("--no_kmers", action="store_true")
ap.add_argument("--no_host", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_composition.py measures on a GPU"
dev = "cuda:0"
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def write_genome(path, n_bases, seed=15):
    rng = np.random.default_rng(seed)
    elements = [ACGT[rng.integers(0, 4, int(n))] for n in (300, 1200, 6000)]
    per = n_bases // 24
    with open(path, "wb") as fp:
        for r in range(24):
            seq = ACGT[rng.integers(0, 4, per, dtype=np.uint8)]
            budget = per // 20                                       # 5 % of the record
            while budget > 0:
                kind = int(rng.integers(0, 4))
                at = int(rng.integers(0, per - 20000))
                if kind == 0:                                        # tandem repeat
                    piece = np.tile(ACGT[rng.integers(0, 4, int(rng.integers(2, 61)))], int(rng.integers(5, 200)))[:10000] | 0x20
                elif kind == 1:                                      # interspersed element
                    piece = elements[int(rng.integers(0, 3))] | 0x20
                elif kind == 2:                                      # homopolymer
                    piece = np.full(int(rng.integers(10, 80)), ACGT[int(rng.integers(0, 4))], dtype=np.uint8)
                else:                                                # N block
                    piece = np.full(int(rng.integers(1, 5000)), ord("N"), dtype=np.uint8)
                seq[at:at + len(piece)] = piece
                budget -= len(piece)
            fp.write(b">chr%d synthetic\n" % (r + 1))
            whole = per // 60 * 60
            lines = np.empty((whole // 60, 61), dtype=np.uint8)
            lines[:, :60] = seq[:whole].reshape(-1, 60)
            lines[:, 60] = ord("\n")
            lines.tofile(fp)
            if per > whole:
                fp.write(seq[whole:].tobytes() + b"\n")
            print("bench_composition: record %d of 24 written" % (r + 1), file=sys.stderr, flush=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


med = lambda v: round(statistics.median(v), 5)
span = lambda v: [round(min(v), 5), round(max(v), 5)]
d = tempfile.mkdtemp(prefix="coral_comp_")
fasta = os.path.join(d, "genome.fa")
t0 = time.perf_counter()
write_genome(fasta, args.bases)
line = {"tool": "bench_composition", "runs": args.runs, "bases": args.bases, "bin_size": args.bin_size, "file_MB": round(os.path.getsize(fasta) / 1e6, 1),
        "chunk_bytes": args.chunk_bytes, "generate_s": round(time.perf_counter() - t0, 1)}

comp_gpu = lambda: composition.reference_composition(fasta, args.bin_size, device=dev, chunk_bytes=args.chunk_bytes)


def kmers_gpu():
    kc = kmers.count_kmers(fasta, 15, device=dev, chunk_bytes=args.chunk_bytes)
    kc.close()


comp, _ = timed(comp_gpu)                                            # warm-up: code objects, the page cache, the allocator
if not args.no_kmers:
    timed(kmers_gpu)
comp_wall, kmer_wall, stages = [], [], []
for run in range(args.runs):
    comp, w = timed(comp_gpu)
    comp_wall.append(w)
    stages.append(dict(composition.LAST_COMPOSITION))
    if not args.no_kmers:
        kmer_wall.append(timed(kmers_gpu)[1])
    print("bench_composition: pair %d: composition %.3f s, kmers %s s" % (run, w, "%.3f" % kmer_wall[-1] if kmer_wall else "-"), file=sys.stderr, flush=True)
line.update(comp.totals)
line.update({"composition_wall_s": med(comp_wall), "composition_wall_min_max": span(comp_wall), "composition_stage_s": {k: med([s[k] for s in stages]) for k in stages[0]},
             "composition_GB_per_s": round(os.path.getsize(fasta) / statistics.median(comp_wall) / 1e9, 2)})
if kmer_wall:
    line.update({"kmers_wall_s": med(kmer_wall), "kmers_wall_min_max": span(kmer_wall), "composition_over_kmers": round(statistics.median(comp_wall) / statistics.median(kmer_wall), 3)})
if not args.no_host:
    t1 = time.perf_counter()
    host = composition.reference_composition(fasta, args.bin_size, device="cpu", chunk_bytes=args.chunk_bytes)
    line["host_wall_s"] = round(time.perf_counter() - t1, 3)
    line["host_stage_s"] = {k: round(v, 4) for k, v in composition.LAST_COMPOSITION.items()}
    assert host.chroms == comp.chroms and host.lengths == comp.lengths and all(np.array_equal(a, b) for a, b in ((host.gc, comp.gc), (host.at, comp.at), (host.masked, comp.masked)))
    line["equals_host"] = True
    line["host_over_gpu"] = round(line["host_wall_s"] / statistics.median(comp_wall), 2)
    del host
os.remove(fasta)
os.rmdir(d)

# ---- the segmenter with and without a composition ----------------------------------------------------------------------------
rng = np.random.default_rng(4)
n = args.bins
per = [n // 24] * 23 + [n - 23 * (n // 24)]
chroms, lengths = ["chr%d" % (k + 1) for k in range(24)], [m * 1000 for m in per]
frac = np.clip(0.41 + 0.07 * np.sin(np.arange(n) / 211.0) + rng.normal(0, 0.03, n), 0.05, 0.95)
called = np.full(n, 1000, dtype=np.int64)
called[rng.integers(0, n, n // 100)] = 0
gc = (called * frac).astype(np.uint32)
at = (called - gc).astype(np.uint32)
mean = np.full(n, 30_000.0) * (1.0 + 0.3 * np.sin(7.0 * frac))
for a in rng.integers(0, n - 5000, 60):
    mean[a:a + int(rng.integers(20, 5000))] *= float(rng.choice([0.5, 1.5, 2.0, 4.0]))
off = np.concatenate([[0], np.cumsum(per)])
depth = bam.BinnedDepth(chroms, lengths, 1000, 0, 0x704, True, off, rng.poisson(mean).astype(np.int64), np.zeros(n, dtype=np.int64))
table = composition.Composition(chroms, lengths, 1000, gc, at, np.zeros(n, dtype=np.uint32))
plain_s, gc_s, gc_stage = [], [], []
cnv.segment_depth(depth, device=dev)
cnv.segment_depth(depth, device=dev, composition=table)
for run in range(args.runs):
    _, w = timed(lambda: cnv.segment_depth(depth, device=dev))
    plain_s.append((w, sum(v for k, v in cnv.LAST_SEGMENT.items() if k != "workspace_bytes")))
    seg, w = timed(lambda: cnv.segment_depth(depth, device=dev, composition=table))
    gc_s.append((w, sum(v for k, v in cnv.LAST_SEGMENT.items() if k != "workspace_bytes")))
    gc_stage.append(cnv.LAST_SEGMENT["gc"])
line.update({"segment_bins": n, "segment_wall_s": med([w for w, _ in plain_s]), "segment_stages_s": med([s for _, s in plain_s]),
             "segment_gc_wall_s": med([w for w, _ in gc_s]), "segment_gc_stages_s": med([s for _, s in gc_s]), "segment_gc_stage_s": med(gc_stage),
             "segment_gc_stage_min_max": span(gc_stage), "segment_gc_rows": len(seg), "segment_gc_uncalled": seg.counts["uncalled"]})
print(json.dumps(line))
