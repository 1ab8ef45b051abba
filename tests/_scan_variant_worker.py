"""Child process of tests/test_gpu_kernel_geometry.py: ONE coral_cigar_scan launch with the tuning overrides of the environment
(CORAL_SCAN_RING / CORAL_SCAN_GROUP / CORAL_SCAN_WG_PER_CU are read once per process, so every variant needs a fresh process).

usage: _scan_variant_worker.py N_REC SEED OUT.npz
Writes the summary rows, ALL gap rows (unsorted, as the kernel left them) and both counter words."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

M, I, D, N, S, H, P, EQ, X = range(9)
MIN_GAP, MIN_MAPQ = 600, 20
GAP_LENGTHS = [1, 2, 149, 150, 151, 299, 300, 301, 302, 599, 600, 601, 1200]      # around min_gap / 2 and min_gap


def variant_alignments(n_rec: int, seed: int):
    """``n_rec`` alignments, the same for the same arguments: mostly 1 .. 8 ops; records without any op at both ends of the file
    and in runs; for every k in 1 .. 13 one record each of 256 k - 1, 256 k and 256 k + 1 ops (with a group of one record: groups
    of k chunks, one quad less and one more - every ring size and its neighbours); D / N runs whose sums sit around min_gap / 2
    and min_gap; a share of MAPQ-19 records, which report no gap."""
    rng = np.random.default_rng(seed)
    long_ops = [256 * k + d for k in range(1, 14) for d in (-1, 0, 1)]
    assert n_rec >= 20 * len(long_ops)
    long_at = {int(r): n for r, n in zip(np.sort(rng.choice(np.arange(10, n_rec - 10), len(long_ops), replace=False)), rng.permutation(long_ops))}
    empty = set(range(3)) | set(range(n_rec - 4, n_rec))
    for a in rng.choice(np.arange(10, n_rec - 20), 12, replace=False):
        empty |= set(range(int(a), int(a) + int(rng.integers(1, 7))))
    alns, pos = [], 100

    def ops_of(n_ops):
        ops = []
        while len(ops) < n_ops:
            kind = rng.random()
            if kind < 0.6:
                ops.append((int(rng.choice([M, EQ, X])), int(rng.integers(1, 40))))
            elif kind < 0.8:
                ops.append((int(rng.choice([D, N])), int(rng.choice(GAP_LENGTHS))))
            elif kind < 0.92:
                ops.append((int(rng.choice([I, P, S])), int(rng.integers(0, 6))))
            else:                                   # a run of non-aligned ops: their D / N lengths add up to one gap
                for _ in range(int(rng.integers(2, 10))):
                    ops.append((int(rng.choice([D, N, I, P])), int(rng.choice([1, 100, 150, 200, 299, 300, 301, 602]))))
        return ops[:n_ops]
    for r in range(n_rec):
        mapq = int(rng.choice([60, 60, 60, 19]))
        if r in long_at:
            alns.append(dict(tid=0, pos=pos, cigar=ops_of(long_at[r]), mapq=mapq, name="v%d" % r))
        elif r in empty:
            alns.append(dict(tid=0, pos=pos, cigar=[], flag=4, has_seq=1, qlen=30, name="v%d" % r))
        else:
            alns.append(dict(tid=0, pos=pos, cigar=ops_of(int(rng.integers(1, 9))), mapq=mapq, name="v%d" % r))
        pos += int(rng.integers(0, 40))
    return alns


def main():
    import ctypes as C
    import torch
    from coral_amd import _lib, synth
    from coral_amd.records import DeviceRecords
    n_rec, seed, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    rec = synth.records_from_alignments(variant_alignments(n_rec, seed))
    dr = DeviceRecords(rec, "cuda:0")
    cap = int(rec.n_cigar.sum()) + 1                 # a gap row belongs to one op: room for every row there can be
    summary = torch.empty((dr.n, 4), dtype=torch.int32, device=dr.device)
    gaps = torch.empty((cap, 4), dtype=torch.int32, device=dr.device)
    cnt = torch.zeros(2, dtype=torch.int32, device=dr.device)
    rs = dr.c_struct()
    _lib.check(_lib.lib().coral_cigar_scan(C.byref(rs), MIN_GAP, MIN_MAPQ, summary.data_ptr(), gaps.data_ptr(), cnt.data_ptr(), cap,
                                           dr.stream()), "coral_cigar_scan")
    torch.cuda.synchronize()
    counters = cnt.cpu().numpy().view(np.uint32)
    assert int(counters[0]) <= cap
    np.savez(out, summary=summary.cpu().numpy(), gaps=gaps[:int(counters[0])].cpu().numpy(), counters=counters)
    print("scan variant ok: ring=%s group=%s wg_per_cu=%s n_rec=%d gap rows=%d cursor=%d" % (
        os.environ.get("CORAL_SCAN_RING"), os.environ.get("CORAL_SCAN_GROUP"), os.environ.get("CORAL_SCAN_WG_PER_CU"), n_rec,
        int(counters[0]), int(counters[1])))


if __name__ == "__main__":
    main()
