"""Rank body of the gloo tests: sharded graph build.  Default (CPU): oracle-backed local kernels.  With ``--device cuda:0``:
the real HIP kernels, every rank on that one device, and for the BAM leg the GPU byte-range decoder.

usage: _shard_worker.py CASE OUTDIR [BAM] [--device DEV]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Patch:
    def setattr(self, obj, name, val):
        setattr(obj, name, val)


def main():
    import torch
    import torch.distributed as dist
    args = sys.argv[1:]
    device = "cpu"
    if "--device" in args:
        k = args.index("--device")
        device = args[k + 1]
        del args[k:k + 2]
    case, outdir = args[0], args[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from coral_amd import sharding, synth
    from coral_amd.breakpoint_graph import graph_text
    from tests.product_check import install_cpu_kernel_fakes
    if device == "cpu":
        install_cpu_kernel_fakes(_Patch())
    cfg, rec = synth.dataset(case, "cpu")
    cn, seeds = os.path.join(outdir, "cn%d.bed" % rank), os.path.join(outdir, "seeds%d.bed" % rank)
    synth.write_cn_bed(cfg, cn)
    synth.write_seed_bed(cfg, seeds)
    if len(args) > 2:          # per-rank input: every rank decodes only its byte range of the BAM written by the test
        dr = sharding.load_bam_sharded(args[2], rank, world, device, n_threads=2)
        assert dr.has_host == (rank == 0)
        if rank == 0:           # unified read-name ids = first appearance over the whole file, as a one-process decode numbers them
            want = rec.materialise_names()
            ids = rec.name_id.tolist()
            assert [dr.names[i] for i in dr.h_name_id.tolist()] == [want[i] for i in ids]
            first_seen = list(dict.fromkeys(want[i] for i in ids))
            assert dr.names == first_seen
    else:
        dr = sharding.shard_records(rec, rank, world, device)
    if world == 1:             # the unsharded run the GPU tests compare with
        assert dr.n == dr.n_total
    elif world <= 3:
        assert 0 < dr.n < dr.n_total
    else:                      # many ranks on a small file: a byte range may hold no record start at all
        assert 0 <= dr.n < dr.n_total
    b = sharding.build_graph_sharded(dr, seeds, cn, os.path.join(outdir, "sh") if rank == 0 else None)
    if rank == 0:
        files = {"out_amplicon%d_graph.txt" % (i + 1): graph_text(g) for i, g in enumerate(b.lr_graph)}
        with open(os.path.join(outdir, "result.json"), "w") as fp:
            json.dump({"files": files, "normal_cov": b.normal_cov, "shard": [dr.lo, dr.hi, dr.n_total], "world": world,
                       "large_indel": len(b.large_indel_alignments)}, fp)
    else:
        assert b is None
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
