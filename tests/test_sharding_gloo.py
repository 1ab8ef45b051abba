"""N > 1 path on CPU: two gloo ranks, records split in two, exchange = all-gather-v of candidate rows + all-reduce
of the per-segment sums.  The merged result must equal the reference golden (== the unsharded result)."""
import json
import os
import signal
import socket
import subprocess
import sys

import pytest

from tests.product_check import compare_graph_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(world, case, tmp_path, extra=()):
    port = _free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ, PYTHONHASHSEED="0", RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="2" if world <= 3 else "1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_shard_worker.py"), case, str(tmp_path)] + list(extra),
                                      env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]


@pytest.mark.parametrize("case,world", [("tiny_edge", 2), ("small", 3), ("small", 8)])
def test_per_rank_bam_decode_equals_reference(case, world, golden_dir, tmp_path):
    """The input side of the N > 1 path: the test writes a BAM, every rank decodes only ITS byte range of it and keeps only
    that shard; rank 0 gets the gathered per-record host fields with unified read-name ids.  Same golden as everywhere."""
    from coral_amd import bam, synth
    cfg, rec = synth.dataset(case, "cpu")
    path = str(tmp_path / "input.bam")
    bam.write_bam_native(rec, path, seed=7, n_threads=2)
    _run_ranks(world, case, tmp_path, extra=[path])
    with open(os.path.join(golden_dir, "e2e_%s.json" % case)) as fp:
        gold = json.load(fp)
    with open(tmp_path / "result.json") as fp:
        res = json.load(fp)
    assert res["normal_cov"] == gold["A2"]["normal_cov"]
    assert 0 < res["shard"][1] < res["shard"][2] == gold["n_records"] and res["world"] == world
    assert sorted(res["files"]) == sorted(gold["files"])
    for k in res["files"]:
        compare_graph_text(res["files"][k], gold["files"][k])


@pytest.mark.parametrize("case,world", [("tiny_edge", 2), ("small", 2), ("small", 8)])
def test_shard_merge_equals_reference(case, world, golden_dir, tmp_path):
    """Records already in memory, split over `world` ranks by CIGAR-op count (world 8 = one node's worth of ranks)."""
    _run_ranks(world, case, tmp_path)
    with open(os.path.join(golden_dir, "e2e_%s.json" % case)) as fp:
        gold = json.load(fp)
    with open(tmp_path / "result.json") as fp:
        res = json.load(fp)
    assert res["normal_cov"] == gold["A2"]["normal_cov"]
    assert 0 < res["shard"][1] < res["shard"][2]
    assert sorted(res["files"]) == sorted(gold["files"])
    for k in res["files"]:
        compare_graph_text(res["files"][k], gold["files"][k])
        assert open(str(tmp_path / ("sh" + k[3:]))).read() == res["files"][k]


@pytest.mark.gpu
def test_rccl_arms_at_world_one():
    """The RCCL arms of the exchange helpers (device tensors, backend "nccl") run — in the only RCCL world one GPU can form."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_rccl_world1.py")], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rccl world-1 ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the same runs with the real HIP kernels: gloo, every rank on cuda:0 -----------------------------------------------
_FATAL = (134, 139, 124, 137, -6, -11)       # abort, segfault, time limit: nothing more may start on the GPU in this session


def _stop_rank(p):
    """End a rank and everything it started.  ``p`` is the ``timeout`` wrapper, which cannot pass SIGKILL on to the rank: the
    whole process group goes (each rank is started as the leader of a session of its own), then the wrapper is reaped."""
    try:
        os.killpg(p.pid, signal.SIGKILL)
    except ProcessLookupError:
        pass
    p.wait()


def _run_ranks_gpu(world, case, outdir, extra=()):
    """One rank per process, all on cuda:0, each under its own time limit; the ranks are polled and the first that exits
    non-zero stops the others.  A crash or a time limit ends the whole session (pytest.exit)."""
    import time
    os.makedirs(str(outdir), exist_ok=True)
    port = _free_port()
    procs, logs = [], []
    failed = None
    try:
        for rank in range(world):
            env = dict(os.environ, PYTHONHASHSEED="0", RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), OMP_NUM_THREADS="2")
            log = open(os.path.join(str(outdir), "rank%d.log" % rank), "w")
            logs.append(log)
            procs.append(subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tests", "_shard_worker.py"),
                                           case, str(outdir)] + list(extra) + ["--device", "cuda:0"],
                                          env=env, cwd=ROOT, stdout=log, stderr=subprocess.STDOUT, start_new_session=True))
        while failed is None and any(p.poll() is None for p in procs):
            failed = next((p for p in procs if p.poll() not in (None, 0)), None)
            time.sleep(0.2)
        failed = failed or next((p for p in procs if p.returncode != 0), None)
    finally:
        if failed is not None or any(p.poll() is None for p in procs):      # a failure, or the test itself was interrupted
            for p in procs:
                _stop_rank(p)
    for log in logs:
        log.close()
    if failed is not None:
        tails = []
        for rank, p in enumerate(procs):
            with open(os.path.join(str(outdir), "rank%d.log" % rank)) as fp:
                tails.append("--- rank %d (exit %s)\n%s" % (rank, p.returncode, fp.read()[-3000:]))
        msg = "world %d %s: rank exited with %s\n%s" % (world, case, failed.returncode, "\n".join(tails))
        if failed.returncode in _FATAL:
            pytest.exit(msg, returncode=1)
        pytest.fail(msg)
    with open(os.path.join(str(outdir), "result.json")) as fp:
        return json.load(fp)


def _check_gpu_run(case, world, golden_dir, tmp_path, extra=()):
    """The sharded run meets the golden, and its graph files are byte-identical to a one-rank run of the same worker."""
    res = _run_ranks_gpu(world, case, tmp_path / ("w%d" % world), extra)
    with open(os.path.join(golden_dir, "e2e_%s.json" % case)) as fp:
        gold = json.load(fp)
    assert res["normal_cov"] == gold["A2"]["normal_cov"]
    assert 0 < res["shard"][1] < res["shard"][2] == gold["n_records"] and res["world"] == world
    assert sorted(res["files"]) == sorted(gold["files"])
    for k in res["files"]:
        compare_graph_text(res["files"][k], gold["files"][k])
        assert open(str(tmp_path / ("w%d" % world) / ("sh" + k[3:]))).read() == res["files"][k]
    one = _run_ranks_gpu(1, case, tmp_path / "w1", extra)
    assert one["world"] == 1 and one["normal_cov"] == res["normal_cov"] and one["large_indel"] == res["large_indel"]
    assert one["files"] == res["files"]
    for k in res["files"]:
        a, b = (open(str(tmp_path / d / ("sh" + k[3:])), "rb").read() for d in ("w%d" % world, "w1"))
        assert a == b, k


@pytest.mark.gpu
@pytest.mark.parametrize("case,world", [("tiny_edge", 2), ("small", 3)])
def test_shard_merge_real_kernels(case, world, golden_dir, tmp_path):
    """In-memory shards on cuda:0, real cigar_scan / segment_coverage / point_cover on every rank, exchange over gloo."""
    _check_gpu_run(case, world, golden_dir, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("case,world", [("tiny_edge", 2)])
def test_per_rank_bam_decode_real_kernels(case, world, golden_dir, tmp_path):
    """Every rank decodes its byte range of the BAM with the GPU decoder, then builds with the real kernels."""
    from coral_amd import bam, synth
    cfg, rec = synth.dataset(case, "cpu")
    path = str(tmp_path / "input.bam")
    bam.write_bam_native(rec, path, seed=7, n_threads=2)
    _check_gpu_run(case, world, golden_dir, tmp_path, extra=[path])
