"""The early search handle on the device: the smallest configuration of tests/test_gpu_e2e.py built twice in one process, with
the handle made beside the CIGAR scan (default) and with ``CORAL_SEARCH_EARLY=0`` — equal results, and the library's counters
show that the early path was taken: the pack was filled when attach began and the seeds' steps were queued before
coral_search_bfs started."""
import json

import pytest

from coral_amd import synth
from tests.canon import canon, graph_snapshot

pytestmark = pytest.mark.gpu


def test_early_and_late_handle_builds_agree_on_the_device(tmp_path, monkeypatch):
    from coral_amd import infer_breakpoint_graph as ibg
    from coral_amd.records import DeviceRecords
    monkeypatch.setenv("CORAL_SEARCH_MIN_READS", "0")
    cfg, rec = synth.dataset("tiny", "cpu")
    cn, seeds = str(tmp_path / "cn.bed"), str(tmp_path / "seeds.bed")
    synth.write_cn_bed(cfg, cn)
    synth.write_seed_bed(cfg, seeds)
    snaps, handles = {}, {}
    for early in ("1", "0"):
        monkeypatch.setenv("CORAL_SEARCH_EARLY", early)
        b = ibg.build_graph_from_records(DeviceRecords(rec, "cuda:0"), seeds, cn, None)
        assert b.rec.device.type == "cuda"
        snaps[early] = dict(intervals=canon(b.amplicon_intervals), bps=canon(b.new_bp_list), stats=canon(b.new_bp_stats),
                            ccids=canon(b.new_bp_ccids), conn=canon(b.amplicon_interval_connections), ccid2id=canon(b.ccid2id),
                            graphs=[graph_snapshot(g) for g in b.lr_graph])
        handles[early] = (b._search_ctx.early, b._search_ctx.stats())
    assert len(snaps["1"]["bps"]) > 0 and len(snaps["1"]["graphs"]) > 0
    for k in snaps["1"]:
        assert json.dumps(snaps["1"][k]) == json.dumps(snaps["0"][k]), k
    made_early, st = handles["1"]
    assert made_early and st["attached"] == 1 and st["fill_ready_at_attach"] == 1 and st["queued_before_bfs"] >= 1 and st["workers"] >= 1, st
    made_early, late = handles["0"]
    assert not made_early and late["queued_before_bfs"] == 0, late
    assert st["queued"] == late["queued"] >= 1, (st, late)       # the prefetched seeds are the steps the search asks for (one entry per key)
