"""The interval search exploring ahead, on the device: the smallest configuration of tests/test_gpu_e2e.py (the one of
tests/test_search_warm_gpu.py) built with ``CORAL_SEARCH_SPECULATE`` on and off in one process — the same graph
text, the same dumped tables, the same containers and the same number of steps queued by the caller; the speculation counters
are non-negative, consistent with each other, and zero when speculation is off."""
import json
import os

import numpy as np
import pytest

from coral_amd import synth
from tests.canon import canon, graph_snapshot

pytestmark = pytest.mark.gpu

SPEC_KEYS = ("spec_queued", "spec_asked", "spec_ready_when_asked", "spec_unused")


def _graph_text(out_dir):
    text = {}
    for name in sorted(os.listdir(out_dir)):
        with open(os.path.join(out_dir, name), "rb") as fp:
            text[name] = fp.read()
    return text


def test_builds_with_and_without_speculation_agree_on_the_device(tmp_path, monkeypatch):
    import bench
    from coral_amd import infer_breakpoint_graph as ibg
    from coral_amd.records import DeviceRecords
    monkeypatch.setenv("CORAL_SEARCH_MIN_READS", "0")
    cfg, rec = synth.dataset("tiny", "cpu")
    cn, seeds = str(tmp_path / "cn.bed"), str(tmp_path / "seeds.bed")
    synth.write_cn_bed(cfg, cn)
    synth.write_seed_bed(cfg, seeds)
    snaps, stats, texts, tables = {}, {}, {}, {}
    for mode in ("0", "1"):
        monkeypatch.setenv("CORAL_SEARCH_SPECULATE", mode)
        out = tmp_path / ("out" + mode)
        out.mkdir()
        b = ibg.build_graph_from_records(DeviceRecords(rec, "cuda:0"), seeds, cn, str(out / "g"))
        assert b.rec.device.type == "cuda"
        snaps[mode] = dict(intervals=canon(b.amplicon_intervals), bps=canon(b.new_bp_list), stats=canon(b.new_bp_stats),
                           ccids=canon(b.new_bp_ccids), conn=canon(b.amplicon_interval_connections), ccid2id=canon(b.ccid2id),
                           graphs=[graph_snapshot(g) for g in b.lr_graph])
        stats[mode] = b._search_ctx.stats()
        texts[mode] = _graph_text(str(out))
        bench.dump_outputs(b, str(tmp_path / ("tables" + mode)))
        tables[mode] = {n: np.load(str(tmp_path / ("tables" + mode) / n)) for n in sorted(os.listdir(str(tmp_path / ("tables" + mode))))}
    assert len(snaps["0"]["bps"]) > 0 and len(snaps["0"]["graphs"]) > 0 and len(texts["0"]) > 0
    off = stats["0"]
    assert off["workers"] >= 1 and off["queued"] >= 1 and all(off[k] == 0 for k in SPEC_KEYS), off
    for mode in ("1",):
        for k in snaps["0"]:
            assert json.dumps(snaps[mode][k]) == json.dumps(snaps["0"][k]), (mode, k)
        assert texts[mode] == texts["0"], "graph text, mode " + mode
        assert sorted(tables[mode]) == sorted(tables["0"]) and len(tables["0"]) > 0
        for name in tables["0"]:
            assert np.array_equal(tables[mode][name], tables["0"][name]), (mode, name)
        st = stats[mode]
        assert st["queued"] == off["queued"], (mode, st, off)
        assert all(st[k] >= 0 for k in SPEC_KEYS), st
        assert st["spec_asked"] <= st["spec_queued"] and st["spec_ready_when_asked"] <= st["spec_asked"], st
        assert st["spec_unused"] == st["spec_queued"] - st["spec_asked"], st
