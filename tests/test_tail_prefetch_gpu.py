"""The tail prefetch on the device: ``tiny_edge`` and ``cfg3_2amp`` built with the candidates behind the search asked for ahead
(look-ahead threads forced with ``CORAL_SEARCH_MIN_READS=0``) and with ``CORAL_TAIL_PREFETCH=0`` — equal containers and equal
graph files, the library's counters show which path ran — and smoke() under both settings."""
import glob
import json
import os

import pytest

from coral_amd import synth
from tests.canon import canon, graph_snapshot

pytestmark = pytest.mark.gpu


def _build(name, rec, cfg, tmp_path, tag):
    from coral_amd import infer_breakpoint_graph as ibg
    from coral_amd.records import DeviceRecords
    d = tmp_path / ("%s_%s" % (name, tag))
    d.mkdir()
    cn, seeds = str(d / "cn.bed"), str(d / "seeds.bed")
    synth.write_cn_bed(cfg, cn)
    synth.write_seed_bed(cfg, seeds)
    b = ibg.build_graph_from_records(DeviceRecords(rec, "cuda:0"), seeds, cn, str(d / "out"))
    assert b.rec.device.type == "cuda"
    files = {}
    for path in sorted(glob.glob(str(d / "out_amplicon*_graph.txt"))):
        with open(path, "rb") as fp:
            files[os.path.basename(path)] = fp.read().decode()
    snap = dict(intervals=canon(b.amplicon_intervals), bps=canon(b.new_bp_list), stats=canon(b.new_bp_stats), ccids=canon(b.new_bp_ccids),
                conn=canon(b.amplicon_interval_connections), indels=canon(dict(b.large_indel_alignments)), ccid2id=canon(b.ccid2id),
                graphs=[graph_snapshot(g) for g in b.lr_graph], files=files)
    return snap, b._search_ctx.tail_stats(), b._search_ctx.stats()


@pytest.mark.parametrize("name", ["tiny_edge", "cfg3_2amp"])
def test_prefetched_and_numpy_tails_agree_on_the_device(name, tmp_path, monkeypatch):
    monkeypatch.setenv("CORAL_SEARCH_MIN_READS", "0")
    cfg, rec = synth.dataset(name, "cpu")
    monkeypatch.setenv("CORAL_TAIL_PREFETCH", "0")
    want, st_off, _ = _build(name, rec, cfg, tmp_path, "off")
    assert st_off == dict(queued=0, served=0, on_demand=0, served_by_caller=0), st_off
    monkeypatch.delenv("CORAL_TAIL_PREFETCH")
    got, st_on, st = _build(name, rec, cfg, tmp_path, "on")
    assert st["workers"] >= 1 and st_on["queued"] == 2 and st_on["served"] == 2 and st_on["on_demand"] == 0, (st, st_on)
    assert len(want["bps"]) > 0 and len(want["files"]) > 0
    assert want.keys() == got.keys()
    for k in want:
        assert json.dumps(got[k]) == json.dumps(want[k]), (name, k)


def test_smoke_with_and_without_the_prefetch(monkeypatch, capsys):
    import __graft_entry__ as entry
    monkeypatch.setenv("CORAL_SEARCH_MIN_READS", "0")
    for flag in ("1", "0"):
        monkeypatch.setenv("CORAL_TAIL_PREFETCH", flag)
        entry.smoke()                                     # (asserts the device graph against the CPU oracle)
    assert capsys.readouterr().out.count("smoke ok") == 2
