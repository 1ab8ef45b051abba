"""`bench.py --dump-outputs DIR`: every column of the tables is the graph field it names, the tables hold exactly the graphs the
timed path built (same lines as its *_graph.txt files, same values as the oracle's graphs), a table set above the size cap is a
seeded, sorted sample under it, and a plain run times exactly --steps steps and leaves the --full measurements out of its line."""
import glob
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench():
    """bench.py as a module, without the thread-count defaults it exports at import staying in this process's environment."""
    before = set(os.environ)
    import bench
    for k in set(os.environ) - before:
        del os.environ[k]
    return bench


def graph_lines_from_tables(d):
    """The edge lines of *_graph.txt (breakpoint_graph.graph_text), rebuilt from the dumped tables, over all amplicons."""
    bench = _bench()
    from coral_amd.global_names import chr_idx
    chrom = {i: c for c, i in chr_idx.items()}
    o = lambda v: "+" if v > 0 else "-"
    t = {}
    for name, cols in bench.DUMP_COLUMNS.items():
        path = os.path.join(d, name + ".npy")
        if not os.path.exists(path):                  # a table without rows is not written
            t[name] = np.zeros((0, len(cols)))
            continue
        t[name] = np.load(path)
        assert t[name].dtype == np.float64 and t[name].ndim == 2 and t[name].shape[1] == len(cols), name
        assert len(t[name]), "%s.npy was written without rows" % name
    lines = []
    for _, c, s, e, _, lr, nc, size, cn in t["sequence_edges"]:
        lines.append("sequence\t%s:%d-\t%s:%d+\t%f\t%f\t%d\t%d" % (chrom[c], s, chrom[c], e, cn, nc / size, size, lr))
    for _, c, p, oo, _, _, _, _, cn in t["source_edges"]:
        lines.append("source\tsource:-1-->%s:%d%s\t%f\t-1" % (chrom[c], p, o(oo), cn))
    for _, c1, p1, o1, c2, p2, o2, _, lr, _, cn in t["concordant_edges"]:
        lines.append("concordant\t%s:%d%s->%s:%d%s\t%f\t%d" % (chrom[c1], p1, o(o1), chrom[c2], p2, o(o2), cn, lr))
    for _, c1, p1, o1, c2, p2, o2, _, _, lr, reads, cn in t["discordant_edges"]:
        assert reads == lr
        lines.append("discordant\t%s:%d%s->%s:%d%s\t%f\t%d" % (chrom[c1], p1, o(o1), chrom[c2], p2, o(o2), cn, lr))
    amp = t["amplicons"]
    assert sorted(amp[:, 0]) == list(range(len(amp)))
    assert amp[:, 2:].sum() == len(lines)
    assert [amp[:, 2 + k].sum() for k in range(4)] == [len(t[n]) for n in ("sequence_edges", "concordant_edges",
                                                                          "discordant_edges", "source_edges")]
    return sorted(lines)


def edge_lines(texts):
    return sorted(l for x in texts for l in x.splitlines() if not l.startswith(("SequenceEdge", "BreakpointEdge")))


def load_tables(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def assert_same_tables(got_dir, want_dir):
    """Same tables, same shapes, equal columns (CN values to the 6 decimals of *_graph.txt)."""
    got, want = load_tables(got_dir), load_tables(want_dir)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name].shape == want[name].shape, name
        np.testing.assert_allclose(got[name], want[name], rtol=0, atol=1e-6, err_msg=name)


def synthetic_graph(n, max_cn=7.25):
    """A BreakpointGraph with n edges of every kind, built through its own add_* methods; every field of edge k is distinct."""
    from coral_amd.breakpoint_graph import BreakpointGraph
    g = BreakpointGraph()
    g.max_cn = max_cn
    for k in range(n):
        c, l, r, v = "chr%d" % (1 + k % 3), 1000 + 1000 * k, 1500 + 1000 * k, 100 * (k + 1)
        for nd in ((c, l, "-"), (c, r, "+"), (c, r + 1, "-")):
            g.add_node(nd)
        g.amplicon_intervals.append([c, l, r])
        g.add_sequence_edge(c, l, r, sr_count=v + 1, lr_count=v + 2, lr_nc=v + 3, cn=v + 0.5)
        g.add_concordant_edge(c, r, "+", c, r + 1, "-", sr_count=v + 4, lr_count=v + 5, reads={"a%d" % k, "b%d" % k}, cn=v + 0.25)
        g.add_discordant_edge(c, r, "+", c, l, "-", sr_count=v + 6, sr_cn=v + 0.125, lr_count=v + 7, reads={"c%d" % k}, cn=v + 0.75)
        g.add_source_edge(c, l, "-", sr_count=v + 8, sr_cn=v + 0.375, lr_cn=v + 0.625, cn=v + 0.875)
    return g


def test_dump_columns_follow_the_edge_fields(tmp_path):
    """Every column of every table is the field DUMP_COLUMNS names, for a graph whose fields are all distinct."""
    bench = _bench()
    from coral_amd.global_names import chr_idx
    bench.dump_outputs(types.SimpleNamespace(lr_graph=[synthetic_graph(1, max_cn=9.5)]), str(tmp_path))
    t = load_tables(str(tmp_path))
    assert sorted(t) == sorted(bench.DUMP_COLUMNS)
    c = chr_idx["chr1"]
    want = {
        "amplicons": dict(amplicon=0, max_cn=9.5, sequence_edges=1, concordant_edges=1, discordant_edges=1, source_edges=1),
        "amplicon_intervals": dict(amplicon=0, chr=c, start=1000, end=1500),
        "sequence_edges": dict(amplicon=0, chr=c, start=1000, end=1500, sr_count=101, lr_count=102, lr_nc=103, size=501, cn=100.5),
        "concordant_edges": dict(amplicon=0, chr1=c, pos1=1500, o1=1, chr2=c, pos2=1501, o2=-1, sr_count=104, lr_count=105, reads=2,
                                 cn=100.25),
        "discordant_edges": dict(amplicon=0, chr1=c, pos1=1500, o1=1, chr2=c, pos2=1000, o2=-1, sr_count=106, sr_cn=100.125,
                                 lr_count=107, reads=1, cn=100.75),
        "source_edges": dict(amplicon=0, chr=c, pos=1000, o=-1, sr_count=108, sr_cn=100.375, lr_cn=100.625, cn=100.875),
    }
    for name, cols in bench.DUMP_COLUMNS.items():
        assert t[name].shape == (1, len(cols)), name
        assert dict(zip(cols, t[name][0].tolist())) == want[name], name


def test_dump_outputs_sample_stays_under_the_cap(tmp_path, monkeypatch):
    """Above DUMP_MAX_BYTES every table keeps the same seeded sample of its sorted rows (at least one), and all files written,
    headers included, stay under the cap."""
    bench = _bench()
    b = types.SimpleNamespace(lr_graph=[synthetic_graph(300), synthetic_graph(200, max_cn=3.0)])
    bench.dump_outputs(b, str(tmp_path / "all"))
    full = load_tables(str(tmp_path / "all"))
    assert sum(os.path.getsize(os.path.join(str(tmp_path / "all"), f)) for f in os.listdir(str(tmp_path / "all"))) > 150000
    cap = 60000
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", cap)
    for d in ("s1", "s2"):
        bench.dump_outputs(b, str(tmp_path / d))
        assert sum(os.path.getsize(os.path.join(str(tmp_path / d), f)) for f in os.listdir(str(tmp_path / d))) <= cap
    s1, s2 = load_tables(str(tmp_path / "s1")), load_tables(str(tmp_path / "s2"))
    assert sorted(s1) == sorted(full)
    for name, t in s1.items():
        assert np.array_equal(t, s2[name]), name                                    # seeded: the same sample every time
        assert 1 <= len(t) < len(full[name]) or len(full[name]) == 1, name
        assert np.array_equal(t, t[np.lexsort(t.T[::-1])]), name                   # still sorted
        rows = {tuple(r) for r in full[name].tolist()}
        assert all(tuple(r) in rows for r in t.tolist()), name                     # a subset of the full table


def test_dump_outputs_holds_the_written_graphs(tmp_path, monkeypatch):
    """CPU: the dumped tables of a build equal the *_graph.txt files the same build wrote, line for line."""
    from tests.product_check import install_cpu_kernel_fakes
    install_cpu_kernel_fakes(monkeypatch)
    bench = _bench()
    from coral_amd import synth, sharding
    cfg = synth.named_config("small")
    rec = synth.generate(cfg, "cpu")
    rec.names = rec.name_table()
    dr = sharding.shard_records(rec, 0, 1, "cpu")
    cn, seeds = str(tmp_path / "cn.bed"), str(tmp_path / "seeds.bed")
    synth.write_cn_bed(cfg, cn)
    synth.write_seed_bed(cfg, seeds)
    b = sharding.build_graph_sharded(dr, seeds, cn, str(tmp_path / "out"))
    assert len(b.lr_graph) >= 2
    bench.dump_outputs(b, str(tmp_path / "dump"))
    written = [open(f).read() for f in glob.glob(str(tmp_path / "out_amplicon*_graph.txt"))]
    assert len(written) == len(b.lr_graph)
    assert graph_lines_from_tables(str(tmp_path / "dump")) == edge_lines(written)
    # every column, including those *_graph.txt leaves out (intervals, max CN, short-read fields), against the oracle's graphs
    from oracle import coral_oracle as O
    from oracle.hostrecords import HostRecords
    ob, _ = O.reconstruct_graph(HostRecords(synth.generate(cfg, "cpu")), seeds, cn)
    bench.dump_outputs(ob, str(tmp_path / "oracle"))
    assert_same_tables(str(tmp_path / "dump"), str(tmp_path / "oracle"))


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_graphs(tmp_path):
    """GPU: `bench.py --steps 3 --warmup 1 --dump-outputs DIR` on the tiny workload times three steps, carries none of the
    --full figures, and its tables equal the CPU oracle's graphs of the same records."""
    from coral_amd import synth
    from oracle import coral_oracle as O
    from oracle.hostrecords import HostRecords
    out = str(tmp_path / "dump")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "tiny", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", out], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = lines[0]
    assert d["steps"] == 3 and len(d["config"]["step_ms"]) == 3 and d["ms_per_step"] > 0
    assert d["unit"] == "reads/s" and d["higher_is_better"] is True and d["dtype"] == "i32" and d["value"] > 0
    assert not {"h2d_ms", "value_incl_h2d", "decode", "decode_host", "end_to_end", "cpu_baseline"} & set(d)
    cfg = synth.named_config("tiny")
    cn, seeds = str(tmp_path / "cn.bed"), str(tmp_path / "seeds.bed")
    synth.write_cn_bed(cfg, cn)
    synth.write_seed_bed(cfg, seeds)
    ob, ofiles = O.reconstruct_graph(HostRecords(synth.generate(cfg, "cpu")), seeds, cn)
    assert graph_lines_from_tables(out) == edge_lines(ofiles.values())
    _bench().dump_outputs(ob, str(tmp_path / "oracle"))
    assert_same_tables(out, str(tmp_path / "oracle"))
