"""GPU parity of the shard-local kernel launches (the N > 1 path) against the whole-file CPU stand-ins.

Every rank of a sharded build runs the ``_*_local`` launches of coral_amd.kernels on its contiguous record range [lo, hi) only;
the exchange then concatenates rows (tagged with lo) and sums the per-segment counts.  Here all shards of one file are cut in one
process (``DeviceRecords(..., rank=r, world=W)`` touches no process group), each runs the real HIP kernels, and the pieces put
back together must equal the oracle-backed stand-ins of tests/product_check.py on the whole file, at world 2, 3, 8 and 16 —
empty shards and shards of two or three records included.
"""
import numpy as np
import pytest

from coral_amd import synth

pytestmark = pytest.mark.gpu

WORLDS = (2, 3, 8, 16)
WIN = 150           # tiling window on the busiest contig
N_WIN = 2200        # > COV_LDS_SEGS (2048): the global-atomic path of k_seg_classify / k_seg_walk


class _Recorder:
    """Stands in for pytest's monkeypatch: keeps the stand-ins instead of installing them."""

    def __init__(self):
        self.fns = {}

    def setattr(self, obj, name, val):
        self.fns[name] = val


def _stand_ins():
    from tests.product_check import install_cpu_kernel_fakes
    r = _Recorder()
    install_cpu_kernel_fakes(r)
    return r.fns


def _records(name):
    from tests.test_gpu_kernels import _adversarial_records, _odd_records
    if name == "odd":
        return _odd_records()
    if name == "adversarial":
        return _adversarial_records()
    if name == "cfg1_8k":
        return synth.generate(synth.scaled_config("cfg1", 8000), "cpu")
    return synth.dataset(name, "cpu")[1]


def _cuts(rec, world):
    """[(lo, hi)] of every rank, as DeviceRecords cuts them (on the CPU: no kernel involved)."""
    from coral_amd.records import DeviceRecords
    return [(d.lo, d.hi) for d in (DeviceRecords(rec, "cpu", rank=r, world=world) for r in range(world))]


def _boundary_positions(host, los):
    """(tid, x) at pos[lo] - 1, pos[lo], pos[lo] + 1 and end[lo - 1] - 1, end[lo - 1], end[lo - 1] + 1 of every shard start."""
    xs = set()
    for lo in los:
        if 0 < lo < host.n:
            for i, base in ((lo, host.pos[lo]), (lo - 1, host.end[lo - 1])):
                if host.tid[i] >= 0:
                    xs.update((int(host.tid[i]), max(int(base) + d, 0)) for d in (-1, 0, 1))
    return sorted(xs)


def _only_longest_point(host):
    """A point covered by the record of the largest reference span and by no other record (its end - 1 if none is)."""
    mapped = np.nonzero(host.tid >= 0)[0]
    L = int(mapped[np.argmax(host.end[mapped] - host.pos[mapped])])
    t, a, b = int(host.tid[L]), int(host.pos[L]), int(host.end[L])
    others = [i for i in host.region(host.chroms[t], a, b) if i != L]
    depth = np.zeros(b - a + 1, dtype=np.int64)
    for i in others:
        depth[max(int(host.pos[i]), a) - a] += 1
        depth[min(int(host.end[i]), b) - a] -= 1
    free = np.nonzero(np.cumsum(depth)[:b - a] == 0)[0]
    return L, (t, a + int(free[-1]) if len(free) else b - 1)


def _coverage_oracle(host, sg):
    """(n_reads, n_bases) of the ``_coverage_local`` stand-in (before the non-ACGT correction) for many segments: the same
    sums — records by the htslib overlap rule, those with an inferred read length counted, the aligned blocks of those with
    SEQ and a CIGAR clipped to the segment — with each record's blocks computed once instead of once per segment."""
    out = np.zeros((2, len(sg)), dtype=np.int64)
    blocks, rlen = {}, {}
    for j, (t, s, e) in enumerate(sg.tolist()):
        for i in host.region(host.chroms[t], s, e).tolist():
            if i not in blocks:
                blocks[i] = host.blocks(i) if host.has_seq[i] and host.n_cigar[i] else []
                rlen[i] = bool(host.infer_read_length(i))
            out[0, j] += rlen[i]
            out[1, j] += sum(max(0, min(b, e) - max(a, s)) for a, b in blocks[i])
    return out


def _tiling_oracle(host, t, start):
    """The same sums for the N_WIN windows of WIN bases from ``start`` on contig ``t``, by one depth profile over the tiling."""
    span = WIN * N_WIN
    out = np.zeros((2, N_WIN), dtype=np.int64)
    depth = np.zeros(span + 1, dtype=np.int64)
    for i in host.region(host.chroms[t], start, start + span).tolist():
        if host.infer_read_length(i):
            k0 = max((int(host.pos[i]) - start) // WIN, 0)                         # first window with end > pos
            k1 = min(-((start - int(host.end[i])) // WIN) - 1, N_WIN - 1)          # last window with start < end
            out[0, k0:k1 + 1] += 1
        if host.has_seq[i] and host.n_cigar[i]:
            for a, b in host.blocks(i):
                a, b = min(max(a - start, 0), span), min(max(b - start, 0), span)
                depth[a] += 1
                depth[b] -= 1
    out[1] = np.cumsum(depth)[:span].reshape(N_WIN, WIN).sum(axis=1)
    return out


@pytest.fixture(scope="module", params=["odd", "adversarial", "tiny_edge", "cfg1_8k"])
def case(request):
    """The whole-file oracle side, computed once per case: stand-in scan (summaries + gap rows in (record, op) order), stand-in
    coverage of the boundary segments and the tiling, the covering records of every query point; plus every world's cuts."""
    from coral_amd.records import DeviceRecords
    from oracle.hostrecords import HostRecords
    name = request.param
    rec = _records(name)
    fns = _stand_ins()
    host = HostRecords(rec)
    whole = DeviceRecords(rec, "cpu")
    summary, rows = fns["_scan_local"](whole, 600, 20, 1 << 16)
    cuts = {w: _cuts(rec, w) for w in WORLDS}
    los = sorted({lo for w in WORLDS for lo, _ in cuts[w]})
    # segments that start or end at each shard's first record, then a tiling of N_WIN windows on the busiest contig
    segs = set()
    for t, x in _boundary_positions(host, los):
        segs.update([(t, x, x + 1), (t, x, x + WIN), (t, max(x - WIN, 0), x)])
    segs = sorted(s for s in segs if s[2] > s[1])
    n_edge = len(segs)
    mapped = host.tid[host.tid >= 0]
    t0 = int(np.bincount(mapped).argmax())
    on_t0 = np.nonzero(host.tid == t0)[0]
    start = max(int(host.pos[on_t0[len(on_t0) // 2]]) - WIN * N_WIN // 2, 0)
    segs += [(t0, start + WIN * k, start + WIN * (k + 1)) for k in range(N_WIN)]
    sg = np.array(segs, dtype=np.int64)
    from coral_amd.kernels import _disjoint_batches
    assert max(len(b) for b in _disjoint_batches(sg)) > 2048       # one launch with > COV_LDS_SEGS segments
    cov = np.concatenate([_coverage_oracle(host, sg[:n_edge]), _tiling_oracle(host, t0, start)], axis=1)
    some = np.unique(np.linspace(0, len(sg) - 1, 12).astype(np.int64))      # the stand-in itself on a sample of both kinds
    assert np.array_equal(fns["_coverage_local"](whole, None, sg[some]).numpy(), cov[:, some])
    L, only_l = _only_longest_point(host)
    pts = sorted(set(_boundary_positions(host, los)) | {only_l})
    uniq = np.array(pts, dtype=np.int64).reshape(-1, 2)
    cover = [host.region(host.chroms[t], p, p + 1).tolist() for t, p in pts]
    assert L in cover[pts.index(only_l)]
    return dict(name=name, rec=rec, summary=summary.numpy(), rows=rows().numpy(), cuts=cuts, sg=sg, cov=cov, uniq=uniq,
                cover=cover, shards={})


def _shards(case, world):
    from coral_amd.records import DeviceRecords
    if world not in case["shards"]:
        case["shards"].clear()                          # one world's shards on the device at a time
        case["shards"][world] = [DeviceRecords(case["rec"], "cuda:0", rank=r, world=world) for r in range(world)]
    shards = case["shards"][world]
    assert [(d.lo, d.hi) for d in shards] == case["cuts"][world]
    return shards


def test_shards_cover_the_edges():
    """The worlds used here do cut empty shards and shards of two or three records (odd: 11 records, one of > 256 ops)."""
    rec = _records("odd")
    assert _cuts(rec, 3) == [(0, 9), (9, 9), (9, 11)]
    sizes = [hi - lo for w in WORLDS for lo, hi in _cuts(rec, w)]
    assert 0 in sizes and (2 in sizes or 3 in sizes)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("gap_cap", [1 << 16, 4])
def test_shard_scan(case, world, gap_cap):
    """coral_cigar_scan per shard: (mbases, qinfer, blk_first, blk_last) equal the whole-file stand-in's rows [lo, hi); the gap
    rows + lo, in (record, op) order, equal the stand-in's rows of those records.  gap_cap 4: the world > 1 relaunch."""
    from coral_amd import kernels
    want_rows = case["rows"]
    got_all = []
    for dr in _shards(case, world):
        summary, pending = kernels._scan_local(dr, 600, 20, gap_cap)
        s = summary.cpu().numpy()
        assert s.shape == (dr.n, 4)
        assert np.array_equal(s, case["summary"][dr.lo:dr.hi]), (case["name"], world, dr.rank)
        g = pending().cpu().numpy().astype(np.int64).reshape(-1, 6)
        g = g[np.lexsort((g[:, 1], g[:, 0]))]
        g[:, 0] += dr.lo
        mine = want_rows[(want_rows[:, 0] >= dr.lo) & (want_rows[:, 0] < dr.hi)]
        assert np.array_equal(g, mine), (case["name"], world, dr.rank, len(g), len(mine))
        got_all.append(g)
    assert np.array_equal(np.concatenate(got_all), want_rows)
    if gap_cap == 4 and case["name"] != "odd":
        assert max(len(g) for g in got_all) > gap_cap          # some shard did overflow its buffer and relaunch


@pytest.mark.parametrize("world", WORLDS)
def test_shard_coverage(case, world):
    """coral_segment_coverage per shard, summed over the shards: the whole-file stand-in's (n_reads, n_bases) before the
    non-ACGT correction, for segments starting / ending at every shard's first record and a > 2048-window tiling."""
    from coral_amd import kernels
    sg = case["sg"]
    tot = np.zeros((2, len(sg)), dtype=np.int64)
    for dr in _shards(case, world):
        summary, _ = kernels._scan_local(dr, 600, 20, 1 << 16)
        out = kernels._coverage_local(dr, kernels.ScanResult(summary), sg).cpu().numpy()
        assert out.shape == (2, len(sg)) and (out >= 0).all()
        tot += out
    bad = np.nonzero((tot != case["cov"]).any(axis=0))[0]
    assert len(bad) == 0, (case["name"], world, [(tuple(sg[j]), tot[:, j].tolist(), case["cov"][:, j].tolist()) for j in bad[:5]])
    assert case["cov"][0, -N_WIN:].sum() > 0


@pytest.mark.parametrize("world", WORLDS)
def test_shard_point_cover(case, world):
    """coral_point_cover per shard with pair_cap 1 (every shard with a hit relaunches), pairs + lo put together: per point the
    covering records in file order, == HostRecords.region(c, p, p + 1).  One point is covered only by the longest record, so
    the shards' max_span differ."""
    from coral_amd import kernels
    uniq = case["uniq"]
    keys = []
    spans = set()
    for dr in _shards(case, world):
        spans.add(dr.max_span)
        k = kernels._points_local(dr, uniq, 1).cpu().numpy().astype(np.int64)
        rec = k & 0xFFFFFFFF
        assert ((rec >= 0) & (rec < dr.n)).all()
        keys.append(((k >> 32) << 32) | (rec + dr.lo))
    keys = np.sort(np.concatenate(keys))
    pt, rec = keys >> 32, keys & 0xFFFFFFFF
    for j, want in enumerate(case["cover"]):
        assert rec[pt == j].tolist() == want, (case["name"], world, tuple(uniq[j]))
    assert len(spans) > 1


@pytest.mark.parametrize("world", WORLDS)
def test_shard_public_wrappers(case, world, monkeypatch):
    """The public wrappers on one shard, the collective replaced by the identity (one shard per call here): cigar_scan and
    point_cover return GLOBAL record ordinals (local + lo), which put together give the whole-file answer."""
    from coral_amd import kernels, sharding
    monkeypatch.setattr(sharding, "allgather_rows", lambda dr, rows: rows)
    uniq = case["uniq"]
    pts = [tuple(p) for p in uniq.tolist()]
    rows, cover = [], [[] for _ in pts]
    for dr in _shards(case, world):
        res = kernels.cigar_scan(dr, 600, 20, gap_cap=4, _worker=True)
        rows.append(np.asarray(res.gaps, dtype=np.int64).reshape(-1, 6))
        pc = kernels.point_cover(dr, pts, pair_cap=1, _worker=True)
        for j in range(len(pts)):
            cover[j] += pc[j].tolist()
    assert np.array_equal(np.concatenate(rows), case["rows"]), case["name"]
    assert cover == case["cover"], case["name"]
