"""The SA-table kernels (K3, csrc/coral_satable.hip) against the reference's known answers, on both drivers - the default one
(coral_sa_table_async through kernels.sa_table_early / kernels.sa_table) and the legacy one (coral_sa_table,
CORAL_DEVICE_QUERIES=legacy).  Each driver is compared with the reference side, never with the other driver.

The tables are real SA text in BAM files, tokenised by the product's decoders (tests/sa_cases.py).  The expectations are the
values the reference recorded for cigar2pos and alignment_from_satags (tests/golden/unit_vectors.json, asserted directly) and,
for the hand-made reads, the oracle's fetch() over the original strings: ties of the stable sort, first-seen de-duplication,
the dict order of the reads, orphans, failed reads, the one-base and zero-length edge of every shape on both strands, the launch
geometry of both drivers, and which error a table with several offending reads raises.

Single-line mutants of coral_satable.hip, built from temporary copies of the tree and run on an MI355X against this module
and against the two modules that covered K3 before it (tests/test_gpu_kernels.py, tests/test_device_queries.py).  "old suite"
says what those two modules made of the mutant (mutants 7 to 9 change lines this module's fix added):
  1. parse_row, `has5 && !has3` reverse branch: `ins ? rl - c5 - 1` -> `ins ? rl - c3 - 1`
       both vector tests, test_table_equals_the_reference_model (one_base), test_first_offending_read_decides_the_error
       (zero_SMI_rev).  old suite: caught (test_sa_table_matches_oracle_fetch: tiny, tiny_edge, small)
  2. parse_row, SMDS / SMIS reverse qe: `rl - c5 - 1` -> `rl - c3 - 1`
       both vector tests, one_base, zero_SMDS_rev, zero_SMIS_rev.  old suite: caught (test_sa_table_matches_oracle_fetch: ultra only)
  3. insertion sort: `q.qe > p.qe` -> `q.qe >= p.qe` (ties leave in reverse input order)
       test_table_equals_the_reference_model (ties, dedup, long_read, many_names).  old suite: MISSED
  4. de-duplication: `bool same = sa_nm[kept_idx[j]] == nmi;` -> `bool same = true;` (NM no longer compared)
       test_table_equals_the_reference_model (dedup).  old suite: MISSED
  5. k_first_primary: `< 256` -> `< 4`
       test_table_equals_the_reference_model (read_length).  old suite: caught (test_sa_table_matches_oracle_fetch and others)
  6. k_row_keys: `tid[r] >= 0 ? name[r] : INVALID_KEY` -> `name[r]` (the SA tags of unplaced records count)
       test_table_equals_the_reference_model (orphans).  old suite: MISSED
  7. group_process_one, unknown shape: `sa_report(err, vals[a], 3)` -> `sa_report(err, a, 3)` (ordinal in name order)
       test_first_offending_read_decides_the_error (error_order_reversed)
  8. group_process_one, zero-length interval: `sa_report(err, vals[a], 4)` -> `sa_report(err, a, 4)` (the same for code 4)
       test_first_offending_read_decides_the_error (error_order_reversed, error_order_behind_a_good_read)
  9. sa_report: `~(2u * (unsigned int)ordinal + (code == 4 ? 1u : 0u))` -> `~(code == 4 ? 1u : 2u)` (the rule before this
     module: ZeroDivisionError beats KeyError wherever the reads are)
       test_first_offending_read_decides_the_error (bad_zero, mixed_bad_first, error_order).  old suite: missed as it stood
       (test_sa_table_errors_equal_legacy asserted that rule); caught by that test as it stands now
Not run: k_group_process_n leaving `g_first[g]` unset in its `g >= n_groups` branch.  The slots behind the groups then sort by
whatever the workspace held, k_count_valid may count them as reads, and k_scatter_n reads `keys[gstart[g]]` for them with a
`gstart[g]` nobody wrote - an index into nowhere.  That mutant changes an address, so it stays off the GPU, and
what a test would make of a wrong padding slot is therefore unverified: long_read has such slots (303 for 4 groups) and passes,
which shows only that the kernel as it stands leaves them empty.

Two things the cases brought in besides the error rule: without a read (no SA tag at all, or orphans only) the legacy driver
left the table's one offset unset, and without an SA tag so did the default driver; both write it now.
"""
import numpy as np
import pytest

from tests import sa_cases
from tests.sa_cases import CASES, ERROR_CASES, SHAPES, STRANDS, shape_of

gpu = pytest.mark.gpu
DRIVERS = ["native", "legacy"]


@pytest.fixture(scope="module")
def sa_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("sa_cases")


@pytest.fixture(params=DRIVERS)
def driver(request, monkeypatch):
    if request.param == "legacy":
        monkeypatch.setenv("CORAL_DEVICE_QUERIES", "legacy")
    else:
        monkeypatch.delenv("CORAL_DEVICE_QUERIES", raising=False)
    return request.param


def _device_table(case, driver):
    """The table of the case's decoded records as a build makes it, on the driver the environment selects."""
    from coral_amd import kernels
    from coral_amd.records import DeviceRecords
    from tests.product_check import device_sa_table
    assert kernels._native_queries(DeviceRecords(case.rec, "cuda:0")) == (driver == "native")
    return device_sa_table(case.rec)


def _assert_equals_model(got, want, what):
    for key in ("cols", "off", "name", "failed", "read_length", "pairs"):
        g, w = np.asarray(got[key]), want[key]
        assert g.shape == w.shape and np.array_equal(g, w), (what, key)
    assert np.array_equal(got["rows"], want["cols"].T), (what, "rows")


# ---- without a GPU: the cases are what they are named after, and the model gives what the reference recorded -----------------
def test_cases_and_model(sa_dir):
    for name, (_, verify) in CASES.items():
        case = sa_cases.load(name, sa_dir)
        assert case.raises is None, name
        e = case.expect
        assert e["cols"].shape == (8, int(e["off"][-1])) and len(e["off"]) == len(e["name"]) + 1 == len(e["failed"]) + 1
        assert len(e["read_length"]) == len(case.names) and e["pairs"].shape == (2 * e["cols"].shape[1], 8)
        if verify is not None:
            verify(sa_cases.Expect(e, case.names))
    for name, (_, exc) in ERROR_CASES.items():
        assert sa_cases.load(name, sa_dir).raises is exc, name
    e = sa_cases.load("one_base", sa_dir).expect
    assert (e["cols"][1] - e["cols"][0]).tolist() == [1] * 18
    for name, n in (("reads255", 255), ("reads256", 256), ("reads257", 257)):
        assert sa_cases.load(name, sa_dir).expect["off"].tolist() == list(range(n + 1))
    e = sa_cases.load("many_names", sa_dir).expect
    assert len(e["name"]) == 6000 and e["name"].max() > 65_536 and e["cols"].shape[1] > 14_000
    assert len(sa_cases.load("no_sa", sa_dir).expect["name"]) == 0 and sa_cases.load("no_sa", sa_dir).rec.sa.shape[0] == 0
    only = sa_cases.load("only_orphans", sa_dir)
    assert len(only.expect["name"]) == 0 and only.rec.sa.shape[0] == 3
    _check_cigar2pos_vectors(sa_cases.load("cigar2pos_vectors", sa_dir).expect)
    _check_satags_vectors(sa_cases.load("satags_vectors", sa_dir).expect)


# ---- the reference's recorded vectors ---------------------------------------------------------------------------------------------
def _check_cigar2pos_vectors(t):
    """A table of the 108 one-entry reads against the recorded (qs, qe, al) of every vector."""
    vec, _ = sa_cases.unit_vectors()
    cols = np.asarray(t["cols"])
    assert np.asarray(t["off"]).tolist() == list(range(109)) and np.asarray(t["name"]).tolist() == list(range(108))
    assert not np.asarray(t["failed"]).any()
    seen = set()
    for k, v in enumerate(vec):
        qs, qe, al = v["out"]
        assert qs != qe
        pos = int(sa_cases.cigar2pos_entry(k, v).split(",")[1])
        ref = (pos - 1, pos + al - 2) if v["strand"] == "+" else (pos + al - 2, pos - 1)
        assert (int(cols[0, k]), int(cols[1, k])) == (qs, qe), (k, v)
        assert (int(cols[3, k]), int(cols[4, k])) == ref, (k, v)
        assert cols[:, k].tolist()[2:3] + cols[:, k].tolist()[5:] == [0, "+-".index(v["strand"]), 60, 1], (k, v)
        assert int(np.asarray(t["read_length"])[k]) == v["read_length"]
        seen.add((shape_of(sa_cases.cigar2pos_entry(k, v)), v["strand"]))
    assert seen == {(s, st) for s in SHAPES for _, st in STRANDS}


def _check_satags_vectors(t):
    """A table of the 40 reads against the recorded alignment_from_satags results: qint, rint, mapq and the NM rate as floats,
    exactly; the vectors recorded as the 3-tuple are failed reads without rows."""
    from coral_amd import synth
    _, vec = sa_cases.unit_vectors()
    cols, off, failed = np.asarray(t["cols"]), np.asarray(t["off"]), np.asarray(t["failed"])
    assert np.asarray(t["name"]).tolist() == list(range(40)) and len(off) == 41
    seen, n_failed = set(), 0
    for k, v in enumerate(vec):
        a, b = int(off[k]), int(off[k + 1])
        seen |= {(shape_of(e), e.split(",")[2]) for e in v["sa_list"] if shape_of(e) in SHAPES}
        if len(v["out"]) == 3:
            assert v["out"] == ([], [], []) and failed[k] and a == b, k
            assert any(shape_of(e) in ("M", "MI", "MD") for e in v["sa_list"])
            n_failed += 1
            continue
        qint, rint, mapq, nm = v["out"]
        assert not failed[k] and b - a == len(qint), k
        assert [[int(cols[0, r]), int(cols[1, r])] for r in range(a, b)] == qint, k
        assert [[synth.CHROMS[cols[2, r]], int(cols[3, r]), int(cols[4, r]), "+-"[cols[5, r]]] for r in range(a, b)] == rint, k
        assert [int(cols[6, r]) for r in range(a, b)] == mapq, k
        assert [int(cols[7, r]) / (int(cols[1, r]) - int(cols[0, r])) for r in range(a, b)] == nm, k
    assert n_failed == 3 and seen == {(s, st) for s in SHAPES for _, st in STRANDS}


@gpu
def test_cigar2pos_vectors_through_the_kernel(sa_dir, driver):
    _check_cigar2pos_vectors(_device_table(sa_cases.load("cigar2pos_vectors", sa_dir), driver))


@gpu
def test_satags_vectors_through_the_kernel(sa_dir, driver):
    _check_satags_vectors(_device_table(sa_cases.load("satags_vectors", sa_dir), driver))


# ---- the product's two tokenisers -------------------------------------------------------------------------------------------------
@gpu
def test_host_and_gpu_tokens_are_equal(sa_dir):
    """Every file of this module through the GPU decoder as well: the SA tokens (and what else the table reads) are the host
    decoder's."""
    from coral_amd import bam
    for name in list(CASES) + list(ERROR_CASES):
        case = sa_cases.load(name, sa_dir)
        back = bam.decode_bam_gpu(case.path)
        for key in ("sa_off", "sa", "sa_nm", "tid", "flag", "qlen", "has_seq", "name_id"):
            x, y = getattr(case.rec, key).cpu().numpy(), getattr(back, key).cpu().numpy()
            assert x.shape == y.shape and np.array_equal(x, y), (name, key)


# ---- hand-made reads against the string-level model ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", [n for n in CASES if not n.endswith("_vectors")])
def test_table_equals_the_reference_model(name, sa_dir, driver):
    case = sa_cases.load(name, sa_dir)
    _assert_equals_model(_device_table(case, driver), case.expect, name)


@gpu
@pytest.mark.parametrize("name", list(ERROR_CASES))
def test_first_offending_read_decides_the_error(name, sa_dir, driver):
    """What the reference raises, both drivers raise: it walks the reads in dict order and stops at the first that offends."""
    case = sa_cases.load(name, sa_dir)
    assert case.raises is ERROR_CASES[name][1]
    with pytest.raises(case.raises):
        _device_table(case, driver)
