"""coral_cn_solve (the Newton iteration of the CN assignment in libcoral_hip) against the numpy iteration it mirrors and against
the optimality conditions themselves, on chain-shaped balance problems like the ones compute_cn_lr builds (bg:495-606)."""
import numpy as np
import pytest

from coral_amd import breakpoint_graph as bg
from tests.cn_reference import _problem


@pytest.mark.parametrize("unsupported", [0, 2])
def test_native_newton_equals_the_numpy_iteration(unsupported, monkeypatch):
    rng = np.random.default_rng(7 + unsupported)
    for trial in range(25):
        w = _problem(rng, int(rng.integers(2, 40)), unsupported)
        monkeypatch.setenv("CORAL_CN_SOLVER", "python")
        want = bg.solve_cn_lr(*w)
        res_py = bg.solve_cn_lr.last_residual
        monkeypatch.setenv("CORAL_CN_SOLVER", "native")
        got = bg.solve_cn_lr(*w)
        assert bg.solve_cn_lr.last_residual < 1e-8 and res_py < 1e-8
        assert np.allclose(got, want, rtol=1e-9, atol=1e-12), trial
        assert (got > 0).all()


def test_native_solver_reports_a_singular_system_instead_of_guessing():
    """Dependent balance rows (the caller normally removes them): status 1, the general numpy path takes over."""
    import ctypes as C
    from coral_amd import _lib
    w_inv, w_lin, w_log, A = _problem(np.random.default_rng(1), 6)
    A = np.vstack([A, A[0]])
    x, nu, it = np.empty(len(w_lin)), np.empty(A.shape[0]), C.c_int32(0)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    a, b, c, d = f(w_inv), f(w_lin), f(w_log), f(A)
    rc = _lib.lib().coral_cn_solve(len(w_lin), A.shape[0], a.ctypes.data, b.ctypes.data, c.ctypes.data, d.ctypes.data, 200, x.ctypes.data,
                                   nu.ctypes.data, C.byref(it))
    assert rc == 1
    assert _lib.lib().coral_cn_solve(0, 0, None, None, None, None, 10, None, None, None) < 0


def test_native_row_selection_equals_the_numpy_one(monkeypatch):
    rng = np.random.default_rng(3)
    for trial in range(40):
        w = _problem(rng, int(rng.integers(2, 30)))
        A = w[3]
        extra = [A[int(rng.integers(0, len(A)))] for _ in range(int(rng.integers(0, 4)))]          # duplicated rows
        extra += [A[0] + A[1]] if len(A) > 1 else []                                               # a dependent combination
        B = np.vstack([A] + extra) if extra else A
        B = B[rng.permutation(len(B))]
        monkeypatch.setenv("CORAL_CN_SOLVER", "python")
        want = bg._independent_rows(B)
        monkeypatch.setenv("CORAL_CN_SOLVER", "native")
        assert bg._independent_rows(B) == want and len(want) == np.linalg.matrix_rank(B)


# ----------------------------------------------------------------------------------------------
# Both product paths against an independent 50-digit solve (tests/cn_reference.py), a second-order certificate for the point they
# return, and the uniqueness of that point over six starts.  The program is not convex in general; these tests are what says
# that the Newton answer is a minimum.
# ----------------------------------------------------------------------------------------------
import glob
import logging
import os

from tests import cn_reference as R
from tests.product_check import install_cpu_kernel_fakes

# max_j |x_j - x_mp_j| / x_mp_j over the variables that are not free, the larger of the two paths (native / python), measured on
# the committed seeds (DESIGN.md §5 has both paths).  Asserted at 10 times that: the margin is for another libm, BLAS and FMA
# contraction.  No bound may exceed CAP, the figure native is held to numpy at above; a measurement that needs more is a finding
# about the solver, not a reason for a wider bound.
MEASURED = {"chain": 1.5e-15, "thin": 3.8e-16, "source": 6.0e-16, "self_loop": 2.8e-15, "unsupported": 3.3e-15,
            "golden": 2.9e-15}     # golden: the amplicon graphs of tests/golden/e2e_*.json with n + p <= MP_LIMIT
CAP = 1e-9
PATHS = ["native", "python"]
GOLDEN_CASES = sorted(os.path.basename(p)[4:-5] for p in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "e2e_*.json")))
MP_LIMIT = 80                      # n + p up to which a real graph is also solved at 50 digits (an LU in mpmath: a second at 80)


def _bound(family):
    assert 10 * MEASURED[family] <= CAP
    return 10 * MEASURED[family]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("family", list(R.FAMILIES))
def test_product_paths_equal_the_50_digit_solve(family, path, monkeypatch):
    monkeypatch.setenv("CORAL_CN_SOLVER", path)
    worst = 0.0
    for seed in R.SEEDS:
        w = R.problem(family, seed)
        x_mp, res = R.solved(family, seed)
        assert res < 1e-30
        got = bg.solve_cn_lr(*w)
        assert bg.solve_cn_lr.last_residual < 1e-8 and (got > 0).all()
        worst = max(worst, R.rel_dev(got, x_mp, R.free_variables(w[0], w[2])))
        # the product's own O(n) flag says what rule 1 of the certificate says about the point it returned
        assert bg.solve_cn_lr.last_min_curvature == R.min_curvature(w[0], w[2], got)
        assert (bg.solve_cn_lr.last_min_curvature > 0) == (R.certificate(*w, got) == "convex-box")
    print("%s/%s: max relative deviation from the 50-digit solve %.3g (bound %.3g)" % (family, path, worst, _bound(family)))
    assert worst <= _bound(family)


def test_the_reference_reproduces_itself_at_30_digits():
    for family in R.FAMILIES:
        w = R.problem(family, 0)
        x50, _ = R.solved(family, 0)
        x30, res = R.mp_solve(*w, np.ones(len(w[1])), dps=30)
        assert res < 1e-25
        assert max(abs(a - b) / b for a, b in zip(x30, x50)) < 1e-25


def test_the_reference_needs_no_float64_head_start():
    """The 50-digit iteration alone, from x = 1, ends where the one that starts in float64 ends."""
    for family in ("chain", "thin", "unsupported"):
        w = R.problem(family, 1)
        x, res = R.mp_solve(*w, np.ones(len(w[1])), float_start=False)
        assert res < 1e-30
        assert max(abs(a - b) / b for a, b in zip(x, R.solved(family, 1)[0])) < 1e-20


@pytest.mark.parametrize("family", list(R.FAMILIES))
def test_certificate_of_the_synthetic_families(family):
    verdicts = [R.certificate(*R.problem(family, seed), R.solved(family, seed)[0]) for seed in R.SEEDS]
    print(family, verdicts)
    assert "not-a-minimum" not in verdicts
    if family == "thin":                                     # the family must keep reaching the non-convex region
        assert set(verdicts) == {"convex-box", "local-min"}
    else:
        assert set(verdicts) == {"convex-box"}


@pytest.mark.parametrize("seed", list(R.SEEDS))
@pytest.mark.parametrize("family", list(R.FAMILIES))
def test_every_start_ends_at_the_same_point(family, seed):
    w = R.problem(family, seed)
    x_ref, _ = R.solved(family, seed)
    for k, x0 in enumerate(R.starts(len(w[1]), seed)):
        x, res = R.mp_solve(*w, x0)
        assert res < 1e-30, (k, res)
        assert max(abs(a - b) / b for a, b in zip(x, x_ref)) < 1e-20, k


def test_the_certificate_can_fail():
    """f = Σ_j 1/x_j − x_j + 4 log x_j on x_1 = x_2: along the constraint F(t) = 2 (1/t − t + 4 log t) has F'(t) = 0 at
    t = 2 ∓ √3, a minimum and a maximum.  At the maximum c_j = −4 + 2/t < 0 on both variables."""
    mp = R._mp()
    w = np.array([1.0, 1.0]), np.array([-1.0, -1.0]), np.array([-4.0, -4.0]), np.array([[1.0, -1.0]])
    with mp.workdps(50):
        for x0, root, verdict in ((3.7, 2 + mp.sqrt(3), "not-a-minimum"), (0.3, 2 - mp.sqrt(3), "convex-box")):
            x, res = R.mp_solve(*w, np.full(2, x0))
            assert res < 1e-30 and all(abs(v - root) < mp.mpf("1e-40") for v in x)
            assert all(-4 + 2 / v < 0 for v in x) == (verdict == "not-a-minimum")
            assert R.certificate(*w, x) == verdict
    # rule 2 on its own: c_2 = −6 < 0 everywhere, so rule 1 never applies.  F(t) = 3/t − 2t + 8 log t has F'(t) = 0 at
    # t = 2 ∓ √2.5 and F''(t) = 6/t³ − 8/t², positive at the first (0.42), negative at the second (3.58)
    w2 = np.array([3.0, 0.0]), np.array([-1.0, -1.0]), np.array([-2.0, -6.0]), np.array([[1.0, -1.0]])
    with mp.workdps(50):
        for x0, root, verdict in ((0.5, 2 - mp.sqrt(2.5), "local-min"), (3.5, 2 + mp.sqrt(2.5), "not-a-minimum")):
            x, res = R.mp_solve(*w2, np.full(2, x0))
            assert res < 1e-30 and all(abs(v - root) < mp.mpf("1e-40") for v in x)
            assert R.certificate(*w2, x) == verdict, (x0, x)


@pytest.mark.parametrize("path", PATHS)
def test_an_unbounded_program_is_reported_not_raised(path, monkeypatch, caplog):
    monkeypatch.setenv("CORAL_CN_SOLVER", path)
    for seed in R.SEEDS:
        w = R.problem("unbounded", seed)
        n_seq = int((w[2] == -0.5).sum())
        d = np.zeros(len(w[1]))                               # the direction of the family's docstring: seq0, conc0, disc0
        d[0], d[n_seq], d[2 * n_seq - 1] = 1, 1, -1
        assert w[0][0] == 0 and w[2][n_seq] == 0 and w[2][2 * n_seq - 1] > 0 and not (w[3] @ d).any()
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            x = bg.solve_cn_lr(*w)
        assert np.isfinite(x).all() and (x > 0).all()
        assert bg.solve_cn_lr.last_residual >= 1e-8
        assert any("did not converge" in r.getMessage() for r in caplog.records)


def _golden_cpu(case, golden_dir, tmp_path):
    with pytest.MonkeyPatch.context() as patch:
        install_cpu_kernel_fakes(patch)
        return R.golden_cn_problems(case, golden_dir, tmp_path, "cpu")


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_real_graphs_are_certified(case, golden_dir, tmp_path, monkeypatch):
    """The CN program of every amplicon graph of every golden case (built on the CPU with the kernel stand-ins, as
    tests/test_host_logic.py does): certified at the product's answer; the small ones also against the 50-digit solve."""
    problems = _golden_cpu(case, golden_dir, tmp_path)
    assert problems
    for gi, w in enumerate(problems):
        if not w[3].shape[0]:
            continue                                          # no balance row: compute_cn_lr sets CN = coverage ratio, no program
        x = {}
        for path in PATHS:
            monkeypatch.setenv("CORAL_CN_SOLVER", path)
            x[path] = bg.solve_cn_lr(*w)
            assert bg.solve_cn_lr.last_residual < 1e-8
            verdict = R.certificate(*w, x[path])
            assert verdict != "not-a-minimum"
            assert (bg.solve_cn_lr.last_min_curvature > 0) == (verdict == "convex-box")
        size = len(w[1]) + len(R.independent_rows(w[3]))
        print("%s graph %d: n + p = %d, %s" % (case, gi, size, verdict))
        if size <= MP_LIMIT:
            x_mp, res = R.mp_solve(*w, np.ones(len(w[1])))
            assert res < 1e-30 and R.certificate(*w, x_mp) == verdict
            for path in PATHS:
                dev = R.rel_dev(x[path], x_mp, R.free_variables(w[0], w[2]))
                print("    %s: relative deviation from the 50-digit solve %.3g" % (path, dev))
                assert dev <= _bound("golden")
