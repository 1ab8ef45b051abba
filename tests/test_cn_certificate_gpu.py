"""The link from the device-side counts to the CN program: a golden case built from records on the GPU hands compute_cn_lr the
same weights and balance rows as the CPU build of that case (kernel stand-ins), the answer carries the certificate of
tests/test_cn_solver.py, and the CN column is the CPU build's bit for bit.  Not a second solver test."""
import numpy as np
import pytest

from coral_amd import breakpoint_graph as bg
from tests import cn_reference as R
from tests.product_check import install_cpu_kernel_fakes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["tiny", "cfg3_2amp"])
def test_gpu_build_hands_the_cpu_builds_cn_program_to_the_solver(case, golden_dir, tmp_path, monkeypatch):
    monkeypatch.setenv("CORAL_CN_SOLVER", "native")
    gpu = R.golden_cn_problems(case, golden_dir, tmp_path, "cuda:0")
    install_cpu_kernel_fakes(monkeypatch)
    cpu = R.golden_cn_problems(case, golden_dir, tmp_path, "cpu")
    assert len(gpu) == len(cpu) >= 1
    for g, c in zip(gpu, cpu):
        for a, b in zip(g, c):                                # w_inv, w_lin, w_log, A
            assert a.shape == b.shape and a.dtype == b.dtype == np.float64 and a.tobytes() == b.tobytes()
        assert g[3].shape[0] > 0
        x = bg.solve_cn_lr(*g)
        assert bg.solve_cn_lr.last_residual < 1e-8
        assert R.certificate(*g, x) == "convex-box" and bg.solve_cn_lr.last_min_curvature > 0
        assert np.array(g.cn).tobytes() == np.array(c.cn).tobytes()
