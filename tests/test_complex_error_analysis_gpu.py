"""The complex twin's MUMPS-style error analysis (complex_solver_hipmf_solve_with_error_analysis) on the MI355X: the cases of
tests/test_complex_error_analysis_cpu.py on the device, and a 250 000-unknown complex shifted 2D system whose real-equivalent factor
reaches the tiled fronts."""
import numpy as np
import pytest

from test_complex_error_analysis_cpu import (CASE_NAMES, COUNTER_ANALYSIS_SOLVES, COUNTER_KRYLOV_ITERATIONS, ZHandle, as_complex, case,
                                             run_case, shifted_convection_diffusion)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", CASE_NAMES)
def test_cpu_cases_on_device(name):
    run_case(None, name)


def test_moduli_on_device():
    A, b, _ = case("golden_general")
    s = ZHandle(None, A)
    _, ea = s.solve_ea(b, 2)
    D = A.toarray()
    assert ea[0] == pytest.approx(np.abs(D).sum(axis=1).max(), rel=1e-14)
    assert abs(ea[0] - (np.abs(D.real) + np.abs(D.imag)).sum(axis=1).max()) > 1e-3 * ea[0]
    assert ea[1] == pytest.approx(np.abs(as_complex(s.solve(b))).max(), rel=1e-14)
    s.close()


def test_shifted_250k():
    A = shifted_convection_diffusion(500)
    n = A.shape[0]
    assert n == 250_000
    rng = np.random.default_rng(5)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    s = ZHandle(None, A)
    ist, _ = s.stats()
    assert ist[6] > 512  # max_front of the real-equivalent factor: tiled fronts at the top of the tree
    x0 = s.solve(b)
    is0, ds0 = s.stats()
    kry0 = s.counter(COUNTER_KRYLOV_ITERATIONS)
    x, ea = s.solve_ea(b, 1)
    assert np.array_equal(x, x0)
    assert np.all(np.isfinite(ea)) and ea[6] >= 1.0
    assert 0 < s.counter(COUNTER_ANALYSIS_SOLVES) <= 22
    is1, ds1 = s.stats()
    assert np.array_equal(is1, is0) and ds1[9] == ds0[9] and s.counter(COUNTER_KRYLOV_ITERATIONS) == kry0
    x2, ea2 = s.solve_ea(b, 1)
    assert np.array_equal(x2, x) and np.array_equal(ea2, ea)
    s.close()
