"""Tangent and adjoint sensitivities with respect to the matrix values (solver_hipmf_values_outer / _solve_tangent / _solve_adjoint, their
_device forms, the complex twin's calls; kernels_sensitivity.hpp) on the device (lib None = the product build).  The cases, the exact
arithmetic and the rules are in tests/sensitivity.py; tests/test_sensitivity_cpu.py runs them on the CPU emulator of the HIP kernels."""
import pytest

import sensitivity as S

pytestmark = pytest.mark.gpu


def test_exports():
    S.check_exports(None)


@pytest.mark.parametrize("name,ncols", S.CASE_COLUMNS)
def test_outer_product_against_exact_arithmetic(name, ncols):
    S.run_outer(None, name, ncols)


@pytest.mark.parametrize("name", S.REAL_CASES + S.COMPLEX_CASES)
def test_same_bits(name):
    S.run_reproducible(None, name)


@pytest.mark.parametrize("name,nrhs", S.CASE_COLUMNS)
def test_tangent_and_adjoint_solves(name, nrhs):
    S.run_solves(None, name, nrhs)


def test_finite_differences():
    S.run_finite_differences(None)


def test_life_cycle_and_status_codes():
    S.run_status_codes(None)


@pytest.mark.parametrize("name", ["poisson", "poisson_lower", "saddle", "coo_dup", "zgrid"])
def test_no_side_effects(name):
    S.run_side_effects(None, name)
