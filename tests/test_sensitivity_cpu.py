"""Tangent and adjoint sensitivities with respect to the matrix values (solver_hipmf_values_outer / _solve_tangent / _solve_adjoint, their
_device forms, the complex twin's calls; kernels_sensitivity.hpp) on the CPU emulator of the HIP kernels.  The cases, the exact
arithmetic and the rules are in tests/sensitivity.py; tests/test_sensitivity_gpu.py repeats them on the device."""
import pytest

import sensitivity as S


def test_exports(emu_lib):
    """the nine entry points, the two counters and their names (none of them exists on the parent commit)"""
    S.check_exports(emu_lib)


@pytest.mark.parametrize("name,ncols", S.CASE_COLUMNS)
def test_outer_product_against_exact_arithmetic(emu_lib, name, ncols):
    S.run_outer(emu_lib, name, ncols)


@pytest.mark.parametrize("name", S.REAL_CASES + S.COMPLEX_CASES)
def test_same_bits(emu_lib, name):
    S.run_reproducible(emu_lib, name)


@pytest.mark.parametrize("name,nrhs", S.CASE_COLUMNS_EMULATED_SOLVES)
def test_tangent_and_adjoint_solves(emu_lib, name, nrhs):
    S.run_solves(emu_lib, name, nrhs)


def test_finite_differences(emu_lib):
    S.run_finite_differences(emu_lib)


def test_life_cycle_and_status_codes(emu_lib):
    S.run_status_codes(emu_lib)


@pytest.mark.parametrize("name", ["poisson", "poisson_lower", "saddle", "coo_dup", "zgrid"])
def test_no_side_effects(emu_lib, name):
    S.run_side_effects(emu_lib, name)
