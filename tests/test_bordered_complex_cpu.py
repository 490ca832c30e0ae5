"""The bordered solves of the complex handle on the kept factor (complex_solver_hipmf_set_border, _solve_bordered,
_solve_bordered_transpose and their _device forms; kernels_border_complex.hpp) on the CPU emulator of the HIP kernels.  The cases, the
NumPy restatement and the bounds are in tests/bordered_complex.py; tests/test_bordered_complex_gpu.py repeats them on the device (the
emulator takes 5 columns of the large matrix where the device takes 17)."""
import pytest

import bordered_complex as Z


def test_exports(emu_lib):
    """the six entry points, HIPMF_COMPLEX_BORDER_MAX, the six counters and their names (none of them exists on the parent commit)"""
    Z.check_exports(emu_lib)


@pytest.mark.parametrize("k", Z.K_SHAPES)
def test_border_widths(emu_lib, k):
    Z.run_shape(emu_lib, "zlap4087", k, 1)


@pytest.mark.parametrize("nrhs", Z.NRHS_SHAPES)
def test_right_hand_side_counts(emu_lib, nrhs):
    Z.run_shape(emu_lib, "zlap483", 3, nrhs, variants=nrhs in (1, 17))


def test_wide_border_of_the_small_matrix(emu_lib):
    Z.run_shape(emu_lib, "zlap483", 17, 1, variants=True)


def test_many_columns_of_the_large_matrix(emu_lib):
    Z.run_shape(emu_lib, "zlap4087", 3, 5)


@pytest.mark.parametrize("name", ["zhopf1e-6", "zhopf1e-10"])
@pytest.mark.parametrize("k", [1, 3, 17])
def test_near_a_hopf_point(emu_lib, name, k):
    Z.run_hopf(emu_lib, name, k)


@pytest.mark.parametrize("name", ["zlap483", "zhopf1e-10"])
@pytest.mark.parametrize("conjugate", [0, 1])
@pytest.mark.parametrize("nrhs", [1, 17])
@pytest.mark.parametrize("k", [1, 17, 32])
def test_both_transposed_forms(emu_lib, name, conjugate, nrhs, k):
    Z.run_transposed(emu_lib, name, k, nrhs, bool(conjugate))


def test_woodbury(emu_lib):
    Z.run_woodbury(emu_lib)


@pytest.mark.parametrize("k", [1, 3, 17, 32])
def test_border_info(emu_lib, k):
    Z.run_border_info(emu_lib, k)


def test_singular_schur_complement(emu_lib):
    Z.run_singular_border(emu_lib)


def test_life_cycle_and_status_codes(emu_lib):
    Z.run_status_codes(emu_lib)


def test_reproducible_and_without_side_effects(emu_lib):
    Z.run_side_effects(emu_lib)
