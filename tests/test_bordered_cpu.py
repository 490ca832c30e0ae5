"""Bordered systems on the kept factor (solver_hipmf_set_border / solver_hipmf_solve_bordered and their _device forms; kernels_border.hpp)
on the CPU emulator of the HIP kernels.  The cases, the NumPy restatement and the exact error measurement are in tests/bordered.py;
tests/test_bordered_gpu.py repeats them on the device."""
import pytest

import bordered as B


def test_exports(emu_lib):
    """the four entry points, the three counters and their names (none of them exists on the parent commit)"""
    B.check_exports(emu_lib)


@pytest.mark.parametrize("k", B.K_SHAPES)
def test_border_widths(emu_lib, k):
    B.run_shape(emu_lib, "lap4087", k, 1)


@pytest.mark.parametrize("nrhs", B.NRHS_SHAPES)
def test_right_hand_side_counts(emu_lib, nrhs):
    B.run_shape(emu_lib, "lap483", 3, nrhs, variants=nrhs in (1, 17))


def test_small_matrix_wide_border_and_many_columns_of_the_large_one(emu_lib):
    B.run_shape(emu_lib, "lap483", 17, 1, variants=True)
    B.run_shape(emu_lib, "lap4087", 3, 17)


@pytest.mark.parametrize("name", ["fold1e-6", "fold1e-10"])
@pytest.mark.parametrize("k", [1, 3, 17])
def test_near_a_fold(emu_lib, name, k):
    B.run_fold(emu_lib, name, k)


@pytest.mark.parametrize("k", [1, 17])
def test_symmetric_handle_keeps_its_factor(emu_lib, k):
    B.run_symmetric(emu_lib, k)


def test_woodbury(emu_lib):
    B.run_woodbury(emu_lib)


@pytest.mark.parametrize("k", [3, 17])
def test_border_info(emu_lib, k):
    B.run_border_info(emu_lib, k)


def test_singular_schur_complement(emu_lib):
    B.run_singular_border(emu_lib)


def test_life_cycle_and_status_codes(emu_lib):
    B.run_status_codes(emu_lib)


@pytest.mark.parametrize("name", ["lap483", "biharm300_lower"])
def test_reproducible_and_without_side_effects(emu_lib, name):
    B.run_side_effects(emu_lib, name)
