"""Extra-precise iterative refinement with forward error bounds (solver_hipmf_solve_extra_precise / _many / _device and the complex twin's
entry point; kernels_refine_extra.hpp) on the CPU emulator of the HIP kernels.  The cases, the exact error measurement and the NumPy
restatement are in tests/extra_precise.py; tests/test_extra_precise_gpu.py repeats them on the device."""
import pytest

import extra_precise as X


def test_exports(emu_lib):
    """the four entry points, the two counters and their names (none of them exists on the parent commit)"""
    X.check_exports(emu_lib)


@pytest.mark.parametrize("name", X.ALL)
def test_forward_error_within_the_bounds(emu_lib, name):
    X.run_plain(emu_lib, name)


@pytest.mark.parametrize("name", X.TAILED)
def test_tail_goes_below_the_rounding_of_x(emu_lib, name):
    X.run_tail(emu_lib, name)


def test_complex_handle(emu_lib):
    X.run_complex(emu_lib)


@pytest.mark.parametrize("name", ["mumps5", "biharm300_lower"])
def test_zero_right_hand_side(emu_lib, name):
    X.run_zero_rhs(emu_lib, name)


def test_exact_zeros_in_the_solution(emu_lib):
    X.run_zeros_in_solution(emu_lib)


@pytest.mark.parametrize("nrhs", [1, 15, 16, 17, 33])
def test_many_right_hand_sides(emu_lib, nrhs):
    X.run_many(emu_lib, nrhs)


@pytest.mark.parametrize("name", ["shift1e-8", "biharm300_lower"])
def test_reproducible_and_without_side_effects(emu_lib, name):
    X.run_side_effects(emu_lib, name)


def test_replaced_pivots(emu_lib, monkeypatch):
    X.run_perturbed(emu_lib, monkeypatch)


def test_status_codes(emu_lib):
    X.run_status_codes(emu_lib)
