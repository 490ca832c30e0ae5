"""Extra-precise iterative refinement on the MI355X: the cases of tests/extra_precise.py through the product build (lib None), with the
exact error measurement, the restatement and the bounds of tests/test_extra_precise_cpu.py."""
import pytest

import extra_precise as X

pytestmark = pytest.mark.gpu


def test_exports():
    X.check_exports(None)


@pytest.mark.parametrize("name", X.ALL)
def test_forward_error_within_the_bounds(name):
    X.run_plain(None, name)


@pytest.mark.parametrize("name", X.TAILED)
def test_tail_goes_below_the_rounding_of_x(name):
    X.run_tail(None, name)


def test_complex_handle():
    X.run_complex(None)


@pytest.mark.parametrize("name", ["mumps5", "biharm300_lower"])
def test_zero_right_hand_side(name):
    X.run_zero_rhs(None, name)


def test_exact_zeros_in_the_solution():
    X.run_zeros_in_solution(None)


@pytest.mark.parametrize("nrhs", [1, 15, 16, 17, 33])
def test_many_right_hand_sides(nrhs):
    X.run_many(None, nrhs)


@pytest.mark.parametrize("name", ["shift1e-8", "biharm300_lower"])
def test_reproducible_and_without_side_effects(name):
    X.run_side_effects(None, name)


def test_replaced_pivots(monkeypatch):
    X.run_perturbed(None, monkeypatch)


def test_status_codes():
    X.run_status_codes(None)
