"""Bordered systems on the kept factor on the MI355X: the cases of tests/bordered.py through the product build (lib None), with the
restatement, the exact error measurement and the bounds of tests/test_bordered_cpu.py."""
import pytest

import bordered as B

pytestmark = pytest.mark.gpu


def test_exports():
    B.check_exports(None)


@pytest.mark.parametrize("k", B.K_SHAPES)
def test_border_widths(k):
    B.run_shape(None, "lap4087", k, 1)


@pytest.mark.parametrize("nrhs", B.NRHS_SHAPES)
def test_right_hand_side_counts(nrhs):
    B.run_shape(None, "lap483", 3, nrhs, variants=nrhs in (1, 17))


def test_small_matrix_wide_border_and_many_columns_of_the_large_one():
    B.run_shape(None, "lap483", 17, 1, variants=True)
    B.run_shape(None, "lap4087", 3, 17)


@pytest.mark.parametrize("name", ["fold1e-6", "fold1e-10"])
@pytest.mark.parametrize("k", [1, 3, 17])
def test_near_a_fold(name, k):
    B.run_fold(None, name, k)


@pytest.mark.parametrize("k", [1, 17])
def test_symmetric_handle_keeps_its_factor(k):
    B.run_symmetric(None, k)


def test_woodbury():
    B.run_woodbury(None)


@pytest.mark.parametrize("k", [3, 17])
def test_border_info(k):
    B.run_border_info(None, k)


def test_singular_schur_complement():
    B.run_singular_border(None)


def test_life_cycle_and_status_codes():
    B.run_status_codes(None)


@pytest.mark.parametrize("name", ["lap483", "biharm300_lower"])
def test_reproducible_and_without_side_effects(name):
    B.run_side_effects(None, name)
