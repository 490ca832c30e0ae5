"""The bordered solves of the complex handle on the kept factor on the MI355X: the cases of tests/bordered_complex.py through the product
build (lib None), with the restatement, the exact error measurement and the bounds of tests/test_bordered_complex_cpu.py."""
import pytest

import bordered_complex as Z

pytestmark = pytest.mark.gpu


def test_exports():
    Z.check_exports(None)


@pytest.mark.parametrize("k", Z.K_SHAPES)
def test_border_widths(k):
    Z.run_shape(None, "zlap4087", k, 1)


@pytest.mark.parametrize("nrhs", Z.NRHS_SHAPES)
def test_right_hand_side_counts(nrhs):
    Z.run_shape(None, "zlap483", 3, nrhs, variants=nrhs in (1, 17))


def test_wide_border_of_the_small_matrix():
    Z.run_shape(None, "zlap483", 17, 1, variants=True)


def test_many_columns_of_the_large_matrix():
    Z.run_shape(None, "zlap4087", 3, 17)


@pytest.mark.parametrize("name", ["zhopf1e-6", "zhopf1e-10"])
@pytest.mark.parametrize("k", [1, 3, 17])
def test_near_a_hopf_point(name, k):
    Z.run_hopf(None, name, k)


@pytest.mark.parametrize("name", ["zlap483", "zhopf1e-10"])
@pytest.mark.parametrize("conjugate", [0, 1])
@pytest.mark.parametrize("nrhs", [1, 17])
@pytest.mark.parametrize("k", [1, 17, 32])
def test_both_transposed_forms(name, conjugate, nrhs, k):
    Z.run_transposed(None, name, k, nrhs, bool(conjugate))


def test_woodbury():
    Z.run_woodbury(None)


@pytest.mark.parametrize("k", [1, 3, 17, 32])
def test_border_info(k):
    Z.run_border_info(None, k)


def test_singular_schur_complement():
    Z.run_singular_border(None)


def test_life_cycle_and_status_codes():
    Z.run_status_codes(None)


def test_reproducible_and_without_side_effects():
    Z.run_side_effects(None)
