"""tests/test_many_rhs_edges_cpu.py on the device, with every column count of the list and the 60 x 60 grid."""
import pytest

from test_many_rhs_edges_cpu import NRHS, run_argument_checks, run_column_counts, run_padded_columns, run_padded_columns_refined, run_zero_and_tiny_columns

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("symmetric", [False, True], ids=["lu", "ldlt"])
@pytest.mark.parametrize("nrhs", [1, 2, 9, 12, 17, 65])
def test_padded_columns(symmetric, nrhs):
    run_padded_columns(None, symmetric, nrhs)


@pytest.mark.parametrize("symmetric", [False, True], ids=["lu", "ldlt"])
@pytest.mark.parametrize("nrhs", [9, 17, 33])
def test_padded_columns_with_refinement(symmetric, nrhs):
    run_padded_columns_refined(None, symmetric, nrhs)


@pytest.mark.parametrize("symmetric", [False, True], ids=["lu", "ldlt"])
def test_column_counts_agree_with_single_solves(symmetric):
    run_column_counts(None, symmetric, 60, NRHS)


@pytest.mark.parametrize("symmetric", [False, True], ids=["lu", "ldlt"])
def test_zero_and_tiny_columns(symmetric):
    run_zero_and_tiny_columns(None, symmetric)


def test_argument_checks():
    run_argument_checks(None)
