"""The transposed bordered solve on the kept factor on the MI355X: the cases of tests/bordered_transpose.py through the product build
(lib None), with the restatement, the exact error measurement and the bounds of tests/test_bordered_transpose_cpu.py."""
import pytest

import bordered_transpose as T

pytestmark = pytest.mark.gpu


def test_exports():
    T.check_exports(None)


@pytest.mark.parametrize("k", T.K_SHAPES)
def test_border_widths(k):
    T.run_shape(None, "ulap4087", k, 1)


@pytest.mark.parametrize("nrhs", T.NRHS_SHAPES)
def test_right_hand_side_counts(nrhs):
    T.run_shape(None, "ulap483", 3, nrhs, variants=nrhs in (1, 17))


def test_many_columns_of_the_large_matrix():
    T.run_shape(None, "ulap4087", 3, 17)


def test_unsymmetric_pattern():
    T.run_shape(None, "upat483", 17, 5, variants=True)


@pytest.mark.parametrize("name", ["ufold1e-6", "ufold1e-10"])
@pytest.mark.parametrize("k", [1, 3, 17])
def test_near_a_fold(name, k):
    T.run_fold(None, name, k)


@pytest.mark.parametrize("k", [1, 17])
def test_symmetric_handle_keeps_its_factor(k):
    T.run_symmetric(None, k)


@pytest.mark.parametrize("name,k", [("ulap483", 3), ("upat483", 17), ("biharm300_lower", 3)])
def test_adjoint_identity_with_the_plain_form(name, k):
    T.run_adjoint_identity(None, name, k)


@pytest.mark.parametrize("name", ["ulap483", "biharm300_lower"])
def test_interleaving_the_two_forms_changes_no_bit(name):
    T.run_interleaved(None, name, 3, 5)


def test_composes_with_values_outer():
    T.run_sensitivity(None)


def test_life_cycle_and_status_codes():
    T.run_status_codes(None)


@pytest.mark.parametrize("name", ["ulap483", "biharm300_lower"])
def test_reproducible_and_without_side_effects(name):
    T.run_side_effects(None, name)
