"""Eigenpairs nearest a shift on the kept factor and the factor's inertia on the MI355X: the cases of tests/eigs.py through the product
build (lib None), with the restatement and the bounds of tests/test_eigs_cpu.py."""
import pytest

import eigs as E
from test_eigs_cpu import SHAPE_CASES

pytestmark = pytest.mark.gpu


def test_exports():
    E.check_exports(None)


@pytest.mark.parametrize("nev,ncv,name,form", SHAPE_CASES)
def test_shapes(nev, ncv, name, form):
    E.run_shape(None, name, form, nev, ncv)


def test_largest_basis_on_four_ragged_tiles():
    E.run_shape(None, "aniso4087", "I", 64, 128)


def test_largest_basis_and_four_ragged_tiles():
    E.run_shape(None, "aniso1025", "I", 64, 128)
    E.run_shape(None, "aniso4087", "I", 1, 8)


def test_one_vector_more_than_pairs():
    assert E.run_shape(None, "aniso1025_spd", "I", 3, 4) >= 1


def test_default_basis_and_value_map_with_duplicates():
    E.run_shape(None, "aniso1023", "mapped", 6, 0)


def test_handle_expanded_to_general_storage():
    E.run_shape(None, "aniso1023_mid", "I", 6, 24, with_values=True, expect_expanded=True)


@pytest.mark.parametrize("max_steps", [12, 13])
def test_step_limit_returns_the_nearest_pairs_not_the_converged_ones(max_steps):
    E.run_step_limit_with_a_converged_pair_further_away(None, max_steps)


def test_expanded_handle_with_a_mass_matrix():
    """M staged through the expansion of a lower triangle to general storage (k_expand_values into the operator's buffer)"""
    E.run_shape(None, "aniso1023_mid", "lumped1", 6, 24, with_values=True, expect_expanded=True)


@pytest.mark.parametrize("tiny", [1e-30, -1e-30, 0.0])
def test_inertia_reports_a_replaced_pivot_as_zero(tiny):
    E.run_inertia_replaced_pivot(None, tiny)


def test_inertia_without_a_small_front():
    E.run_inertia_tiled_front_only(None)


@pytest.mark.parametrize("start", ["e70", "e134"])
def test_first_of_tied_entries_is_made_positive(start):
    E.run_tied_entries(None, start)


def test_step_limit():
    E.run_step_limit(None, "aniso1025", "diag", 6, 24)


@pytest.mark.parametrize("name,form,below", [("aniso1025_spd", "I", 0), ("aniso1025", "I", 61), ("aniso1023", "I", 32), ("aniso1025", "full", None),
                                             ("aniso4087", "I", None)])
def test_inertia(name, form, below):
    got = E.run_inertia(None, name, form)
    assert below is None or got == below


@pytest.mark.parametrize("start", ["hash", "e1"])
def test_whole_spectrum_but_one_and_breakdown(start):
    E.run_diag12(None, start)


@pytest.mark.parametrize("name,form,with_values", [("aniso1023", "diag", False), ("aniso1023_mid", "I", True)])
def test_reproducible_and_without_side_effects(name, form, with_values):
    E.run_side_effects(None, name, form, with_values)


def test_life_cycle_and_status_codes():
    E.run_status_codes(None)
