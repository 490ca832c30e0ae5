"""Eigenpairs nearest a shift on the kept factor and the factor's inertia (solver_hipmf_eigs_near_shift / _device,
solver_hipmf_get_inertia; kernels_eigs.hpp) on the CPU emulator of the HIP kernels.  The cases, the NumPy restatement and the bounds are
in tests/eigs.py; tests/test_eigs_gpu.py repeats them on the device."""
import pytest

import eigs as E

# (nev, ncv) on both sides of the multiples of 4 and 16 in k_eig_rotate, the mass matrix and the matrix taking turns
SHAPE_CASES = [(1, 8, "aniso1025", "I"), (6, 24, "aniso1025", "diag"), (15, 31, "aniso1023", "full"), (16, 32, "aniso1025_spd", "I"), (17, 40, "aniso1023", "diag"),
               (33, 70, "aniso1025", "full")]


def test_exports(emu_lib):
    """the three entry points, the eight counters and their names (none of them exists on the parent commit)"""
    E.check_exports(emu_lib)


@pytest.mark.parametrize("nev,ncv,name,form", SHAPE_CASES)
def test_shapes(emu_lib, nev, ncv, name, form):
    E.run_shape(emu_lib, name, form, nev, ncv)


def test_largest_basis_and_four_ragged_tiles(emu_lib):
    """nev = 64, ncv = 128, and the matrix of four ragged row tiles -- apart on the emulator, where one refined solve of 4087 unknowns takes
    0.3 s and the 140 steps of the two together a minute; tests/test_eigs_gpu.py runs (64, 128) on aniso4087 as well"""
    E.run_shape(emu_lib, "aniso1025", "I", 64, 128)
    E.run_shape(emu_lib, "aniso4087", "I", 1, 8)


def test_one_vector_more_than_pairs(emu_lib):
    """nev + 1 = ncv: every restart keeps ncv - 1 vectors (k_eig_rotate with k = m - 1)"""
    assert E.run_shape(emu_lib, "aniso1025_spd", "I", 3, 4) >= 1


def test_default_basis_and_value_map_with_duplicates(emu_lib):
    E.run_shape(emu_lib, "aniso1023", "mapped", 6, 0)


def test_handle_expanded_to_general_storage(emu_lib):
    E.run_shape(emu_lib, "aniso1023_mid", "I", 6, 24, with_values=True, expect_expanded=True)


@pytest.mark.parametrize("max_steps", [12, 13])
def test_step_limit_returns_the_nearest_pairs_not_the_converged_ones(emu_lib, max_steps):
    E.run_step_limit_with_a_converged_pair_further_away(emu_lib, max_steps)


def test_expanded_handle_with_a_mass_matrix(emu_lib):
    """M staged through the expansion of a lower triangle to general storage (k_expand_values into the operator's buffer)"""
    E.run_shape(emu_lib, "aniso1023_mid", "lumped1", 6, 24, with_values=True, expect_expanded=True)


@pytest.mark.parametrize("tiny", [1e-30, -1e-30, 0.0])
def test_inertia_reports_a_replaced_pivot_as_zero(emu_lib, tiny):
    E.run_inertia_replaced_pivot(emu_lib, tiny)


def test_inertia_without_a_small_front(emu_lib):
    E.run_inertia_tiled_front_only(emu_lib)


@pytest.mark.parametrize("start", ["e70", "e134"])
def test_first_of_tied_entries_is_made_positive(emu_lib, start):
    E.run_tied_entries(emu_lib, start)


def test_step_limit(emu_lib):
    E.run_step_limit(emu_lib, "aniso1025", "diag", 6, 24)


@pytest.mark.parametrize("name,form,below", [("aniso1025_spd", "I", 0), ("aniso1025", "I", 61), ("aniso1023", "I", 32), ("aniso1025", "full", None),
                                             ("aniso4087", "I", None)])
def test_inertia(emu_lib, name, form, below):
    got = E.run_inertia(emu_lib, name, form)
    assert below is None or got == below


@pytest.mark.parametrize("start", ["hash", "e1"])
def test_whole_spectrum_but_one_and_breakdown(emu_lib, start):
    E.run_diag12(emu_lib, start)


@pytest.mark.parametrize("name,form,with_values", [("aniso1023", "diag", False), ("aniso1023_mid", "I", True)])
def test_reproducible_and_without_side_effects(emu_lib, name, form, with_values):
    E.run_side_effects(emu_lib, name, form, with_values)


def test_life_cycle_and_status_codes(emu_lib):
    E.run_status_codes(emu_lib)
