"""Several right-hand sides with new complex values on a kept factor on the MI355X: the cases of
tests/test_solve_updated_complex_many_cpu.py through the product build (its run_* functions with lib = None, its references and its
accuracy rule) and the 200 x 150 complex shifted grid -- tiled fronts: the blocked pass pair inside the iteration takes the
dependency-driven schedule."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import test_solve_updated_complex_cpu as T
import test_solve_updated_complex_many_cpu as U
from test_complex_many_rhs_cpu import ZM, bits
from test_solve_updated_complex_gpu import cond2_shifted_grid
from test_solve_updated_many_cpu import eigvec

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("h1", [0.5, 2.0, 0.1])
def test_complex_arithmetic_per_column(h1):
    U.run_shift_many(None, h1)


@pytest.mark.parametrize("nrhs,pad", [(5, 0), (17, 0), (33, 0), (16, 3)])
def test_narrow_block_tail_block_and_padding(nrhs, pad):
    U.run_shift_many(None, 0.5, nrhs, pad)


@pytest.mark.parametrize("n", [512, 513, 2049])
def test_tile_edges(n):
    U.run_tile_edges(None, "zchain%d" % n)


@pytest.mark.parametrize("restart", [T.ZPASSV, T.ZPASSV - 1])
def test_basis_count_edges(monkeypatch, restart):
    U.run_basis_edges(None, monkeypatch, restart, 0.5, 200, False)


def test_restart_four_columns_finish_in_different_cycles(monkeypatch):
    U.run_basis_edges(None, monkeypatch, 4, 10.0, 400, True)


def test_one_column_is_the_single_form():
    U.run_single_is_single(None)


def test_not_converged_per_column():
    U.run_not_converged_many(None)


@pytest.mark.parametrize("kind", ["symlower", "weak300", "mapped", "pairs0"])
def test_handle_kinds(kind):
    U.run_handle_kind(None, kind)


def test_perturbed_factor():
    U.run_perturbed_many(None)


def test_map_mismatch():
    U.run_map_mismatch(None)


@pytest.mark.parametrize("name", ["random200", "symlower"])
def test_no_side_effects(name):
    U.run_no_side_effects_many(None, name)


@pytest.mark.parametrize("name", ["random200", "symlower"])
def test_reproducible_and_device_entry(name):
    U.run_reproducible_many(None, name)


def test_status_codes():
    U.run_status_codes_many(None)


def test_host_mirror():
    U.run_host_mirror_many(None)


def test_grid_200x150_tiled_fronts():
    """30 000 complex unknowns, K(1) -> K(0.5), 16 columns: two random, one eigenvector, one two-eigenvector, twelve random.  The forward
    error is measured for two of the columns against a direct sparse LU in double, whose own error, cond eps, is far below the bound"""
    nx, ny = 200, 150
    n, rp, ci, vals = T.shifted_grid(nx, ny)
    v0, v1 = vals(1.0), vals(0.5)
    B = np.array([T.rhs_for(n, 12), T.rhs_for(n, 14), (1 + 2j) * eigvec(1, 1, nx, ny), (0.5 - 1j) * eigvec(3, 5, nx, ny) + (2 + 0.3j) * eigvec(20, 11, nx, ny)] +
                 [T.rhs_for(n, 300 + c) for c in range(12)])
    s = ZM(None, n, rp, ci, v0)
    try:
        istats, _ = s.stats()
        assert istats[6] > 256, istats[6]  # max_front
        X, steps, relres, status = s.solve_updated_many(B, v1, rel_tol=T.TOL)
        print("steps %s in %d cycle(s), max_front %d" % (steps.tolist(), s.counter("updated_cycles"), istats[6]))
        assert status == 0 and s.counter("fused_fallbacks") == 0 and s.counter("updated_complex_arithmetic") == 1
        assert steps[2] == 1 and steps[2] < steps[0]
        assert steps[3] <= 3  # (a Krylov space of dimension 2: two steps in exact arithmetic, + 1 as for every reference count)
        U.block_counters(s, steps, 16, n)
        A1 = T.full(n, rp, ci, v1)
        cond = cond2_shifted_grid(nx, ny, 0.5)
        for c in range(16):
            own, bound, bound_double = T.own_relres(A1, X[c], B[c])
            print("column %d: reported %.3e, own %.3e, rounding bounds %.3e (own) %.3e (double)" % (c, relres[c], own, bound, bound_double))
            assert relres[c] <= T.TOL and abs(relres[c] - own) <= bound + bound_double, c
        XD = spla.spsolve(A1.tocsc(), B[[0, 2]].T)
        for q, c in enumerate((0, 2)):
            xd = XD[:, q]
            err = np.linalg.norm(X[c] - xd) / np.linalg.norm(xd)
            print("column %d: forward error %.3e, cond_2 %.3e" % (c, err, cond))
            assert err <= cond * 2 * T.TOL, (c, err)
        X2, steps2, relres2, status2 = s.solve_updated_many(B, v1, rel_tol=T.TOL)
        assert status2 == 0 and np.array_equal(steps, steps2) and np.array_equal(bits(relres), bits(relres2)) and np.array_equal(bits(X), bits(X2))
    finally:
        s.close()
