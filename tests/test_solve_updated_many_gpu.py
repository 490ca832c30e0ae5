"""Several right-hand sides with new matrix values on a kept factor on the MI355X: the cases of tests/test_solve_updated_many_cpu.py
through the product build (its run_* functions with lib = None; reference and accuracy rule of tests/test_solve_updated_cpu.py), and the
300 x 200 grid -- tiled fronts: the blocked pass pair inside the iteration takes the dependency-driven schedule -- against the CPU oracle."""
import numpy as np
import pytest

import test_solve_updated_cpu as T
import test_solve_updated_many_cpu as M
from test_gpu_parity import oracle_solve
from test_solve_updated_gpu import cond2_shifted_laplacian, shifted_grid, sparse_relres

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mats():
    return T.matrices()


@pytest.mark.parametrize("name", ["poisson", "poisson_lower"])
def test_one_column_is_the_single_form(mats, name):
    M.run_single_column(None, *mats[name])


@pytest.mark.parametrize("nrhs,pad", [(5, 0), (16, 0), (17, 0), (33, 0), (5, 3)])
def test_columns_converge_at_different_steps(nrhs, pad):
    M.run_shift_many(None, nrhs, ld=3024 + pad if pad else None)


def test_columns_finish_in_different_cycles(monkeypatch):
    steps, ref_steps = M.run_cycles_many(None, 100.0, 4, 400, monkeypatch)
    assert ref_steps[0] >= 20 and steps[0] > 8


@pytest.mark.parametrize("restart", [T.PASSV, T.PASSV - 1])
def test_basis_count_edges(monkeypatch, restart):
    steps, ref_steps = M.run_cycles_many(None, 2.0, restart, 200, monkeypatch)
    assert ref_steps[0] == 13 and steps[0] > restart


def test_not_converged_per_column():
    M.run_not_converged_many(None)


@pytest.mark.parametrize("name", T.GENERAL)
def test_rank_three_change(mats, name):
    M.run_rank_change_many(None, name, *mats[name])


@pytest.mark.parametrize("name", ["poisson", "poisson_lower", "saddle"])
def test_mapped_values(mats, name):
    M.run_mapped_many(None, *mats[name])


@pytest.mark.parametrize("name", ["poisson", "poisson_lower", "saddle"])
def test_no_side_effects(mats, name):
    M.run_no_side_effects_many(None, *mats[name])


@pytest.mark.parametrize("name", ["bfwb62", "poisson_lower"])
def test_reproducible(mats, name):
    M.run_reproducible_many(None, *mats[name])


@pytest.mark.parametrize("name", ["poisson", "poisson_lower"])
def test_device_entry_point(mats, name):
    M.run_device_entry_many(None, *mats[name])


def test_perturbed_factor():
    M.run_perturbed_many(None)


def test_status_codes():
    M.run_status_codes(None)


@pytest.mark.parametrize("lower", [False, True])
def test_grid_300x200_sixteen_columns_against_the_oracle(lower):
    """60 000 unknowns, tiled fronts (LU and L D L^T): A_old = L + I, A_new = L + 2 I, one full block"""
    nx, ny = 300, 200
    init, kw, vals, full, (n, rp, ci) = shifted_grid(nx, ny, lower)
    s = T.handle(None, init, kw, vals(1.0))
    try:
        assert s.stats()["max_front"] > 256 and s.counter("symmetric_ldlt") == int(lower)
        B = np.array([T.rhs_for(n, 3), M.eigvec(1, 1, nx, ny), M.eigvec(3, 5, nx, ny) + M.eigvec(20, 11, nx, ny), T.rhs_for(n, 21)] +
                     [T.rhs_for(n, 100 + c) for c in range(12)])
        fb = s.stats()["fused_fallbacks"]
        x, steps, relres, status = s.solve_updated_many(B, vals(2.0), rel_tol=T.TOL)
        print("steps", steps.tolist())
        assert status == 0 and s.stats()["fused_fallbacks"] == fb
        assert steps[1] == 1 and steps[0] > 1
        assert s.counter("updated_blocks") == 1 and s.counter("updated_steps") >= steps.max() and s.counter("updated_column_steps") == steps.sum()
        for c in range(16):
            own, bound, bound_double = sparse_relres(n, rp, ci, full(2.0), x[c], B[c])
            assert bound < T.TOL and own <= 2 * T.TOL and relres[c] <= T.TOL and abs(relres[c] - own) <= bound + bound_double, (c, own, relres[c])
        cond = cond2_shifted_laplacian(nx, ny, 2.0)
        for c in (0, 1):
            xo, _ = oracle_solve(n, rp, ci, full(2.0), B[c], q=s.permutation())
            err = np.linalg.norm(x[c] - xo) / np.linalg.norm(xo)
            print("column %d: forward error %.3e, cond_2 %.3e" % (c, err, cond))
            assert err <= cond * 2 * T.TOL
        x2, steps2, relres2, status2 = s.solve_updated_many(B, vals(2.0), rel_tol=T.TOL)
        assert status2 == 0 and np.array_equal(steps2, steps) and np.array_equal(relres2.view(np.uint64), relres.view(np.uint64))
        assert np.array_equal(x2.view(np.uint64), x.view(np.uint64))
    finally:
        s.close()
