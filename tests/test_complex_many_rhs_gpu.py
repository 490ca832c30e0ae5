"""Many right-hand sides on the complex handle on the MI355X: the cases of tests/test_complex_many_rhs_cpu.py through the product build (its
run_* functions with lib = None and its rules) and the 200 x 150 complex shifted grid, whose real-equivalent root front is tiled."""
import numpy as np
import pytest

import test_complex_many_rhs_cpu as M
import test_solve_updated_complex_cpu as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", M.MATRICES)
def test_column_counts_padding_and_single_solves(name):
    M.run_counts_and_padding(None, name)


@pytest.mark.parametrize("name", M.MATRICES)
def test_zero_and_tiny_columns(name):
    M.run_zero_and_tiny(None, name)


def test_argument_checks():
    M.run_argument_checks(None)


def test_grid_200x150_tiled_fronts():
    """30 000 complex unknowns, a real-equivalent root separator of more than 256 rows, 16 columns in one block.  Per column
    |b - A x|_2 / |b|_2, recomputed on the sparse matrix in np.clongdouble (T.own_relres), is at most twice that of the single solve of
    the same column plus the rounding bounds of the recomputations: once for the blocked figure, twice for the doubled single one."""
    n, rp, ci, vals = T.shifted_grid(200, 150)
    v0 = vals(1.0)
    A = T.full(n, rp, ci, v0)
    s = M.ZM(None, n, rp, ci, v0, nstep=-1)
    try:
        istats, _ = s.stats()
        assert istats[6] > 256, istats[6]  # max_front
        B = M.columns(n, 16, seed=200)
        singles = [M.zview(s.solve(B[j])) for j in range(16)]
        X = s.solve_many(B)
        assert s.counter("fused_fallbacks") == 0 and s.counter("block_groups") >= 1
        for j in range(16):
            blk, bound, _ = T.own_relres(A, X[j], B[j])
            one, bound_one, _ = T.own_relres(A, singles[j], B[j])
            print("column %d: relative residual %.3e blocked, %.3e single, rounding bounds %.3e / %.3e" % (j, blk, one, bound, bound_one))
            assert blk <= 2.0 * one + bound + 2.0 * bound_one, j
    finally:
        s.close()
