"""Transposed solves with new values on a kept factor on the MI355X: the cases of tests/test_solve_updated_transpose_cpu.py through the
product build (its run_* functions with lib = None, its references and the accuracy rule it takes from tests/test_solve_updated_cpu.py),
and two tiled-front cases: the 300 x 200 convection grid with 17 columns, and its complex twin on the 120 x 100 shifted grid."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import test_solve_updated_complex_cpu as Z
import test_solve_updated_cpu as T
import test_solve_updated_transpose_cpu as U
from test_complex_many_rhs_cpu import bits
from test_complex_transpose_many_cpu import ZTM, check_against_single
from test_solve_updated_gpu import sparse_relres

pytestmark = pytest.mark.gpu
TOL = T.TOL


@pytest.fixture(scope="module")
def mats():
    return T.matrices()


@pytest.mark.parametrize("name", ["mumps5", "bfwb62", "poisson", "chain257"])
def test_transposed_not_plain(mats, name):
    U.run_transposed_not_plain(None, name, *mats[name])


@pytest.mark.parametrize("name", ["mumps5", "bfwb62", "poisson", "chain257"])
def test_unchanged_values_take_one_step(mats, name):
    U.run_unchanged(None, *mats[name])


@pytest.mark.parametrize("name", ["poisson_lower", "saddle"])
def test_symmetric_handles_return_the_plain_bits(mats, name):
    U.run_symmetric_is_plain(None, *mats[name])


def test_edge_one_past_a_workgroup(mats):
    init, kw, values = mats["chain257"]
    U.run_edges(None, "chain257", mats["chain257"], T.redraw_rows(init, values))


def test_edge_one_past_4096(mats):
    init, kw, values = mats["chain4097"]
    U.run_edges(None, "chain4097", mats["chain4097"], T.redraw_rows(init, values))


def test_edge_long_row_of_the_transpose():
    case, v1 = U.arrow()
    U.run_edges(None, "arrow1025", case, v1)


@pytest.mark.parametrize("nrhs,pad", [(1, 0), (5, 3), (16, 0), (17, 1), (33, 2)])
def test_block_form(nrhs, pad):
    U.run_block(None, nrhs, pad)


def test_column_does_not_depend_on_its_position():
    U.run_position_independence(None)


def test_restart_four_columns_finish_in_different_cycles(monkeypatch):
    U.run_cycles(None, monkeypatch)


def test_not_converged_and_nan_per_column():
    U.run_not_converged_and_nan(None)


def test_mapped_values(mats):
    U.run_mapped(None, *mats["poisson"])


def test_status_codes():
    U.run_status_codes(None)


@pytest.mark.parametrize("name", ["poisson", "bfwb62"])
def test_no_side_effects(mats, name):
    U.run_no_side_effects(None, *mats[name])


@pytest.mark.parametrize("name", ["bfwb62", "poisson"])
def test_reproducible(mats, name):
    U.run_reproducible(None, *mats[name])


def test_device_entry_points(mats):
    U.run_device_entry(None, *mats["poisson"])


def test_perturbed_factor():
    U.run_perturbed(None)


def test_host_mirror():
    U.run_host_mirror(None)


@pytest.mark.parametrize("name", ["ref5", "zchain257", "grid", "symlower"])
def test_complex_forms(name):
    U.run_complex(None, name)


@pytest.mark.parametrize("name", ["random200", "symlower"])
def test_complex_reproducible(name):
    U.run_complex_reproducible(None, name)


@pytest.mark.parametrize("name", ["random200", "grid"])
def test_complex_plain_real_equivalent_factor(name):
    U.run_complex_reproducible(None, name, env={"HIPMF_COMPLEX_PAIRS": "0"})


def test_complex_no_side_effects():
    U.run_complex_no_side_effects(None)


def test_complex_status_codes():
    U.run_complex_status_codes(None)


def test_complex_host_mirror():
    U.run_complex_host_mirror(None)


def test_grid_300x200_tiled_fronts():
    """A(s) = L + s I + C on the 300 x 200 grid, the factor of A(1), the values of A(2); 17 columns: a full block and a block of one.
    Forward error against a direct sparse LU of A(2)^T with the DERIVED bound cond_2 <= (8 + s + 0.6) / s = 5.3: sigma_min(A) >= the
    smallest eigenvalue of the symmetric part L + s I >= s, and |A|_2 <= |L|_2 + s + |C|_inf <= 8 + s + 0.6."""
    nx, ny, s1 = 300, 200, 2.0
    init, vals = U.conv_grid(nx, ny)
    n, rp, ci = init
    v0, v1 = vals(1.0), vals(s1)
    At = sp.csr_matrix((v1, ci, rp), shape=(n, n)).T.tocsr()
    At.sort_indices()
    B = np.array([T.rhs_for(n, 12), U.eig_t(1, 1, nx, ny), U.eig_t(3, 5, nx, ny) + U.eig_t(20, 11, nx, ny), np.zeros(n)] + [T.rhs_for(n, 300 + c) for c in range(13)])
    s = T.handle(None, init, dict(values=v0), v0)
    try:
        assert s.stats()["max_front"] > 256 and s.counter("symmetric_ldlt") == 0
        fb = s.stats()["fused_fallbacks"]
        X, steps, relres, status = s.solve_updated_many(B, v1, rel_tol=TOL, transpose=True)
        print("steps %s in %d cycle(s)" % (steps.tolist(), s.counter("updated_cycles")))
        assert status == 0 and s.stats()["fused_fallbacks"] == fb and s.counter("updated_blocks") == 2
        assert steps[1] == 1 and steps[2] <= 3 and steps[3] == 0 and not X[3].any() and steps[0] > steps[2]
        lu = spla.splu(At.tocsc())
        cond = (8.0 + s1 + 0.6) / s1
        for c in range(17):
            if c == 3:
                continue
            own, bound, bound_double = sparse_relres(n, At.indptr, At.indices, At.data, X[c], B[c])
            print("column %d: reported %.3e, own %.3e, rounding bounds %.3e (own) %.3e (double)" % (c, relres[c], own, bound, bound_double))
            assert bound < TOL and own <= 2 * TOL and relres[c] <= TOL and abs(relres[c] - own) <= bound + bound_double, c
            xd = lu.solve(B[c])
            err = np.linalg.norm(X[c] - xd) / np.linalg.norm(xd)
            assert err <= cond * 2 * TOL, (c, err)
        X2, steps2, relres2, status2 = s.solve_updated_many(B, v1, rel_tol=TOL, transpose=True)
        assert status2 == 0 and np.array_equal(steps, steps2) and np.array_equal(U.u64(relres), U.u64(relres2)) and np.array_equal(U.u64(X), U.u64(X2))
    finally:
        s.close()


@pytest.mark.parametrize("conjugate", [1, 0])
def test_complex_grid_120x100_tiled_fronts(conjugate):
    """the complex twin: K(1) -> K(0.5) on the 120 x 100 shifted grid with unsymmetric values, 16 columns, against a second handle that
    factorises the new values and calls complex_solver_hipmf_solve_transpose_many (itself held to the rule of
    tests/test_complex_transpose_many_cpu.py against its single solves).  The distance of the two solutions of one system is bounded by
    their residuals, |x - xf| / |xf| <= cond_2 (relres(x) + relres(xf)), with the DERIVED bound cond_2 <= 6.3: the Hermitian part of
    K(h) is alpha / h I + sym(L'), L' the Laplacian with entries scaled by factors in [0.7, 1.3], whose symmetric part has, by Gershgorin,
    eigenvalues >= 4 x 0.7 - 4 x 1.3 = -2.4, so sigma_min >= alpha / h - 2.4 = 2.96; |K|_2 <= |alpha + i beta| / h + sqrt(|L'|_1 |L'|_inf)
    <= 8.13 + 10.4."""
    h1 = 0.5
    n, rp, ci, vals = Z.shifted_grid(120, 100, unsym=True)
    v0, v1 = vals(1.0), vals(h1)
    B = np.array([Z.rhs_for(n, 400 + c) for c in range(16)])
    s, f = U.ZT(None, n, rp, ci, v0), ZTM(None, n, rp, ci, v1, nstep=-1)
    try:
        assert s.stats()[0][6] > 256  # max_front
        X, steps, relres, status = s.solve_updated_t_many(B, v1, conjugate, rel_tol=TOL)
        print("conjugate %d: steps %s" % (conjugate, steps.tolist()))
        assert status == 0 and s.counter("fused_fallbacks") == 0 and s.counter("updated_blocks") == 1
        O1 = Z.full(n, rp, ci, v1)
        O1 = sp.csr_matrix(O1.conj().T if conjugate else O1.T)
        XF = f.solve_transpose_many(B, conjugate)
        assert f.counter("transposed_blocks") == 1
        check_against_single(n, XF[:2], [f.solve_transpose(B[c], conjugate) for c in range(2)], "second handle")
        cond = (abs(complex(Z.ALPHA, Z.BETA)) / h1 + 10.4) / (Z.ALPHA / h1 - 2.4)
        assert cond <= 6.3
        for c in range(16):
            own, bound, bound_double = Z.own_relres(O1, X[c], B[c])
            own_f, bound_f, _ = Z.own_relres(O1, XF[c], B[c])
            assert bound < TOL and own <= 2 * TOL and relres[c] <= TOL and abs(relres[c] - own) <= bound + bound_double, c
            err = np.linalg.norm(X[c] - XF[c]) / np.linalg.norm(XF[c])
            print("column %d: reported %.3e, own %.3e, second handle's %.3e, distance %.3e" % (c, relres[c], own, own_f, err))
            assert err <= cond * (own + bound + own_f + bound_f), (c, err)
        X2, steps2, relres2, _ = s.solve_updated_t_many(B, v1, conjugate, rel_tol=TOL)
        assert np.array_equal(steps, steps2) and np.array_equal(bits(relres), bits(relres2)) and np.array_equal(bits(X), bits(X2))
    finally:
        s.close()
        f.close()
