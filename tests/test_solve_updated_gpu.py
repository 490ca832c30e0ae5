"""Solve with new matrix values on a kept factor on the MI355X: the cases of tests/test_solve_updated_cpu.py through the product build (its
run_* functions with lib = None, its reference and its accuracy rule), the 300 x 200 grid -- tiled fronts: the pass pair inside the
iteration takes the dependency-driven schedule -- against the CPU oracle, and the 1M-DOF grid through device pointers."""
import numpy as np
import pytest

import test_solve_updated_cpu as T
from russell_amd import problems as P
from test_gpu_parity import oracle_solve

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mats():
    return T.matrices()


@pytest.mark.parametrize("name", T.ALL)
def test_unchanged_values_take_one_step(mats, name):
    T.run_unchanged(None, *mats[name])


@pytest.mark.parametrize("name", T.GENERAL)
def test_rank_three_change(mats, name):
    T.run_rank_change(None, *mats[name])


def test_diagonal_shift_by_two():
    steps, _ = T.run_shift(None, 2.0)
    assert steps >= T.PASSV + 2


def test_diagonal_shift_by_hundred_restart_four(monkeypatch):
    steps, _ = T.run_shift(None, 100.0, restart=4, max_steps=400, monkeypatch=monkeypatch)
    assert steps > 8


@pytest.mark.parametrize("restart", [T.PASSV, T.PASSV - 1])
def test_basis_count_edges(monkeypatch, restart):
    steps, ref_steps = T.run_shift(None, 2.0, restart=restart, max_steps=200, monkeypatch=monkeypatch)
    assert ref_steps >= T.PASSV + 2 and steps > restart


def test_not_converged():
    T.run_not_converged(None)


@pytest.mark.parametrize("name", ["poisson", "poisson_lower", "saddle"])
def test_mapped_values(mats, name):
    T.run_mapped(None, *mats[name])


@pytest.mark.parametrize("name", ["poisson", "poisson_lower", "saddle"])
def test_no_side_effects(mats, name):
    T.run_no_side_effects(None, *mats[name])


@pytest.mark.parametrize("name", ["bfwb62", "poisson_lower"])
def test_reproducible(mats, name):
    T.run_reproducible(None, *mats[name])


def test_perturbed_factor():
    T.run_perturbed(None)


@pytest.mark.parametrize("name", ["poisson", "poisson_lower"])
def test_device_entry_point(mats, name):
    T.run_device_entry(None, *mats[name])


def shifted_grid(nx, ny, lower):
    """(initialize arguments, keywords, shift -> values in the handle's order, shift -> the full CSR matrix's values, the full structure)"""
    n, rp, ci, v = P.poisson2d(nx, ny)
    diag_full = np.repeat(np.arange(n), np.diff(rp)) == ci
    if not lower:
        return (n, rp, ci), {}, (lambda s: v + s * diag_full), (lambda s: v + s * diag_full), (n, rp, ci)
    lrp, lci, lv = P.lower_triangle(n, rp, ci, v)
    diag = np.repeat(np.arange(n), np.diff(lrp)) == lci
    return (n, lrp, lci), dict(general_symmetric=True), (lambda s: lv + s * diag), (lambda s: v + s * diag_full), (n, rp, ci)


def sparse_relres(n, rp, ci, v, x, b):
    """T.own_relres for a CSR matrix: the recomputation in extended precision, its rounding bound and the same bound for double"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    ax = np.zeros(n, T.LD)
    np.add.at(ax, rows, v.astype(T.LD) * x.astype(T.LD)[ci])
    r = b.astype(T.LD) - ax
    bnorm = float(np.sqrt(b.astype(T.LD) @ b.astype(T.LD)))
    scale = float(np.linalg.norm(np.bincount(rows, np.abs(v) * np.abs(x)[ci], n))) / bnorm
    return float(np.sqrt(r @ r)) / bnorm, n * T.EPS_LD * scale, n * T.EPS * scale


def cond2_shifted_laplacian(nx, ny, s):
    """cond_2 of the 5-point Laplacian on an nx x ny grid (Dirichlet) + s I: symmetric positive definite, eigenvalues known in closed form"""
    lx = 2.0 - 2.0 * np.cos(np.pi * np.arange(1, nx + 1) / (nx + 1))
    ly = 2.0 - 2.0 * np.cos(np.pi * np.arange(1, ny + 1) / (ny + 1))
    lam = np.add.outer(lx, ly) + s
    return float(lam.max() / lam.min())


def test_closed_form_condition_number():
    """the formula above against NumPy's cond on a small grid"""
    n, rp, ci, v = P.poisson2d(9, 7)
    import scipy.sparse as sp
    A = (sp.csr_matrix((v, ci, rp), shape=(n, n)) + 2.0 * sp.identity(n)).toarray()
    assert abs(cond2_shifted_laplacian(9, 7, 2.0) - np.linalg.cond(A)) <= 1e-10 * np.linalg.cond(A)


@pytest.mark.parametrize("lower", [False, True])
def test_grid_300x200_diagonal_shift_against_the_oracle(lower):
    """60 000 unknowns, tiled fronts of several hundred rows (LU and L D L^T): A_old = L + I, A_new = L + 2 I"""
    init, kw, vals, full, (n, rp, ci) = shifted_grid(300, 200, lower)
    s = T.handle(None, init, kw, vals(1.0))
    try:
        assert s.stats()["max_front"] > 256 and s.counter("symmetric_ldlt") == int(lower)
        b = T.rhs_for(n, 12)
        fb = s.stats()["fused_fallbacks"]
        x, steps, relres, status = s.solve_updated(b, vals(2.0), rel_tol=T.TOL)
        print("%d steps, relres %.3e" % (steps, relres))
        assert status == 0 and s.stats()["fused_fallbacks"] == fb
        own, bound, bound_double = sparse_relres(n, rp, ci, full(2.0), x, b)
        print("own relres %.3e, rounding bound %.3e" % (own, bound))
        assert bound < T.TOL and own <= 2 * T.TOL and relres <= T.TOL and abs(relres - own) <= bound + bound_double
        xo, _ = oracle_solve(n, rp, ci, full(2.0), b, q=s.permutation())
        err, cond = np.linalg.norm(x - xo) / np.linalg.norm(xo), cond2_shifted_laplacian(300, 200, 2.0)
        print("forward error %.3e, cond_2 %.3e" % (err, cond))
        assert err <= cond * 2 * T.TOL
    finally:
        s.close()


def test_1m_dof_diagonal_shift_through_device_pointers():
    """BASELINE config 2 as a lower triangle, A_old = L + I, A_new = L + 2 I, default tolerance 1e-12.  A_new A_old^{-1} is a normal matrix
    with spectrum in [1, 2]: the Chebyshev bound 2 ((sqrt 2 - 1) / (sqrt 2 + 1))^k <= 1e-12 holds from k = 17."""
    init, kw, vals, full, (n, rp, ci) = shifted_grid(1000, 1000, True)
    s = T.handle(None, init, kw, vals(1.0))
    ptrs = []
    try:
        b, v1 = T.rhs_for(n, 13), vals(2.0)
        d_x, d_b, d_v = s.dev_alloc(8 * n), s.dev_alloc(8 * n), s.dev_alloc(8 * v1.size)
        ptrs += [d_x, d_b, d_v]
        s.h2d(d_b, b)
        s.h2d(d_v, v1)
        out = []
        for _ in range(2):
            steps, relres, status = s.solve_updated_device(d_x, d_b, d_v)
            x = np.zeros(n)
            s.d2h(x, d_x)
            out.append((steps, relres, status, x))
        steps, relres, status, x = out[0]
        print("%d steps in %d cycle(s), relres %.3e" % (steps, s.counter("updated_cycles"), relres))
        assert status == 0 and steps <= 17 and relres <= 1e-12
        assert out[1][:3] == out[0][:3] and np.array_equal(out[1][3].view(np.uint64), x.view(np.uint64))
        assert s.counter("fused_fallbacks") == 0
        assert s.counter("updated_basis_bytes") == 61 * n * 8
        own, bound, bound_double = sparse_relres(n, rp, ci, full(2.0), x, b)
        print("own relres %.3e (rounding bounds %.3e own, %.3e double)" % (own, bound, bound_double))
        assert abs(relres - own) <= bound + bound_double
    finally:
        for p in ptrs:
            s.dev_free(p)
        s.close()
