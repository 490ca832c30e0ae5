"""Transposed solves and the MUMPS-style error analysis on the MI355X, through the C-ABI: the cases of
tests/test_transpose_solve_cpu.py on the device, a matrix zoo (golden files, the families of tests/test_matrix_zoo_gpu.py -- generators
copied here --, every front kind, the +-1 family with replaced pivots and the transposed Krylov rescue), large factors (the 1M-unknown
convection-diffusion matrix, a 3D factor whose top front exceeds the LDS staging of the level-set kernels), the complex twin (A^T, A^H),
interleaving with the tagged default solve, repeatability, and the error analysis on the device."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from helpers import read_mtx
from russell_amd import problems as P
from russell_amd._capi import load
from russell_amd.backend import Hipmf
from test_transpose_solve_cpu import CASES, _constructed_i2_case, _from_dense, check_error_analysis, error_analysis_numpy, mumps_5x5

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mtx")


def _arrays(A):
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64), A


def _handle(n, rp, ci, v, **kw):
    s = Hipmf()
    assert s.initialize(n, rp, ci, values=v, **kw) == 0
    code = s.factorize(v)
    assert code == 0, code
    return s


def _omega_t(A, x, b):
    """componentwise backward error of x as a solution of A^T x = b"""
    At = sp.csr_matrix(A.T)
    r = b - At @ x
    den = abs(At) @ np.abs(x) + np.abs(b)
    return float(np.max(np.where(den > 0, np.abs(r) / np.where(den > 0, den, 1.0), np.where(r != 0, np.inf, 0.0))))


# ---- the CPU cases on the device ----
@pytest.mark.parametrize("name", sorted(CASES))
def test_cpu_cases_on_device(name):
    n, rp, ci, v = CASES[name]()
    n, rp, ci, v, A = _arrays(sp.csr_matrix((v, ci, rp), shape=(n, n)))
    s = _handle(n, rp, ci, v)
    b = np.random.default_rng(3).standard_normal(n)
    x = s.solve_transpose(b)
    xr = spla.spsolve(A.T.tocsc(), b)
    assert np.abs(x - xr).max() <= 1e-11 * np.abs(xr).max()
    assert np.array_equal(x, s.solve_transpose(b))  # repeatable
    u = np.random.default_rng(4).standard_normal(n)
    lhs, rhs = b @ s.solve(u), x @ u  # adjointness
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
    s.close()


def test_mumps_5x5_on_device():
    (n, rp, ci, v), b = mumps_5x5()
    D = sp.csr_matrix((v, ci, rp), shape=(n, n)).toarray()
    s = _handle(n, rp, ci, v)
    assert np.abs(s.solve_transpose(b) - np.linalg.solve(D.T, b)).max() <= 1e-11 * 5.0
    x0 = s.solve(b)
    x, ea = s.solve_with_error_analysis(b, 1)
    assert np.array_equal(x, x0)
    check_error_analysis(ea, error_analysis_numpy(D, b, x)[0])
    s.close()


# ---- matrix zoo (generators of tests/test_matrix_zoo_gpu.py) ----
def _convdiff(nx, ny, rng):
    n = nx * ny
    idx = lambda i, j: i + j * nx
    rows, cols, vals = [], [], []
    for j in range(ny):
        for i in range(nx):
            x, y = (i + 0.5) / nx, (j + 0.5) / ny
            bx, by = 200.0 * np.sin(np.pi * x) * np.cos(np.pi * y), -200.0 * np.cos(np.pi * x) * np.sin(np.pi * y)
            d = 4.0
            for (di, dj, b) in ((1, 0, bx), (-1, 0, -bx), (0, 1, by), (0, -1, -by)):
                ii, jj = i + di, j + dj
                c = -1.0 + min(b, 0.0) / max(nx, ny)
                d += max(b, 0.0) / max(nx, ny)
                if 0 <= ii < nx and 0 <= jj < ny:
                    rows.append(idx(i, j)), cols.append(idx(ii, jj)), vals.append(c)
            rows.append(idx(i, j)), cols.append(idx(i, j)), vals.append(d)
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    return sp.diags(10.0 ** rng.uniform(-4, 4, n)) @ A


def _circuit(n, rng):
    m = n // 8
    G = sp.random(n - m, n - m, density=4.0 / n, random_state=int(rng.integers(1 << 30)), format="csr")
    G = G + G.T
    G = G + sp.diags(np.asarray(abs(G).sum(axis=1)).ravel() + 1e-3)
    B = sp.csr_matrix((np.ones(m), (rng.choice(n - m, m, replace=False), np.arange(m))), shape=(n - m, m))
    return sp.bmat([[G, B], [B.T, None]], format="csr")


def _shuffled(n, rng):
    D = (sp.random(n, n, density=5.0 / n, random_state=int(rng.integers(1 << 30)), format="csr") + sp.diags(3.0 + rng.random(n))).tocsr()
    Pm = sp.csr_matrix((np.ones(n), (rng.permutation(n), np.arange(n))), shape=(n, n))
    return (Pm @ D).tocsr()


def _weak_random(n, rng):
    return (sp.random(n, n, density=6.0 / n, random_state=int(rng.integers(1 << 30)), format="csr") + sp.diags(0.05 * rng.standard_normal(n))).tocsr()


def _anisotropic3d(k, rng):
    T = lambda m, a: sp.diags([-a, 2 * a, -a], [-1, 0, 1], shape=(m, m))
    I = sp.identity
    A = sp.kron(sp.kron(I(k), I(k)), T(k, 1.0)) + sp.kron(sp.kron(I(k), T(k, 1e-3)), I(k)) + sp.kron(sp.kron(T(k, 1e3), I(k)), I(k))
    return A.tocsr()


def _pm1(n, k, rng):
    rows = np.repeat(np.arange(n), k)
    A = sp.csr_matrix((rng.choice([-1.0, 1.0], n * k), (rows, rng.integers(0, n, n * k))), shape=(n, n))
    A = A + sp.csr_matrix((rng.choice([-1.0, 1.0], n), (np.arange(n), rng.permutation(n))), shape=(n, n))
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    return A.tocsr()


def _problem(t):
    n, rp, ci, v = t
    return sp.csr_matrix((v, ci, rp), shape=(n, n))


def _golden(name):
    (nr, nc, _), r, c, v, sym = read_mtx(os.path.join(GOLDEN, name + ".mtx"))
    A = sp.coo_matrix((v, (r, c)), shape=(nr, nc)).tocsr()
    if sym:
        A = A + sp.tril(A, -1).T
    return A


ZOO = {
    "golden_bfwb62": lambda rng: _golden("bfwb62"),
    "golden_ok_general": lambda rng: _golden("ok_general"),
    "golden_ok_simple_general": lambda rng: _golden("ok_simple_general"),
    "convection_diffusion_scaled": lambda rng: _convdiff(48, 40, rng),
    "circuit_mna_zero_diagonal": lambda rng: _circuit(2400, rng),
    "row_shuffled_dominant": lambda rng: _shuffled(3000, rng),
    "random_weak_diagonal": lambda rng: _weak_random(1500, rng),
    "anisotropic_3d": lambda rng: _anisotropic3d(14, rng),
    "convection_diffusion_matching": lambda rng: _problem(P.convection_diffusion2d(60, peclet=30, scale_decades=6.0)),
}


@pytest.mark.parametrize("name", sorted(ZOO))
def test_zoo_backward_error(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    n, rp, ci, v, A = _arrays(ZOO[name](rng))
    s = _handle(n, rp, ci, v)
    b = A.T @ rng.standard_normal(n)
    x = s.solve_transpose(b)
    assert _omega_t(A, x, b) <= 64 * EPS, (name, _omega_t(A, x, b))
    if name.startswith("golden"):
        xr = np.linalg.solve(A.toarray().T, b)
        assert np.abs(x - xr).max() <= 1e-6 * max(1.0, np.abs(xr).max())
    s.close()


def test_every_front_kind_is_reached():
    """small fronts (f <= 64) everywhere; mid fronts (one workgroup, FD_DENSE_TOP) and tiled fronts on these cases"""
    n, rp, ci, v = P.poisson2d(44, 40)
    s = _handle(n, rp, ci, v)
    assert s.counter("mid_fronts") > 0
    s.close()
    n, rp, ci, v = P.poisson2d(200, 200)
    n, rp, ci, v, A = _arrays(sp.csr_matrix((v, ci, rp), shape=(n, n)) + sp.diags(np.linspace(0.0, 1.0, n), 1, shape=(n, n)))
    s = _handle(n, rp, ci, v)
    st = s.stats()
    assert st["max_front"] > 64 and st["max_pivots"] > 64  # (more pivots than any one-workgroup front takes, MID_PMAX = 64: tiled)
    b = np.random.default_rng(8).standard_normal(n)
    x = s.solve_transpose(b)
    assert _omega_t(A, x, b) <= 64 * EPS
    xr = spla.spsolve(A.T.tocsc(), b)
    assert np.abs(x - xr).max() <= 1e-10 * np.abs(xr).max()
    s.close()


@pytest.mark.parametrize("seed,n,k", [(100, 800, 4), (102, 1400, 6), (107, 6000, 4)])
def test_pm1_family_transposed_rescue(seed, n, k):
    rng = np.random.default_rng(seed)
    A = _pm1(n, k, rng)
    n, rp, ci, v, A = _arrays(A)
    xs = rng.standard_normal(n)
    b = A.T @ xs
    e_ref = float(np.max(np.abs(spla.splu(A.T.tocsc()).solve(b) - xs)) / np.max(np.abs(xs)))
    s = _handle(n, rp, ci, v)
    assert s.num_perturbed > 0, seed  # (replaced pivots: the rescue's trigger)
    x = s.solve_transpose(b)
    assert float(np.max(np.abs(x - xs)) / np.max(np.abs(xs))) <= 10.0 * e_ref + 1e-12, (seed, s.num_perturbed, s.counter("transposed_krylov_iterations"))
    s.close()


@pytest.mark.parametrize("seed,n,k", [(100, 800, 4), (102, 1400, 6)])
def test_transposed_rescue_runs_without_refinement(seed, n, k):
    """With refinement switched off (refinement_nstep = 0) every transposed solve after a factorisation that replaced pivots goes through
    the FGMRES rescue with A^T as the operator and the transposed pass pair as the preconditioner: it must run and reach SuperLU's
    accuracy, and the ordinary solve's rescue statistics stay the ordinary solve's."""
    rng = np.random.default_rng(seed)
    n, rp, ci, v, A = _arrays(_pm1(n, k, rng))
    xs = rng.standard_normal(n)
    b = A.T @ xs
    e_ref = float(np.max(np.abs(spla.splu(A.T.tocsc()).solve(b) - xs)) / np.max(np.abs(xs)))
    s = _handle(n, rp, ci, v, refinement_nstep=0)
    assert s.num_perturbed > 0
    s.solve(A @ xs)
    k_ordinary = s.counter("krylov_iterations")
    x = s.solve_transpose(b)
    assert s.counter("transposed_krylov_iterations") > 0
    assert s.counter("krylov_iterations") == k_ordinary
    assert float(np.max(np.abs(x - xs)) / np.max(np.abs(xs))) <= 10.0 * e_ref + 1e-12, (seed, s.counter("transposed_krylov_iterations"))
    s.close()


# ---- large factors ----
def _cd3d(k, peclet=20.0):
    """7-point convection-diffusion on a k^3 grid (unsymmetric), built with kron as _anisotropic3d"""
    h = 1.0 / (k + 1)
    T = sp.diags([-1.0 - 0.5 * peclet * h, 2.0, -1.0 + 0.5 * peclet * h], [-1, 0, 1], shape=(k, k))
    D = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(k, k))
    I = sp.identity(k)
    return (sp.kron(sp.kron(I, I), T) + sp.kron(sp.kron(I, D), I) + sp.kron(sp.kron(D, I), I)).tocsr()


def _large_check(A, min_front=0):
    n, rp, ci, v, A = _arrays(A)
    s = _handle(n, rp, ci, v)
    assert s.stats()["max_front"] > min_front, s.stats()["max_front"]
    rng = np.random.default_rng(12)
    b, u = rng.standard_normal(n), rng.standard_normal(n)
    x = s.solve_transpose(b)
    assert _omega_t(A, x, b) <= 64 * EPS
    lhs, rhs = b @ s.solve(u), x @ u
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs))
    s.close()


def test_c2_convection_diffusion_1m():
    n, rp, ci, v = P.convection_diffusion2d(1000)
    _large_check(sp.csr_matrix((v, ci, rp), shape=(n, n)))


def test_3d_top_front_beyond_lds_staging():
    _large_check(_cd3d(96), min_front=7936)


# ---- complex twin ----
def _read_complex_mtx(name):
    rows, cols, vals, dims = [], [], [], None
    with open(os.path.join(GOLDEN, name + ".mtx")) as fh:
        sym = fh.readline().split()[4].lower() == "symmetric"
        for line in fh:
            t = line.strip()
            if not t or t.startswith("%"):
                continue
            a = t.split()
            if dims is None:
                dims = [int(q) for q in a]
                continue
            rows.append(int(a[0]) - 1), cols.append(int(a[1]) - 1), vals.append(float(a[2]) + 1j * float(a[3]))
    A = sp.coo_matrix((vals, (rows, cols)), shape=(dims[0], dims[1])).tocsr()
    return A, sym


def _zcsr(A):
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), np.ascontiguousarray(np.stack([A.data.real, A.data.imag], axis=1).ravel())


def _complex_case(A, lower=False):
    lib = load()
    h = lib.complex_solver_hipmf_new()
    n = A.shape[0]
    rp, ci, zv = _zcsr(sp.tril(A).tocsr() if lower else A)
    assert lib.complex_solver_hipmf_initialize(h, 0, 1, -1.0, -1, 0, int(lower), n, rp, ci, zv.ctypes.data) == 0
    npert = C.c_int32()
    assert lib.complex_solver_hipmf_factorize(h, None, None, C.byref(npert), None, None, None, None, 0, 0, zv) == 0
    Af = sp.csr_matrix(A) if not lower else sp.csr_matrix(sp.tril(A) + sp.tril(A, -1).T)
    rng = np.random.default_rng(5)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    bi = np.ascontiguousarray(np.stack([b.real, b.imag], axis=1).ravel())
    D = Af.toarray()
    for conj, M in ((0, D.T), (1, D.conj().T)):
        x = np.zeros(2 * n)
        assert lib.complex_solver_hipmf_solve_transpose(h, x, bi, conj, 0) == 0
        z = x[0::2] + 1j * x[1::2]
        zr = np.linalg.solve(M, b)
        assert np.abs(z - zr).max() <= 1e-9 * max(1.0, np.abs(zr).max()), conj
    x = np.zeros(2 * n)
    assert lib.complex_solver_hipmf_solve_transpose(h, x, bi, 2, 0) == 803
    lib.complex_solver_hipmf_drop(h)


def test_complex_golden_general():
    A, _ = _read_complex_mtx("ok_complex_general")
    _complex_case(A)


def test_complex_symmetric_lower_handle():
    A, sym = _read_complex_mtx("ok_complex_symmetric_small")
    assert sym
    _complex_case(sp.csr_matrix(sp.tril(A) + sp.tril(A, -1).T), lower=True)


def test_complex_random_convection_diffusion():
    n0, rp, ci, v = P.convection_diffusion2d(50, peclet=20)
    A = sp.csr_matrix((v, ci, rp), shape=(n0, n0)) * (1.0 + 0.3j) + 0.2j * sp.identity(n0)
    _complex_case(sp.csr_matrix(A))


# ---- interleaving with the tagged default solve, repeatability ----
def test_interleaving_keeps_the_tagged_solve_bits():
    n, rp, ci, v = P.convection_diffusion2d(1000)
    s = _handle(n, rp, ci, v)
    assert s.counter("tagged_solve") == 1  # (the default single-column path: data-tagged hand-offs)
    b = np.random.default_rng(21).standard_normal(n)
    fb0 = s.counter("fused_fallbacks")
    x1 = s.solve(b)
    t1 = s.solve_transpose(b)
    x2 = s.solve(b)
    t2 = s.solve_transpose(b)
    assert np.array_equal(x1, x2)
    assert np.array_equal(t1, t2)
    assert s.counter("fused_fallbacks") == fb0
    _, e1 = s.solve_with_error_analysis(b, 2)
    _, e2 = s.solve_with_error_analysis(b, 2)
    assert np.array_equal(e1, e2)
    s.close()


# ---- error analysis on the device ----
def test_error_analysis_convection_diffusion_60():
    n, rp, ci, v = P.convection_diffusion2d(60, peclet=30)
    D = sp.csr_matrix((v, ci, rp), shape=(n, n)).toarray()
    s = _handle(n, rp, ci, v)
    b = np.random.default_rng(4).standard_normal(n)
    x0 = s.solve(b)
    x, ea = s.solve_with_error_analysis(b, 1)
    assert np.array_equal(x, x0)
    check_error_analysis(ea, error_analysis_numpy(D, b, x)[0])
    x2, ea2 = s.solve_with_error_analysis(b, 1)
    assert np.array_equal(x2, x) and np.array_equal(ea2, ea)
    s.close()


def test_error_analysis_constructed_i2():
    D, b = _constructed_i2_case()
    n, rp, ci, v = _from_dense(D)
    s = _handle(n, rp, ci, v)
    x, ea = s.solve_with_error_analysis(b, 1)
    ref, has_i2 = error_analysis_numpy(D, b, x)
    assert has_i2 and ea[7] > 0.0
    check_error_analysis(ea, ref)
    s.close()


def test_error_analysis_c2_solve_budget():
    n, rp, ci, v = P.convection_diffusion2d(1000)
    s = _handle(n, rp, ci, v)
    b = np.random.default_rng(2).standard_normal(n)
    x0 = s.solve(b)
    x, ea = s.solve_with_error_analysis(b, 1)
    assert np.array_equal(x, x0)
    assert 0 < s.counter("analysis_solves") <= 22
    assert np.all(np.isfinite(ea)) and ea[6] >= 1.0
    s.close()
