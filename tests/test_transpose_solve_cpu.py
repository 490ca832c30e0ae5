"""Transposed solves (solver_hipmf_solve_transpose, kernels_solve_transpose.hpp) and the MUMPS-style error analysis
(solver_hipmf_solve_with_error_analysis) on the CPU emulator of the HIP kernels: against scipy's solves of A^T, against a numpy
restatement of the pinned definitions (include/russell_hipmf.h), bit-for-bit against the ordinary solve where A^T = A, and the status
codes.  tests/test_transpose_solve_gpu.py repeats the cases on the device."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from russell_amd import problems as P
from russell_amd.backend import Hipmf, HipmfError

EPS = np.finfo(float).eps
ERROR_NULL_POINTER, ERROR_NEED_FACTORIZATION, ERROR_HIPMF_INVALID_VALUE = 100000, 600000, 803


def _csr(n, rp, ci, v):
    A = sp.csr_matrix((np.asarray(v, float), np.asarray(ci), np.asarray(rp)), shape=(n, n))
    return A


def _from_dense(D):
    A = sp.csr_matrix(D)
    A.sort_indices()
    return A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def mumps_5x5():
    """the system of the reference's examples/mumps_solve_small.rs"""
    D = np.array([[2, 3, 0, 0, 0], [3, 0, 4, 0, 6], [0, -1, -3, 2, 0], [0, 0, 1, 0, 0], [0, 4, 2, 0, 1]], float)
    return _from_dense(D), np.array([8.0, 45.0, -3.0, 3.0, 19.0])


def _omega(s):
    """HIPMF_OPTION_ERROR_ESTIMATES read back: omega of the last solve"""
    val = C.c_double()
    assert s.lib.solver_hipmf_get_option(s.h, 3, C.byref(val)) == 0
    return val.value


def _handle(lib, n, rp, ci, v, **kw):
    s = Hipmf(lib)
    assert s.initialize(n, rp, ci, values=v, **kw) == 0
    assert s.factorize(v) == 0
    return s


def exact_residual(D, b, x):
    """b - D x in rational arithmetic, rounded once (the kernel's residual is accurate to about that: twice the working precision)"""
    r = np.zeros(len(b))
    for i in range(len(b)):
        t = Fraction(float(b[i]))
        for j in np.nonzero(D[i])[0]:
            t -= Fraction(float(D[i, j])) * Fraction(float(x[j]))
        r[i] = float(t)
    return r


def error_analysis_numpy(D, b, x):
    """The pinned definitions (include/russell_hipmf.h), restated with the explicit dense inverse (exact |A^{-1}| w)."""
    n = D.shape[0]
    absA = np.abs(D)
    a = absA.sum(axis=1)
    NA, NX = a.max(), np.abs(x).max()
    r = exact_residual(D, b, x)
    ax = absA @ np.abs(x)
    d = ax + np.abs(b)
    tau = 1000.0 * n * EPS * (a * NX + np.abs(b))
    I1 = d > tau
    I2 = ~I1
    out = np.zeros(8)
    out[0], out[1] = NA, NX
    out[2] = np.abs(r).max() / (NA * NX) if NA * NX > 0 else 0.0
    out[3] = (np.abs(r[I1]) / d[I1]).max() if I1.any() else 0.0
    if I2.any():
        den2 = ax[I2] + a[I2] * NX
        rr = np.abs(r[I2])
        out[4] = np.where(rr == 0.0, 0.0, rr / np.where(den2 == 0.0, 1.0, den2)).max()
    Ainv = np.abs(np.linalg.inv(D))
    w1 = np.where(I1, d, 0.0)
    w2 = np.where(I2, ax + a * NX, 0.0)
    out[6] = np.abs(Ainv @ w1).max() / NX
    out[7] = np.abs(Ainv @ w2).max() / NX if I2.any() else 0.0
    out[5] = out[3] * out[6] + out[4] * out[7]
    return out, I2.any()


def check_error_analysis(ea, ref):
    for k in range(5):
        assert ea[k] == pytest.approx(ref[k], rel=1e-12, abs=1e-300), (k, ea[k], ref[k])
    for k in (6, 7):
        assert ref[k] / 10.0 <= ea[k] <= ref[k] * (1.0 + 1e-10), (k, ea[k], ref[k])
    assert ea[5] == pytest.approx(ea[3] * ea[6] + ea[4] * ea[7], rel=1e-14, abs=1e-300)


CASES = {
    "poisson_12x9_small_fronts": lambda: P.poisson2d(12, 9),
    "poisson_44x40_mid_fronts": lambda: P.poisson2d(44, 40),
    "convection_diffusion_40_pe30": lambda: P.convection_diffusion2d(40, peclet=30),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_transpose_against_scipy(emu_lib, name):
    n, rp, ci, v = CASES[name]()
    A = _csr(n, rp, ci, v)
    s = _handle(emu_lib, n, rp, ci, v)
    b = np.random.default_rng(3).standard_normal(n)
    x = s.solve_transpose(b)
    xr = spla.spsolve(A.T.tocsc(), b)
    assert np.abs(x - xr).max() <= 1e-11 * np.abs(xr).max()
    # same bits on a repeat call; the counter counts both
    assert np.array_equal(x, s.solve_transpose(b))
    assert s.counter("transposed_solves") == 2
    s.close()


@pytest.mark.parametrize("mid", ["1", "0"])
def test_transpose_on_mid_and_tiled_fronts(emu_lib, monkeypatch, mid):
    """Big fronts in both forms of E / E': one-workgroup (mid) fronts, FD_DENSE_TOP, and -- with HIPMF_MID_FRONT=0 -- the tiled form,
    whose pivot rows of E are block lower triangular (the GEMV skips the blocks above column c's 32-row block) and whose inv(U11) in E'
    is upper triangular.  More than 32 pivots: the skip is taken."""
    monkeypatch.setenv("HIPMF_MID_FRONT", mid)
    n, rp, ci, v = P.convection_diffusion2d(44, 40, peclet=30)
    A = _csr(n, rp, ci, v)
    s = _handle(emu_lib, n, rp, ci, v)
    st = s.stats()
    assert st["max_front"] > 64 and st["max_pivots"] > 32
    assert (s.counter("mid_fronts") > 0) == (mid == "1")
    b = np.random.default_rng(13).standard_normal(n)
    x = s.solve_transpose(b)
    xr = spla.spsolve(A.T.tocsc(), b)
    assert np.abs(x - xr).max() <= 1e-11 * np.abs(xr).max()
    s.close()


def test_transpose_mumps_5x5(emu_lib):
    (n, rp, ci, v), b = mumps_5x5()
    D = _csr(n, rp, ci, v).toarray()
    s = _handle(emu_lib, n, rp, ci, v)
    x = s.solve_transpose(b)
    assert np.abs(x - np.linalg.solve(D.T, b)).max() <= 1e-11 * np.abs(x).max()
    s.close()


def test_adjointness(emu_lib):
    n, rp, ci, v = P.convection_diffusion2d(40, peclet=30)
    s = _handle(emu_lib, n, rp, ci, v)
    rng = np.random.default_rng(11)
    u, w = rng.standard_normal(n), rng.standard_normal(n)
    lhs = w @ s.solve(u)
    rhs = s.solve_transpose(w) @ u
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
    s.close()


def test_transpose_device_entry_point(emu_lib):
    n, rp, ci, v = P.poisson2d(20, 17)
    A = _csr(n, rp, ci, v)
    s = _handle(emu_lib, n, rp, ci, v)
    B = np.random.default_rng(2).standard_normal((3, n))
    d_b, d_x = s.dev_alloc(B.nbytes), s.dev_alloc(B.nbytes)
    s.h2d(d_b, B)
    s.solve_transpose_device(d_x, d_b, nrhs=3)
    X = np.zeros_like(B)
    s.d2h(X, d_x)
    for k in range(3):
        assert np.abs(X[k] - spla.spsolve(A.T.tocsc(), B[k])).max() <= 1e-11 * np.abs(X[k]).max()
    with pytest.raises(HipmfError) as e:
        s.solve_transpose_device(d_x, d_b, nrhs=0)
    assert e.value.code == ERROR_HIPMF_INVALID_VALUE
    with pytest.raises(HipmfError) as e:
        s.solve_transpose_device(d_x, d_b, nrhs=1, ld=n - 1)
    assert e.value.code == ERROR_HIPMF_INVALID_VALUE
    s.dev_free(d_b), s.dev_free(d_x)
    s.close()


def _constructed_i2_case():
    """Row 0 has b_0 = 0 and its pattern misses the support of x (x_1 = x_2 = 0 there): d_0 = 0, so I2 is not empty and cond2 > 0."""
    D = np.array([[4.0, 1.0, -1.0, 0.0, 0.0], [0.5, 3.0, 0.0, 0.0, 1.0], [0.0, 0.3, 5.0, 1.0, 0.0], [0.0, 0.0, 1.0, 2.0, 0.2], [1.0, 0.0, 0.0, 0.4, 6.0]])
    xs = np.array([0.0, 0.0, 0.0, 1.0, 2.0])
    D[0, 3] = D[0, 4] = 0.0
    return D, D @ xs


@pytest.mark.parametrize("which", ["mumps_5x5", "convection_diffusion_40", "constructed_i2"])
def test_error_analysis_against_numpy(emu_lib, which):
    if which == "mumps_5x5":
        (n, rp, ci, v), b = mumps_5x5()
    elif which == "convection_diffusion_40":
        n, rp, ci, v = P.convection_diffusion2d(40, peclet=30)
        b = np.random.default_rng(4).standard_normal(n)
    else:
        D, b = _constructed_i2_case()
        n, rp, ci, v = _from_dense(D)
    D = _csr(n, rp, ci, v).toarray()
    s = _handle(emu_lib, n, rp, ci, v)
    x0 = s.solve(b)
    omega0 = _omega(s)
    x, ea = s.solve_with_error_analysis(b, 1)
    assert np.array_equal(x, x0)  # the solve is solver_hipmf_solve's, bit for bit
    assert _omega(s) == omega0  # (last_omega: the analysis leaves the solve's statistics alone)
    ref, has_i2 = error_analysis_numpy(D, b, x)
    check_error_analysis(ea, ref)
    assert 0 < s.counter("analysis_solves") <= 22
    if which == "constructed_i2":
        assert has_i2 and ea[7] > 0.0
    # repeatable to the bit
    x2, ea2 = s.solve_with_error_analysis(b, 1)
    assert np.array_equal(x2, x) and np.array_equal(ea2, ea)
    # option 2: entries 0 - 4, the rest keeps what the caller put there; option 0: nothing
    arr = np.full(8, -7.0)
    _, ea3 = s.solve_with_error_analysis(b, 2, array=arr)
    assert np.array_equal(ea3[:5], ea[:5]) and np.all(ea3[5:] == -7.0)
    arr = np.full(8, -7.0)
    _, ea4 = s.solve_with_error_analysis(b, 0, array=arr)
    assert np.all(ea4 == -7.0)
    s.close()


def test_error_analysis_keeps_solve_statistics(emu_lib):
    n, rp, ci, v = P.convection_diffusion2d(30, peclet=30)
    s = _handle(emu_lib, n, rp, ci, v)
    b = np.random.default_rng(9).standard_normal(n)
    s.solve(b)
    st0 = s.stats()
    kry0 = s.counter("krylov_iterations")
    x, ea = s.solve_with_error_analysis(b, 1)
    st1 = s.stats()
    for k in ("refinement_steps", "residual_inf", "solve_launches"):
        assert st1[k] == st0[k], k
    assert s.counter("krylov_iterations") == kry0
    s.close()


def test_ldlt_handle_transpose_is_the_solve(emu_lib):
    n, rp, ci, v = P.poisson2d(30, 28)
    lrp, lci, lv = P.lower_triangle(n, rp, ci, v)
    s = Hipmf(emu_lib)
    assert s.initialize(n, lrp, lci, general_symmetric=True) == 0
    assert s.factorize(lv) == 0
    assert s.counter("symmetric_ldlt") == 1
    b = np.random.default_rng(6).standard_normal(n)
    assert np.array_equal(s.solve_transpose(b), s.solve(b))
    s.close()


def test_status_codes(emu_lib):
    (n, rp, ci, v), b = mumps_5x5()
    s = Hipmf(emu_lib)
    assert s.initialize(n, rp, ci) == 0
    x, ea = np.zeros(n), np.zeros(8)
    lib = s.lib
    assert lib.solver_hipmf_solve_transpose(s.h, x, b, 0) == ERROR_NEED_FACTORIZATION
    assert lib.solver_hipmf_solve_with_error_analysis(s.h, x, b, ea, 1, 0) == ERROR_NEED_FACTORIZATION
    assert lib.solver_hipmf_solve_transpose_device(s.h, C.c_void_p(1), C.c_void_p(1), 1, n) == ERROR_NEED_FACTORIZATION
    assert s.factorize(v) == 0
    raw = C.CDLL(emu_lib)  # (untyped bindings: NULL pointers pass)
    for fn in (raw.solver_hipmf_solve_transpose, raw.solver_hipmf_solve_transpose_device, raw.solver_hipmf_solve_with_error_analysis):
        fn.restype = C.c_int32
    xp, bp, ep = x.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), ea.ctypes.data_as(C.c_void_p)
    h = C.c_void_p(s.h)
    assert raw.solver_hipmf_solve_transpose(None, xp, bp, 0) == ERROR_NULL_POINTER
    assert raw.solver_hipmf_solve_transpose(h, None, bp, 0) == ERROR_NULL_POINTER
    assert raw.solver_hipmf_solve_transpose(h, xp, None, 0) == ERROR_NULL_POINTER
    assert raw.solver_hipmf_solve_transpose_device(h, None, None, 1, n) == ERROR_NULL_POINTER
    assert raw.solver_hipmf_solve_with_error_analysis(h, xp, bp, None, 1, 0) == ERROR_NULL_POINTER
    assert raw.solver_hipmf_solve_with_error_analysis(h, None, bp, ep, 1, 0) == ERROR_NULL_POINTER
    assert lib.solver_hipmf_solve_with_error_analysis(s.h, x, b, ea, 3, 0) == ERROR_HIPMF_INVALID_VALUE
    assert lib.solver_hipmf_solve_with_error_analysis(s.h, x, b, ea, -1, 0) == ERROR_HIPMF_INVALID_VALUE
    assert lib.solver_hipmf_solve_with_error_analysis(s.h, x, b, ea, 2, 0) == 0
    s.close()
