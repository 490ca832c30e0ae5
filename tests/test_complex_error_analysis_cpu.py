"""The MUMPS-style error analysis of the complex twin (complex_solver_hipmf_solve_with_error_analysis,
kernels_error_analysis_complex.hpp) on the CPU emulator of the HIP kernels: against a numpy restatement of the pinned complex definitions
(include/russell_hipmf.h: moduli, an exact complex residual, exact |A^{-1}| w from the dense complex inverse), bit-for-bit against the
plain complex solve, the options, the statistics the solve leaves, the status codes, and the host mirror (ComplexSolverHIPMF, the
harness's -x / -y on a complex .mtx).  tests/test_complex_error_analysis_gpu.py repeats the cases on the device."""
import ctypes as C
import json
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

from russell_amd import problems as P
from russell_amd._capi import load

EPS = np.finfo(float).eps
ERROR_NULL_POINTER, ERROR_NEED_FACTORIZATION, ERROR_HIPMF_INVALID_VALUE = 100000, 600000, 803
COUNTER_KRYLOV_ITERATIONS, COUNTER_ANALYSIS_SOLVES = 19, 21
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MTX = os.path.join(ROOT, "tests", "golden", "mtx")
HARNESS = os.path.join(ROOT, "russell_amd", "lib", "solve_matrix_market")


def read_complex_mtx(name):
    """(full CSR matrix, symmetric flag) of a complex MatrixMarket file; a symmetric file is mirrored"""
    rows, cols, vals, dims = [], [], [], None
    with open(os.path.join(MTX, name + ".mtx")) as fh:
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
    if sym:
        A = sp.csr_matrix(sp.tril(A) + sp.tril(A, -1).T)
    return A, sym


def interleave(z):
    z = np.asarray(z, np.complex128)
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=1).ravel())


class ZHandle:
    """a factorised complex_solver_hipmf handle (lower=True: the lower triangle of a complex-symmetric A is handed over)"""

    def __init__(self, lib_path, A, lower=False, ordering=0, scaling=1):
        self.lib = load(lib_path)
        self.h = self.lib.complex_solver_hipmf_new()
        assert self.h
        S = sp.csr_matrix(sp.tril(A) if lower else A)
        S.sum_duplicates()
        S.sort_indices()
        self.n = A.shape[0]
        rp, ci, zv = S.indptr.astype(np.int32), S.indices.astype(np.int32), interleave(S.data)
        assert self.lib.complex_solver_hipmf_initialize(self.h, ordering, scaling, -1.0, -1, 0, int(lower), self.n, rp, ci, zv.ctypes.data) == 0
        self._keep = zv
        code = self.lib.complex_solver_hipmf_factorize(self.h, None, None, None, None, None, None, None, 0, 0, zv)
        assert code == 0, code

    def solve(self, b):
        x = np.zeros(2 * self.n)
        assert self.lib.complex_solver_hipmf_solve(self.h, x, interleave(b), 0) == 0
        return x

    def solve_ea(self, b, option, array=None):
        x = np.zeros(2 * self.n)
        ea = np.zeros(8) if array is None else array
        code = self.lib.complex_solver_hipmf_solve_with_error_analysis(self.h, x, interleave(b), ea, option, 0)
        assert code == 0, code
        return x, ea

    def stats(self):
        i, d = np.zeros(16, np.int64), np.zeros(16)
        assert self.lib.complex_solver_hipmf_get_stats(self.h, i, d) == 0
        return i, d

    def counter(self, which):
        return int(self.lib.complex_solver_hipmf_get_counter(self.h, which))

    def close(self):
        if self.h:
            self.lib.complex_solver_hipmf_drop(self.h)
            self.h = None


def as_complex(x):
    return x[0::2] + 1j * x[1::2]


def exact_complex_residual(D, b, x):
    """b - D x in rational arithmetic, the real and the imaginary part each rounded once"""
    r = np.zeros(len(b), np.complex128)
    for i in range(len(b)):
        tr, ti = Fraction(float(b[i].real)), Fraction(float(b[i].imag))
        for j in np.nonzero(D[i])[0]:
            ar, ai = Fraction(float(D[i, j].real)), Fraction(float(D[i, j].imag))
            xr, xi = Fraction(float(x[j].real)), Fraction(float(x[j].imag))
            tr -= ar * xr - ai * xi
            ti -= ar * xi + ai * xr
        r[i] = complex(float(tr), float(ti))
    return r


def zerror_analysis_numpy(D, b, x):
    """The pinned complex definitions (include/russell_hipmf.h), restated with moduli and the explicit dense inverse (exact |A^{-1}| w)."""
    n = D.shape[0]
    absA = np.abs(D)
    a = absA.sum(axis=1)
    NA, NX = a.max(), np.abs(x).max()
    r = exact_complex_residual(D, b, x)
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
    out[6] = (Ainv @ w1).max() / NX
    out[7] = (Ainv @ w2).max() / NX if I2.any() else 0.0
    out[5] = out[3] * out[6] + out[4] * out[7]
    return out, I2.any()


def check_error_analysis(ea, ref):
    for k in range(5):
        assert ea[k] == pytest.approx(ref[k], rel=1e-12, abs=1e-300), (k, ea[k], ref[k])
    for k in (6, 7):
        assert ref[k] / 10.0 <= ea[k] <= ref[k] * (1.0 + 1e-10), (k, ea[k], ref[k])
    assert ea[5] == pytest.approx(ea[3] * ea[6] + ea[4] * ea[7], rel=1e-14, abs=1e-300)


def shifted_convection_diffusion(nx, gamma=2.0, omega=1.5):
    """(gamma + i omega) I - A: the complex shifted system russell_ode's Radau5 solves on every Newton step"""
    n, rp, ci, v = P.convection_diffusion2d(nx, peclet=30)
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))
    return sp.csr_matrix((gamma + 1j * omega) * sp.identity(n) - A)


def constructed_i2_case():
    """Row 0 has b_0 = 0 and its pattern misses the support of x (x_1 = x_2 = 0 there): d_0 = 0, so I2 is not empty and cond2 > 0."""
    D = np.array([[4.0 + 1.0j, 1.0 - 0.5j, -1.0 + 0.2j, 0.0, 0.0], [0.5j, 3.0 - 1.0j, 0.0, 0.0, 1.0 + 1.0j], [0.0, 0.3 + 0.3j, 5.0, 1.0j, 0.0],
                  [0.0, 0.0, 1.0 - 1.0j, 2.0 + 2.0j, 0.2], [1.0, 0.0, 0.0, 0.4 - 0.1j, 6.0 - 1.0j]])
    xs = np.array([0.0, 0.0, 0.0, 1.0 + 1.0j, 2.0 - 0.5j])
    return D, D @ xs


def complex_symmetric_case():
    """a complex-symmetric (not Hermitian) shifted Laplacian, handed over as its lower triangle"""
    nx, ny = 14, 13
    T = lambda m: sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    L = sp.kron(sp.identity(ny), T(nx)) + sp.kron(T(ny), sp.identity(nx))
    n = nx * ny
    rng = np.random.default_rng(21)
    A = L.astype(np.complex128) + sp.diags((1.0 + rng.random(n)) * (0.5 + 0.8j))
    return sp.csr_matrix(A)


def case(name):
    """(A, b, lower)"""
    rng = np.random.default_rng(len(name))
    if name == "golden_general":
        A, _ = read_complex_mtx("ok_complex_general")
        lower = False
    elif name == "shifted_convection_diffusion_30":
        A, lower = shifted_convection_diffusion(30), False
    elif name == "complex_symmetric_lower":
        A, lower = complex_symmetric_case(), True
    else:
        D, b = constructed_i2_case()
        return sp.csr_matrix(D), b, False
    n = A.shape[0]
    return A, rng.standard_normal(n) + 1j * rng.standard_normal(n), lower


CASE_NAMES = ["golden_general", "shifted_convection_diffusion_30", "complex_symmetric_lower", "constructed_i2"]


def run_case(lib_path, name):
    A, b, lower = case(name)
    D = A.toarray()
    s = ZHandle(lib_path, A, lower=lower)
    x0 = s.solve(b)
    x, ea = s.solve_ea(b, 1)
    assert np.array_equal(x, x0)  # the solve is complex_solver_hipmf_solve's, bit for bit
    ref, has_i2 = zerror_analysis_numpy(D, b, as_complex(x))
    check_error_analysis(ea, ref)
    assert 0 < s.counter(COUNTER_ANALYSIS_SOLVES) <= 22
    if name == "constructed_i2":
        assert has_i2 and ea[7] > 0.0
    # repeatable to the bit
    x2, ea2 = s.solve_ea(b, 1)
    assert np.array_equal(x2, x) and np.array_equal(ea2, ea)
    # option 2: entries 0 - 4, the rest keeps what the caller put there; option 0: nothing
    _, ea3 = s.solve_ea(b, 2, array=np.full(8, -7.0))
    assert np.array_equal(ea3[:5], ea[:5]) and np.all(ea3[5:] == -7.0)
    x4, ea4 = s.solve_ea(b, 0, array=np.full(8, -7.0))
    assert np.all(ea4 == -7.0) and np.array_equal(x4, x0)
    s.close()
    return ea


@pytest.mark.parametrize("name", CASE_NAMES)
def test_error_analysis_against_numpy(emu_lib, name):
    run_case(emu_lib, name)


def test_moduli_not_the_real_equivalent_analysis(emu_lib):
    """N_A is the row sum of MODULI; the real analysis of the 2n system would report the larger sum of |Re| + |Im|"""
    A, b, _ = case("golden_general")
    s = ZHandle(emu_lib, A)
    _, ea = s.solve_ea(b, 2)
    D = A.toarray()
    assert np.abs(D.imag).max() > 0.0
    modulus_sum, split_sum = np.abs(D).sum(axis=1).max(), (np.abs(D.real) + np.abs(D.imag)).sum(axis=1).max()
    assert ea[0] == pytest.approx(modulus_sum, rel=1e-14)
    assert abs(ea[0] - split_sum) > 1e-3 * split_sum
    x = as_complex(s.solve(b))
    assert ea[1] == pytest.approx(np.abs(x).max(), rel=1e-14)  # N_x: the largest modulus, not max(|Re|, |Im|)
    s.close()


def test_analysis_keeps_solve_statistics(emu_lib):
    A, b, _ = case("shifted_convection_diffusion_30")
    s = ZHandle(emu_lib, A)
    s.solve(b)
    is0, ds0 = s.stats()
    kry0 = s.counter(COUNTER_KRYLOV_ITERATIONS)
    assert kry0 >= 0
    s.solve_ea(b, 1)
    is1, ds1 = s.stats()
    assert np.array_equal(is1, is0)  # refinement steps (is[10]), solve launches, ...
    assert ds1[9] == ds0[9]  # the residual of the solve
    assert s.counter(COUNTER_KRYLOV_ITERATIONS) == kry0
    s.close()


def test_status_codes(emu_lib):
    A, b, _ = case("golden_general")
    S = sp.csr_matrix(A)
    S.sort_indices()
    lib = load(emu_lib)
    n = A.shape[0]
    h = lib.complex_solver_hipmf_new()
    zv = interleave(S.data)
    assert lib.complex_solver_hipmf_initialize(h, 0, 1, -1.0, -1, 0, 0, n, S.indptr.astype(np.int32), S.indices.astype(np.int32), zv.ctypes.data) == 0
    x, bi, ea = np.zeros(2 * n), interleave(b), np.zeros(8)
    assert lib.complex_solver_hipmf_solve_with_error_analysis(h, x, bi, ea, 1, 0) == ERROR_NEED_FACTORIZATION
    assert lib.complex_solver_hipmf_factorize(h, None, None, None, None, None, None, None, 0, 0, zv) == 0
    raw = C.CDLL(emu_lib)  # (untyped binding: NULL pointers pass)
    fn = raw.complex_solver_hipmf_solve_with_error_analysis
    fn.restype = C.c_int32
    xp, bp, ep, hp = x.ctypes.data_as(C.c_void_p), bi.ctypes.data_as(C.c_void_p), ea.ctypes.data_as(C.c_void_p), C.c_void_p(h)
    assert fn(None, xp, bp, ep, 1, 0) == ERROR_NULL_POINTER
    assert fn(hp, None, bp, ep, 1, 0) == ERROR_NULL_POINTER
    assert fn(hp, xp, None, ep, 1, 0) == ERROR_NULL_POINTER
    assert fn(hp, xp, bp, None, 1, 0) == ERROR_NULL_POINTER
    for bad in (3, -1):
        assert lib.complex_solver_hipmf_solve_with_error_analysis(h, x, bi, ea, bad, 0) == ERROR_HIPMF_INVALID_VALUE
    assert lib.complex_solver_hipmf_solve_with_error_analysis(h, x, bi, ea, 2, 0) == 0
    lib.complex_solver_hipmf_drop(h)


# ---- the host mirror ----
def _run_harness(emu_lib, *args):
    env = dict(os.environ, RUSSELL_HIPMF_LIB=emu_lib)
    p = subprocess.run([HARNESS] + list(args), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    out = p.stdout
    return json.loads(out[out.index("{"):])["mumps_stats"]


def test_harness_complex_error_analysis_flags(emu_lib):
    f = os.path.join(MTX, "ok_complex_general.mtx")
    plain = _run_harness(emu_lib, f)
    assert all(v == 0.0 for v in plain.values())
    est = _run_harness(emu_lib, "-x", f)
    for k in ("inf_norm_a", "inf_norm_x", "scaled_residual"):
        assert est[k] > 0.0, k
    assert est["backward_error_omega1"] > 0.0 or est["backward_error_omega2"] > 0.0 or est["scaled_residual"] > 0.0
    assert est["condition_number1"] == 0.0 and est["condition_number2"] == 0.0 and est["normalized_delta_x"] == 0.0
    full = _run_harness(emu_lib, "-x", "-y", f)
    assert full["inf_norm_a"] == est["inf_norm_a"] and full["condition_number1"] >= 1.0
    assert full["normalized_delta_x"] == pytest.approx(full["backward_error_omega1"] * full["condition_number1"]
                                                       + full["backward_error_omega2"] * full["condition_number2"], rel=1e-14, abs=1e-300)


@pytest.fixture
def emu_backend(emu_lib):
    """the host mirror of russell_amd.sparse bound to the emulator library for one test"""
    from russell_amd import sparse as S
    S._L().rh_set_hipmf_library(emu_lib.encode())
    yield S
    S._L().rh_set_hipmf_library(os.path.join(ROOT, "russell_amd", "lib", "librussell_hipmf.so").encode())


def test_complex_lin_solver_mumps_stats(emu_backend, emu_lib):
    S = emu_backend
    A, b, _ = case("shifted_convection_diffusion_30")
    Acoo = sp.coo_matrix(A)
    n = A.shape[0]
    coo = S.ComplexCooMatrix(n, n, Acoo.nnz, S.Sym.No)
    for i, j, v in zip(Acoo.row, Acoo.col, Acoo.data):
        coo.put(int(i), int(j), complex(v))
    # without the flags: zeros
    plain = S.ComplexLinSolver(S.Genie.Hipmf)
    plain.actual.factorize(coo, S.LinSolParams())
    plain.actual.solve(b)
    assert np.all(plain.actual.mumps_stats() == 0.0)
    params = S.LinSolParams()
    params.compute_condition_numbers = True
    solver = S.ComplexLinSolver(S.Genie.Hipmf)
    solver.actual.factorize(coo, params)
    x = solver.actual.solve(b)
    ms = solver.actual.mumps_stats()
    # the same eight values as the C-ABI call on the same system (the mirror's defaults: nested dissection, sum scaling)
    h = ZHandle(emu_lib, A, ordering=0, scaling=1)
    xc, ea = h.solve_ea(b, 1)
    h.close()
    assert np.array_equal(interleave(x), xc)
    assert np.array_equal(ms, ea), (ms, ea)
    assert np.all(ms[:2] > 0.0) and ms[6] >= 1.0
