"""Many right-hand sides on the complex handle (complex_solver_hipmf_solve_many / complex_solver_hipmf_solve_device) on the CPU emulator of
the HIP kernels.  tests/test_complex_many_rhs_gpu.py repeats the run_* cases on the device (lib None = the product build).

x and rhs are column-major ld x nrhs complex arrays: here NumPy arrays of shape (nrhs, ld), complex128, whose float64 view is the
interleaved layout the C-ABI takes (columns 2 ld doubles apart).

Agreement with the single solve of the same column follows tests/test_many_rhs_edges_cpu.py, on the interleaved doubles (the real vectors
of the handle): max |x_blk - x_single| <= 1e-12 max |x_single| on the well-conditioned matrices (cond_2 of random200, symlower, zchain513:
5.2, 12.4, 2.9).  On weak300 (cond_2 5.2e3, matched and scaled) the yardstick is the componentwise backward error
omega = max_i |r_i| / (|A| |x| + |b|)_i with complex moduli, recomputed in np.clongdouble: omega_blk <= 2 max_j omega_single_j + the
rounding bound of the recomputation.  That bound: row i of r = b - A x is a complex dot product of k_i + 1 terms, in real arithmetic two
dot products of 2 (k_i + 1) terms each, so |r_i computed - r_i| <= 2 (k + 2) eps_ld sqrt(2) (|A| |x| + |b|)_i with k the longest row; it
enters once for the blocked column and twice for the doubled single figure: 3 x 2 sqrt(2) (k + 2) eps_ld."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import test_solve_updated_complex_cpu as T
from test_solve_updated_many_cpu import padded

CLD = T.CLD
SENTINEL = complex(-7.5, -7.5)  # test_solve_updated_many_cpu.padded fills the padding of the real and of the imaginary parts with -7.5
COUNTERS = dict(T.COUNTERS, block_groups=16, transposed_krylov_iterations=22, updated_blocks=34, updated_column_steps=35, updated_block_basis_bytes=36)
MATRICES = ["random200", "symlower", "weak300", "zchain513"]


class ZM(T.ZH):
    """T.ZH with the entry points for several right-hand sides; arrays of shape (nrhs, ld), complex128"""

    def counter(self, name):
        return int(self.lib.complex_solver_hipmf_get_counter(self.h, COUNTERS[name]))

    def solve_many(self, B, ld=None):
        """X in the shape of B (rows: right-hand sides, ld complex elements each); a status other than 0 raises ZError"""
        B = np.ascontiguousarray(B, np.complex128)
        nrhs, ld = B.shape[0], ld or B.shape[1]
        X = np.full((nrhs, ld), SENTINEL, np.complex128)
        code = self.lib.complex_solver_hipmf_solve_many(self.h, X.view(np.float64).reshape(-1), B.view(np.float64).reshape(-1), nrhs, ld, 0)
        if code != 0:
            raise self.error(code)
        return X

    def solve_many_device(self, B):
        """the same through complex_solver_hipmf_solve_device; returns (X, B as read back from the device)"""
        B = np.ascontiguousarray(B, np.complex128)
        nrhs, ld = B.shape
        X = np.full((nrhs, ld), SENTINEL, np.complex128)
        d_x, d_b = self.dev_alloc(X.nbytes), self.dev_alloc(B.nbytes)
        try:
            self.h2d(d_x, X)
            self.h2d(d_b, B)
            code = self.lib.complex_solver_hipmf_solve_device(self.h, d_x, d_b, nrhs, ld)
            if code != 0:
                raise self.error(code)
            Bb = np.zeros_like(B)
            self.d2h(X, d_x)
            self.d2h(Bb, d_b)
            return X, Bb
        finally:
            self.dev_free(d_x)
            self.dev_free(d_b)

    def solve_updated_many(self, B, v, mapped=False, rel_tol=0.0, max_steps=0, ld=None):
        """(X in the shape of B, steps, relres, status); status 0 or 2, anything else raises ZError"""
        B = np.ascontiguousarray(B, np.complex128)
        nrhs, ld = B.shape[0], ld or B.shape[1]
        X = np.full((nrhs, ld), SENTINEL, np.complex128)
        steps, relres = np.full(nrhs, -1, np.int32), np.full(nrhs, -1.0)
        code = self.lib.complex_solver_hipmf_solve_updated_many(self.h, X.view(np.float64).reshape(-1), B.view(np.float64).reshape(-1), nrhs, ld, T.interleave(v),
                                                                int(bool(mapped)), float(rel_tol), int(max_steps), steps.ctypes.data, relres.ctypes.data, 0)
        if code not in (0, T.NOT_CONVERGED):
            raise self.error(code)
        return X, steps, relres, code

    def solve_updated_many_device(self, B, v, mapped=False, rel_tol=0.0, max_steps=0):
        B = np.ascontiguousarray(B, np.complex128)
        nrhs, ld = B.shape
        X = np.full((nrhs, ld), SENTINEL, np.complex128)
        zv = T.interleave(v)
        steps, relres = np.full(nrhs, -1, np.int32), np.full(nrhs, -1.0)
        d_x, d_b, d_v = self.dev_alloc(X.nbytes), self.dev_alloc(B.nbytes), self.dev_alloc(zv.nbytes)
        try:
            self.h2d(d_x, X)
            self.h2d(d_b, B)
            self.h2d(d_v, zv)
            code = self.lib.complex_solver_hipmf_solve_updated_many_device(self.h, d_x, d_b, nrhs, ld, d_v, int(bool(mapped)), float(rel_tol), int(max_steps),
                                                                           steps.ctypes.data, relres.ctypes.data)
            if code not in (0, T.NOT_CONVERGED):
                raise self.error(code)
            self.d2h(X, d_x)
            return X, steps, relres, code
        finally:
            for p in (d_x, d_b, d_v):
                self.dev_free(p)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def doubles(a):
    return np.ascontiguousarray(a, np.complex128).view(np.float64)


def zview(x):
    """interleaved doubles as complex numbers, bit for bit"""
    return np.ascontiguousarray(x, np.float64).view(np.complex128)


def zpadded(B, ld):
    """the columns in rows of ld complex elements, the padding filled with SENTINEL"""
    return padded(B.real, ld) + 1j * padded(B.imag, ld)


def columns(n, nrhs, seed=50):
    return np.array([T.rhs_for(n, seed + c) for c in range(nrhs)])


def handle(lib, name, **kw):
    """the handle of T.matrix(name) with the default refinement of the ordinary solves; returns (handle, n, the full matrix)"""
    case, mkw = T.matrix(name)
    n, rp, ci, v0 = case
    return ZM(lib, *case, nstep=-1, **mkw, **kw), n, T.full(n, rp, ci, v0, mkw.get("lower", False))


def agree(xb, xs, what):
    """the rule of the real twin on the interleaved doubles"""
    d, s = np.max(np.abs(doubles(xb) - doubles(xs))), np.max(np.abs(doubles(xs)))
    assert d <= 1e-12 * s, (what, d, s)


def omega(A, x, b):
    """(componentwise backward error max_i |r_i| / (|A| |x| + |b|)_i in extended precision, the rounding bound of one such figure)"""
    M = sp.coo_matrix(A)
    n = b.size
    ax = np.zeros(n, CLD)
    np.add.at(ax, M.row, M.data.astype(CLD) * x.astype(CLD)[M.col])
    r = np.abs(b.astype(CLD) - ax)
    d = np.bincount(M.row, np.abs(M.data) * np.abs(x)[M.col], n) + np.abs(b)
    k = int(np.bincount(M.row, minlength=n).max())
    return float(np.max(r / d)), 2.0 * np.sqrt(2.0) * (k + 2) * T.EPS_LD


# ---- the run functions (lib: the emulator's path, or None for the product build) ----

def run_counts_and_padding(lib, name):
    """items 1 to 3 of the module docstring's rule: every column count around the block width, ld = n and n + 3, host and device"""
    s, n, A = handle(lib, name)
    try:
        B = columns(n, 33)
        singles = [zview(s.solve(B[j])) for j in range(33)]
        worst_single = max(omega(A, xs, B[j])[0] for j, xs in enumerate(singles)) if name == "weak300" else None
        for nrhs in (1, 2, 9, 16, 17, 33):
            for ld in (n, n + 3):
                B0 = zpadded(B[:nrhs], ld)
                for entry in ("host", "device"):
                    Bin = B0.copy()
                    if entry == "host":
                        X = s.solve_many(Bin, ld)
                        Bback = Bin
                    else:
                        X, Bback = s.solve_many_device(Bin)
                    assert np.array_equal(bits(Bback), bits(B0)), (nrhs, ld, entry)  # rhs unchanged
                    assert np.array_equal(bits(X[:, n:]), bits(np.full((nrhs, ld - n), SENTINEL, np.complex128))), (nrhs, ld, entry)
                    if nrhs > 1:
                        assert s.counter("block_groups") >= 1
                    for j in range(nrhs):
                        if nrhs == 1:
                            assert np.array_equal(bits(X[j, :n]), bits(singles[j])), (ld, entry)  # the single solve, bit for bit
                        elif name != "weak300":
                            agree(X[j, :n], singles[j], (nrhs, ld, entry, j))
                        else:
                            w, bound = omega(A, X[j, :n], B[j])
                            print("weak300 nrhs %d ld %d %s column %d: omega %.3e, largest of the single solves %.3e, rounding bound %.3e" %
                                  (nrhs, ld, entry, j, w, worst_single, 3 * bound))
                            assert w <= 2.0 * worst_single + 3 * bound, (nrhs, ld, entry, j)
    finally:
        s.close()


def run_zero_and_tiny(lib, name):
    s, n, A = handle(lib, name)
    try:
        B = columns(n, 11, seed=70)
        plain = s.solve_many(B)
        B2 = B.copy()
        B2[3] = 0.0
        B2[6] *= 1e-300
        X = s.solve_many(B2)
        assert np.all(np.isfinite(X.view(np.float64)))
        assert not X[3].any()
        for j in range(11):
            if j in (3, 6):
                continue
            if name != "weak300":
                agree(X[j], plain[j], j)
                agree(X[j], zview(s.solve(B[j])), j)
            else:
                w, bound = omega(A, X[j], B[j])
                ws = omega(A, zview(s.solve(B[j])), B[j])[0]
                print("weak300 column %d: omega %.3e, single %.3e" % (j, w, ws))
                assert w <= 2.0 * ws + 3 * bound, j
    finally:
        s.close()


def run_argument_checks(lib):
    case, kw = T.matrix("random200")
    n = case[0]
    B = columns(n, 2)
    s = ZM(lib, *case, factorize=False)
    try:
        x, b = np.zeros(4 * n), np.ascontiguousarray(B).view(np.float64).reshape(-1)
        many, dev = s.lib.complex_solver_hipmf_solve_many, s.lib.complex_solver_hipmf_solve_device
        assert many(s.h, x, b, 2, n, 0) == T.ERROR_NEED_FACTORIZATION
        assert many(s.h, x, b, 0, n, 0) == T.ERROR_NEED_FACTORIZATION  # (before the invalid values)
        assert dev(s.h, C.c_void_p(16), C.c_void_p(16), 2, n) == T.ERROR_NEED_FACTORIZATION
        assert s.lib.complex_solver_hipmf_factorize(s.h, None, None, None, None, None, None, None, 0, 0, T.interleave(case[3])) == 0
        for nrhs, ld in ((0, n), (-1, n), (2, n - 1)):
            assert many(s.h, x, b, nrhs, ld, 0) == T.ERROR_HIPMF_INVALID_VALUE
            assert dev(s.h, C.c_void_p(16), C.c_void_p(16), nrhs, ld) == T.ERROR_HIPMF_INVALID_VALUE
        assert many(s.h, x, b, 2, n, 0) == 0
        raw = C.CDLL(s.lib._name)  # (untyped bindings: NULL pointers pass)
        raw.complex_solver_hipmf_solve_many.restype = raw.complex_solver_hipmf_solve_device.restype = C.c_int32
        raw.complex_solver_hipmf_solve_many.argtypes = [C.c_void_p] * 3 + [C.c_int32] * 3
        raw.complex_solver_hipmf_solve_device.argtypes = [C.c_void_p] * 3 + [C.c_int32] * 2
        h, xp, bp = C.c_void_p(s.h), x.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
        for args in ((None, xp, bp), (h, None, bp), (h, xp, None)):
            assert raw.complex_solver_hipmf_solve_many(*args, 2, n, 0) == T.ERROR_NULL_POINTER
            assert raw.complex_solver_hipmf_solve_device(*args, 2, n) == T.ERROR_NULL_POINTER
        assert raw.complex_solver_hipmf_solve_many(h, None, bp, 0, n, 0) == T.ERROR_NULL_POINTER  # (before the invalid values)
    finally:
        s.close()


# ---- the tests on the emulator ----

def test_exports(emu_lib):
    raw = C.CDLL(emu_lib)
    for name in ("complex_solver_hipmf_solve_many", "complex_solver_hipmf_solve_device"):
        assert hasattr(raw, name), name


@pytest.mark.parametrize("name", MATRICES)
def test_column_counts_padding_and_single_solves(emu_lib, name):
    run_counts_and_padding(emu_lib, name)


@pytest.mark.parametrize("name", MATRICES)
def test_zero_and_tiny_columns(emu_lib, name):
    run_zero_and_tiny(emu_lib, name)


def test_argument_checks(emu_lib):
    run_argument_checks(emu_lib)
