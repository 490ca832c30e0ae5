"""Blocked transposed solves on the complex handle (complex_solver_hipmf_solve_transpose_many / _many_device: A^T X = B and A^H X = B, 16
columns per transposed pass pair, k_tr_conj_cols around the A^T blocks) on the CPU emulator of the HIP kernels.
tests/test_complex_transpose_many_gpu.py repeats the run_* cases on the device (lib None = the product build).

Arrays of right-hand sides have the shape (nrhs, ld), complex128: the column-major ld x nrhs interleaved layout of the C-ABI.
The bounds.  Against complex_solver_hipmf_solve_transpose of the same column (both refined as the handle is set up; the blocked and the
single pass pair sum in different orders): max |x_blk - x_single| <= 8 n eps max |x_single|, n the order of the complex matrix.  Against
NumPy's dense solve with A^T / A^H: max |x - x_ref| <= 1e-11 max |x_ref|, the bound tests/test_transpose_many_cpu.py has for the real
pair against scipy.  One column is the single call, bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import test_solve_updated_complex_cpu as Z
from test_complex_many_rhs_cpu import COUNTERS, SENTINEL, ZM, bits, zpadded

EPS = np.finfo(float).eps
ERROR_NULL_POINTER, ERROR_NEED_FACTORIZATION, ERROR_HIPMF_INVALID_VALUE = Z.ERROR_NULL_POINTER, Z.ERROR_NEED_FACTORIZATION, Z.ERROR_HIPMF_INVALID_VALUE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NRHS = [1, 5, 16, 17]


class ZTM(ZM):
    """ZM with the transposed solves; conjugate: 1 -> A^H, 0 -> A^T"""

    def counter(self, name):
        return int(self.lib.complex_solver_hipmf_get_counter(self.h, dict(COUNTERS, transposed_blocks=23)[name]))

    def solve_transpose(self, b, conjugate):
        x = np.zeros(2 * self.n)
        code = self.lib.complex_solver_hipmf_solve_transpose(self.h, x, Z.interleave(b), int(conjugate), 0)
        if code != 0:
            raise self.error(code)
        return Z.as_complex(x)

    def solve_transpose_many(self, B, conjugate, ld=None):
        B = np.ascontiguousarray(B, np.complex128)
        nrhs, ld = B.shape[0], ld or B.shape[1]
        X = np.full((nrhs, ld), SENTINEL, np.complex128)
        code = self.lib.complex_solver_hipmf_solve_transpose_many(self.h, X.view(np.float64).reshape(-1), B.view(np.float64).reshape(-1), nrhs, ld, int(conjugate), 0)
        if code != 0:
            raise self.error(code)
        return X

    def solve_transpose_many_device(self, B, conjugate, in_place=False):
        """(X, B as read back from the device); in_place: d_x aliases d_rhs"""
        B = np.ascontiguousarray(B, np.complex128)
        nrhs, ld = B.shape
        X = np.full((nrhs, ld), SENTINEL, np.complex128)
        d_b = self.dev_alloc(B.nbytes)
        d_x = d_b if in_place else self.dev_alloc(X.nbytes)
        try:
            if not in_place:
                self.h2d(d_x, X)
            self.h2d(d_b, B)
            code = self.lib.complex_solver_hipmf_solve_transpose_many_device(self.h, d_x, d_b, nrhs, ld, int(conjugate))
            if code != 0:
                raise self.error(code)
            Bb = np.zeros_like(B)
            self.d2h(X, d_x)
            self.d2h(Bb, d_b)
            return X, Bb
        finally:
            self.dev_free(d_b)
            if not in_place:
                self.dev_free(d_x)


def case(name):
    """name -> (n, rp, ci, v, keywords of ZH): ref5, zchain257, the 24 x 20 shifted grid with unsymmetric values"""
    if name == "grid":
        n, rp, ci, vals = Z.shifted_grid(24, 20, unsym=True)
        return n, rp, ci, vals(1.0), {}
    c, kw = Z.matrix(name)
    return c + (kw,)


def op(A, conjugate):
    D = np.asarray(A.todense())
    return D.conj().T if conjugate else D.T


def check_against_single(n, X, singles, what=""):
    """max |x_blk - x_single| <= 8 n eps max |x_single| per column"""
    for j, (x, x1) in enumerate(zip(X, singles)):
        d, bound = np.abs(x[:n] - x1).max(), 8 * n * EPS * np.abs(x1).max()
        print("%s column %d: |x_blk - x_single|_inf %.3e, bound %.3e" % (what, j, d, bound))
        assert d <= bound, (what, j, d, bound)


def run_against_single_and_numpy(lib, name, nrhs_list=NRHS, pad=3):
    n, rp, ci, v, kw = case(name)
    A = Z.full(n, rp, ci, v, kw.get("lower", False))
    B = np.array([Z.rhs_for(n, 50 + c) for c in range(max(nrhs_list))])
    s = ZTM(lib, n, rp, ci, v, nstep=-1, **kw)
    try:
        for conjugate in (1, 0):
            singles = [s.solve_transpose(b, conjugate) for b in B]
            XR = np.linalg.solve(op(A, conjugate), B.T).T
            for nrhs in nrhs_list:
                t0 = s.counter("transposed_solves")
                Bp = zpadded(B[:nrhs], n + pad)
                X = s.solve_transpose_many(Bp, conjugate, ld=n + pad)
                assert s.counter("transposed_blocks") == (0 if nrhs == 1 else (nrhs + 15) // 16), nrhs
                assert s.counter("transposed_solves") == t0 + nrhs
                assert np.array_equal(bits(X[:, n:]), bits(np.full((nrhs, pad), SENTINEL, np.complex128)))  # (the padding rows are not written)
                if nrhs == 1:
                    assert np.array_equal(bits(X[0, :n]), bits(singles[0]))
                check_against_single(n, X, singles[:nrhs], "%s conjugate %d nrhs %d" % (name, conjugate, nrhs))
                for j in range(nrhs):
                    assert np.abs(X[j, :n] - XR[j]).max() <= 1e-11 * np.abs(XR[j]).max(), (nrhs, j)
                assert np.array_equal(bits(X), bits(s.solve_transpose_many(Bp, conjugate, ld=n + pad)))  # the same bits on a repeat call
            # the device form, out of place (rhs unchanged) and in place
            Bp = zpadded(B[:17], n + pad)
            Xh = s.solve_transpose_many(Bp, conjugate, ld=n + pad)
            Xd, Bd = s.solve_transpose_many_device(Bp, conjugate)
            assert np.array_equal(bits(Xd), bits(Xh)) and np.array_equal(bits(Bd), bits(Bp))
            Xi, _ = s.solve_transpose_many_device(Bp, conjugate, in_place=True)
            assert np.array_equal(bits(Xi[:, :n]), bits(Xh[:, :n])) and np.array_equal(bits(Xi[:, n:]), bits(Bp[:, n:]))
    finally:
        s.close()


def run_column_loop(lib, monkeypatch):
    """HIPMF_TRANSPOSE_BLOCKED=0: the single solve column by column, its bits, no blocks counted"""
    n, rp, ci, v, kw = case("zchain257")
    B = np.array([Z.rhs_for(n, 50 + c) for c in range(5)])
    s = ZTM(lib, n, rp, ci, v, nstep=-1)
    try:
        for conjugate in (1, 0):
            blocked = s.solve_transpose_many(B, conjugate)
            assert s.counter("transposed_blocks") == 1
            monkeypatch.setenv("HIPMF_TRANSPOSE_BLOCKED", "0")
            X = s.solve_transpose_many(B, conjugate)
            monkeypatch.delenv("HIPMF_TRANSPOSE_BLOCKED")
            assert s.counter("transposed_blocks") == 0
            for j in range(5):
                assert np.array_equal(bits(X[j]), bits(s.solve_transpose(B[j], conjugate)))
            check_against_single(n, blocked, X, "column loop conjugate %d" % conjugate)
    finally:
        s.close()


def run_status_codes(lib):
    c, _ = Z.matrix("ref5")
    n, rp, ci, v = c
    zv = Z.interleave(v)
    X, B = np.zeros(4 * n), np.ones(4 * n)
    s = ZTM(lib, n, rp, ci, v, factorize=False)
    try:
        call = lambda nrhs=2, ld=n, conj=1: s.lib.complex_solver_hipmf_solve_transpose_many(s.h, X, B, nrhs, ld, conj, 0)
        dv = C.c_void_p(8)
        assert call() == ERROR_NEED_FACTORIZATION and call(conj=5) == ERROR_NEED_FACTORIZATION
        assert s.lib.complex_solver_hipmf_solve_transpose_many_device(s.h, dv, dv, 2, n, 1) == ERROR_NEED_FACTORIZATION
        assert s.lib.complex_solver_hipmf_factorize(s.h, None, None, None, None, None, None, None, 0, 0, zv) == 0
        assert call() == 0 and call(conj=0) == 0
        for bad in (dict(conj=2), dict(conj=-1), dict(nrhs=0), dict(ld=n - 1)):
            assert call(**bad) == ERROR_HIPMF_INVALID_VALUE, bad
        assert s.lib.complex_solver_hipmf_solve_transpose_many_device(s.h, dv, dv, 2, n, 2) == ERROR_HIPMF_INVALID_VALUE
        raw = C.CDLL(s.lib._name)
        raw.complex_solver_hipmf_solve_transpose_many.restype = C.c_int32
        raw.complex_solver_hipmf_solve_transpose_many.argtypes = [C.c_void_p] * 3 + [C.c_int32] * 4
        h, xp, bp = C.c_void_p(s.h), X.ctypes.data_as(C.c_void_p), B.ctypes.data_as(C.c_void_p)
        for args in ((None, xp, bp), (h, None, bp), (h, xp, None)):
            assert raw.complex_solver_hipmf_solve_transpose_many(*args, 2, n, 1, 0) == ERROR_NULL_POINTER
    finally:
        s.close()


def run_host_mirror(lib):
    from russell_amd import sparse as S

    S._L().rh_set_hipmf_library((lib or os.path.join(ROOT, "russell_amd", "lib", "librussell_hipmf.so")).encode())
    try:
        n, rp, ci, vals = Z.shifted_grid(12, 10, unsym=True)
        m = S.ComplexCooMatrix(n, n, ci.size)
        m.put_many(np.repeat(np.arange(n), np.diff(rp)), ci, vals(1.0))
        A = Z.full(n, rp, ci, vals(1.0))
        B = np.array([Z.rhs_for(n, 10 + c) for c in range(17)])
        solver = S.ComplexLinSolver()
        solver.actual.factorize(m)
        for conjugate in (True, False):
            X = solver.solve_transpose_many(B, conjugate=conjugate)
            singles = [solver.actual.solve_transpose(b, conjugate=conjugate) for b in B]
            check_against_single(n, X, singles, "host mirror conjugate %d" % conjugate)
            XR = np.linalg.solve(op(A, conjugate), B.T).T
            assert np.abs(X - XR).max() <= 1e-11 * np.abs(XR).max()
        with pytest.raises(S.StrError, match="expects an array of shape"):
            solver.solve_transpose_many(B[0])
    finally:
        S._L().rh_set_hipmf_library(os.path.join(ROOT, "russell_amd", "lib", "librussell_hipmf.so").encode())


# ---- the tests on the emulator ----

def test_exports(emu_lib):
    raw = C.CDLL(emu_lib)
    header = open(os.path.join(ROOT, "include", "russell_hipmf.h")).read()
    for name in ("complex_solver_hipmf_solve_transpose_many", "complex_solver_hipmf_solve_transpose_many_device"):
        assert hasattr(raw, name) and "int32_t %s(" % name in header, name


@pytest.mark.parametrize("name", ["ref5", "zchain257", "grid"])
def test_against_single_and_numpy(emu_lib, name):
    run_against_single_and_numpy(emu_lib, name)


def test_column_loop(emu_lib, monkeypatch):
    run_column_loop(emu_lib, monkeypatch)


def test_status_codes(emu_lib):
    run_status_codes(emu_lib)


def test_host_mirror(emu_lib):
    run_host_mirror(emu_lib)
