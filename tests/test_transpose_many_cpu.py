"""Blocked transposed solves (solver_hipmf_solve_transpose_many / _many_device, kernels_solve_transpose_blocked.hpp) on the CPU emulator of the
HIP kernels: every column against scipy's solve of A^T and against the one-at-a-time solve of that column, the blocks counter,
repeatability, independence of a column from the block and the position it travels in, a zero column, padded columns (ld > n) through both
entry points, the delegations (one column, A^T = A, no block buffers), the status codes, and the Krylov rescue after replaced pivots.
tests/test_transpose_many_gpu.py repeats the cases on the device (the run_* functions take the library: None = the product build)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import front_shapes as F
from russell_amd import problems as P
from russell_amd.backend import Hipmf, HipmfError
from test_many_rhs_edges_cpu import SENTINEL
from test_transpose_solve_cpu import CASES, ERROR_HIPMF_INVALID_VALUE, ERROR_NEED_FACTORIZATION, ERROR_NULL_POINTER
from test_transpose_solve_gpu import _pm1

NRHS = [2, 15, 16, 17, 33]


def _new(lib):
    return Hipmf(lib) if lib else Hipmf()


def _handle(lib, n, rp, ci, v, **kw):
    s = _new(lib)
    assert s.initialize(n, rp, ci, values=v, **kw) == 0
    assert s.factorize(v) == 0
    return s


def _csr(n, rp, ci, v):
    return sp.csr_matrix((np.asarray(v, float), np.asarray(ci), np.asarray(rp)), shape=(n, n))


def _blocks(nrhs):
    return (nrhs + 15) // 16


def run_against_scipy_and_single(lib, problem, nrhs_list=NRHS, seed=3):
    """every column within 1e-11 max|x_ref| of spsolve(A^T, b_j) and within 1e-12 max|x_j| of solve_transpose(b_j) (the bound between blocked
    and single solves of tests/test_many_rhs_edges_cpu.py); the counters; the same bits on a repeat call"""
    n, rp, ci, v = problem
    lu = spla.splu(_csr(n, rp, ci, v).T.tocsc())
    s = _handle(lib, n, rp, ci, v)
    try:
        B = np.random.default_rng(seed).standard_normal((max(nrhs_list), n))
        singles = [s.solve_transpose(B[j]) for j in range(B.shape[0])]
        for nrhs in nrhs_list:
            t0 = s.counter("transposed_solves")
            X = s.solve_transpose_many(B[:nrhs])
            assert s.counter("transposed_blocks") == _blocks(nrhs), nrhs
            assert s.counter("transposed_solves") == t0 + nrhs
            for j in range(nrhs):
                xr = lu.solve(B[j])
                e_ref, e_one = np.abs(X[j] - xr).max() / np.abs(xr).max(), np.abs(X[j] - singles[j]).max() / np.abs(singles[j]).max()
                print("nrhs %d column %d: against scipy %.2e, against the single solve %.2e" % (nrhs, j, e_ref, e_one))
                assert e_ref <= 1e-11, (nrhs, j)
                assert e_one <= 1e-12, (nrhs, j)
            assert np.array_equal(X, s.solve_transpose_many(B[:nrhs])), nrhs
    finally:
        s.close()


def run_column_independence(lib, problem):
    """33 columns in a fixed random order: X[:, pi] exactly (columns move between full and tail blocks and between positions); a zero
    column gives exactly zero and leaves the other columns' bits alone"""
    n, rp, ci, v = problem
    s = _handle(lib, n, rp, ci, v)
    try:
        rng = np.random.default_rng(17)
        B = rng.standard_normal((33, n))
        pi = rng.permutation(33)
        X = s.solve_transpose_many(B)
        Xp = s.solve_transpose_many(B[pi])
        assert np.array_equal(Xp.view(np.uint64), X[pi].view(np.uint64))
        B0 = B.copy()
        B0[5] = 0.0
        B0[32] = 0.0
        X0 = s.solve_transpose_many(B0)
        assert np.array_equal(X0[5], np.zeros(n)) and np.array_equal(X0[32], np.zeros(n))
        keep = [j for j in range(33) if j not in (5, 32)]
        assert np.array_equal(X0[keep].view(np.uint64), X[keep].view(np.uint64))
    finally:
        s.close()


def _padded(s, n, ld, B0, fn_name):
    """B0 (nrhs, ld) through one of the two new calls: (X, B afterwards), both (nrhs, ld)"""
    nrhs = B0.shape[0]
    if fn_name == "host":
        B = B0.copy()
        X = np.full((nrhs, ld), SENTINEL)
        code = s.lib.solver_hipmf_solve_transpose_many(s.h, X, B, nrhs, ld, 0)  # (the raw call: x arrives with its sentinels)
        assert code == 0, code
        return X, B
    d_b, d_x = s.dev_alloc(B0.nbytes), s.dev_alloc(B0.nbytes)
    try:
        s.h2d(d_b, B0)
        s.h2d(d_x, np.full((nrhs, ld), SENTINEL))
        s.solve_transpose_many_device(d_x, d_b, nrhs, ld=ld)
        X, B = np.zeros((nrhs, ld)), np.zeros((nrhs, ld))
        s.d2h(X, d_x)
        s.d2h(B, d_b)
        return X, B
    finally:
        s.dev_free(d_b)
        s.dev_free(d_x)


def run_padded_columns(lib, nrhs):
    """ld = n + 3, no refinement, the chain of tests/front_shapes.py: every column to its tolerance, padding and rhs untouched"""
    case = F.chain(32, 100, 97, 31, seed=11)
    n = case.n
    s = _new(lib)
    try:
        assert s.initialize(n, case.rp, case.ci, ordering=F.ORDERING_NONE, refinement_nstep=0) == 0
        assert s.factorize(case.v) == 0
        assert s.num_perturbed == 0
        ld = n + 3
        B0 = np.full((nrhs, ld), SENTINEL)
        B0[:, :n] = np.random.default_rng(nrhs).standard_normal((nrhs, n))
        ref_t = F.Reference(case.A).transposed()
        pad = np.full((nrhs, 3), SENTINEL).view(np.uint64)
        for which in ("host", "device"):
            X, B = _padded(s, n, ld, B0, which)
            assert s.counter("transposed_blocks") == _blocks(nrhs)
            assert np.array_equal(B.view(np.uint64), B0.view(np.uint64)), which
            assert np.array_equal(X[:, n:].view(np.uint64), pad), which
            for j in range(nrhs):
                ref_t.check(X[j, :n], B0[j, :n], "solve_transpose_many (%s) ld=n+3 column %d" % (which, j))
    finally:
        s.close()


def run_padded_columns_refined(lib, nrhs):
    """the same layout with default refinement on a grid matrix (k_tr_residual_cols and the correcting launches with cstr = ld > n): each
    column against the single refined solve of that column"""
    n, rp, ci, v = P.poisson2d(24)
    v = v * (1.0 + 0.2 * np.random.default_rng(24).uniform(-1, 1, v.size))
    A = _csr(n, rp, ci, v).toarray()
    s = _handle(lib, n, rp, ci, v)
    try:
        ld = n + 3
        B0 = np.full((nrhs, ld), SENTINEL)
        B0[:, :n] = np.random.default_rng(nrhs).standard_normal((nrhs, n)) @ A
        pad = np.full((nrhs, 3), SENTINEL).view(np.uint64)
        for which in ("host", "device"):
            X, B = _padded(s, n, ld, B0, which)
            assert np.array_equal(B.view(np.uint64), B0.view(np.uint64)), which
            assert np.array_equal(X[:, n:].view(np.uint64), pad), which
            for j in range(nrhs):
                xj = s.solve_transpose(B0[j, :n])
                assert np.max(np.abs(X[j, :n] - xj)) <= 1e-12 * np.max(np.abs(xj)), (which, j)
    finally:
        s.close()


def run_delegation(lib):
    n, rp, ci, v = P.convection_diffusion2d(40, peclet=30)
    s = _handle(lib, n, rp, ci, v)
    try:
        B = np.random.default_rng(6).standard_normal((3, n))
        x1 = s.solve_transpose(B[0])
        t0 = s.counter("transposed_solves")
        X = s.solve_transpose_many(B[:1])  # one column: the single-column path, its bits
        assert np.array_equal(X[0], x1) and s.counter("transposed_blocks") == 0 and s.counter("transposed_solves") == t0 + 1
        d_b, d_x = s.dev_alloc(B.nbytes), s.dev_alloc(B.nbytes)
        try:
            s.h2d(d_b, B)
            s.solve_transpose_many_device(d_x, d_b, 1)
            Xd = np.zeros_like(B)
            s.d2h(Xd, d_x)
            assert np.array_equal(Xd[0], x1)
            # in place (d_x = d_rhs): the block's columns are staged
            Xh = s.solve_transpose_many(B)
            s.solve_transpose_many_device(d_b, d_b, 3)
            s.d2h(Xd, d_b)
            assert np.array_equal(Xd, Xh) and s.counter("transposed_blocks") == 1
        finally:
            s.dev_free(d_b)
            s.dev_free(d_x)
    finally:
        s.close()
    # A^T = A (symmetric-lower handle): the ordinary blocked solve, its bits; the columns are still counted
    n, rp, ci, v = P.poisson2d(30, 28)
    lrp, lci, lv = P.lower_triangle(n, rp, ci, v)
    s = _new(lib)
    try:
        assert s.initialize(n, lrp, lci, general_symmetric=True) == 0
        assert s.factorize(lv) == 0
        assert s.counter("symmetric_ldlt") == 1
        B = np.random.default_rng(7).standard_normal((18, n))
        X = s.solve_transpose_many(B)
        assert s.counter("transposed_blocks") == 0 and s.counter("transposed_solves") == 18
        assert np.array_equal(X, s.solve_many(B))
    finally:
        s.close()


def run_status_codes(lib):
    n, rp, ci, v = P.poisson2d(12)
    s = _new(lib)
    try:
        assert s.initialize(n, rp, ci) == 0
        b = np.zeros((2, n))
        x = np.zeros((2, n))
        assert s.lib.solver_hipmf_solve_transpose_many(s.h, x, b, 2, n, 0) == ERROR_NEED_FACTORIZATION
        assert s.lib.solver_hipmf_solve_transpose_many_device(s.h, C.c_void_p(1), C.c_void_p(1), 2, n) == ERROR_NEED_FACTORIZATION
        assert s.factorize(v) == 0
        assert s.lib.solver_hipmf_solve_transpose_many(s.h, x, b, 0, n, 0) == ERROR_HIPMF_INVALID_VALUE
        assert s.lib.solver_hipmf_solve_transpose_many(s.h, x, b, 2, n - 1, 0) == ERROR_HIPMF_INVALID_VALUE
        d = s.dev_alloc(b.nbytes)
        try:
            for nrhs, ld in ((0, n), (2, n - 1)):
                with pytest.raises(HipmfError) as e:
                    s.solve_transpose_many_device(d, d, nrhs, ld=ld)
                assert e.value.code == ERROR_HIPMF_INVALID_VALUE
        finally:
            s.dev_free(d)
        with pytest.raises(ValueError):
            s.solve_transpose_many(b, ld=n + 1)
        raw = C.CDLL(s.lib._name)  # (untyped bindings: NULL pointers pass)
        for fn in (raw.solver_hipmf_solve_transpose_many, raw.solver_hipmf_solve_transpose_many_device):
            fn.restype = C.c_int32
        h, xp, bp = C.c_void_p(s.h), x.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
        assert raw.solver_hipmf_solve_transpose_many(h, None, bp, 2, n, 0) == ERROR_NULL_POINTER
        assert raw.solver_hipmf_solve_transpose_many(h, xp, None, 2, n, 0) == ERROR_NULL_POINTER
        assert raw.solver_hipmf_solve_transpose_many(None, xp, bp, 2, n, 0) == ERROR_NULL_POINTER
        assert raw.solver_hipmf_solve_transpose_many_device(h, None, bp, 2, n) == ERROR_NULL_POINTER
    finally:
        s.close()


def run_replaced_pivots(lib):
    """_pm1(800, 4), seed 100, five columns: replaced pivots, every column to 10 e_ref + 1e-12 against SuperLU (the bound of
    test_pm1_family_transposed_rescue); the ordinary solve's rescue statistics stay the ordinary solve's"""
    rng = np.random.default_rng(100)
    A = _pm1(800, 4, rng)
    n, rp, ci, v = A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
    XS = rng.standard_normal((5, n))
    B = XS @ A  # rows: A^T xs_j
    lu = spla.splu(A.T.tocsc())
    s = _handle(lib, n, rp, ci, v)
    try:
        assert s.num_perturbed > 0
        s.solve(A @ XS[0])
        k_ordinary = s.counter("krylov_iterations")
        X = s.solve_transpose_many(B)
        assert s.counter("transposed_blocks") == 1
        assert s.counter("krylov_iterations") == k_ordinary
        for j in range(5):
            e_ref = float(np.max(np.abs(lu.solve(B[j]) - XS[j])) / np.max(np.abs(XS[j])))
            assert np.isfinite(e_ref)
            err = float(np.max(np.abs(X[j] - XS[j])) / np.max(np.abs(XS[j])))
            print("column %d: forward error %.2e, SuperLU %.2e" % (j, err, e_ref))
            assert err <= 10.0 * e_ref + 1e-12, (j, err, e_ref, s.counter("transposed_krylov_iterations"))
    finally:
        s.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_many_against_scipy_and_single(emu_lib, name):
    run_against_scipy_and_single(emu_lib, CASES[name]())


@pytest.mark.parametrize("mid", ["1", "0"])
def test_many_on_mid_and_tiled_fronts(emu_lib, monkeypatch, mid):
    """big fronts in both forms of E / E' (FD_DENSE_TOP and the tiled form with its skipped blocks), more than 32 pivots"""
    monkeypatch.setenv("HIPMF_MID_FRONT", mid)
    problem = P.convection_diffusion2d(44, 40, peclet=30)
    s = _handle(emu_lib, *problem)
    st = s.stats()
    assert st["max_front"] > 64 and st["max_pivots"] > 32
    assert (s.counter("mid_fronts") > 0) == (mid == "1")
    s.close()
    run_against_scipy_and_single(emu_lib, problem, seed=13)


@pytest.mark.parametrize("mid", ["1", "0"])
def test_column_independence_and_zero_column(emu_lib, monkeypatch, mid):
    monkeypatch.setenv("HIPMF_MID_FRONT", mid)
    run_column_independence(emu_lib, P.convection_diffusion2d(44, 40, peclet=30))


@pytest.mark.parametrize("nrhs", [9, 17])
def test_padded_columns(emu_lib, nrhs):
    run_padded_columns(emu_lib, nrhs)


@pytest.mark.parametrize("nrhs", [9, 17])
def test_padded_columns_with_refinement(emu_lib, nrhs):
    run_padded_columns_refined(emu_lib, nrhs)


def test_delegation(emu_lib):
    run_delegation(emu_lib)


def test_column_loop_without_block_buffers(emu_lib, monkeypatch):
    """HIPMF_TRANSPOSE_BLOCKED=0 takes the path of a failed allocation of the block buffers: the column loop, no error, blocks counter 0"""
    n, rp, ci, v = P.convection_diffusion2d(40, peclet=30)
    s = _handle(emu_lib, n, rp, ci, v)
    B = np.random.default_rng(8).standard_normal((5, n))
    monkeypatch.setenv("HIPMF_TRANSPOSE_BLOCKED", "0")
    X = s.solve_transpose_many(B)
    assert s.counter("transposed_blocks") == 0 and s.counter("transposed_solves") == 5
    for j in range(5):
        assert np.array_equal(X[j], s.solve_transpose(B[j]))
    s.close()


def test_status_codes(emu_lib):
    run_status_codes(emu_lib)


def test_replaced_pivots_rescue(emu_lib):
    run_replaced_pivots(emu_lib)
