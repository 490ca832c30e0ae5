"""Transposed solves with new values on a kept factor (solver_hipmf_solve_updated_transpose / _device / _many / _many_device and the
complex forms with `conjugate`; kernels_krylov_transpose.hpp) on the CPU emulator of the HIP kernels.
tests/test_solve_updated_transpose_gpu.py repeats the run_* cases on the device (lib None = the product build).

Matrices, references, own_relres and the accuracy rule are those of tests/test_solve_updated_cpu.py (T), per column those of
tests/test_solve_updated_many_cpu.py (M), for the complex handle those of tests/test_solve_updated_complex_cpu.py (Z) and
tests/test_solve_updated_complex_many_cpu.py (ZMANY) -- see their docstrings: rel_tol = 1e-10, the test's own residual recomputed in an
extended format <= 2 rel_tol with its rounding bound asserted below rel_tol first, the reported relres <= rel_tol and within the two
rounding bounds of the recomputation, forward error <= cond_2 2 rel_tol, steps <= the NumPy reference's + 1.  Nothing is a tuned number.
Everything is applied to the TRANSPOSED matrices: the operator is A_new^T (A_new^H / A_new^T for the complex handle), the reference
runs on (A_new^T, A_old^T).

Two matrices are this file's own.  arrow(1025): diagonal 4, first row and first column dense with entries +-1/1024 of independent signs
(strictly diagonally dominant, unsymmetric in value): A^T has one row of 1025 entries -- more than a row block of the product kernels
holds, summed by a whole workgroup -- next to rows of 2.  conv_grid(nx, ny): the 5-point Laplacian plus the skew convection term +0.3 /
-0.3 on the east / west neighbour; A(s) = conv_grid + s I.  The eigenvectors of its TRANSPOSE are known in closed form (eig_t), so the
block tests have columns that converge in one and in two steps next to random ones."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import test_solve_updated_complex_cpu as Z
import test_solve_updated_complex_many_cpu as ZMANY
import test_solve_updated_cpu as T
import test_solve_updated_many_cpu as M
from russell_amd import _capi
from test_complex_many_rhs_cpu import SENTINEL, ZM, bits, zpadded
from test_transpose_solve_cpu import ERROR_HIPMF_INVALID_VALUE, ERROR_NEED_FACTORIZATION, ERROR_NULL_POINTER, mumps_5x5

TOL = T.TOL
NOT_CONVERGED = T.NOT_CONVERGED
ERROR_NEED_INITIALIZATION = T.ERROR_NEED_INITIALIZATION
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL_SYMBOLS = ["solver_hipmf_solve_updated_transpose", "solver_hipmf_solve_updated_transpose_device", "solver_hipmf_solve_updated_transpose_many",
                "solver_hipmf_solve_updated_transpose_many_device"]
COMPLEX_SYMBOLS = ["complex_solver_hipmf_solve_updated_transpose", "complex_solver_hipmf_solve_updated_transpose_device",
                   "complex_solver_hipmf_solve_updated_transpose_many", "complex_solver_hipmf_solve_updated_transpose_many_device",
                   "complex_solver_hipmf_solve_transpose_many", "complex_solver_hipmf_solve_transpose_many_device"]
GRID = (24, 20)


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- this file's matrices ----

def case_of(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return (A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32)), dict(values=A.data.copy()), A.data.copy()


def arrow(n=1025):
    """(case, new values: the diagonal scaled by 1.5)"""
    rng = np.random.default_rng(n)
    A = sp.lil_matrix((n, n))
    A[0, 1:] = rng.choice([-1.0, 1.0], n - 1) / 1024.0
    A[1:, 0] = (rng.choice([-1.0, 1.0], n - 1) / 1024.0).reshape(-1, 1)
    A.setdiag(4.0)
    init, kw, v = case_of(A)
    diag = np.repeat(np.arange(n), np.diff(init[1])) == init[2]
    return (init, kw, v), v * np.where(diag, 1.5, 1.0)


def conv_grid(nx, ny):
    """(init, s -> values of A(s) = L + s I + C in CSR order): L the 5-point Laplacian, C = +0.3 on the east, -0.3 on the west neighbour"""
    lap = lambda m: sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    Cx = sp.diags([-0.3 * np.ones(nx - 1), 0.3 * np.ones(nx - 1)], [-1, 1])
    init, _, v = case_of(sp.kron(sp.identity(ny), lap(nx) + Cx) + sp.kron(lap(ny), sp.identity(nx)))
    diag = np.repeat(np.arange(init[0]), np.diff(init[1])) == init[2]
    return init, lambda s: v + s * diag


def eig_t(p, q, nx, ny):
    """eigenvector of A(s)^T for every s, x index fastest (the x part is a left eigenvector of tridiag(-1.3, 2, -0.7))"""
    i = np.arange(1, nx + 1)
    return np.outer((0.7 / 1.3) ** (i / 2.0) * np.sin(np.pi * p * i / (nx + 1)), np.sin(np.pi * q * np.arange(1, ny + 1) / (ny + 1))).flatten(order="F")


def conv_columns(n, nrhs, grid=GRID):
    """M.shift_columns for A(s)^T: random, one eigenvector (one step), two eigenvectors (two steps), zeros, random ones"""
    cols = [T.rhs_for(n, 3), eig_t(1, 1, *grid), eig_t(3, 5, *grid) + eig_t(20, 11, *grid), np.zeros(n), T.rhs_for(n, 21)]
    cols += [T.rhs_for(n, 100 + c) for c in range(5, nrhs)]
    return np.array(cols[:nrhs])


def conv_case(s1):
    """A(1) -> A(s1) on GRID: (init, kw, v0, v1, dense A(1)^T, dense A(s1)^T), computed once"""
    def make():
        init, vals = conv_grid(*GRID)
        v0, v1 = vals(1.0), vals(s1)
        kw = dict(values=v0)
        return init, kw, v0, v1, np.ascontiguousarray(T.dense(init, kw, v0).T), np.ascontiguousarray(T.dense(init, kw, v1).T)
    return M.cached(("conv_case", s1), make)


# ---- real handle: single form ----

def run_transposed_not_plain(lib, name, init, kw, values):
    """values changed in three rows: the accuracy rule holds for A_new^T, and the same x violates it for A_new"""
    v1 = T.redraw_rows(init, values)
    A0, A1 = T.dense(init, kw, values), T.dense(init, kw, v1)
    b = T.rhs_for(init[0], 2)
    own_plain_numpy = T.own_relres(A1, np.linalg.solve(A1.T, b), b)[0]
    assert own_plain_numpy > 2 * TOL, own_plain_numpy  # (the premise, in NumPy: this right-hand side tells A_new^T from A_new)
    _, ref_steps, ref_rel = T.fgmres_reference(A1.T, A0.T, b, TOL, 30, 120)
    print("reference: %d steps, relres %.3e" % (ref_steps, ref_rel))
    assert ref_steps <= 5 and ref_rel <= TOL
    s = T.handle(lib, init, kw, values)
    try:
        x, steps, relres, status = s.solve_updated(b, v1, rel_tol=TOL, transpose=True)
        print("device: %d steps, relres %.3e" % (steps, relres))
        assert status == 0 and steps <= ref_steps + 1
        assert s.counter("updated_steps") == steps and s.counter("updated_cycles") >= 1
        T.check_accuracy(A1.T, x, b, relres)
        assert T.own_relres(A1, x, b)[0] > 2 * TOL
    finally:
        s.close()


def run_unchanged(lib, init, kw, values):
    A = T.dense(init, kw, values)
    b = T.rhs_for(A.shape[0])
    s = T.handle(lib, init, kw, values)
    try:
        x, steps, relres, status = s.solve_updated(b, values, rel_tol=TOL, transpose=True)
        assert (steps, status) == (1, 0), (steps, status, relres)
        assert s.counter("updated_steps") == 1 and s.counter("updated_cycles") == 1
        T.check_accuracy(A.T, x, b, relres)
    finally:
        s.close()


def run_symmetric_is_plain(lib, init, kw, values):
    """A^T = A: the bits of the plain forms, single and blocked"""
    n = init[0]
    v1 = T.redraw_rows(init, values)
    B = np.array([T.rhs_for(n, 70 + c) for c in range(17)])
    s = T.handle(lib, init, kw, values)
    try:
        xp, stp, rp_, cp = s.solve_updated(B[0], v1, rel_tol=TOL)
        xt, stt, rt, ct = s.solve_updated(B[0], v1, rel_tol=TOL, transpose=True)
        assert (stp, rp_, cp) == (stt, rt, ct) and cp == 0 and np.array_equal(u64(xp), u64(xt))
        Xp, Sp, Rp, Cp = s.solve_updated_many(B, v1, rel_tol=TOL)
        Xt, St, Rt, Ct = s.solve_updated_many(B, v1, rel_tol=TOL, transpose=True)
        assert Cp == Ct == 0 and np.array_equal(Sp, St) and np.array_equal(u64(Rp), u64(Rt)) and np.array_equal(u64(Xp), u64(Xt))
    finally:
        s.close()


def run_edges(lib, key, case, v1, nrhs=3):
    """single and block form on a matrix whose size or row lengths sit at an edge of the product kernels (per-column rule, step bound)"""
    init, kw, values = case
    n = init[0]
    A0t, A1t = M.cached(("A0t", key), lambda: np.ascontiguousarray(T.dense(init, kw, values).T)), M.cached(("A1t", key), lambda: np.ascontiguousarray(T.dense(init, kw, v1).T))
    B = np.array([T.rhs_for(n, 2 + c) for c in range(nrhs)])
    ref = M.reference_columns("edge_" + key, A1t, A0t, B, 30, 120)
    print("reference", ref)
    assert all(r[1] <= TOL and r[0] <= 30 for r in ref)  # (the reference reaches the tolerance within the default restart)
    s = T.handle(lib, init, kw, values)
    try:
        x, steps, relres, status = s.solve_updated(B[0], v1, rel_tol=TOL, transpose=True)
        assert status == 0 and steps <= ref[0][0] + 1
        X, St, Rr, status = s.solve_updated_many(B, v1, rel_tol=TOL, transpose=True)
        print("device steps", steps, St.tolist())
        assert status == 0 and all(St[c] <= ref[c][0] + 1 for c in range(nrhs))
        M.check_columns("edge_" + key, A1t, np.vstack([x[None, :], X]), np.vstack([B[:1], B]), np.concatenate([[relres], Rr]))
    finally:
        s.close()


def mapped_inputs(init, values, seed=11):
    """T.run_mapped's inputs: every CSR entry the sum of two triplets in a shuffled order -> (seg_ptr, seg_idx, inputs, the summed values)"""
    nnz = values.size
    rng = np.random.default_rng(seed)
    v1 = T.redraw_rows(init, values)
    parts = np.concatenate([v1 * rng.uniform(0.2, 0.8, nnz), np.zeros(nnz)])
    parts[nnz:] = v1 - parts[:nnz]
    order = rng.permutation(2 * nnz)
    where = np.argsort(order)
    seg_idx = np.empty(2 * nnz, np.int64)
    seg_idx[0::2], seg_idx[1::2] = where[:nnz], where[nnz:]
    inputs = parts[order]
    return 2 * np.arange(nnz + 1), seg_idx, inputs, (0.0 + inputs[seg_idx[0::2]]) + inputs[seg_idx[1::2]]


def run_mapped(lib, init, kw, values):
    n = init[0]
    seg_ptr, seg_idx, inputs, summed = mapped_inputs(init, values)
    B = np.array([T.rhs_for(n, 4), T.rhs_for(n, 14), T.rhs_for(n, 24)])
    s = T.handle(lib, init, kw, values)
    try:
        for call in (lambda: s.solve_updated(B[0], inputs, mapped=True, rel_tol=TOL, transpose=True),
                     lambda: s.solve_updated_many(B, inputs, mapped=True, rel_tol=TOL, transpose=True)):
            with pytest.raises(Exception) as e:
                call()
            assert e.value.code == ERROR_HIPMF_INVALID_VALUE  # no map yet
        assert s.set_value_map(seg_ptr, seg_idx) == 0
        xm, steps_m, rel_m, st_m = s.solve_updated(B[0], inputs, mapped=True, rel_tol=TOL, transpose=True)
        x0, steps_0, rel_0, st_0 = s.solve_updated(B[0], summed, mapped=False, rel_tol=TOL, transpose=True)
        assert (steps_m, st_m) == (steps_0, st_0) and st_0 == 0 and rel_m == rel_0 and np.array_equal(u64(xm), u64(x0))
        T.check_accuracy(T.dense(init, kw, summed).T, xm, B[0], rel_m)
        Xm, Sm, Rm, Cm = s.solve_updated_many(B, inputs, mapped=True, rel_tol=TOL, transpose=True)
        X0, S0, R0, C0 = s.solve_updated_many(B, summed, mapped=False, rel_tol=TOL, transpose=True)
        assert Cm == C0 == 0 and np.array_equal(Sm, S0) and np.array_equal(u64(Rm), u64(R0)) and np.array_equal(u64(Xm), u64(X0))
    finally:
        s.close()


def run_status_codes(lib):
    (n, rp, ci, v), _ = mumps_5x5()
    v = np.array(v, float)
    s = T._new(lib)
    try:
        x, b = np.zeros(n), np.ones(n)
        one, many = s.lib.solver_hipmf_solve_updated_transpose, s.lib.solver_hipmf_solve_updated_transpose_many
        X, B = np.zeros((2, n)), np.ones((2, n))
        assert one(s.h, x, b, v, 0, TOL, 0, None, None, 0) == ERROR_NEED_INITIALIZATION
        assert many(s.h, X, B, 2, n, v, 0, TOL, 0, None, None, 0) == ERROR_NEED_INITIALIZATION
        assert s.initialize(n, rp, ci) == 0
        assert one(s.h, x, b, v, 0, TOL, 0, None, None, 0) == ERROR_NEED_FACTORIZATION
        assert many(s.h, X, B, 2, n, v, 0, TOL, 0, None, None, 0) == ERROR_NEED_FACTORIZATION
        dv = C.c_void_p(8)
        assert s.lib.solver_hipmf_solve_updated_transpose_device(s.h, dv, dv, dv, 0, TOL, 0, None, None) == ERROR_NEED_FACTORIZATION
        assert s.lib.solver_hipmf_solve_updated_transpose_many_device(s.h, dv, dv, 2, n, dv, 0, TOL, 0, None, None) == ERROR_NEED_FACTORIZATION
        assert s.factorize(v) == 0
        assert one(s.h, x, b, v, 0, TOL, 0, None, None, 0) == 0  # (steps and relres may be NULL)
        assert many(s.h, X, B, 2, n, v, 0, TOL, 0, None, None, 0) == 0
        for bad in (float("nan"), float("inf")):
            assert one(s.h, x, b, v, 0, bad, 0, None, None, 0) == ERROR_HIPMF_INVALID_VALUE
            assert many(s.h, X, B, 2, n, v, 0, bad, 0, None, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert one(s.h, x, b, v, 1, TOL, 0, None, None, 0) == ERROR_HIPMF_INVALID_VALUE  # mapped without a map
        assert many(s.h, X, B, 2, n, v, 1, TOL, 0, None, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert many(s.h, X, B, 0, n, v, 0, TOL, 0, None, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert many(s.h, X, B, 2, n - 1, v, 0, TOL, 0, None, None, 0) == ERROR_HIPMF_INVALID_VALUE
        xz, steps, relres, status = s.solve_updated(np.zeros(n), v, transpose=True)
        assert (steps, relres, status) == (0, 0.0, 0) and not xz.any()
        xd, steps, relres, status = s.solve_updated(b, v, transpose=True)  # the defaults: 1e-12, 4 x restart
        assert status == 0 and relres <= 1e-12 and steps == 1
        raw = C.CDLL(s.lib._name)  # (untyped bindings: NULL pointers pass)
        raw.solver_hipmf_solve_updated_transpose.restype = C.c_int32
        raw.solver_hipmf_solve_updated_transpose.argtypes = [C.c_void_p] * 4 + [C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
        h, xp, bp, vp = C.c_void_p(s.h), x.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)
        for args in ((None, xp, bp, vp), (h, None, bp, vp), (h, xp, None, vp), (h, xp, bp, None)):
            assert raw.solver_hipmf_solve_updated_transpose(*args, 0, TOL, 0, None, None, 0) == ERROR_NULL_POINTER
    finally:
        s.close()


TR_COUNTERS = ("krylov_iterations", "transposed_solves", "transposed_blocks", "transposed_krylov_iterations", "updated_basis_bytes")


def run_no_side_effects(lib, init, kw, values):
    """a solve, a solve_transpose, a solve_transpose_many and a solve_updated with their counters and statistics: the same bits before and
    after transposed updated calls (single and block form); HIPMF_COUNTER_UPDATED_* report the transposed call"""
    n = init[0]
    v1 = T.redraw_rows(init, values)
    B = np.array([T.rhs_for(n, 30 + c) for c in range(17)])
    b = B[0]
    s = T.handle(lib, init, kw, values, nstep=-1)
    try:
        def snapshot():
            out = [u64(s.solve(b)).copy()]
            st = s.stats()
            out += [st["refinement_steps"], st["fused_fallbacks"], s.num_perturbed]
            out += [u64(s.solve_transpose(b)).copy(), u64(s.solve_transpose_many(B[:5])).copy()]
            out += [s.counter(k) for k in TR_COUNTERS[2:4]]
            xu, su, ru, cu = s.solve_updated(b, v1, rel_tol=TOL)
            return out + [u64(xu).copy(), su, ru, cu, u64(s.mat_vec_mul(b)).copy()]
        before = snapshot()
        keep = [s.counter(k) for k in TR_COUNTERS] + [s.stats()["refinement_steps"]]
        x, steps, relres, status = s.solve_updated(b, v1, rel_tol=TOL, transpose=True)
        assert status == 0 and s.counter("updated_steps") == steps and s.counter("updated_blocks") == 0
        assert [s.counter(k) for k in TR_COUNTERS] + [s.stats()["refinement_steps"]] == keep
        X, St, Rr, status = s.solve_updated_many(B, v1, rel_tol=TOL, transpose=True)
        assert status == 0 and s.counter("updated_blocks") == 2 and s.counter("updated_column_steps") == int(St.sum())
        assert [s.counter(k) for k in TR_COUNTERS[:4]] + [s.stats()["refinement_steps"]] == keep[:4] + keep[5:]
        after = snapshot()
        for a, c in zip(before, after):
            assert np.array_equal(a, c)
        T.check_accuracy(T.dense(init, kw, v1).T, x, b, relres)
    finally:
        s.close()


def run_reproducible(lib, init, kw, values):
    n = init[0]
    v1 = T.redraw_rows(init, values)
    B = np.array([T.rhs_for(n, 40 + c) for c in range(17)])
    s = T.handle(lib, init, kw, values)
    try:
        a, b = s.solve_updated(B[0], v1, rel_tol=TOL, transpose=True), s.solve_updated(B[0], v1, rel_tol=TOL, transpose=True)
        assert a[1:] == b[1:] and a[3] == 0 and np.array_equal(u64(a[0]), u64(b[0]))
        X1, S1, R1, C1 = s.solve_updated_many(B, v1, rel_tol=TOL, transpose=True)
        X2, S2, R2, C2 = s.solve_updated_many(B, v1, rel_tol=TOL, transpose=True)
        assert C1 == C2 == 0 and np.array_equal(S1, S2) and np.array_equal(u64(R1), u64(R2)) and np.array_equal(u64(X1), u64(X2))
        assert s.counter("updated_blocks") == 2
    finally:
        s.close()


def run_device_entry(lib, init, kw, values):
    """the _device entry points (the block form with leading dimension n + 1) give the bits of the host entry points"""
    n, nrhs, ld = init[0], 17, init[0] + 1
    v1 = T.redraw_rows(init, values)
    B = np.array([T.rhs_for(n, 60 + c) for c in range(nrhs)])
    s = T.handle(lib, init, kw, values)
    ptrs = []
    try:
        xh, steps, relres, status = s.solve_updated(B[0], v1, rel_tol=TOL, transpose=True)
        Xh, St, Rr, Cs = s.solve_updated_many(B, v1, rel_tol=TOL, transpose=True)
        assert status == 0 and Cs == 0
        d_x, d_b, d_v = s.dev_alloc(8 * ld * nrhs), s.dev_alloc(8 * ld * nrhs), s.dev_alloc(8 * v1.size)
        ptrs += [d_x, d_b, d_v]
        s.h2d(d_v, v1)
        s.h2d(d_b, B[0])
        assert s.solve_updated_device(d_x, d_b, d_v, rel_tol=TOL, transpose=True) == (steps, relres, status)
        xd = np.zeros(n)
        s.d2h(xd, d_x)
        assert np.array_equal(u64(xd), u64(xh))
        Bp = M.padded(B, ld)
        s.h2d(d_b, Bp)
        s.h2d(d_x, np.full((nrhs, ld), 3.25))
        st_d, rel_d, c_d = s.solve_updated_many_device(d_x, d_b, nrhs, d_v, rel_tol=TOL, ld=ld, transpose=True)
        assert c_d == Cs and np.array_equal(st_d, St) and np.array_equal(u64(rel_d), u64(Rr))
        Xd, Bd = np.zeros((nrhs, ld)), np.zeros((nrhs, ld))
        s.d2h(Xd, d_x)
        s.d2h(Bd, d_b)
        assert np.array_equal(u64(Xd[:, :n]), u64(Xh)) and np.all(Xd[:, n:] == 3.25)  # (entries ndim ... ld-1 are not written)
        assert np.array_equal(u64(Bd), u64(Bp))
    finally:
        for p in ptrs:
            s.dev_free(p)
        s.close()


def run_perturbed(lib):
    """T.run_perturbed's matrix (replaced pivots: only a weaker preconditioner, no rescue inside): converged or honestly NOT_CONVERGED, the
    reported relres is the recomputed one"""
    A = T._pm1(400, 4, np.random.default_rng(3))
    n, rp, ci, v = A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
    At = A.T.toarray()
    s = T._new(lib)
    try:
        assert s.initialize(n, rp, ci, values=v) == 0 and s.factorize(v) == 0
        assert s.num_perturbed > 0
        B = np.array([T.rhs_for(n, 8), T.rhs_for(n, 9)])
        x, steps, relres, status = s.solve_updated(B[0], v, rel_tol=TOL, transpose=True)
        X, St, Rr, Cs = s.solve_updated_many(B, v, rel_tol=TOL, transpose=True)
        print("%d replaced pivots: %d steps, relres %.3e; block %s %s" % (s.num_perturbed, steps, relres, St.tolist(), Rr.tolist()))
        for xx, bb, rel, code, st in [(x, B[0], relres, status, steps)] + [(X[c], B[c], Rr[c], Cs, St[c]) for c in range(2)]:
            own, bound, bound_double = T.own_relres(At, xx, bb)
            assert code in (0, NOT_CONVERGED) and st >= 1 and np.isfinite(rel)
            assert abs(rel - own) <= bound + bound_double, (rel, own)
            assert (rel <= TOL) if code == 0 else True
        assert (Cs == 0) == bool(np.all(Rr <= TOL))
    finally:
        s.close()


# ---- real handle: block form ----

def run_block(lib, nrhs, pad):
    """A(1) -> A(2) on the convection grid: columns that converge at different steps, a zero column, padded leading dimension; per column
    the rule and the step bound; one column is the single form"""
    init, kw, v0, v1, A0t, A1t = conv_case(2.0)
    n = init[0]
    B = conv_columns(n, nrhs)
    ref = M.reference_columns("conv2", A1t, A0t, B, 30, 120)
    ref_steps = [r[0] for r in ref]
    print("reference steps", ref_steps)
    assert all(r[1] <= TOL for r in ref)
    if nrhs >= 5:
        assert ref_steps[1:4] == [1, 2, 0] and ref_steps[0] > 2 and len(set(ref_steps)) >= 4  # (what makes the case meaningful)
    s = T.handle(lib, init, kw, v0)
    try:
        assert s.counter("symmetric_ldlt") == 0
        ld = n + pad
        Bp = M.padded(B, ld)
        X, steps, relres, status = s.solve_updated_many(Bp, v1, rel_tol=TOL, ld=ld, transpose=True)
        print("device steps", steps.tolist())
        assert status == 0 and all(steps[c] <= ref_steps[c] + 1 for c in range(nrhs)), (steps, ref_steps)
        assert np.array_equal(u64(X[:, n:]), u64(Bp[:, n:]))  # (the padding is not written)
        skip = (3,) if nrhs > 3 else ()
        if nrhs > 3:
            assert not X[3, :n].any() and steps[3] == 0 and relres[3] == 0.0
        if nrhs == 1:
            x1, st1, r1, c1 = s.solve_updated(B[0], v1, rel_tol=TOL, transpose=True)
            assert (int(steps[0]), float(relres[0]), status) == (st1, r1, c1) and np.array_equal(u64(X[0, :n]), u64(x1))
            assert s.counter("updated_blocks") == 0 and s.counter("updated_column_steps") == st1
        else:
            M.block_counters(s, steps, nrhs, n)
        M.check_columns("conv2", A1t, X[:, :n], B, relres, skip=skip)
    finally:
        s.close()


def run_position_independence(lib):
    """the same column in slot 0 of the first block and in slot 7 of the second, between other neighbours: the same bits, steps, relres"""
    init, kw, v0, v1, _, _ = conv_case(2.0)
    n = init[0]
    B = np.array([T.rhs_for(n, 200 + c) for c in range(24)])
    B[23] = B[0]
    B[5], B[20] = eig_t(1, 1, *GRID), 0.0
    s = T.handle(lib, init, kw, v0)
    try:
        X, steps, relres, status = s.solve_updated_many(B, v1, rel_tol=TOL, transpose=True)
        assert status == 0 and steps[5] == 1 and steps[0] > 2
        assert steps[0] == steps[23] and relres[0] == relres[23] and np.array_equal(u64(X[0]), u64(X[23]))
        Y, st2, rr2, status = s.solve_updated_many(B[[7, 0, 5]], v1, rel_tol=TOL, transpose=True)
        assert status == 0 and np.array_equal(st2, steps[[7, 0, 5]]) and np.array_equal(u64(rr2), u64(relres[[7, 0, 5]]))
        assert np.array_equal(u64(Y), u64(X[[7, 0, 5]]))
    finally:
        s.close()


def run_cycles(lib, monkeypatch, restart=4, s1=100.0, max_steps=400):
    """a short restart length: the columns finish in different cycles"""
    monkeypatch.setenv("HIPMF_UPDATED_RESTART", str(restart))
    init, kw, v0, v1, A0t, A1t = conv_case(s1)
    n = init[0]
    B = conv_columns(n, 3)
    ref = M.reference_columns("conv%g" % s1, A1t, A0t, B, restart, max_steps)
    ref_steps = [r[0] for r in ref]
    print("reference steps", ref_steps)
    assert ref_steps[0] > restart and ref_steps[1:] == [1, 2] and all(r[1] <= TOL for r in ref)
    s = T.handle(lib, init, kw, v0)
    try:
        X, steps, relres, status = s.solve_updated_many(B, v1, rel_tol=TOL, max_steps=max_steps, transpose=True)
        print("device steps", steps.tolist(), "cycles", s.counter("updated_cycles"))
        assert status == 0 and all(steps[c] <= ref_steps[c] + 1 for c in range(3)), (steps, ref_steps)
        assert steps[0] > restart and s.counter("updated_cycles") >= (int(steps.max()) + restart - 1) // restart
        M.check_columns("conv%g" % s1, A1t, X, B, relres)
    finally:
        s.close()


def run_not_converged_and_nan(lib):
    """max_steps = 2 on A(1) -> A(100): NOT_CONVERGED per column with the best iterate; a column with a NaN entry leaves the others alone"""
    init, kw, v0, v1, A0t, A1t = conv_case(100.0)
    n = init[0]
    bad = T.rhs_for(n, 21)
    bad[n // 2] = np.nan
    B = np.array([T.rhs_for(n, 3), eig_t(1, 1, *GRID), np.zeros(n), bad])
    s = T.handle(lib, init, kw, v0)
    try:
        X, steps, relres, status = s.solve_updated_many(B, v1, rel_tol=TOL, max_steps=2, transpose=True)
        print("steps %s relres %s" % (steps.tolist(), relres.tolist()))
        assert status == NOT_CONVERGED and steps.tolist() == [2, 1, 0, 0]
        assert TOL < relres[0] < 1.0 and relres[1] <= TOL and relres[2] == 0.0 and np.isnan(relres[3])
        assert not X[2].any() and not X[3].any() and np.all(np.isfinite(X))
        own, bound, bound_double = M.relres_columns(A1t, X[:1], B[:1])[0]
        assert bound < TOL and abs(relres[0] - own) <= bound + bound_double
        M.check_columns("conv100", A1t, X[1:2], B[1:2], relres[1:2])
        x, st, rel, code = s.solve_updated(B[0], v1, rel_tol=TOL, max_steps=2, transpose=True)
        assert (code, st) == (NOT_CONVERGED, 2) and TOL < rel < 1.0
        # the rest of the block converges when it is given the steps
        X, steps, relres, status = s.solve_updated_many(B, v1, rel_tol=TOL, transpose=True)
        assert status == NOT_CONVERGED and np.isnan(relres[3]) and np.all(relres[:3] <= TOL) and steps[0] > 2
        M.check_columns("conv100", A1t, X[:2], B[:2], relres[:2])
    finally:
        s.close()


def run_host_mirror(lib):
    """LinSolver.solve_updated / solve_updated_many of russell_amd.sparse with transpose=True, as T.test_host_mirror"""
    from russell_amd import sparse as S

    S._L().rh_set_hipmf_library((lib or os.path.join(ROOT, "russell_amd", "lib", "librussell_hipmf.so")).encode())
    try:
        init, vals = conv_grid(12, 10)
        n, rp, ci = init
        A0 = sp.csr_matrix((vals(1.0), ci, rp), shape=(n, n)).tocoo()
        A1 = sp.csr_matrix((vals(2.0), ci, rp), shape=(n, n))
        mat0 = S.CooMatrix.from_arrays(n, n, A0.row, A0.col, A0.data)
        mat1 = S.CooMatrix.from_arrays(n, n, A0.row, A0.col, A1.tocoo().data)
        B = np.array([T.rhs_for(n, 10), T.rhs_for(n, 11), T.rhs_for(n, 12)])
        solver = S.LinSolver(S.Genie.Hipmf)
        solver.actual.factorize(mat0)
        x, steps, relres = solver.solve_updated(mat1, B[0], rel_tol=TOL, transpose=True)
        assert 1 < steps <= 30
        T.check_accuracy(A1.toarray().T, x, B[0], relres)
        X, St, Rr = solver.solve_updated_many(mat1, B, rel_tol=TOL, transpose=True)
        M.check_columns("host_conv", A1.toarray().T, X, B, Rr)
        mat100 = S.CooMatrix.from_arrays(n, n, A0.row, A0.col, sp.csr_matrix((vals(100.0), ci, rp), shape=(n, n)).tocoo().data)
        with pytest.raises(S.StrError, match=r"Error\(2\): the iteration on the kept factorization did not converge"):
            solver.solve_updated(mat100, B[0], rel_tol=TOL, max_steps=2, transpose=True)
    finally:
        S._L().rh_set_hipmf_library(os.path.join(ROOT, "russell_amd", "lib", "librussell_hipmf.so").encode())


# ---- complex handle ----

class ZT(ZM):
    """ZM with the transposed updated entry points; conjugate: 1 -> A^H, 0 -> A^T"""

    def solve_updated_t(self, b, v, conjugate, mapped=False, rel_tol=0.0, max_steps=0):
        x = np.zeros(2 * self.n)
        steps, relres = C.c_int32(-1), C.c_double(-1.0)
        code = self.lib.complex_solver_hipmf_solve_updated_transpose(self.h, x, Z.interleave(b), Z.interleave(v), int(bool(mapped)), float(rel_tol), int(max_steps),
                                                                     C.byref(steps), C.byref(relres), int(conjugate), 0)
        if code not in (0, NOT_CONVERGED):
            raise self.error(code)
        return Z.as_complex(x), steps.value, relres.value, code

    def solve_updated_t_many(self, B, v, conjugate, mapped=False, rel_tol=0.0, max_steps=0, ld=None, device=False):
        B = np.ascontiguousarray(B, np.complex128)
        nrhs, ld = B.shape[0], ld or B.shape[1]
        X = np.full((nrhs, ld), SENTINEL, np.complex128)
        zv = Z.interleave(v)
        steps, relres = np.full(nrhs, -1, np.int32), np.full(nrhs, -1.0)
        if not device:
            code = self.lib.complex_solver_hipmf_solve_updated_transpose_many(self.h, X.view(np.float64).reshape(-1), B.view(np.float64).reshape(-1), nrhs, ld, zv,
                                                                              int(bool(mapped)), float(rel_tol), int(max_steps), steps.ctypes.data, relres.ctypes.data,
                                                                              int(conjugate), 0)
        else:
            d_x, d_b, d_v = self.dev_alloc(X.nbytes), self.dev_alloc(B.nbytes), self.dev_alloc(zv.nbytes)
            try:
                self.h2d(d_x, X)
                self.h2d(d_b, B)
                self.h2d(d_v, zv)
                code = self.lib.complex_solver_hipmf_solve_updated_transpose_many_device(self.h, d_x, d_b, nrhs, ld, d_v, int(bool(mapped)), float(rel_tol),
                                                                                         int(max_steps), steps.ctypes.data, relres.ctypes.data, int(conjugate))
                self.d2h(X, d_x)
                Bb = np.zeros_like(B)
                self.d2h(Bb, d_b)
                assert np.array_equal(bits(Bb), bits(B))  # (the right-hand sides are not changed, conjugate = 0 included)
            finally:
                for p in (d_x, d_b, d_v):
                    self.dev_free(p)
        if code not in (0, NOT_CONVERGED):
            raise self.error(code)
        return X, steps, relres, code


def complex_case(name):
    """name -> (n, rp, ci, v0, v1, keywords of ZH): ref5 and zchain257 with three rows redrawn, the 24 x 20 shifted grid (unsym) K(1) -> K(0.8)"""
    if name == "grid":
        n, rp, ci, vals = Z.shifted_grid(24, 20, unsym=True)
        return n, rp, ci, vals(1.0), vals(0.8), {}
    case, kw = Z.matrix(name)
    return case + (Z.redraw_rows(case), kw)


def op(A, conjugate):
    """the operator of the transposed forms as a dense matrix: A^H (conjugate = 1) or A^T"""
    D = np.asarray(A.todense()) if sp.issparse(A) else np.asarray(A)
    return np.ascontiguousarray(D.conj().T if conjugate else D.T)


def run_complex(lib, name, nrhs_list=(1, 16, 17)):
    """conjugate = 1 against NumPy's A_new^H, conjugate = 0 against A_new^T; the step bound from the complex reference on the transposed /
    adjoint matrices; conjugate = 0 is conj of the conjugate = 1 result for conj(b), bit for bit; the block form per column; the device form"""
    n, rp, ci, v0, v1, kw = complex_case(name)
    lower = kw.get("lower", False)
    A0, A1 = Z.full(n, rp, ci, v0, lower), Z.full(n, rp, ci, v1, lower)
    B = np.array([Z.rhs_for(n, 2 + c) for c in range(max(nrhs_list))])
    s = ZT(lib, n, rp, ci, v0, **kw)
    try:
        for conjugate in (1, 0):
            O0, O1 = op(A0, conjugate), op(A1, conjugate)
            cond = M.cached(("zcond", name, conjugate), lambda: float(np.linalg.cond(O1)))
            refs = [M.cached(("zref", name, conjugate, c), lambda: Z.fgmres_reference(O1, O0, B[c], TOL, 30, 120)[1:]) for c in range(len(B))]
            assert all(r[1] <= TOL for r in refs)
            x, steps, relres, status = s.solve_updated_t(B[0], v1, conjugate, rel_tol=TOL)
            print("%s conjugate %d: %d steps (reference %d), relres %.3e" % (name, conjugate, steps, refs[0][0], relres))
            assert status == 0 and steps <= refs[0][0] + 1
            assert s.counter("updated_complex_arithmetic") == 1 and s.counter("updated_steps") == steps
            Z.check_accuracy(sp.csr_matrix(O1), x, B[0], relres, cond)
            if not lower:
                assert Z.own_relres(A1, x, B[0])[0] > 2 * TOL  # (not the plain system)
            for nrhs in nrhs_list:
                X, St, Rr, code = s.solve_updated_t_many(zpadded(B[:nrhs], n + 2), v1, conjugate, rel_tol=TOL, ld=n + 2)
                assert code == 0 and np.array_equal(bits(X[:, n:]), bits(np.full((nrhs, 2), SENTINEL, np.complex128)))
                assert all(St[c] <= refs[c][0] + 1 for c in range(nrhs)), (St.tolist(), [r[0] for r in refs])
                if nrhs == 1:
                    assert (int(St[0]), float(Rr[0])) == (steps, relres) and np.array_equal(bits(X[0, :n]), bits(x))
                    assert s.counter("updated_blocks") == 0
                else:
                    assert s.counter("updated_blocks") == (nrhs + 15) // 16
                ZMANY.check_columns(O1, X, B[:nrhs], Rr, cond)
                if nrhs == max(nrhs_list) and conjugate == 0:  # (the device form: the same bits, the right-hand sides unchanged)
                    Xd, Sd, Rd, cd = s.solve_updated_t_many(zpadded(B[:nrhs], n + 2), v1, conjugate, rel_tol=TOL, ld=n + 2, device=True)
                    assert cd == code and np.array_equal(Sd, St) and np.array_equal(bits(Rd), bits(Rr)) and np.array_equal(bits(Xd), bits(X))
        # A^T through the A^H iteration on conjugated data
        xh, sh, rh, ch = s.solve_updated_t(np.conj(B[0]), v1, 1, rel_tol=TOL)
        xt, st, rt, ct = s.solve_updated_t(B[0], v1, 0, rel_tol=TOL)
        if not lower:
            assert (st, rt, ct) == (sh, rh, ch) and np.array_equal(bits(xt), bits(np.conj(xh)))
            XH, SH, RH, _ = s.solve_updated_t_many(np.conj(B[:3]), v1, 1, rel_tol=TOL)
            XT, ST, RT, _ = s.solve_updated_t_many(B[:3], v1, 0, rel_tol=TOL)
            assert np.array_equal(ST, SH) and np.array_equal(bits(RT), bits(RH)) and np.array_equal(bits(XT), bits(np.conj(XH)))
        else:  # complex symmetric: A^T = A, the plain form's bits
            xp, sp_, rp_, cp = s.solve_updated(B[0], v1, rel_tol=TOL)
            assert (st, rt, ct) == (sp_, rp_, cp) and np.array_equal(bits(xt), bits(xp))
            XP, SP, RP, _ = s.solve_updated_many(B[:3], v1, rel_tol=TOL)
            XT, ST, RT, _ = s.solve_updated_t_many(B[:3], v1, 0, rel_tol=TOL)
            assert np.array_equal(ST, SP) and np.array_equal(bits(RT), bits(RP)) and np.array_equal(bits(XT), bits(XP))
    finally:
        s.close()


def run_complex_reproducible(lib, name, env=None):
    """Z.run_reproducible for the transposed forms, single and blocked, both conjugate values: two calls give the same bits of x, steps
    and relres, and the result is held to the accuracy rule.  env: e.g. HIPMF_COMPLEX_PAIRS=0, the plain real-equivalent factorisation,
    whose transposed pass pair is not complex-linear, as preconditioner.  A zero column (and a zero right-hand side of the single form)
    comes back as +0.0 in every entry for both conjugate values, as the plain forms return it"""
    n, rp, ci, v0, v1, kw = complex_case(name)
    lower = kw.get("lower", False)
    A1 = Z.full(n, rp, ci, v1, lower)
    B = np.array([Z.rhs_for(n, 6 + c) for c in range(17)])
    B[3] = 0.0
    s = ZT(lib, n, rp, ci, v0, env=env, **kw)
    try:
        for conjugate in (1, 0):
            O1 = sp.csr_matrix(op(A1, conjugate))
            x1, st1, r1, c1 = s.solve_updated_t(B[0], v1, conjugate, rel_tol=TOL)
            x2, st2, r2, c2 = s.solve_updated_t(B[0], v1, conjugate, rel_tol=TOL)
            print("%s %s conjugate %d: %d steps, relres %.3e" % (name, env, conjugate, st1, r1))
            assert (st1, c1) == (st2, c2) and c1 == 0 and st1 >= 1 and r1 == r2 and np.array_equal(bits(x1), bits(x2))
            Z.check_accuracy(O1, x1, B[0], r1)
            X1, S1, R1, C1 = s.solve_updated_t_many(B, v1, conjugate, rel_tol=TOL)
            X2, S2, R2, C2 = s.solve_updated_t_many(B, v1, conjugate, rel_tol=TOL)
            assert C1 == C2 == 0 and np.array_equal(S1, S2) and np.array_equal(bits(R1), bits(R2)) and np.array_equal(bits(X1), bits(X2))
            assert s.counter("updated_blocks") == 2
            for c in (1, 16):
                Z.check_accuracy(O1, X1[c], B[c], float(R1[c]))
            xz, stz, rz, cz = s.solve_updated_t(B[3], v1, conjugate, rel_tol=TOL)
            assert (stz, rz, cz) == (0, 0.0, 0) and not bits(xz).any()
            assert (S1[3], R1[3]) == (0, 0.0) and not bits(X1[3]).any()
    finally:
        s.close()


def run_complex_no_side_effects(lib):
    n, rp, ci, v0, v1, kw = complex_case("grid")
    B = np.array([Z.rhs_for(n, 30 + c) for c in range(17)])
    s = ZT(lib, n, rp, ci, v0, nstep=-1)
    try:
        def snapshot():
            x = s.solve(B[0])
            xt = np.zeros(2 * n)
            assert s.lib.complex_solver_hipmf_solve_transpose(s.h, xt, Z.interleave(B[0]), 1, 0) == 0
            xu, su, ru, cu = s.solve_updated(B[0], v1, rel_tol=TOL)
            return [bits(x).copy(), bits(xt).copy(), bits(xu).copy(), su, ru, cu, s.stats()[0][10]] + [s.counter(k) for k in ("krylov_iterations", "transposed_krylov_iterations",
                                                                                                                       "fused_fallbacks")]
        before, t0 = snapshot(), s.counter("transposed_solves")
        for conjugate in (1, 0):
            assert s.solve_updated_t(B[0], v1, conjugate, rel_tol=TOL)[3] == 0
            assert s.solve_updated_t_many(B, v1, conjugate, rel_tol=TOL)[3] == 0
        assert s.counter("transposed_solves") == t0
        for a, c in zip(before, snapshot()):
            assert np.array_equal(a, c)
    finally:
        s.close()


def run_complex_status_codes(lib):
    """the codes of the plain complex forms in their order, plus the conjugate check; the map check comes last"""
    case, _ = Z.matrix("ref5")
    n, rp, ci, v0 = case
    zv, x, b = Z.interleave(v0), np.zeros(2 * n), Z.interleave(Z.rhs_for(n))
    X, B = np.zeros(4 * n), np.concatenate([b, b])
    s = ZT(lib, n, rp, ci, v0, factorize=False)
    try:
        one = lambda conj=1, tol=TOL, mapped=0: s.lib.complex_solver_hipmf_solve_updated_transpose(s.h, x, b, zv, mapped, tol, 0, None, None, conj, 0)
        many = lambda conj=1, tol=TOL, mapped=0, nrhs=2, ld=n: s.lib.complex_solver_hipmf_solve_updated_transpose_many(s.h, X, B, nrhs, ld, zv, mapped, tol, 0, None, None,
                                                                                                                    conj, 0)
        assert one() == ERROR_NEED_FACTORIZATION and many() == ERROR_NEED_FACTORIZATION
        assert one(conj=2) == ERROR_NEED_FACTORIZATION  # (the order: factorisation before the arguments)
        assert s.lib.complex_solver_hipmf_factorize(s.h, None, None, None, None, None, None, None, 0, 0, zv) == 0
        assert one() == 0 and many() == 0 and one(conj=0) == 0 and many(conj=0) == 0
        for bad in (2, -1):
            assert one(conj=bad) == ERROR_HIPMF_INVALID_VALUE and many(conj=bad) == ERROR_HIPMF_INVALID_VALUE
        assert one(tol=float("nan")) == ERROR_HIPMF_INVALID_VALUE and many(tol=float("inf")) == ERROR_HIPMF_INVALID_VALUE
        assert many(nrhs=0) == ERROR_HIPMF_INVALID_VALUE and many(ld=n - 1) == ERROR_HIPMF_INVALID_VALUE
        # the map check comes last: with mapped = 1 and no map installed, any other bad argument is what is refused -- the message of
        # the map check has not been written yet (no call before this line fails it)
        last = lambda h=s: h.lib.complex_solver_hipmf_last_error(h.h).decode()
        for conj in (1, 0):
            assert one(conj=conj, mapped=1, tol=float("nan")) == ERROR_HIPMF_INVALID_VALUE and "no triplet map" not in last()
            assert many(conj=conj, mapped=1, tol=float("inf")) == ERROR_HIPMF_INVALID_VALUE and "no triplet map" not in last()
            assert many(conj=conj, mapped=1, nrhs=0) == ERROR_HIPMF_INVALID_VALUE and "no triplet map" not in last()
            assert many(conj=conj, mapped=1, ld=n - 1) == ERROR_HIPMF_INVALID_VALUE and "no triplet map" not in last()
        assert one(conj=2, mapped=1) == ERROR_HIPMF_INVALID_VALUE and many(conj=2, mapped=1) == ERROR_HIPMF_INVALID_VALUE and "no triplet map" not in last()
        assert one(mapped=1) == ERROR_HIPMF_INVALID_VALUE and "no triplet map" in last()
        assert many(mapped=1) == ERROR_HIPMF_INVALID_VALUE and "no triplet map" in last()
        # the same order on a complex-symmetric handle, whose A^T form takes the plain core
        (ns, rps, cis, vs), kws = Z.matrix("symlower")
        sym = ZT(lib, ns, rps, cis, vs, **kws)
        try:
            xs, bs, zs = np.zeros(2 * ns), Z.interleave(Z.rhs_for(ns)), Z.interleave(vs)
            for conj in (1, 0):
                assert sym.lib.complex_solver_hipmf_solve_updated_transpose(sym.h, xs, bs, zs, 1, float("nan"), 0, None, None, conj, 0) == ERROR_HIPMF_INVALID_VALUE
                assert "no triplet map" not in last(sym)
            assert sym.lib.complex_solver_hipmf_solve_updated_transpose(sym.h, xs, bs, zs, 1, TOL, 0, None, None, 0, 0) == ERROR_HIPMF_INVALID_VALUE
            assert "no triplet map" in last(sym)
        finally:
            sym.close()
        raw = C.CDLL(s.lib._name)
        raw.complex_solver_hipmf_solve_updated_transpose.restype = C.c_int32
        raw.complex_solver_hipmf_solve_updated_transpose.argtypes = [C.c_void_p] * 4 + [C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
        h, xp, bp, vp = C.c_void_p(s.h), x.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), zv.ctypes.data_as(C.c_void_p)
        for args in ((None, xp, bp, vp), (h, None, bp, vp), (h, xp, None, vp), (h, xp, bp, None)):
            assert raw.complex_solver_hipmf_solve_updated_transpose(*args, 0, TOL, 0, None, None, 1, 0) == ERROR_NULL_POINTER
    finally:
        s.close()


def run_complex_host_mirror(lib):
    from russell_amd import sparse as S

    S._L().rh_set_hipmf_library((lib or os.path.join(ROOT, "russell_amd", "lib", "librussell_hipmf.so")).encode())
    try:
        n, rp, ci, vals = Z.shifted_grid(12, 10, unsym=True)
        rows = np.repeat(np.arange(n), np.diff(rp))
        mats = []
        for h in (1.0, 0.5):
            m = S.ComplexCooMatrix(n, n, ci.size)
            m.put_many(rows, ci, vals(h))
            mats.append(m)
        A1 = Z.full(n, rp, ci, vals(0.5))
        B = np.array([Z.rhs_for(n, 10), Z.rhs_for(n, 11)])
        solver = S.ComplexLinSolver()
        solver.actual.factorize(mats[0])
        for call in (lambda: solver.solve_updated(mats[1], B[0], conjugate=True), lambda: solver.solve_updated_many(mats[1], B, conjugate=True)):
            with pytest.raises(S.StrError, match="conjugate=True needs transpose=True"):
                call()
        for conjugate in (True, False):
            O1 = sp.csr_matrix(op(A1, conjugate))
            x, steps, relres = solver.solve_updated(mats[1], B[0], rel_tol=TOL, transpose=True, conjugate=conjugate)
            assert 1 < steps <= 30
            Z.check_accuracy(O1, x, B[0], relres)
            X, St, Rr = solver.solve_updated_many(mats[1], B, rel_tol=TOL, transpose=True, conjugate=conjugate)
            Z.check_accuracy(O1, X[0], B[0], float(Rr[0]))
            Z.check_accuracy(O1, X[1], B[1], float(Rr[1]))
    finally:
        S._L().rh_set_hipmf_library(os.path.join(ROOT, "russell_amd", "lib", "librussell_hipmf.so").encode())


# ---- the tests on the emulator ----

@pytest.fixture(scope="module")
def mats():
    return T.matrices()


def test_exports(emu_lib):
    """the new entry points exist, are declared and are bound (none of this holds on the parent commit)"""
    raw = C.CDLL(emu_lib)
    header = open(os.path.join(ROOT, "include", "russell_hipmf.h")).read()
    for name in REAL_SYMBOLS + COMPLEX_SYMBOLS:
        assert hasattr(raw, name), name
        assert "int32_t %s(" % name in header, name
        assert name in _capi.SYMBOLS, name
    host = open(os.path.join(ROOT, "include", "russell_host.h")).read()
    for name in ("rh_linsolver_solve_updated_transpose", "rh_linsolver_solve_updated_transpose_many", "rh_clinsolver_solve_updated_transpose",
                 "rh_clinsolver_solve_updated_transpose_many", "rh_clinsolver_solve_transpose_many"):
        assert "const char *%s(" % name in host, name


@pytest.mark.parametrize("name", ["mumps5", "bfwb62", "poisson", "chain257"])
def test_transposed_not_plain(emu_lib, mats, name):
    run_transposed_not_plain(emu_lib, name, *mats[name])


@pytest.mark.parametrize("name", ["mumps5", "bfwb62", "poisson", "chain257"])
def test_unchanged_values_take_one_step(emu_lib, mats, name):
    run_unchanged(emu_lib, *mats[name])


@pytest.mark.parametrize("name", ["poisson_lower", "saddle"])
def test_symmetric_handles_return_the_plain_bits(emu_lib, mats, name):
    run_symmetric_is_plain(emu_lib, *mats[name])


def test_edge_one_past_a_workgroup(emu_lib, mats):
    init, kw, values = mats["chain257"]
    run_edges(emu_lib, "chain257", mats["chain257"], T.redraw_rows(init, values))


def test_edge_one_past_4096(emu_lib, mats):
    init, kw, values = mats["chain4097"]
    run_edges(emu_lib, "chain4097", mats["chain4097"], T.redraw_rows(init, values))


def test_edge_long_row_of_the_transpose(emu_lib):
    case, v1 = arrow()
    A = sp.csr_matrix((case[2], case[0][2], case[0][1]))
    assert np.diff(A.T.tocsr().indptr).tolist()[:2] == [1025, 2] and abs(A - A.T).max() > 0  # (one long row of A^T, unsymmetric in value)
    run_edges(emu_lib, "arrow1025", case, v1)


@pytest.mark.parametrize("nrhs,pad", [(1, 0), (5, 3), (16, 0), (17, 1), (33, 2)])
def test_block_form(emu_lib, nrhs, pad):
    run_block(emu_lib, nrhs, pad)


def test_column_does_not_depend_on_its_position(emu_lib):
    run_position_independence(emu_lib)


def test_restart_four_columns_finish_in_different_cycles(emu_lib, monkeypatch):
    run_cycles(emu_lib, monkeypatch)


def test_not_converged_and_nan_per_column(emu_lib):
    run_not_converged_and_nan(emu_lib)


def test_mapped_values(emu_lib, mats):
    run_mapped(emu_lib, *mats["poisson"])


def test_status_codes(emu_lib):
    run_status_codes(emu_lib)


@pytest.mark.parametrize("name", ["poisson", "bfwb62"])
def test_no_side_effects(emu_lib, mats, name):
    run_no_side_effects(emu_lib, *mats[name])


@pytest.mark.parametrize("name", ["bfwb62", "poisson"])
def test_reproducible(emu_lib, mats, name):
    run_reproducible(emu_lib, *mats[name])


def test_device_entry_points(emu_lib, mats):
    run_device_entry(emu_lib, *mats["poisson"])


def test_perturbed_factor(emu_lib):
    run_perturbed(emu_lib)


def test_host_mirror(emu_lib):
    run_host_mirror(emu_lib)


@pytest.mark.parametrize("name", ["ref5", "zchain257", "grid", "symlower"])
def test_complex_forms(emu_lib, name):
    run_complex(emu_lib, name)


@pytest.mark.parametrize("name", ["random200", "symlower"])
def test_complex_reproducible(emu_lib, name):
    run_complex_reproducible(emu_lib, name)


@pytest.mark.parametrize("name", ["random200", "grid"])
def test_complex_plain_real_equivalent_factor(emu_lib, name):
    run_complex_reproducible(emu_lib, name, env={"HIPMF_COMPLEX_PAIRS": "0"})


def test_complex_no_side_effects(emu_lib):
    run_complex_no_side_effects(emu_lib)


def test_complex_status_codes(emu_lib):
    run_complex_status_codes(emu_lib)


def test_complex_host_mirror(emu_lib):
    run_complex_host_mirror(emu_lib)
