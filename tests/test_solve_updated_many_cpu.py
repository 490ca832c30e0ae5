"""Several right-hand sides with new matrix values on a kept factor (solver_hipmf_solve_updated_many / _device,
kernels_krylov_blocked.hpp) on the CPU emulator of the HIP kernels.  tests/test_solve_updated_many_gpu.py repeats the run_* cases on the
device (lib None = the product build).

Matrices, reference (fgmres_reference), own_relres and the accuracy rule are those of tests/test_solve_updated_cpu.py (imported as T; see
its docstring: nothing is a tuned number).  Per column: the accuracy rule with rel_tol = T.TOL, and steps <= the reference's steps for that
column + 1.  The rule is evaluated for all columns of a case at once: the recomputed residual runs over the stored entries of the matrix
(the same sums in np.longdouble as T.own_relres forms with the dense matrix, without its zeros), the forward error against ONE
np.linalg.solve with all columns, and cond_2 is computed by NumPy once per matrix."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import test_solve_updated_cpu as T
from russell_amd.backend import Hipmf
from test_transpose_solve_cpu import ERROR_HIPMF_INVALID_VALUE, ERROR_NEED_FACTORIZATION, ERROR_NULL_POINTER, mumps_5x5

TOL = T.TOL
NOT_CONVERGED = T.NOT_CONVERGED
KRYB_COLS = 16  # kernels_krylov_blocked.hpp

_cache = {}  # references and condition numbers, computed once per session (the GPU file shares them)


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def relres_columns(A_new, X, B):
    """per column (T.own_relres: recomputed |b - A x|_2 / |b|_2 in extended precision, its rounding bound, the bound for double)"""
    A = sp.csr_matrix(A_new)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    vl, out = A.data.astype(T.LD), []
    for x, b in zip(X, B):
        ax = np.zeros(b.size, T.LD)
        np.add.at(ax, rows, vl * x.astype(T.LD)[A.indices])
        bl = b.astype(T.LD)
        r, bnorm = bl - ax, np.sqrt(bl @ bl)
        scale = float(np.linalg.norm(np.bincount(rows, np.abs(A.data) * np.abs(x)[A.indices], b.size)) / float(bnorm))
        out.append((float(np.sqrt(r @ r) / bnorm), b.size * T.EPS_LD * scale, b.size * T.EPS * scale))
    return out


def check_columns(key, A_new, X, B, relres, skip=()):
    """the accuracy rule of T's docstring for every column (rows of X, B) but those of `skip` (zero right-hand sides)"""
    cols = [c for c in range(len(B)) if c not in skip]
    for c, (own, bound, bound_double) in zip(cols, relres_columns(A_new, X[cols], B[cols])):
        print("column %d: own relres %.3e, rounding bound of it %.3e, reported %.3e" % (c, own, bound, relres[c]))
        assert bound < TOL, (c, bound)
        assert own <= 2 * TOL, (c, own)
        assert relres[c] <= TOL and abs(relres[c] - own) <= bound + bound_double, (c, relres[c], own)
    cond = cached(("cond", key), lambda: float(np.linalg.cond(A_new)))
    XD = np.linalg.solve(A_new, B[cols].T).T
    for c, xd in zip(cols, XD):
        err = np.linalg.norm(X[c] - xd) / np.linalg.norm(xd)
        assert err <= cond * 2 * TOL, (c, err, cond)


def reference_columns(key, A_new, A_old, B, restart, max_steps):
    """[(steps, relres)] of T.fgmres_reference per column, each distinct column of a case computed once"""
    out = []
    for b in B:
        if not b.any():
            out.append((0, 0.0))
            continue
        out.append(cached(("ref", key, restart, max_steps, b.tobytes()[:64]), lambda: T.fgmres_reference(A_new, A_old, b, TOL, restart, max_steps)[1:]))
    return out


def eigvec(p, q, nx=56, ny=54):
    """eigenvector of the 5-point Laplacian on the nx x ny grid, x index fastest"""
    return np.outer(np.sin(np.pi * p * np.arange(1, nx + 1) / (nx + 1)), np.sin(np.pi * q * np.arange(1, ny + 1) / (ny + 1))).flatten(order="F")


def shift_columns(n, nrhs, grid=(56, 54)):
    cols = [T.rhs_for(n, 3), eigvec(1, 1, *grid), eigvec(3, 5, *grid) + eigvec(20, 11, *grid), np.zeros(n), T.rhs_for(n, 21)]
    cols += [T.rhs_for(n, 100 + c) for c in range(5, nrhs)]
    return np.array(cols[:nrhs])


def padded(B, ld):
    """the columns in rows of length ld, the padding filled with a sentinel"""
    out = np.full((B.shape[0], ld), -7.5)
    out[:, :B.shape[1]] = B
    return out


def block_counters(s, steps, nrhs, n, m=30):
    """the counters of the block form after a call that returned `steps`"""
    assert s.counter("updated_blocks") == (nrhs + KRYB_COLS - 1) // KRYB_COLS
    assert s.counter("updated_column_steps") == int(steps.sum())
    assert s.counter("updated_steps") == sum(int(steps[j:j + KRYB_COLS].max()) for j in range(0, nrhs, KRYB_COLS))
    assert s.counter("updated_block_basis_bytes") == (2 * m + 1) * n * 8 * min(nrhs, KRYB_COLS)


def run_single_column(lib, init, kw, values):
    """nrhs = 1 is the single form: its bits, on the host and on the device"""
    n = init[0]
    v1 = T.redraw_rows(init, values)
    b = T.rhs_for(n, 9)
    s = T.handle(lib, init, kw, values)
    ptrs = []
    try:
        x1, st1, r1, c1 = s.solve_updated(b, v1, rel_tol=TOL)
        xm, stm, rm, cm = s.solve_updated_many(b[None, :], v1, rel_tol=TOL)
        assert (int(stm[0]), float(rm[0]), cm) == (st1, r1, c1) and np.array_equal(xm[0].view(np.uint64), x1.view(np.uint64))
        assert s.counter("updated_blocks") == 0 and s.counter("updated_column_steps") == st1
        d_x, d_b, d_v = s.dev_alloc(8 * n), s.dev_alloc(8 * n), s.dev_alloc(8 * v1.size)
        ptrs += [d_x, d_b, d_v]
        s.h2d(d_b, b)
        s.h2d(d_v, v1)
        std, rd, cd = s.solve_updated_many_device(d_x, d_b, 1, d_v, rel_tol=TOL)
        assert (int(std[0]), float(rd[0]), cd) == (st1, r1, c1)
        xd = np.zeros(n)
        s.d2h(xd, d_x)
        assert np.array_equal(xd.view(np.uint64), x1.view(np.uint64)) and s.counter("updated_blocks") == 0
    finally:
        for p in ptrs:
            s.dev_free(p)
        s.close()


def run_shift_many(lib, nrhs, ld=None):
    """columns that converge at different steps: A_old = L + I, A_new = L + 2 I on the 56 x 54 grid"""
    init, kw, vals = T.shifted_poisson()
    n = init[0]
    v0, v1 = vals(1.0), vals(2.0)
    A0, A1 = cached("A0_shift", lambda: T.dense(init, kw, v0)), cached("A1_shift2", lambda: T.dense(init, kw, v1))
    B = shift_columns(n, nrhs)
    ref = reference_columns("shift2", A1, A0, B, 30, 120)
    ref_steps = [r[0] for r in ref]
    print("reference steps", ref_steps)
    assert ref_steps[:5] == [12, 1, 2, 0, 12]  # (the condition that makes the test meaningful)
    assert len(set(ref_steps)) >= 3 and all(r[1] <= TOL for r in ref)
    s = T.handle(lib, init, kw, v0)
    try:
        assert s.counter("symmetric_ldlt") == 1
        ld = n if ld is None else ld
        Bp = padded(B, ld)
        x, steps, relres, status = s.solve_updated_many(Bp, v1, rel_tol=TOL, ld=ld)
        print("device steps", steps.tolist())
        assert status == 0
        assert all(steps[c] <= ref_steps[c] + 1 for c in range(nrhs)), (steps, ref_steps)
        assert not x[3, :n].any() and steps[3] == 0 and relres[3] == 0.0
        assert np.array_equal(x[:, n:], Bp[:, n:])  # (the padding is not written)
        block_counters(s, steps, nrhs, n)
        check_columns("shift2", A1, x[:, :n], B, relres, skip=(3,))
    finally:
        s.close()


def run_cycles_many(lib, ratio, restart, max_steps, monkeypatch):
    """columns that finish in different cycles"""
    init, kw, vals = T.shifted_poisson()
    n = init[0]
    v0, v1 = vals(1.0), vals(ratio)
    monkeypatch.setenv("HIPMF_UPDATED_RESTART", str(restart))
    A0, A1 = cached("A0_shift", lambda: T.dense(init, kw, v0)), cached("A1_shift%g" % ratio, lambda: T.dense(init, kw, v1))
    B = shift_columns(n, 3)
    ref = reference_columns("shift%g" % ratio, A1, A0, B, restart, max_steps)
    ref_steps = [r[0] for r in ref]
    print("reference steps", ref_steps)
    assert ref_steps[0] > restart and ref_steps[1:] == [1, 2] and all(r[1] <= TOL for r in ref)
    s = T.handle(lib, init, kw, v0)
    try:
        x, steps, relres, status = s.solve_updated_many(B, v1, rel_tol=TOL, max_steps=max_steps)
        print("device steps", steps.tolist(), "cycles", s.counter("updated_cycles"))
        assert status == 0
        assert all(steps[c] <= ref_steps[c] + 1 for c in range(3)), (steps, ref_steps)
        assert s.counter("updated_cycles") >= (int(steps.max()) + restart - 1) // restart
        assert s.counter("updated_block_basis_bytes") == (2 * restart + 1) * n * 8 * 3
        check_columns("shift%g" % ratio, A1, x, B, relres)
        return steps, ref_steps
    finally:
        s.close()


def run_not_converged_many(lib):
    init, kw, vals = T.shifted_poisson()
    n = init[0]
    v0, v1 = vals(1.0), vals(100.0)
    A1 = cached("A1_shift100", lambda: T.dense(init, kw, v1))
    B = np.array([T.rhs_for(n, 3), eigvec(1, 1), np.zeros(n)])
    s = T.handle(lib, init, kw, v0)
    try:
        x, steps, relres, status = s.solve_updated_many(B, v1, rel_tol=TOL, max_steps=2)
        assert status == NOT_CONVERGED and steps.tolist() == [2, 1, 0], (status, steps)
        assert TOL < relres[0] < 1.0 and relres[1] <= TOL and relres[2] == 0.0 and not x[2].any()
        own, bound, bound_double = relres_columns(A1, x[:1], B[:1])[0]
        print("reported %.6e, own %.6e, rounding bounds %.3e (own) %.3e (double)" % (relres[0], own, bound, bound_double))
        assert bound < TOL and abs(relres[0] - own) <= bound + bound_double
    finally:
        s.close()


def rank_columns(n):
    rows = np.random.default_rng(7).choice(n, size=min(3, n), replace=False)  # (the rows T.redraw_rows redraws)
    return np.array([T.rhs_for(n, 2)] + [np.eye(n)[i] for i in rows] + [T.rhs_for(n, 5)])


def run_rank_change_many(lib, name, init, kw, values):
    v1 = T.redraw_rows(init, values)
    A0, A1 = T.dense(init, kw, values), T.dense(init, kw, v1)
    B = rank_columns(init[0])
    ref = reference_columns("rank_" + name, A1, A0, B, 30, 120)
    ref_steps = [r[0] for r in ref]
    print("reference steps", ref_steps)
    assert all(st <= 5 for st in ref_steps) and all(r[1] <= TOL for r in ref)
    s = T.handle(lib, init, kw, values)
    try:
        x, steps, relres, status = s.solve_updated_many(B, v1, rel_tol=TOL)
        print("device steps", steps.tolist())
        assert status == 0 and all(steps[c] <= ref_steps[c] + 1 for c in range(len(B))), (steps, ref_steps)
        check_columns("rank_" + name, A1, x, B, relres)
    finally:
        s.close()


def run_mapped_many(lib, init, kw, values):
    """the shuffled two-part inputs of T.run_mapped: mapped = 1 gives the bits of mapped = 0 on the summed values"""
    n, rp, ci = init
    nnz = values.size
    rng = np.random.default_rng(11)
    v1 = T.redraw_rows(init, values)
    parts = np.concatenate([v1 * rng.uniform(0.2, 0.8, nnz), np.zeros(nnz)])
    parts[nnz:] = v1 - parts[:nnz]
    order = rng.permutation(2 * nnz)
    where = np.argsort(order)
    seg_ptr = 2 * np.arange(nnz + 1)
    seg_idx = np.empty(2 * nnz, np.int64)
    seg_idx[0::2], seg_idx[1::2] = where[:nnz], where[nnz:]
    inputs = parts[order]
    summed = (0.0 + inputs[seg_idx[0::2]]) + inputs[seg_idx[1::2]]
    B = np.array([T.rhs_for(n, 4), T.rhs_for(n, 14), T.rhs_for(n, 24)])
    s = T.handle(lib, init, kw, values)
    try:
        with pytest.raises(Exception) as e:
            s.solve_updated_many(B, inputs, mapped=True, rel_tol=TOL)
        assert e.value.code == ERROR_HIPMF_INVALID_VALUE  # no map yet
        assert s.set_value_map(seg_ptr, seg_idx) == 0
        xm, st_m, rel_m, c_m = s.solve_updated_many(B, inputs, mapped=True, rel_tol=TOL)
        x0, st_0, rel_0, c_0 = s.solve_updated_many(B, summed, mapped=False, rel_tol=TOL)
        assert c_m == c_0 == 0 and np.array_equal(st_m, st_0) and np.array_equal(rel_m, rel_0)
        assert np.array_equal(xm.view(np.uint64), x0.view(np.uint64))
        assert all(r <= TOL for r in rel_m)
    finally:
        s.close()


def run_no_side_effects_many(lib, init, kw, values):
    """the snapshot of T.run_no_side_effects, a solve_many of 5 columns and a single solve_updated: the same bits before and after"""
    n = init[0]
    v1 = T.redraw_rows(init, values)
    B = np.array([T.rhs_for(n, 30 + c) for c in range(5)])
    b = B[0]
    s = T.handle(lib, init, kw, values, nstep=-1)
    try:
        def snapshot():
            x = s.solve(b)
            st = s.stats()
            xu, su, ru, cu = s.solve_updated(b, v1, rel_tol=TOL)
            return (x.view(np.uint64).copy(), s.mat_vec_mul(b).view(np.uint64).copy(), s.num_perturbed, s.counter("krylov_iterations"), st["refinement_steps"],
                    st["fused_fallbacks"], s.solve_many(B).view(np.uint64).copy(), xu.view(np.uint64).copy(), su, ru, cu, s.counter("updated_basis_bytes"))
        before = snapshot()
        st = s.stats()
        ref_steps, kry = st["refinement_steps"], s.counter("krylov_iterations")
        x, steps, relres, status = s.solve_updated_many(B, v1, rel_tol=TOL)
        assert status == 0 and all(r <= TOL for r in relres)
        assert s.stats()["refinement_steps"] == ref_steps and s.counter("krylov_iterations") == kry
        after = snapshot()
        for a, c in zip(before, after):
            assert np.array_equal(a, c)
    finally:
        s.close()


def run_reproducible_many(lib, init, kw, values):
    n = init[0]
    v1 = T.redraw_rows(init, values)
    B = np.array([T.rhs_for(n, 40 + c) for c in range(17)])
    s = T.handle(lib, init, kw, values)
    try:
        x1, st1, r1, c1 = s.solve_updated_many(B, v1, rel_tol=TOL)
        x2, st2, r2, c2 = s.solve_updated_many(B, v1, rel_tol=TOL)
        assert c1 == c2 == 0 and np.array_equal(st1, st2) and np.array_equal(r1.view(np.uint64), r2.view(np.uint64))
        assert np.array_equal(x1.view(np.uint64), x2.view(np.uint64))
        assert s.counter("updated_blocks") == 2
    finally:
        s.close()


def run_device_entry_many(lib, init, kw, values):
    """the _device entry point (leading dimension n + 1) gives the bits of the host entry point"""
    n, nrhs, ld = init[0], 17, init[0] + 1
    v1 = T.redraw_rows(init, values)
    B = np.array([T.rhs_for(n, 60 + c) for c in range(nrhs)])
    s = T.handle(lib, init, kw, values)
    ptrs = []
    try:
        xh, steps, relres, status = s.solve_updated_many(B, v1, rel_tol=TOL)
        assert status == 0
        d_x, d_b, d_v = s.dev_alloc(8 * ld * nrhs), s.dev_alloc(8 * ld * nrhs), s.dev_alloc(8 * v1.size)
        ptrs += [d_x, d_b, d_v]
        s.h2d(d_b, padded(B, ld))
        s.h2d(d_x, np.full((nrhs, ld), 3.25))
        s.h2d(d_v, v1)
        st_d, rel_d, c_d = s.solve_updated_many_device(d_x, d_b, nrhs, d_v, rel_tol=TOL, ld=ld)
        assert c_d == status and np.array_equal(st_d, steps) and np.array_equal(rel_d.view(np.uint64), relres.view(np.uint64))
        xd = np.zeros((nrhs, ld))
        s.d2h(xd, d_x)
        assert np.array_equal(xd[:, :n].view(np.uint64), xh.view(np.uint64))
        assert np.all(xd[:, n:] == 3.25)  # (entries ndim ... ld-1 are not written)
    finally:
        for p in ptrs:
            s.dev_free(p)
        s.close()


def run_perturbed_many(lib):
    A = T._pm1(400, 4, np.random.default_rng(3))
    n, rp, ci, v = A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
    s = T._new(lib)
    try:
        assert s.initialize(n, rp, ci, values=v) == 0 and s.factorize(v) == 0
        assert s.num_perturbed > 0
        B = np.array([T.rhs_for(n, 8), T.rhs_for(n, 18), T.rhs_for(n, 28)])
        x, steps, relres, status = s.solve_updated_many(B, v, rel_tol=TOL)
        print("%d replaced pivots: steps %s, relres %s" % (s.num_perturbed, steps.tolist(), relres.tolist()))
        assert status == 0 and all(r <= TOL for r in relres) and all(st >= 1 for st in steps)
        for xc, b in zip(x, B):
            assert np.linalg.norm(b - A @ xc) <= 2 * TOL * np.linalg.norm(b)
    finally:
        s.close()


def run_status_codes(lib):
    (n, rp, ci, v), _ = mumps_5x5()
    v = np.array(v, float)
    s = T._new(lib)
    try:
        x, b = np.zeros((2, n)), np.ones((2, n))
        call = s.lib.solver_hipmf_solve_updated_many
        assert call(s.h, x, b, 2, n, v, 0, TOL, 0, None, None, 0) == T.ERROR_NEED_INITIALIZATION
        assert s.initialize(n, rp, ci) == 0
        assert call(s.h, x, b, 2, n, v, 0, TOL, 0, None, None, 0) == ERROR_NEED_FACTORIZATION
        assert s.lib.solver_hipmf_solve_updated_many_device(s.h, C.c_void_p(8), C.c_void_p(8), 2, n, C.c_void_p(8), 0, TOL, 0, None, None) == ERROR_NEED_FACTORIZATION
        assert s.factorize(v) == 0
        assert call(s.h, x, b, 2, n, v, 0, TOL, 0, None, None, 0) == 0  # (steps and relres may be NULL)
        assert np.array_equal(x[0], x[1]) and np.linalg.norm(T.dense((n, rp, ci), {}, v) @ x[0] - b[0]) <= 2 * TOL * np.linalg.norm(b[0])
        assert call(s.h, x, b, 0, n, v, 0, TOL, 0, None, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert call(s.h, x, b, 2, n - 1, v, 0, TOL, 0, None, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert call(s.h, x, b, 2, n, v, 0, float("inf"), 0, None, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert call(s.h, x, b, 2, n, v, 0, float("nan"), 0, None, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert call(s.h, x, b, 2, n, v, 1, TOL, 0, None, None, 0) == ERROR_HIPMF_INVALID_VALUE  # mapped without a map
        # a non-finite right-hand side: x_c = 0 and relres NaN for that column alone
        bn = np.array([np.ones(n), np.ones(n)])
        bn[0, 2] = np.inf
        xn, steps, relres, status = s.solve_updated_many(bn, v, rel_tol=TOL)
        assert status == NOT_CONVERGED and not xn[0].any() and np.isnan(relres[0]) and steps[0] == 0
        assert relres[1] <= TOL and np.array_equal(xn[1], x[1])
        raw = C.CDLL(s.lib._name)  # (untyped bindings: NULL pointers pass)
        raw.solver_hipmf_solve_updated_many.restype = C.c_int32
        raw.solver_hipmf_solve_updated_many.argtypes = [C.c_void_p] * 3 + [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
        h, xp, bp, vp = C.c_void_p(s.h), x.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)
        for hh, xx, bb, vv in ((None, xp, bp, vp), (h, None, bp, vp), (h, xp, None, vp), (h, xp, bp, None)):
            assert raw.solver_hipmf_solve_updated_many(hh, xx, bb, 2, n, vv, 0, TOL, 0, None, None, 0) == ERROR_NULL_POINTER
    finally:
        s.close()


# ---- the tests on the emulator ----

@pytest.fixture(scope="module")
def mats():
    return T.matrices()


def test_exports(emu_lib):
    """the two entry points and the three counters exist (they do not on the parent commit)"""
    raw = C.CDLL(emu_lib)
    for name in ("solver_hipmf_solve_updated_many", "solver_hipmf_solve_updated_many_device"):
        assert hasattr(raw, name), name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "russell_hipmf.h")).read()
    for name, num in (("UPDATED_BLOCKS", 34), ("UPDATED_COLUMN_STEPS", 35), ("UPDATED_BLOCK_BASIS_BYTES", 36)):
        assert "#define HIPMF_COUNTER_%s %d" % (name, num) in header
        assert Hipmf.COUNTERS[name.lower()] == num
    (n, rp, ci, v), _ = mumps_5x5()
    s = T.handle(emu_lib, (n, rp, ci), dict(values=v), v)
    try:
        assert [s.counter(k) for k in ("updated_blocks", "updated_column_steps", "updated_block_basis_bytes")] == [0, 0, 0]
    finally:
        s.close()


@pytest.mark.parametrize("name", ["poisson", "poisson_lower"])
def test_one_column_is_the_single_form(emu_lib, mats, name):
    run_single_column(emu_lib, *mats[name])


@pytest.mark.parametrize("nrhs,pad", [(5, 0), (16, 0), (17, 0), (33, 0), (5, 3)])
def test_columns_converge_at_different_steps(emu_lib, nrhs, pad):
    run_shift_many(emu_lib, nrhs, ld=3024 + pad if pad else None)


def test_columns_finish_in_different_cycles(emu_lib, monkeypatch):
    steps, ref_steps = run_cycles_many(emu_lib, 100.0, 4, 400, monkeypatch)
    assert ref_steps[0] >= 20 and steps[0] > 8  # tens of steps in many cycles


@pytest.mark.parametrize("restart", [T.PASSV, T.PASSV - 1])
def test_basis_count_edges(emu_lib, monkeypatch, restart):
    steps, ref_steps = run_cycles_many(emu_lib, 2.0, restart, 200, monkeypatch)
    assert ref_steps[0] == 13 and steps[0] > restart


def test_not_converged_per_column(emu_lib):
    run_not_converged_many(emu_lib)


@pytest.mark.parametrize("name", T.GENERAL)
def test_rank_three_change(emu_lib, mats, name):
    run_rank_change_many(emu_lib, name, *mats[name])


@pytest.mark.parametrize("name", ["poisson", "poisson_lower", "saddle"])
def test_mapped_values(emu_lib, mats, name):
    run_mapped_many(emu_lib, *mats[name])


@pytest.mark.parametrize("name", ["poisson", "poisson_lower", "saddle"])
def test_no_side_effects(emu_lib, mats, name):
    run_no_side_effects_many(emu_lib, *mats[name])


@pytest.mark.parametrize("name", ["bfwb62", "poisson_lower"])
def test_reproducible(emu_lib, mats, name):
    run_reproducible_many(emu_lib, *mats[name])


@pytest.mark.parametrize("name", ["poisson", "poisson_lower"])
def test_device_entry_point(emu_lib, mats, name):
    run_device_entry_many(emu_lib, *mats[name])


def test_perturbed_factor(emu_lib):
    run_perturbed_many(emu_lib)


def test_status_codes(emu_lib):
    run_status_codes(emu_lib)


def test_host_mirror(emu_lib):
    """LinSolver.solve_updated_many of russell_amd.sparse on bfwb62: the accuracy rule per column, the error string of status 2"""
    from russell_amd import sparse as S

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    S._L().rh_set_hipmf_library(emu_lib.encode())
    try:
        A = T._golden("bfwb62").tocoo()
        n = A.shape[0]
        v1 = A.data * (1.0 + 0.3 * np.random.default_rng(5).uniform(-1, 1, A.nnz))
        mat0 = S.CooMatrix.from_arrays(n, n, A.row, A.col, A.data.astype(float))
        mat1 = S.CooMatrix.from_arrays(n, n, A.row, A.col, v1)
        A1 = sp.csr_matrix((v1, (A.row, A.col)), shape=(n, n)).toarray()
        B = np.array([T.rhs_for(n, 70), T.rhs_for(n, 71), T.rhs_for(n, 72)])
        solver = S.LinSolver(S.Genie.Hipmf)
        with pytest.raises(S.StrError, match="factorize must be called"):
            solver.solve_updated_many(mat1, B)
        solver.actual.factorize(mat0)
        x, steps, relres = solver.solve_updated_many(mat1, B, rel_tol=TOL)
        assert x.shape == B.shape and all(1 < st <= 30 for st in steps)
        check_columns("host_bfwb62", A1, x, B, relres)
        with pytest.raises(S.StrError, match=r"Error\(2\): the iteration on the kept factorization did not converge"):
            solver.solve_updated_many(mat1, B, rel_tol=TOL, max_steps=1)
        with pytest.raises(S.StrError, match="right-hand side vector is incorrect"):
            solver.solve_updated_many(mat1, B[:, :-1])
    finally:
        S._L().rh_set_hipmf_library(os.path.join(root, "russell_amd", "lib", "librussell_hipmf.so").encode())
