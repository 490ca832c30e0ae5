"""Solve several right-hand sides with new complex values on a kept factor (complex_solver_hipmf_solve_updated_many / _many_device,
kernels_krylov_complex_blocked.hpp) on the CPU emulator of the HIP kernels.  tests/test_solve_updated_complex_many_gpu.py repeats the
run_* cases on the device (lib None = the product build).

The references, the tolerance and the accuracy rule are those of tests/test_solve_updated_complex_cpu.py (its docstring), applied PER
COLUMN: fgmres_reference in complex arithmetic and on the real-equivalent system gives each column's step counts, own_relres /
check_accuracy judge each column's x, with cond_2 and the dense solutions computed once per matrix.  Arrays of right-hand sides have the
shape (nrhs, ld), complex128: the column-major ld x nrhs interleaved layout of the C-ABI."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import test_solve_updated_complex_cpu as T
from test_complex_many_rhs_cpu import SENTINEL, ZM, bits, zpadded, zview
from test_solve_updated_many_cpu import eigvec

TOL = T.TOL
NOT_CONVERGED = T.NOT_CONVERGED
KRYB_COLS = 16  # kernels_krylov_blocked.hpp
GRID = (24, 20)


def shift_columns(n, nrhs):
    """a random column, one eigenvector of the grid's Laplacian (of every K(h): one step), two eigenvectors (two steps), zeros, random ones"""
    cols = [T.rhs_for(n, 3), (1 + 2j) * eigvec(1, 1, *GRID), (0.5 - 1j) * eigvec(3, 5, *GRID) + (2 + 0.3j) * eigvec(20, 11, *GRID), np.zeros(n, complex),
            T.rhs_for(n, 21)]
    cols += [T.rhs_for(n, 100 + c) for c in range(5, nrhs)]
    return np.array(cols[:nrhs])


RANDOM = lambda c: c not in (1, 2, 3)  # the columns of shift_columns that are random vectors


@functools.lru_cache(maxsize=None)
def grid_matrices(h1):
    """K(1) -> K(h1) on the 24 x 20 grid: (structure, v0, v1, dense K(1), dense K(h1), cond_2 of K(h1)), computed once"""
    n, rp, ci, vals = T.shifted_grid(*GRID)
    v0, v1 = vals(1.0), vals(h1)
    A0, A1 = T.full(n, rp, ci, v0).toarray(), T.full(n, rp, ci, v1).toarray()
    return (n, rp, ci), v0, v1, A0, A1, float(np.linalg.cond(A1))


@functools.lru_cache(maxsize=None)
def column_reference(h1, c, restart=30, max_steps=120, real_too=True):
    """(steps of the complex reference, steps of the real-equivalent one or None) for column c of shift_columns, computed once"""
    (n, _, _), _, _, A0, A1, _ = grid_matrices(h1)
    b = shift_columns(n, c + 1)[c]
    _, zsteps, zrel = T.fgmres_reference(A1, A0, b, TOL, restart, max_steps)
    assert zrel <= TOL, (c, zrel)
    rsteps = None
    if real_too:
        _, rsteps, rrel = T.fgmres_reference(T.real_equivalent(A1), T.real_equivalent(A0), T.interleave(b), TOL, restart, max_steps)
        assert rrel <= TOL, (c, rrel)
    return zsteps, rsteps


def check_columns(A1, X, B, relres, cond, skip=()):
    """the accuracy rule per column; the dense solutions of all columns at once"""
    n = B.shape[1]
    XD = np.linalg.solve(A1, B.T).T
    for c in range(B.shape[0]):
        if c not in skip:
            T.check_accuracy(A1, X[c, :n], B[c], float(relres[c]), cond, XD[c])


def block_counters(s, steps, nrhs, n, m=30):
    assert s.counter("updated_complex_arithmetic") == 1
    assert s.counter("updated_blocks") == (nrhs + KRYB_COLS - 1) // KRYB_COLS
    assert s.counter("updated_column_steps") == int(steps.sum())
    assert s.counter("updated_steps") == sum(int(steps[j:j + KRYB_COLS].max()) for j in range(0, nrhs, KRYB_COLS))
    assert s.counter("updated_block_basis_bytes") == (2 * m + 1) * min(nrhs, KRYB_COLS) * 2 * n * 8


# ---- the run functions (lib: the emulator's path, or None for the product build) ----

def run_shift_many(lib, h1, nrhs=16, pad=0):
    """complex arithmetic per column, columns that converge at different steps, a zero column, the counters of the block form"""
    (n, rp, ci), v0, v1, A0, A1, cond = grid_matrices(h1)
    B = shift_columns(n, nrhs)
    refs = [column_reference(h1, c) if c != 3 else (0, 0) for c in range(nrhs)]
    print("reference steps (complex, real-equivalent):", refs)
    for c in range(nrhs):
        if RANDOM(c):
            assert refs[c][1] >= refs[c][0] + 3, (c, refs[c])  # the premise: these inputs tell the two iterations apart
    s = ZM(lib, n, rp, ci, v0)
    try:
        X, steps, relres, status = s.solve_updated_many(zpadded(B, n + pad), v1, rel_tol=TOL, ld=n + pad)
        print("device: steps %s, %d cycle(s)" % (steps.tolist(), s.counter("updated_cycles")))
        assert status == 0
        assert np.array_equal(bits(X[:, n:]), bits(np.full((nrhs, pad), SENTINEL, np.complex128)))
        for c in range(nrhs):
            if c == 3:
                continue
            assert steps[c] <= refs[c][0] + 1, (c, steps[c], refs[c])
            if RANDOM(c):
                assert steps[c] <= refs[c][1] - 2, (c, steps[c], refs[c])
        assert steps[1] < steps[0] and (nrhs < 3 or steps[2] < steps[0])
        if nrhs > 3:
            assert steps[3] == 0 and relres[3] == 0.0 and not X[3, :n].any()
        block_counters(s, steps, nrhs, n)
        check_columns(A1, X, B, relres, cond, skip=(3,))
    finally:
        s.close()


@functools.lru_cache(maxsize=None)
def chain_case(name):
    """three rows of T.matrix(name) redrawn, three right-hand sides: (case, v1, B, complex reference steps per column, cond_2, dense A_new)"""
    case, kw, v1, _, _, cond, _ = T.rank_case(name)  # (cond_2 of A_new: computed once, shared with test_solve_updated_complex_cpu)
    n, rp, ci, v0 = case
    A0, A1 = T.full(n, rp, ci, v0).toarray(), T.full(n, rp, ci, v1).toarray()
    B = np.array([T.rhs_for(n, seed) for seed in (2, 61, 62)])
    zsteps = []
    for b in B:
        _, st, rel = T.fgmres_reference(A1, A0, b, TOL, 30, 120)
        assert rel <= TOL
        zsteps.append(st)
    return case, v1, B, zsteps, cond, A1


def run_tile_edges(lib, name):
    case, v1, B, zsteps, cond, A1 = chain_case(name)
    n = case[0]
    s = ZM(lib, *case)
    try:
        X, steps, relres, status = s.solve_updated_many(B, v1, rel_tol=TOL)
        print("device: steps %s, reference %s" % (steps.tolist(), zsteps))
        assert status == 0 and all(steps[c] <= zsteps[c] + 1 for c in range(3))
        block_counters(s, steps, 3, n)
        check_columns(A1, X, B, relres, cond)
    finally:
        s.close()


def run_basis_edges(lib, monkeypatch, restart, h1, max_steps, eigen):
    """short restart lengths: several cycles; eigen: an eigenvector column and a two-eigenvector column among the random ones, so that
    the columns finish in different cycles"""
    monkeypatch.setenv("HIPMF_UPDATED_RESTART", str(restart))
    (n, rp, ci), v0, v1, A0, A1, cond = grid_matrices(h1)
    cols = (0, 1, 2, 4) if eigen else (0, 4, 5, 6)
    B = shift_columns(n, 7)[list(cols)]
    zsteps = [column_reference(h1, c, restart, max_steps, False)[0] for c in cols]
    s = ZM(lib, n, rp, ci, v0)
    try:
        X, steps, relres, status = s.solve_updated_many(B, v1, rel_tol=TOL, max_steps=max_steps)
        cycles = s.counter("updated_cycles")
        print("device: steps %s in %d cycles, reference %s" % (steps.tolist(), cycles, zsteps))
        assert status == 0 and all(steps[c] <= zsteps[c] + 1 for c in range(4))
        assert steps.max() > restart and cycles >= 2
        if eigen:
            assert steps[1] == 1 and len(set(((steps + restart - 1) // restart).tolist())) > 1  # the columns finish in different cycles
        block_counters(s, steps, 4, n, m=restart)
        check_columns(A1, X, B, relres, cond)
    finally:
        s.close()


def run_single_is_single(lib):
    """nrhs == 1 is the single complex form, bit for bit, on the host and on the device"""
    (n, rp, ci), v0, v1, _, _, _ = grid_matrices(0.5)
    b = T.rhs_for(n, 3)
    s = ZM(lib, n, rp, ci, v0)
    ptrs = []
    try:
        xs, st, rel, code = s.solve_updated(b, v1, rel_tol=TOL)
        X, steps, relres, status = s.solve_updated_many(b[None, :], v1, rel_tol=TOL)
        assert (int(steps[0]), float(relres[0]), status) == (st, rel, code) and st > 1
        assert np.array_equal(bits(X[0]), bits(T.interleave(xs)))
        assert s.counter("updated_blocks") == 0 and s.counter("updated_column_steps") == st
        Xd, steps_d, relres_d, status_d = s.solve_updated_many_device(b[None, :], v1, rel_tol=TOL)
        assert (int(steps_d[0]), float(relres_d[0]), status_d) == (st, rel, code) and np.array_equal(bits(Xd), bits(X))
        assert s.counter("updated_blocks") == 0
        d_x, d_b, d_v = s.dev_alloc(16 * n), s.dev_alloc(16 * n), s.dev_alloc(16 * v1.size)
        ptrs += [d_x, d_b, d_v]
        s.h2d(d_b, T.interleave(b))
        s.h2d(d_v, T.interleave(v1))
        assert s.solve_updated_device(d_x, d_b, d_v, rel_tol=TOL) == (st, rel, code)
        xd = np.zeros(2 * n)
        s.d2h(xd, d_x)
        assert np.array_equal(bits(xd), bits(Xd[0]))
    finally:
        for p in ptrs:
            s.dev_free(p)
        s.close()


def run_not_converged_many(lib):
    """max_steps = 3 on h -> h / 10: an ordinary column (not converged, the best iterate), a zero column, a column with a NaN entry, an
    eigenvector column (one step, full accuracy: nothing leaked across the columns)"""
    (n, rp, ci), v0, v1, A0, A1, cond = grid_matrices(0.1)
    assert column_reference(0.1, 0)[0] > 3
    bad = T.rhs_for(n, 21)
    bad[n // 2] = complex(1.0, np.nan)
    B = np.array([T.rhs_for(n, 3), np.zeros(n, complex), bad, (1 + 2j) * eigvec(1, 1, *GRID)])
    s = ZM(lib, n, rp, ci, v0)
    try:
        X, steps, relres, status = s.solve_updated_many(B, v1, rel_tol=TOL, max_steps=3)
        print("steps %s relres %s" % (steps.tolist(), relres.tolist()))
        assert status == NOT_CONVERGED
        assert steps[0] == 3 and TOL < relres[0] < 1.0
        own, bound, bound_double = T.own_relres(A1, X[0], B[0])
        print("reported %.6e, own %.6e, rounding bounds %.3e (own) %.3e (double)" % (relres[0], own, bound, bound_double))
        assert bound < TOL and abs(relres[0] - own) <= bound + bound_double
        assert steps[1] == 0 and relres[1] == 0.0 and not X[1].any()
        assert steps[2] == 0 and np.isnan(relres[2]) and not X[2].any()
        assert steps[3] == 1
        T.check_accuracy(A1, X[3], B[3], float(relres[3]), cond, np.linalg.solve(A1, B[3]))
        assert np.all(np.isfinite(X.view(np.float64)))
    finally:
        s.close()


def triplet_inputs(case, v1, seed=11):
    """every CSR entry as the sum of two triplets in a shuffled order, as T.run_mapped builds them: (seg_ptr, seg_idx, inputs, summed)"""
    nnz = case[3].size
    rng = np.random.default_rng(seed)
    parts = np.concatenate([v1 * rng.uniform(0.2, 0.8, nnz), np.zeros(nnz, complex)])
    parts[nnz:] = v1 - parts[:nnz]
    order = rng.permutation(2 * nnz)
    where = np.argsort(order)
    seg_ptr = 2 * np.arange(nnz + 1)
    seg_idx = np.empty(2 * nnz, np.int64)
    seg_idx[0::2], seg_idx[1::2] = where[:nnz], where[nnz:]
    inputs = parts[order]
    return seg_ptr, seg_idx, inputs, (0.0 + inputs[seg_idx[0::2]]) + inputs[seg_idx[1::2]]


@functools.lru_cache(maxsize=None)
def kind_case(name):
    """(case, keywords, v1 with three rows redrawn, cond_2 of the full A_new), computed once"""
    case, kw = T.matrix(name)
    n, rp, ci, _ = case
    v1 = T.redraw_rows(case)
    return case, kw, v1, float(np.linalg.cond(T.full(n, rp, ci, v1, kw.get("lower", False)).toarray()))


def run_handle_kind(lib, kind):
    """five columns on the other kinds of handle"""
    name, env, mapped = dict(symlower=("symlower", None, False), weak300=("weak300", None, False), mapped=("random200", None, True),
                             pairs0=("random200", {"HIPMF_COMPLEX_PAIRS": "0"}, False))[kind]
    case, kw, v1, cond = kind_case(name)
    n, rp, ci, v0 = case
    B = np.array([T.rhs_for(n, 80 + c) for c in range(5)])
    s = ZM(lib, *case, env=env, **kw)
    try:
        values = v1
        if mapped:
            seg_ptr, seg_idx, values, summed = triplet_inputs(case, v1)
            assert s.set_value_map(seg_ptr, seg_idx) == 0
            A1 = T.full(n, rp, ci, summed, kw.get("lower", False))
        else:
            A1 = T.full(n, rp, ci, v1, kw.get("lower", False))
        if kind == "weak300":
            assert s.stats()[0][14] == 1  # matched
        X, steps, relres, status = s.solve_updated_many(B, values, mapped=mapped, rel_tol=TOL)
        print("%s: steps %s" % (kind, steps.tolist()))
        assert status == 0 and steps.min() >= 1
        block_counters(s, steps, 5, n)
        check_columns(A1.toarray(), X, B, relres, cond)
    finally:
        s.close()


def run_perturbed_many(lib):
    """a factor with replaced pivots is only a weaker preconditioner: per column converged, or not with a truthful relres"""
    A = T.perturbed_matrix()
    case = T.structure(A)
    n = case[0]
    v1 = T.redraw_rows(case)
    A1 = T.full(n, case[1], case[2], v1)
    B = np.array([T.rhs_for(n, 90 + c) for c in range(5)])
    s = ZM(lib, *case, env={"HIPMF_MATCHING": "0"}, pivot_epsilon=1e-13, ordering=2)
    try:
        assert s.num_perturbed > 0
        X, steps, relres, status = s.solve_updated_many(B, v1, rel_tol=TOL, max_steps=60)
        print("%d replaced pivots: status %d, steps %s, relres %s" % (s.num_perturbed, status, steps.tolist(), relres.tolist()))
        assert steps.min() >= 1 and (status == 0) == bool(np.all(relres <= TOL))
        cond, XD = float(np.linalg.cond(A1.toarray())), np.linalg.solve(A1.toarray(), B.T).T
        for c in range(5):
            own, bound, bound_double = T.own_relres(A1, X[c], B[c])
            assert bound < TOL and abs(relres[c] - own) <= bound + bound_double
            if relres[c] <= TOL:
                T.check_accuracy(A1, X[c], B[c], float(relres[c]), cond, XD[c])
    finally:
        s.close()


def run_map_mismatch(lib):
    case, kw = T.matrix("random200")
    n = case[0]
    v1 = T.redraw_rows(case)
    seg_ptr, seg_idx, inputs, summed = triplet_inputs(case, v1)
    B = np.array([T.rhs_for(n, 4), T.rhs_for(n, 5)])
    s = ZM(lib, *case, **kw)
    try:
        with pytest.raises(T.ZError) as e:
            s.solve_updated_many(B, inputs, mapped=True, rel_tol=TOL)
        assert e.value.code == T.ERROR_HIPMF_INVALID_VALUE and "no triplet map" in str(e.value)
        assert s.set_value_map(seg_ptr, seg_idx) == 0
        with pytest.raises(T.ZError) as e:
            s.solve_updated_many(B, summed, mapped=False, rel_tol=TOL)
        assert e.value.code == T.ERROR_HIPMF_INVALID_VALUE and "triplet map" in str(e.value)
        X, steps, relres, status = s.solve_updated_many(B, inputs, mapped=True, rel_tol=TOL)
        assert status == 0
    finally:
        s.close()


def run_no_side_effects_many(lib, name):
    """around a call: the bits of the ordinary solve and of a single solve_updated, get_stats, the determinant, the counters 19 - 22 of the
    ordinary solves and 28 - 30 as that single solve_updated leaves them"""
    case, kw = T.matrix(name)
    n, rp, ci, v0 = case
    v1 = T.redraw_rows(case)
    B = np.array([T.rhs_for(n, 30 + c) for c in range(5)])
    b = B[0]
    s = ZM(lib, *case, nstep=-1, **kw)
    try:
        def snapshot():
            x = s.solve(b)
            i, d = s.stats()
            keep = np.concatenate([i[:11], i[13:]])  # (without the launch counts and timers, which every solve moves)
            xu, su, ru, cu = s.solve_updated(b, v1, rel_tol=TOL)
            counters = [s.counter(k) for k in ("krylov_iterations", "transposed_solves", "analysis_solves", "transposed_krylov_iterations", "updated_steps",
                                               "updated_cycles", "updated_basis_bytes")]
            return (bits(x).copy(), keep, d[:4].copy(), d[9], np.array(s.determinant()), bits(T.interleave(xu)).copy(), su, ru, cu, np.array(counters))
        before = snapshot()
        i0, d0 = s.stats()
        det0 = s.determinant()
        X, steps, relres, status = s.solve_updated_many(B, v1, rel_tol=TOL)
        assert status == 0 and steps.min() > 1
        i1, d1 = s.stats()
        assert np.array_equal(i0, i1) and np.array_equal(bits(d0), bits(d1))  # every statistic, the timers included
        assert s.determinant() == det0
        after = snapshot()
        for a, c in zip(before, after):
            assert np.array_equal(a, c)
    finally:
        s.close()


def run_reproducible_many(lib, name):
    """two calls give the same bits, and the device entry point those of the host entry point; 17 columns: a full block and a tail"""
    case, kw = T.matrix(name)
    n = case[0]
    v1 = T.redraw_rows(case)
    B = np.array([T.rhs_for(n, 40 + c) for c in range(17)])
    s = ZM(lib, *case, **kw)
    try:
        x1, st1, r1, c1 = s.solve_updated_many(B, v1, rel_tol=TOL)
        x2, st2, r2, c2 = s.solve_updated_many(B, v1, rel_tol=TOL)
        assert c1 == c2 == 0 and np.array_equal(st1, st2) and np.array_equal(bits(r1), bits(r2)) and np.array_equal(bits(x1), bits(x2))
        assert s.counter("updated_blocks") == 2
        x3, st3, r3, c3 = s.solve_updated_many_device(B, v1, rel_tol=TOL)
        assert c3 == 0 and np.array_equal(st1, st3) and np.array_equal(bits(r1), bits(r3)) and np.array_equal(bits(x1), bits(x3))
    finally:
        s.close()


def run_status_codes_many(lib):
    """the order of the contract: NULL pointers, initialize, factorize, nrhs < 1, ld < n, a non-finite rel_tol; steps and relres may be NULL"""
    case, _ = T.matrix("ref5")
    n, rp, ci, v0 = case
    zv, x = T.interleave(v0), np.zeros(4 * n)
    b = np.ascontiguousarray(np.array([T.rhs_for(n, 1), T.rhs_for(n, 2)])).view(np.float64).reshape(-1)
    s = ZM(lib, *case, factorize=False)
    fresh = s.lib.complex_solver_hipmf_new()
    try:
        call, dev = s.lib.complex_solver_hipmf_solve_updated_many, s.lib.complex_solver_hipmf_solve_updated_many_device
        nan = float("nan")
        assert call(fresh, x, b, 0, n - 1, zv, 0, nan, 0, None, None, 0) == T.ERROR_NEED_INITIALIZATION
        assert call(s.h, x, b, 0, n - 1, zv, 0, nan, 0, None, None, 0) == T.ERROR_NEED_FACTORIZATION  # (before the invalid values)
        assert dev(s.h, C.c_void_p(16), C.c_void_p(16), 2, n, C.c_void_p(16), 0, TOL, 0, None, None) == T.ERROR_NEED_FACTORIZATION
        assert s.lib.complex_solver_hipmf_factorize(s.h, None, None, None, None, None, None, None, 0, 0, zv) == 0
        assert call(s.h, x, b, 2, n, zv, 0, TOL, 0, None, None, 0) == 0  # (steps and relres may be NULL)
        for nrhs, ld, tol in ((0, n, TOL), (-3, n, TOL), (2, n - 1, TOL), (2, n, nan), (2, n, float("inf"))):
            assert call(s.h, x, b, nrhs, ld, zv, 0, tol, 0, None, None, 0) == T.ERROR_HIPMF_INVALID_VALUE
            assert dev(s.h, C.c_void_p(16), C.c_void_p(16), nrhs, ld, C.c_void_p(16), 0, tol, 0, None, None) == T.ERROR_HIPMF_INVALID_VALUE
        assert call(s.h, x, b, 2, n, zv, 1, TOL, 0, None, None, 0) == T.ERROR_HIPMF_INVALID_VALUE  # mapped without a triplet map
        raw = C.CDLL(s.lib._name)  # (untyped bindings: NULL pointers pass)
        fn = raw.complex_solver_hipmf_solve_updated_many
        fn.restype = C.c_int32
        fn.argtypes = [C.c_void_p] * 3 + [C.c_int32] * 2 + [C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
        h, xp, bp, vp = C.c_void_p(s.h), x.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), zv.ctypes.data_as(C.c_void_p)
        for hh, xx, bb, vv in ((None, xp, bp, vp), (h, None, bp, vp), (h, xp, None, vp), (h, xp, bp, None)):
            assert fn(hh, xx, bb, 2, n, vv, 0, TOL, 0, None, None, 0) == T.ERROR_NULL_POINTER
        assert fn(C.c_void_p(fresh), None, bp, 0, n, vp, 0, TOL, 0, None, None, 0) == T.ERROR_NULL_POINTER  # (before initialize and the invalid values)
    finally:
        s.lib.complex_solver_hipmf_drop(fresh)
        s.close()


def run_host_mirror_many(lib):
    """ComplexLinSolver.solve_many / solve_updated_many of russell_amd.sparse give what the C-ABI gives for the same inputs (a handle set
    up as the mirror sets its own up: default ordering, scaling and refinement; the triplets in CSR order)"""
    from russell_amd import sparse as S

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    product = os.path.join(root, "russell_amd", "lib", "librussell_hipmf.so")
    S._L().rh_set_hipmf_library((lib or product).encode())
    s = None
    try:
        n, rp, ci, vals = T.shifted_grid(12, 10)
        rows = np.repeat(np.arange(n), np.diff(rp)).astype(np.int32)

        def coo(v, order=None):
            order = np.arange(v.size) if order is None else order
            mat = S.ComplexCooMatrix(n, n, v.size)
            mat.put_many(rows[order], ci[order], v[order])
            return mat
        v0, v1 = vals(1.0), vals(0.5)
        B = np.array([T.rhs_for(n, 10 + c) for c in range(5)])
        B[3] = 0.0
        solver = S.ComplexLinSolver(S.Genie.Hipmf)
        with pytest.raises(S.StrError, match="factorize must be called"):
            solver.solve_many(B)
        with pytest.raises(S.StrError, match="factorize must be called"):
            solver.solve_updated_many(coo(v1), B)
        solver.actual.factorize(coo(v0))
        s = ZM(lib, n, rp, ci, v0, nstep=-1)
        X = solver.solve_many(B)
        assert X.shape == B.shape and np.array_equal(bits(X), bits(s.solve_many(B)))
        Xu, steps, relres = solver.solve_updated_many(coo(v1), B, rel_tol=TOL)
        Xc, steps_c, relres_c, status = s.solve_updated_many(B, v1, rel_tol=TOL)
        assert status == 0 and np.array_equal(steps, steps_c) and np.array_equal(bits(relres), bits(relres_c)) and np.array_equal(bits(Xu), bits(Xc))
        assert steps[3] == 0 and steps[0] > 1
        A1 = T.full(n, rp, ci, v1).toarray()
        check_columns(A1, Xu, B, relres, float(np.linalg.cond(A1)), skip=(3,))
        pi = np.random.default_rng(1).permutation(v1.size)  # another triplet order: summed on the host, through the same map
        Xp, steps_p, relres_p = solver.solve_updated_many(coo(v1, pi), B, rel_tol=TOL)
        assert np.array_equal(steps_p, steps) and np.array_equal(bits(Xp), bits(Xu))
        with pytest.raises(S.StrError, match=r"Error\(2\): the iteration on the kept factorization did not converge"):
            solver.solve_updated_many(coo(vals(0.01)), B, rel_tol=TOL, max_steps=2)
        with pytest.raises(S.StrError, match="right-hand side vector is incorrect"):
            solver.actual.solve_updated_many(coo(v1), B[:, :-1])
        with pytest.raises(S.StrError, match="shape"):
            solver.solve_many(B[0])
    finally:
        if s is not None:
            s.close()
        S._L().rh_set_hipmf_library(product.encode())


# ---- the tests on the emulator ----

def test_exports(emu_lib):
    """the entry points, the kernels and the counters exist (they do not on the parent commit)"""
    raw = C.CDLL(emu_lib)
    for name in ("complex_solver_hipmf_solve_updated_many", "complex_solver_hipmf_solve_updated_many_device"):
        assert hasattr(raw, name), name
    kernels = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "russell_amd", "csrc", "kernels_krylov_complex_blocked.hpp")).read()
    for k in ("k_zkryb_dots", "k_zkryb_update", "k_zkryb_combine"):
        assert "__global__ void __launch_bounds__(256) %s(" % k in kernels
    s = ZM(emu_lib, *T.matrix("ref5")[0])
    try:
        assert [s.counter(k) for k in ("block_groups", "updated_blocks", "updated_column_steps", "updated_block_basis_bytes")] == [0, 0, 0, 0]
    finally:
        s.close()


@pytest.mark.parametrize("h1", [0.5, 2.0, 0.1])
def test_complex_arithmetic_per_column(emu_lib, h1):
    run_shift_many(emu_lib, h1)


@pytest.mark.parametrize("nrhs,pad", [(5, 0), (17, 0), (33, 0), (16, 3)])
def test_narrow_block_tail_block_and_padding(emu_lib, nrhs, pad):
    run_shift_many(emu_lib, 0.5, nrhs, pad)


@pytest.mark.parametrize("n", [512, 513, 2049])
def test_tile_edges(emu_lib, n):
    """2 n doubles: exactly one workgroup tile, one pair past it, one pair past four tiles"""
    run_tile_edges(emu_lib, "zchain%d" % n)


@pytest.mark.parametrize("restart", [T.ZPASSV, T.ZPASSV - 1])
def test_basis_count_edges(emu_lib, monkeypatch, restart):
    run_basis_edges(emu_lib, monkeypatch, restart, 0.5, 200, False)


def test_restart_four_columns_finish_in_different_cycles(emu_lib, monkeypatch):
    run_basis_edges(emu_lib, monkeypatch, 4, 10.0, 400, True)


def test_one_column_is_the_single_form(emu_lib):
    run_single_is_single(emu_lib)


def test_not_converged_per_column(emu_lib):
    run_not_converged_many(emu_lib)


@pytest.mark.parametrize("kind", ["symlower", "weak300", "mapped", "pairs0"])
def test_handle_kinds(emu_lib, kind):
    run_handle_kind(emu_lib, kind)


def test_perturbed_factor(emu_lib):
    run_perturbed_many(emu_lib)


def test_map_mismatch(emu_lib):
    run_map_mismatch(emu_lib)


@pytest.mark.parametrize("name", ["random200", "symlower"])
def test_no_side_effects(emu_lib, name):
    run_no_side_effects_many(emu_lib, name)


@pytest.mark.parametrize("name", ["random200", "symlower"])
def test_reproducible_and_device_entry(emu_lib, name):
    run_reproducible_many(emu_lib, name)


def test_status_codes(emu_lib):
    run_status_codes_many(emu_lib)


def test_host_mirror(emu_lib):
    run_host_mirror_many(emu_lib)
