"""Solve with new matrix values on a kept factor (solver_hipmf_solve_updated / _device, kernels_krylov.hpp) on the CPU emulator of the
HIP kernels.  tests/test_solve_updated_gpu.py repeats the run_* cases on the device (lib None = the product build).

The reference is a short NumPy right-preconditioned flexible GMRES of its own (fgmres_reference): dense LU of A_old as M^{-1}, the same
restart, the same tolerance, modified Gram-Schmidt.  Step counts are compared with it: steps <= reference_steps + 1.

The accuracy rule (nothing is a tuned number).  With rel_tol = 1e-10 the test's own |b - A_new x|_2 / |b|_2 must be <= 2 rel_tol; the
rounding bound n eps | |A_new| |x| |_2 / |b|_2 of that recomputation is asserted to be below rel_tol first, which covers the factor 2.
Forward error against np.linalg.solve(A_new, b): <= cond_2(A_new) * 2 rel_tol, the condition number computed by NumPy here.
The recomputation runs in np.longdouble and eps in the bound is that format's: in double the bound itself is 2.3e-10 > rel_tol on the plain
5-point Laplacian of order 3024 (| |A| |x| |_2 = 340 |b|_2 there), so the premise of the rule could not hold for a matrix of the list.
Where the solver's own relres (computed in double on the device) is compared with the recomputation, the same formula with the eps of
double bounds the solver's rounding."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

from russell_amd import problems as P
from russell_amd.backend import Hipmf
from test_sym_indefinite_cpu import saddle_point
from test_transpose_solve_cpu import ERROR_HIPMF_INVALID_VALUE, ERROR_NEED_FACTORIZATION, ERROR_NULL_POINTER, mumps_5x5
from test_transpose_solve_gpu import _golden, _pm1

EPS = np.finfo(float).eps
ERROR_NEED_INITIALIZATION = 500000
NOT_CONVERGED = 2
TOL = 1e-10
PASSV = 8  # KRY_PASSV of kernels_krylov.hpp: basis vectors per pass of k_kry_dots


def _new(lib):
    return Hipmf(lib) if lib else Hipmf()


def chain(n):
    """unsymmetric diagonally dominant tridiagonal matrix"""
    rng = np.random.default_rng(n)
    A = sp.diags([rng.uniform(-1.0, -0.5, n - 1), rng.uniform(3.0, 4.0, n), rng.uniform(-1.0, -0.5, n - 1)], [-1, 0, 1]).tocsr()
    A.sort_indices()
    return A


def matrices():
    """name -> (initialize arguments, keyword arguments, values in the handle's CSR order)"""
    out = {}
    (n, rp, ci, v), _ = mumps_5x5()
    out["mumps5"] = ((n, rp, ci), dict(values=v), np.array(v, float))
    A = _golden("bfwb62").tocsr()
    A.sort_indices()
    out["bfwb62"] = ((A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32)), dict(values=A.data.astype(float)), A.data.astype(float))
    n, rp, ci, v = P.poisson2d(56, 54)
    v = v * (1.0 + 0.1 * np.random.default_rng(56).uniform(-1, 1, v.size))  # (general: not symmetric in value)
    out["poisson"] = ((n, rp, ci), dict(values=v), v)
    n, rp, ci, v = P.poisson2d(56, 54)
    lrp, lci, lv = P.lower_triangle(n, rp, ci, v)
    out["poisson_lower"] = ((n, lrp, lci), dict(general_symmetric=True), lv)
    A, L = saddle_point(24, 60)
    out["saddle"] = ((A.shape[0], L.indptr.astype(np.int32), L.indices.astype(np.int32)), dict(general_symmetric=True, values=L.data.astype(float)),
                     L.data.astype(float))
    for n in (257, 4097):  # one past a workgroup, one past a 4096 boundary (and past four tiles of the vector kernels)
        A = chain(n)
        out["chain%d" % n] = ((n, A.indptr.astype(np.int32), A.indices.astype(np.int32)), dict(values=A.data.copy()), A.data.copy())
    return out


GENERAL = ["mumps5", "bfwb62", "poisson", "chain257", "chain4097"]
ALL = GENERAL + ["poisson_lower", "saddle"]


def dense(init, kw, values):
    n, rp, ci = init
    M = sp.csr_matrix((np.asarray(values, float), ci, rp), shape=(n, n))
    if kw.get("general_symmetric"):
        M = M + sp.tril(M, -1).T
    return M.toarray()


def handle(lib, init, kw, values, nstep=0):
    s = _new(lib)
    assert s.initialize(*init, refinement_nstep=nstep, **kw) == 0
    assert s.factorize(values) in (0, 1)
    return s


def fgmres_reference(A_new, A_old, b, tol, restart, max_steps):
    """right-preconditioned flexible GMRES from x = 0; returns (x, steps, relres)"""
    n = b.size
    lu = sla.lu_factor(A_old)
    m = max(4, min(restart, n))
    x, steps = np.zeros(n), 0
    bnorm = np.linalg.norm(b)
    r = b.copy()
    rnorm = np.linalg.norm(r)
    while rnorm > tol * bnorm and steps < max_steps:
        V, Z = [r / rnorm], []
        H = np.zeros((m + 1, m))
        g = np.zeros(m + 1)
        g[0] = rnorm
        cs, sn = np.zeros(m), np.zeros(m)
        k = 0
        while k < m and steps < max_steps:
            Z.append(sla.lu_solve(lu, V[k]))
            w = A_new @ Z[k]
            steps += 1
            for j in range(k + 1):
                H[j, k] = w @ V[j]
                w = w - H[j, k] * V[j]
            H[k + 1, k] = np.linalg.norm(w)
            for j in range(k):
                H[j, k], H[j + 1, k] = cs[j] * H[j, k] + sn[j] * H[j + 1, k], -sn[j] * H[j, k] + cs[j] * H[j + 1, k]
            d = np.hypot(H[k, k], H[k + 1, k])
            cs[k], sn[k] = (H[k, k] / d, H[k + 1, k] / d) if d > 0 else (1.0, 0.0)
            hn = H[k + 1, k]
            H[k, k], H[k + 1, k] = d, 0.0
            g[k + 1], g[k] = -sn[k] * g[k], cs[k] * g[k]
            k += 1
            if abs(g[k]) <= tol * bnorm or not hn > 0:
                break
            V.append(w / hn)
        y = sla.solve_triangular(H[:k, :k], g[:k])
        x = x + np.array(Z[:k]).T @ y
        before = rnorm
        r = b - A_new @ x
        rnorm = np.linalg.norm(r)
        if not rnorm < before:
            break
    return x, steps, rnorm / bnorm


LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
assert EPS_LD < EPS / 1000  # (an extended format is needed for the premise of the accuracy rule)


def own_relres(A_new, x, b):
    """(|b - A_new x|_2 / |b|_2 recomputed in extended precision, the rounding bound of that recomputation, the same bound for double)"""
    Al, xl, bl = A_new.astype(LD), x.astype(LD), b.astype(LD)
    bnorm = np.sqrt(bl @ bl)
    r = bl - Al @ xl
    scale = float(np.linalg.norm(np.abs(A_new) @ np.abs(x)) / float(bnorm))
    return float(np.sqrt(r @ r) / bnorm), b.size * EPS_LD * scale, b.size * EPS * scale


def check_accuracy(A_new, x, b, relres=None, forward=True):
    """the accuracy rule of the module docstring"""
    own, bound, bound_double = own_relres(A_new, x, b)
    print("own relres %.3e, rounding bound of it %.3e, reported %s" % (own, bound, relres))
    assert bound < TOL, bound
    assert own <= 2 * TOL, own
    if relres is not None:
        assert relres <= TOL and abs(relres - own) <= bound + bound_double
    if forward:
        xd = np.linalg.solve(A_new, b)
        err, cond = np.linalg.norm(x - xd) / np.linalg.norm(xd), np.linalg.cond(A_new)
        print("forward error %.3e, cond_2 %.3e" % (err, cond))
        assert err <= cond * 2 * TOL, (err, cond)


def rhs_for(n, seed=1):
    return np.random.default_rng(seed).standard_normal(n)


def run_unchanged(lib, init, kw, values):
    A = dense(init, kw, values)
    b = rhs_for(A.shape[0])
    s = handle(lib, init, kw, values)
    try:
        x, steps, relres, status = s.solve_updated(b, values, rel_tol=TOL)
        assert (steps, status) == (1, 0), (steps, status, relres)
        assert s.counter("updated_steps") == 1 and s.counter("updated_cycles") == 1
        m = max(4, min(30, A.shape[0]))
        assert s.counter("updated_basis_bytes") == (2 * m + 1) * A.shape[0] * 8
        check_accuracy(A, x, b, relres)
    finally:
        s.close()


def redraw_rows(init, values, nrows=3, seed=7):
    """all entries of `nrows` rows redrawn (scaled by factors in [0.5, 1.5], sign kept: the matrices stay well conditioned)"""
    n, rp, ci = init
    rng = np.random.default_rng(seed)
    rows = rng.choice(n, size=min(nrows, n), replace=False)
    v = np.array(values, float)
    for i in rows:
        v[rp[i]:rp[i + 1]] *= rng.uniform(0.5, 1.5, rp[i + 1] - rp[i])
    return v


def run_rank_change(lib, init, kw, values):
    """A_new M^{-1} = I + (a matrix of rank 3): exact arithmetic needs at most 4 steps"""
    v1 = redraw_rows(init, values)
    A0, A1 = dense(init, kw, values), dense(init, kw, v1)
    b = rhs_for(A0.shape[0], 2)
    _, ref_steps, ref_rel = fgmres_reference(A1, A0, b, TOL, 30, 120)
    print("reference: %d steps, relres %.3e" % (ref_steps, ref_rel))
    assert ref_steps <= 5 and ref_rel <= TOL
    s = handle(lib, init, kw, values)
    try:
        x, steps, relres, status = s.solve_updated(b, v1, rel_tol=TOL)
        print("device: %d steps, relres %.3e" % (steps, relres))
        assert status == 0 and steps <= ref_steps + 1
        check_accuracy(A1, x, b, relres)
    finally:
        s.close()


def shifted_poisson(nx=56, ny=54):
    """the lower triangle of the 5-point Laplacian and the positions of its diagonal: values(s) = L + s I"""
    n, rp, ci, v = P.poisson2d(nx, ny)
    lrp, lci, lv = P.lower_triangle(n, rp, ci, v)
    diag = np.repeat(np.arange(n), np.diff(lrp)) == lci
    return (n, lrp, lci), dict(general_symmetric=True), lambda s: lv + s * diag


def run_shift(lib, ratio, restart=None, max_steps=0, monkeypatch=None, grid=(56, 54)):
    """the Radau5 step-size change: A_old = L + s0 I, A_new = L + s1 I; returns the device's step count"""
    init, kw, vals = shifted_poisson(*grid)
    v0, v1 = vals(1.0), vals(ratio)
    if restart is not None:
        monkeypatch.setenv("HIPMF_UPDATED_RESTART", str(restart))
    m = restart or 30
    A0, A1 = dense(init, kw, v0), dense(init, kw, v1)
    b = rhs_for(init[0], 3)
    _, ref_steps, ref_rel = fgmres_reference(A1, A0, b, TOL, m, max_steps or 4 * m)
    print("reference: %d steps, relres %.3e" % (ref_steps, ref_rel))
    assert ref_rel <= TOL
    s = handle(lib, init, kw, v0)
    try:
        assert s.counter("symmetric_ldlt") == 1
        x, steps, relres, status = s.solve_updated(b, v1, rel_tol=TOL, max_steps=max_steps)
        print("device: %d steps in %d cycles, relres %.3e" % (steps, s.counter("updated_cycles"), relres))
        assert status == 0 and steps <= ref_steps + 1
        assert s.counter("updated_cycles") >= (steps + m - 1) // m
        check_accuracy(A1, x, b, relres)
        return steps, ref_steps
    finally:
        s.close()


def run_not_converged(lib):
    init, kw, vals = shifted_poisson()
    v0, v1 = vals(1.0), vals(100.0)
    A1 = dense(init, kw, v1)
    b = rhs_for(init[0], 3)
    s = handle(lib, init, kw, v0)
    try:
        x, steps, relres, status = s.solve_updated(b, v1, rel_tol=TOL, max_steps=2)
        assert (status, steps) == (NOT_CONVERGED, 2)
        assert TOL < relres < 1.0
        own, bound, bound_double = own_relres(A1, x, b)
        print("reported %.6e, own %.6e, rounding bounds %.3e (own) %.3e (double)" % (relres, own, bound, bound_double))
        assert bound < TOL and abs(relres - own) <= bound + bound_double
    finally:
        s.close()


def run_mapped(lib, init, kw, values):
    """every CSR entry is the sum of two triplets, handed over in a shuffled order: the bits of mapped = 0 on the summed values"""
    n, rp, ci = init
    nnz = values.size
    rng = np.random.default_rng(11)
    v1 = redraw_rows(init, values)
    parts = np.concatenate([v1 * rng.uniform(0.2, 0.8, nnz), np.zeros(nnz)])
    parts[nnz:] = v1 - parts[:nnz]
    order = rng.permutation(2 * nnz)  # input k holds part order[k]
    where = np.argsort(order)  # part q is input where[q]
    seg_ptr = 2 * np.arange(nnz + 1)
    seg_idx = np.empty(2 * nnz, np.int64)
    seg_idx[0::2], seg_idx[1::2] = where[:nnz], where[nnz:]
    inputs = parts[order]
    summed = (0.0 + inputs[seg_idx[0::2]]) + inputs[seg_idx[1::2]]  # (the order of the device's gather)
    b = rhs_for(n, 4)
    s = handle(lib, init, kw, values)
    try:
        with pytest.raises(Exception) as e:
            s.solve_updated(b, inputs, mapped=True, rel_tol=TOL)
        assert e.value.code == ERROR_HIPMF_INVALID_VALUE  # no map yet
        assert s.set_value_map(seg_ptr, seg_idx) == 0
        xm, steps_m, rel_m, st_m = s.solve_updated(b, inputs, mapped=True, rel_tol=TOL)
        x0, steps_0, rel_0, st_0 = s.solve_updated(b, summed, mapped=False, rel_tol=TOL)
        assert (steps_m, st_m) == (steps_0, st_0) and st_0 == 0 and rel_m == rel_0
        assert np.array_equal(xm.view(np.uint64), x0.view(np.uint64))
        check_accuracy(dense(init, kw, summed), xm, b, rel_m)
    finally:
        s.close()


def run_no_side_effects(lib, init, kw, values):
    """the ordinary solves, the product, the counters and istats[10] are the same before and after; a factorize(new values) + solve agrees"""
    n = init[0]
    v1 = redraw_rows(init, values)
    A1 = dense(init, kw, v1)
    b = rhs_for(n, 5)
    s = handle(lib, init, kw, values, nstep=-1)
    try:
        def snapshot():
            x = s.solve(b)
            st = s.stats()
            return (x.view(np.uint64).copy(), s.mat_vec_mul(b).view(np.uint64).copy(), s.num_perturbed, s.counter("krylov_iterations"), st["refinement_steps"],
                    st["fused_fallbacks"])
        before = snapshot()
        x, steps, relres, status = s.solve_updated(b, v1, rel_tol=TOL)
        assert status == 0
        st = s.stats()
        assert st["refinement_steps"] == before[4] and s.counter("krylov_iterations") == before[3]
        after = snapshot()
        for a, c in zip(before, after):
            assert np.array_equal(a, c)
        check_accuracy(A1, x, b, relres)
        assert s.factorize(v1) == 0
        xf = s.solve(b)
        xd = np.linalg.solve(A1, b)
        cond = np.linalg.cond(A1)
        assert np.linalg.norm(x - xf) / np.linalg.norm(xd) <= cond * 2 * TOL + cond * n * EPS
    finally:
        s.close()


def run_reproducible(lib, init, kw, values):
    v1 = redraw_rows(init, values)
    b = rhs_for(init[0], 6)
    s = handle(lib, init, kw, values)
    try:
        x1, st1, r1, c1 = s.solve_updated(b, v1, rel_tol=TOL)
        x2, st2, r2, c2 = s.solve_updated(b, v1, rel_tol=TOL)
        assert (st1, c1) == (st2, c2) and r1 == r2 and np.array_equal(x1.view(np.uint64), x2.view(np.uint64))
    finally:
        s.close()


def run_perturbed(lib):
    """a small member of the +-1 family of tests/test_matrix_zoo_gpu.py whose factorisation replaces pivots: only a weaker preconditioner"""
    A = _pm1(400, 4, np.random.default_rng(3))
    n, rp, ci, v = A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
    s = _new(lib)
    try:
        assert s.initialize(n, rp, ci, values=v) == 0 and s.factorize(v) == 0
        assert s.num_perturbed > 0
        b = rhs_for(n, 8)
        x, steps, relres, status = s.solve_updated(b, v, rel_tol=TOL)
        print("%d replaced pivots: %d steps, relres %.3e" % (s.num_perturbed, steps, relres))
        assert status == 0 and relres <= TOL and steps >= 1
        assert np.linalg.norm(b - A @ x) <= 2 * TOL * np.linalg.norm(b)
    finally:
        s.close()


def run_device_entry(lib, init, kw, values):
    """the _device entry point gives the bits of the host entry point"""
    n = init[0]
    v1 = redraw_rows(init, values)
    b = rhs_for(n, 9)
    s = handle(lib, init, kw, values)
    ptrs = []
    try:
        xh, steps, relres, status = s.solve_updated(b, v1, rel_tol=TOL)
        d_x, d_b, d_v = s.dev_alloc(8 * n), s.dev_alloc(8 * n), s.dev_alloc(8 * v1.size)
        ptrs += [d_x, d_b, d_v]
        s.h2d(d_b, b)
        s.h2d(d_v, v1)
        assert s.solve_updated_device(d_x, d_b, d_v, rel_tol=TOL) == (steps, relres, status)
        xd = np.zeros(n)
        s.d2h(xd, d_x)
        assert np.array_equal(xd.view(np.uint64), xh.view(np.uint64))
    finally:
        for p in ptrs:
            s.dev_free(p)
        s.close()


# ---- the tests on the emulator ----

@pytest.fixture(scope="module")
def mats():
    return matrices()


def test_exports(emu_lib):
    """the two entry points, the status and the counters exist (they do not on the parent commit)"""
    raw = C.CDLL(emu_lib)
    for name in ("solver_hipmf_solve_updated", "solver_hipmf_solve_updated_device"):
        assert hasattr(raw, name), name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "russell_hipmf.h")).read()
    assert "#define HIPMF_WARNING_NOT_CONVERGED 2" in header
    for name, num in (("UPDATED_STEPS", 28), ("UPDATED_CYCLES", 29), ("UPDATED_BASIS_BYTES", 30)):
        assert "#define HIPMF_COUNTER_%s %d" % (name, num) in header
        assert Hipmf.COUNTERS[name.lower()] == num
    (n, rp, ci, v), _ = mumps_5x5()
    s = handle(emu_lib, (n, rp, ci), dict(values=v), v)
    try:
        assert [s.counter(k) for k in ("updated_steps", "updated_cycles", "updated_basis_bytes")] == [0, 0, 0]
    finally:
        s.close()


@pytest.mark.parametrize("name", ALL)
def test_unchanged_values_take_one_step(emu_lib, mats, name):
    init, kw, values = mats[name]
    if name == "saddle":
        s = handle(emu_lib, init, kw, values)
        assert s.stats()["matched"] == 1 and s.counter("sym_expanded") == 1
        s.close()
    run_unchanged(emu_lib, init, kw, values)


@pytest.mark.parametrize("name", GENERAL)
def test_rank_three_change(emu_lib, mats, name):
    run_rank_change(emu_lib, *mats[name])


def test_diagonal_shift_by_two(emu_lib):
    steps, _ = run_shift(emu_lib, 2.0)
    assert steps >= PASSV + 2  # (k crosses the pass boundary of k_kry_dots / k_kry_update)


def test_diagonal_shift_by_hundred_restart_four(emu_lib, monkeypatch):
    steps, _ = run_shift(emu_lib, 100.0, restart=4, max_steps=400, monkeypatch=monkeypatch)
    assert steps > 8  # several cycles


@pytest.mark.parametrize("restart", [PASSV, PASSV - 1])
def test_basis_count_edges(emu_lib, monkeypatch, restart):
    """the restart length at the number of vectors per pass and one below it; the case needs more steps than that"""
    steps, ref_steps = run_shift(emu_lib, 2.0, restart=restart, max_steps=200, monkeypatch=monkeypatch)
    assert ref_steps >= PASSV + 2 and steps > restart


def test_not_converged(emu_lib):
    run_not_converged(emu_lib)


@pytest.mark.parametrize("name", ["poisson", "poisson_lower", "saddle"])
def test_mapped_values(emu_lib, mats, name):
    run_mapped(emu_lib, *mats[name])


@pytest.mark.parametrize("name", ["poisson", "poisson_lower", "saddle"])
def test_no_side_effects(emu_lib, mats, name):
    run_no_side_effects(emu_lib, *mats[name])


@pytest.mark.parametrize("name", ["bfwb62", "poisson_lower"])
def test_reproducible(emu_lib, mats, name):
    run_reproducible(emu_lib, *mats[name])


def test_perturbed_factor(emu_lib):
    run_perturbed(emu_lib)


def test_device_entry_point(emu_lib, mats):
    run_device_entry(emu_lib, *mats["poisson"])


def test_status_codes(emu_lib):
    (n, rp, ci, v), _ = mumps_5x5()
    v = np.array(v, float)
    s = _new(emu_lib)
    try:
        x, b = np.zeros(n), np.ones(n)
        call = s.lib.solver_hipmf_solve_updated
        assert call(s.h, x, b, v, 0, TOL, 0, None, None, 0) == ERROR_NEED_INITIALIZATION
        assert s.initialize(n, rp, ci) == 0
        assert call(s.h, x, b, v, 0, TOL, 0, None, None, 0) == ERROR_NEED_FACTORIZATION
        assert s.lib.solver_hipmf_solve_updated_device(s.h, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), 0, TOL, 0, None, None) == ERROR_NEED_FACTORIZATION
        assert s.factorize(v) == 0
        assert call(s.h, x, b, v, 0, TOL, 0, None, None, 0) == 0  # (steps and relres may be NULL)
        assert call(s.h, x, b, v, 0, float("nan"), 0, None, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert call(s.h, x, b, v, 0, float("inf"), 0, None, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert call(s.h, x, b, v, 1, TOL, 0, None, None, 0) == ERROR_HIPMF_INVALID_VALUE  # mapped without a map
        x[:] = 7.0
        xz, steps, relres, status = s.solve_updated(np.zeros(n), v)
        assert (steps, relres, status) == (0, 0.0, 0) and not xz.any()
        xd, steps, relres, status = s.solve_updated(b, v)  # the defaults: 1e-12, 4 x restart
        assert status == 0 and relres <= 1e-12 and steps == 1
        raw = C.CDLL(s.lib._name)  # (untyped bindings: NULL pointers pass)
        raw.solver_hipmf_solve_updated.restype = C.c_int32
        raw.solver_hipmf_solve_updated.argtypes = [C.c_void_p] * 4 + [C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
        h, xp, bp, vp = C.c_void_p(s.h), x.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)
        for args in ((None, xp, bp, vp), (h, None, bp, vp), (h, xp, None, vp), (h, xp, bp, None)):
            assert raw.solver_hipmf_solve_updated(*args, 0, TOL, 0, None, None, 0) == ERROR_NULL_POINTER
    finally:
        s.close()


def test_host_mirror(emu_lib):
    """LinSolver.solve_updated of russell_amd.sparse: triplets in the order of the factorisation (mapped) and in another order (converted on
    the host), the error string of status 2, a changed pattern"""
    from russell_amd import sparse as S

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    S._L().rh_set_hipmf_library(emu_lib.encode())
    try:
        n, rp, ci, v = P.poisson2d(20, 18)
        A0 = sp.csr_matrix((v, ci, rp), shape=(n, n)).tocoo()
        shift = np.where(A0.row == A0.col, 1.0, 0.0)
        mat0 = S.CooMatrix.from_arrays(n, n, A0.row, A0.col, A0.data + shift)
        mat1 = S.CooMatrix.from_arrays(n, n, A0.row, A0.col, A0.data + 2.0 * shift)
        A1 = (sp.csr_matrix((v, ci, rp), shape=(n, n)) + 2.0 * sp.identity(n)).toarray()
        b = rhs_for(n, 10)
        solver = S.LinSolver(S.Genie.Hipmf)
        with pytest.raises(S.StrError, match="factorize must be called"):
            solver.solve_updated(mat1, b)
        solver.actual.factorize(mat0)
        x, steps, relres = solver.solve_updated(mat1, b, rel_tol=TOL)
        assert 1 < steps <= 30
        check_accuracy(A1, x, b, relres)
        pi = np.random.default_rng(1).permutation(A0.nnz)
        mat1p = S.CooMatrix.from_arrays(n, n, A0.row[pi], A0.col[pi], (A0.data + 2.0 * shift)[pi])
        xp, steps_p, relres_p = solver.solve_updated(mat1p, b, rel_tol=TOL)
        assert steps_p == steps and np.array_equal(xp.view(np.uint64), x.view(np.uint64))
        mat100 = S.CooMatrix.from_arrays(n, n, A0.row, A0.col, A0.data + 100.0 * shift)
        with pytest.raises(S.StrError, match=r"Error\(2\): the iteration on the kept factorization did not converge"):
            solver.solve_updated(mat100, b, rel_tol=TOL, max_steps=2)
        moved = A0.col.copy()
        k = int(np.flatnonzero(A0.row == A0.col + 1)[0])  # a sub-diagonal entry moves to the (empty) corner of its row
        moved[k] = n - 1
        with pytest.raises(S.StrError, match="sparsity pattern differs"):
            solver.solve_updated(S.CooMatrix.from_arrays(n, n, A0.row, moved, A0.data), b)
        with pytest.raises(S.StrError, match="right-hand side vector is incorrect"):
            solver.solve_updated(mat1, b[:-1])
    finally:
        S._L().rh_set_hipmf_library(os.path.join(root, "russell_amd", "lib", "librussell_hipmf.so").encode())
