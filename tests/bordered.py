"""Cases of the bordered solve on the kept factor (solver_hipmf_set_border / solver_hipmf_solve_bordered and their _device forms,
kernels_border.hpp), shared by tests/test_bordered_cpu.py (the CPU emulator of the HIP kernels) and tests/test_bordered_gpu.py (lib None =
the product build).

    [ A   B ] [x]   [f]
    [ C^T D ] [z] = [g]      M = the assembled (n + k) matrix

The NumPy restatement (restate): the loop of the issue -- y = pass pair of f, t = g - C^T y, z = S^{-1} t, x = y - W z, then refinement on
the whole system by the stopping rule of solve() -- with SuperLU of A as the pass pair, W = SuperLU's A^{-1} B, S = D - C^T W.  Step counts
are compared with it by the project's rule, steps <= restatement's steps + 1.

The comparison solution (comparison): SuperLU on M plus one refinement step.

How the error is measured: exactly.  exact_residual (tests/extra_precise.py) forms rhs - M (x; z) in fractions.Fraction and rounds once.
From it: the componentwise backward error of every row i, bounded by (p_i + 2) eps with p_i the entries of row i of M, dense border entries
included -- the bound on a residual evaluated in double, which is all the device's stop test omega <= eps can see --, and the forward error
of the stacked (x; z) in the infinity norm, relative (the error from the exact residual through SuperLU of M plus one correction; that
needs two digits, its premise cond(M) eps <= 1e-3 is asserted).  Forward error <= max(10 x the comparison's, floor_bound(n + k)): ten
times SuperLU is the project's rule (test_matrix_zoo_gpu.py).

The restatement evaluates its residual in working precision, the kernels accumulate theirs beyond twice that and round once
(kernels_border.hpp): omega <= eps sits at the noise of a working-precision residual, and the restatement itself ends 28 of the 134
columns checked here as "no progress" (state 1) at an omega of 2.3e-16 - 2.7e-16, where the device ends all of them converged.  Only the
restatement's step counts are asserted against, by the rule above."""
import ctypes as C
import functools
import os

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from extra_precise import (EPS, ERROR_NEED_INITIALIZATION, SENTINEL, TR_COUNTERS, _new, biharmonic, exact_residual, floor_bound, handle, laplacian, lu_of, shifted)
from russell_amd import problems as P
from russell_amd.backend import Hipmf
from test_transpose_solve_cpu import ERROR_HIPMF_INVALID_VALUE, ERROR_NEED_FACTORIZATION, ERROR_NULL_POINTER

WARNING_SINGULAR_MATRIX = 1
K_SHAPES = [1, 3, 15, 16, 17, 33, 64]
NRHS_SHAPES = [1, 15, 16, 17, 33]


# ---- matrices and borders ----

@functools.lru_cache(None)
def matrix(name):
    """name -> (initialize arguments, keyword arguments, values in the handle's CSR order, the full matrix (scipy CSR))"""
    if name == "lap4087":  # 67 x 61: n odd, no multiple of 4 or 16, four row chunks of the Gram kernel (BORDER_CHUNK = 1024) with a ragged last one
        A = sp.csr_matrix(laplacian(67, 61) + sp.identity(4087))
    elif name == "lap483":
        A = sp.csr_matrix(laplacian(23, 21) + sp.identity(483))
    elif name == "fold1e-6":
        A = shifted(1e-6)
    elif name == "fold1e-10":
        A = shifted(1e-10)
    elif name == "biharm300_lower":
        A = biharmonic(300)
        A.sort_indices()
        lrp, lci, lv = P.lower_triangle(300, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(float))
        return (300, lrp, lci), dict(general_symmetric=True), lv, A
    else:
        raise KeyError(name)
    A.sort_indices()
    return (A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32)), dict(values=A.data.astype(float)), A.data.astype(float), A


@functools.lru_cache(None)
def border(name, k, symmetric=False):
    """(B, C, D) with entries uniform in (-1, 1) from a seeded generator; symmetric: C = B, D = D^T"""
    n = matrix(name)[0][0]
    rng = np.random.default_rng(1000 * k + n)
    B, Cm, D = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (k, k))
    if symmetric:
        Cm, D = B, 0.5 * (D + D.T)
    return B, Cm, D


@functools.lru_cache(None)
def right_hand_sides(name, k, nrhs):
    n = matrix(name)[0][0]
    rng = np.random.default_rng(7 * n + 13 * k + nrhs)
    return rng.standard_normal((nrhs, n)), rng.standard_normal((nrhs, k))


def assembled(A, B, Cm, D):
    M = sp.csr_matrix(sp.bmat([[A, sp.csr_matrix(B)], [sp.csr_matrix(Cm.T), sp.csr_matrix(D)]]))
    M.sort_indices()
    return M


# ---- the NumPy restatement ----

def omega_of(A, B, Cm, D, f, g, x, z):
    """the componentwise backward error over all n + k rows as solve defines it, and the residual"""
    rf, rg = f - A @ x - B @ z, g - Cm.T @ x - D @ z
    df = abs(A) @ np.abs(x) + np.abs(B) @ np.abs(z) + np.abs(f)
    dg = np.abs(Cm).T @ np.abs(x) + np.abs(D) @ np.abs(z) + np.abs(g)
    r, d = np.concatenate([rf, rg]), np.concatenate([df, dg])
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d > 0, np.abs(r) / d, np.where(np.abs(r) > 0, 1.0, 0.0))
    return float(np.max(q)), rf, rg


class Restatement:
    def __init__(self, A, B, Cm, D, key):
        self.A, self.B, self.C, self.D = A, B, Cm, D
        self.lu = lu_of(A, key)
        self.W = self.lu.solve(B)
        self.S = D - Cm.T @ self.W
        self.luS = sla.lu_factor(self.S)

    def eliminate(self, rf, rg):
        y = self.lu.solve(rf)
        z = sla.lu_solve(self.luS, rg - self.C.T @ y)
        return y - self.W @ z, z

    def solve(self, f, g, max_steps=0):
        """(x, z, steps, state, omega before the first step)"""
        limit = max_steps if max_steps > 0 else 4
        x, z = self.eliminate(f, g)
        prev, steps, omega0 = np.inf, 0, None
        while True:
            omega, rf, rg = omega_of(self.A, self.B, self.C, self.D, f, g, x, z)
            if steps == 0:
                omega0 = omega
            if steps > 0 and not omega < prev:
                return xs, zs, steps, 1, omega0
            if omega <= EPS:
                return x, z, steps, 0, omega0
            if steps > 0 and omega > 0.5 * prev:
                return x, z, steps, 1, omega0
            if steps >= limit:
                return x, z, steps, 2, omega0
            prev, xs, zs = omega, x, z
            dx, dz = self.eliminate(rf, rg)
            x, z, steps = x + dx, z + dz, steps + 1


@functools.lru_cache(None)
def restatement(name, k, symmetric=False):
    B, Cm, D = border(name, k, symmetric)
    return Restatement(matrix(name)[3], B, Cm, D, "A:" + name)


def comparison(M, rhs, key):
    """SuperLU on the assembled matrix plus one refinement step"""
    lu = lu_of(M, key)
    y = lu.solve(rhs)
    return y + lu.solve(rhs - M @ y)


# ---- the exact measurement ----

def exact_errors(M, rhs, y, key):
    """(max over the rows of the exact componentwise backward error / ((p_i + 2) eps), forward error of y in the infinity norm, relative)"""
    lu = lu_of(M, key)
    r = exact_residual(M, rhs, y)
    den = abs(M) @ np.abs(y) + np.abs(rhs)
    p = np.diff(M.indptr)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(den > 0, np.abs(r) / den, np.where(np.abs(r) > 0, np.inf, 0.0))
    e = lu.solve(r)
    e = e + lu.solve(r - M @ e)
    assert np.all(np.isfinite(e))
    return float(np.max(q / ((p + 2) * EPS))), float(np.max(np.abs(e)) / np.max(np.abs(y + e)))


@functools.lru_cache(None)
def cond_assembled(name, k, symmetric=False):
    B, Cm, D = border(name, k, symmetric)
    return float(np.linalg.cond(assembled(matrix(name)[3], B, Cm, D).toarray(), np.inf))


def check_column(label, name, k, f, g, x, z, info, symmetric=False, unstable=False):
    """the assertions of case 1 for one column ((B, C, D) = border(name, k, symmetric)); unstable: those of case 2 beside them"""
    A = matrix(name)[3]
    n = A.shape[0]
    B, Cm, D = border(name, k, symmetric)
    M = assembled(A, B, Cm, D)
    assert np.all(np.diff(M.indptr)[:n] == np.diff(A.indptr) + k) and np.all(np.diff(M.indptr)[n:] == n + k)  # (dense border entries included)
    key = "M:%s:%d:%d" % (name, k, symmetric)
    assert cond_assembled(name, k, symmetric) * EPS <= 1e-3  # (the premise of the forward error)
    rhs, y = np.concatenate([f, g]), np.concatenate([x, z])
    _, _, ref_steps, ref_state, ref_omega0 = restatement(name, k, symmetric).solve(f, g)
    back, fe = exact_errors(M, rhs, y, key)
    _, fe_cmp = exact_errors(M, rhs, comparison(M, rhs, key), key)
    print("%s: steps %d (restatement %d, state %d), omega %.3e, before %.3e (restatement %.3e), state %d; exact backward error / ((p + 2) eps) %.3f, "
          "forward error %.3e (comparison %.3e, floor %.3e)" % (label, info[0], ref_steps, ref_state, info[1], info[2], ref_omega0, info[3], back, fe, fe_cmp,
                                                               floor_bound(n + k)))
    assert info[3] == 0, info
    assert info[0] <= ref_steps + 1, (info[0], ref_steps)
    assert back <= 1.0, back
    assert fe <= max(10.0 * fe_cmp, floor_bound(n + k)), (fe, fe_cmp)
    if unstable:
        assert info[2] > 1e3 * EPS, info[2]  # (the unrefined elimination really is unstable here)
        assert info[0] >= 1


# ---- case 1: shapes ----

def bordered_handle(lib, name, k, symmetric=False):
    init, kw, values, _ = matrix(name)
    s = handle(lib, init, kw, values)
    B, Cm, D = border(name, k, symmetric)
    binfo, status = s.set_border(B, Cm, D)
    assert status == 0, status
    return s, binfo


def run_shape(lib, name, k, nrhs, variants=False):
    n = matrix(name)[0][0]
    F, G = right_hand_sides(name, k, nrhs)
    ldx, ldz = n + 5, k + 2
    s, _ = bordered_handle(lib, name, k)
    try:
        Fp, Gp = np.full((nrhs, ldx), SENTINEL), np.full((nrhs, ldz), SENTINEL)
        Fp[:, :n], Gp[:, :k] = F, G
        X, Z = np.full((nrhs, ldx), SENTINEL), np.full((nrhs, ldz), SENTINEL)
        x, z, info = s.solve_bordered(Fp, Gp, ldx=ldx, ldz=ldz, x=X, z=Z)
        assert np.all(x[:, n:] == SENTINEL) and np.all(z[:, k:] == SENTINEL)  # (entries beyond n and k are not touched)
        assert s.counter("bordered_blocks") == (nrhs + 15) // 16 and s.counter("border_columns") == k
        for c in range(nrhs):
            check_column("%s k %d column %d of %d" % (name, k, c, nrhs), name, k, F[c], G[c], x[c, :n], z[c, :k], info[c])
        if variants:
            # z = NULL: the same x, bit for bit
            X2 = np.full((nrhs, ldx), SENTINEL)
            x2, z2, info2 = s.solve_bordered(Fp, Gp, ldx=ldx, ldz=ldz, x=X2, want_z=False)
            assert z2 is None and np.array_equal(x2.view(np.uint64), x.view(np.uint64)) and np.array_equal(info2, info)
            # g = NULL: g = 0
            X3, Z3 = np.full((nrhs, ldx), SENTINEL), np.full((nrhs, ldz), SENTINEL)
            x3, z3, info3 = s.solve_bordered(Fp, None, ldx=ldx, ldz=ldz, x=X3, z=Z3)
            assert np.all(x3[:, n:] == SENTINEL) and np.all(z3[:, k:] == SENTINEL)
            for c in range(nrhs):
                check_column("%s k %d column %d, g = NULL" % (name, k, c), name, k, F[c], np.zeros(k), x3[c, :n], z3[c, :k], info3[c])
    finally:
        s.close()


# ---- case 2: near a fold ----

def run_fold(lib, name, k):
    n = matrix(name)[0][0]
    condA = float(np.linalg.cond(matrix(name)[3].toarray(), np.inf))
    print("%s: cond_inf(A) %.3e, cond_inf(M) %.3e" % (name, condA, cond_assembled(name, k)))
    F, G = right_hand_sides(name, k, 1)
    s, _ = bordered_handle(lib, name, k)
    try:
        x, z, info = s.solve_bordered(F[0], G[0])
        check_column("%s k %d" % (name, k), name, k, F[0], G[0], x, z, info, unstable=True)
        assert s.counter("bordered_steps") == info[0]
    finally:
        s.close()


# ---- case 3: the symmetric handle ----

def run_symmetric(lib, k):
    name = "biharm300_lower"
    F, G = right_hand_sides(name, k, 1)
    s, _ = bordered_handle(lib, name, k, symmetric=True)
    try:
        x, z, info = s.solve_bordered(F[0], G[0])
        check_column("%s k %d" % (name, k), name, k, F[0], G[0], x, z, info, symmetric=True)
        assert s.counter("symmetric_ldlt") == 1
    finally:
        s.close()


# ---- case 4: Woodbury ----

def run_woodbury(lib):
    name, k = "lap483", 5
    init, kw, values, A = matrix(name)
    n = init[0]
    U, V, _ = border(name, k)
    D = -np.identity(k)
    b = right_hand_sides(name, k, 1)[0][0]
    Ad = A.toarray() + U @ V.T
    Am = sp.csr_matrix(Ad)
    assert np.linalg.cond(Ad, np.inf) * EPS <= 1e-3
    R = Restatement(A, U, V, D, "A:" + name)
    _, _, ref_steps, ref_state, _ = R.solve(b, np.zeros(k))
    s = handle(lib, init, kw, values)
    try:
        _, status = s.set_border(U, V, D)
        assert status == 0
        x, z, info = s.solve_bordered(b, None, want_z=False)
        assert z is None
        lu = lu_of(Am, "woodbury")
        xc = lu.solve(b)
        xc = xc + lu.solve(b - Am @ xc)

        def fe_of(v):
            r = exact_residual(Am, b, v)
            e = lu.solve(r)
            e = e + lu.solve(r - Am @ e)
            return float(np.max(np.abs(e)) / np.max(np.abs(v + e)))

        fe, fe_cmp = fe_of(x), fe_of(xc)
        print("Woodbury k %d: steps %d (restatement %d, state %d), omega %.3e, state %d, forward error %.3e (comparison %.3e)" %
              (k, info[0], ref_steps, ref_state, info[1], info[3], fe, fe_cmp))
        assert info[3] == 0 and info[0] <= ref_steps + 1
        assert fe <= max(10.0 * fe_cmp, floor_bound(n)), (fe, fe_cmp)
        # with z returned: the same x, and the exact backward error of the bordered form
        x2, z2, info2 = s.solve_bordered(b, None)
        assert np.array_equal(x2.view(np.uint64), x.view(np.uint64))
        M = assembled(A, U, V, D + 0.0)
        Md = sp.csr_matrix(M)
        rhs, y = np.concatenate([b, np.zeros(k)]), np.concatenate([x2, z2])
        r = exact_residual(Md, rhs, y)
        den = abs(Md) @ np.abs(y) + np.abs(rhs)
        p = np.concatenate([np.diff(A.indptr) + k, np.full(k, n + k)])
        assert np.all(np.abs(r) <= (p + 2) * EPS * den)
    finally:
        s.close()


# ---- case 5: what set_border returns ----

def run_border_info(lib, k):
    name = "lap483"
    init, kw, values, A = matrix(name)
    n = init[0]
    B, Cm, D = border(name, k)
    s, binfo = bordered_handle(lib, name, k)
    try:
        M = assembled(A, B, Cm, D).toarray()
        sM, lM = np.linalg.slogdet(M)
        sA, lA = np.linalg.slogdet(A.toarray())
        want = lM - lA  # log |det S|
        Sref = restatement(name, k).S
        sS, lS = np.linalg.slogdet(Sref)
        gap = abs(lS - want)  # (what the restatement's own S, from SuperLU's W, shows against the same quantity)
        got = np.log(abs(binfo[1])) + binfo[2] * np.log(10.0)
        print("k %d: log |det S| %.15e, device %.15e (off by %.3e), restatement's S off by %.3e; min / max |u_ii| %.6e" % (k, want, got, abs(got - want), gap, binfo[0]))
        assert np.sign(binfo[1]) == sM * sA
        assert 1.0 <= abs(binfo[1]) < 10.0 and binfo[2] == np.floor(binfo[2])
        assert abs(got - want) <= 100.0 * gap, (got, want, gap)
        u = np.abs(np.diag(sla.lu(Sref)[2]))
        ratio = float(u.min() / u.max())
        assert ratio / 2 <= binfo[0] <= 2 * ratio, (binfo[0], ratio)
        assert binfo[3] >= 8 * (3 * n * k + k * k)
        assert s.counter("border_columns") == k
    finally:
        s.close()


def run_singular_border(lib):
    name = "lap483"
    init, kw, values, A = matrix(name)
    n = init[0]
    s = handle(lib, init, kw, values)
    try:
        Cm = border(name, 1)[1]
        info, status = s.set_border(np.zeros((n, 1)), Cm, np.zeros((1, 1)))
        assert status == WARNING_SINGULAR_MATRIX
        assert s.counter("border_columns") == 0
        x = np.zeros(n)
        assert s.lib.solver_hipmf_solve_bordered(s.h, x.ctypes.data, None, np.ones(n).ctypes.data, None, 1, n, 1, 0, None, 0) == ERROR_HIPMF_INVALID_VALUE
    finally:
        s.close()


# ---- case 6: life cycle and status codes ----

def run_status_codes(lib):
    name, k = "lap483", 3
    init, kw, values, A = matrix(name)
    n = init[0]
    B, Cm, D = (np.asfortranarray(a) for a in border(name, k))
    f, g = right_hand_sides(name, k, 1)
    f, g = np.ascontiguousarray(f[0]), np.ascontiguousarray(g[0])
    s = _new(lib)
    try:
        x, z = np.zeros(n), np.zeros(k)
        setb, solve = s.lib.solver_hipmf_set_border, s.lib.solver_hipmf_solve_bordered
        setd, solved = s.lib.solver_hipmf_set_border_device, s.lib.solver_hipmf_solve_bordered_device
        p = lambda a: a.ctypes.data
        border_args = (k, p(B), n, p(Cm), n, p(D), k, None, 0)
        solve_args = (p(x), p(z), p(f), p(g), 1, n, k, 0, None, 0)
        # NULL pointers first
        assert setb(None, *border_args) == ERROR_NULL_POINTER and solve(None, *solve_args) == ERROR_NULL_POINTER
        assert solve(s.h, None, p(z), p(f), p(g), 1, n, k, 0, None, 0) == ERROR_NULL_POINTER
        assert solve(s.h, p(x), p(z), None, p(g), 1, n, k, 0, None, 0) == ERROR_NULL_POINTER
        assert setb(s.h, k, None, n, p(Cm), n, p(D), k, None, 0) == ERROR_NULL_POINTER
        assert solved(None, *solve_args) == ERROR_NULL_POINTER and setd(None, *border_args) == ERROR_NULL_POINTER
        # then the state of the handle
        assert setb(s.h, *border_args) == ERROR_NEED_INITIALIZATION and solve(s.h, *solve_args) == ERROR_NEED_INITIALIZATION
        assert s.initialize(*init, **kw) == 0
        assert setb(s.h, *border_args) == ERROR_NEED_FACTORIZATION and solve(s.h, *solve_args) == ERROR_NEED_FACTORIZATION
        assert solved(s.h, C.c_void_p(8), None, C.c_void_p(8), None, 1, n, k, 0, None, 0) == ERROR_NEED_FACTORIZATION
        assert s.factorize(values) == 0
        # then the values
        assert solve(s.h, *solve_args) == ERROR_HIPMF_INVALID_VALUE  # (no border was set)
        assert setb(s.h, -1, p(B), n, p(Cm), n, p(D), k, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert setb(s.h, 65, p(B), n, p(Cm), n, p(D), 65, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert setb(s.h, k, p(B), n - 1, p(Cm), n, p(D), k, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert setb(s.h, k, p(B), n, p(Cm), n - 1, p(D), k, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert setb(s.h, k, p(B), n, p(Cm), n, p(D), k - 1, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert s.counter("border_columns") == 0
        assert setb(s.h, *border_args) == 0 and s.counter("border_columns") == k
        assert solve(s.h, *solve_args) == 0  # (info may be NULL)
        x0 = x.copy()
        assert solve(s.h, p(x), p(z), p(f), p(g), 0, n, k, 0, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert solve(s.h, p(x), p(z), p(f), p(g), 1, n - 1, k, 0, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert solve(s.h, p(x), p(z), p(f), p(g), 1, n, k - 1, 0, None, 0) == ERROR_HIPMF_INVALID_VALUE
        # max_steps <= 0 selects 4
        info_a, info_b = np.zeros(4), np.zeros(4)
        xa, xb = np.zeros(n), np.zeros(n)
        assert solve(s.h, p(xa), None, p(f), p(g), 1, n, k, -3, p(info_a), 0) == 0 and solve(s.h, p(xb), None, p(f), p(g), 1, n, k, 4, p(info_b), 0) == 0
        assert np.array_equal(xa, xb) and np.array_equal(info_a, info_b) and np.array_equal(xa, x0)
        # a second factorize drops the border until set_border is called again
        assert s.factorize(values) == 0
        assert s.counter("border_columns") == 0
        assert solve(s.h, *solve_args) == ERROR_HIPMF_INVALID_VALUE
        assert setb(s.h, *border_args) == 0
        assert solve(s.h, *solve_args) == 0 and np.array_equal(x, x0)
        # k = 0 frees the border (the pointers may be NULL)
        assert setb(s.h, 0, None, 0, None, 0, None, 0, None, 0) == 0
        assert s.counter("border_columns") == 0
        assert solve(s.h, *solve_args) == ERROR_HIPMF_INVALID_VALUE
    finally:
        s.close()


# ---- case 7: reproducible and without side effects ----

def run_side_effects(lib, name):
    k, nrhs = 3, 3
    init, kw, values, A = matrix(name)
    n = init[0]
    symmetric = name == "biharm300_lower"
    B, Cm, D = border(name, k, symmetric)
    F, G = right_hand_sides(name, k, nrhs)
    s = handle(lib, init, kw, values, nstep=-1)  # (the default refinement of the ordinary solves)
    ptrs = []
    try:
        assert s.counter("bordered_steps") == 0 and s.counter("bordered_blocks") == 0 and s.counter("border_columns") == 0
        x0, t0, m0 = s.solve(F[0]), s.solve_transpose(F[0]), s.solve_many(F)
        keep = [s.counter(c) for c in TR_COUNTERS] + [s.stats()["refinement_steps"]]
        fixed = ("n_perturbed", "factor_launches", "solve_launches", "acc_factor_count", "acc_tri_count", "residual_inf")
        st = {q: s.stats()[q] for q in fixed}
        x0b, t0b, m0b = s.solve(F[0]), s.solve_transpose(F[0]), s.solve_many(F)  # (what a repetition without bordered calls changes)
        keep_b = [s.counter(c) for c in TR_COUNTERS] + [s.stats()["refinement_steps"]]
        st_b = {q: s.stats()[q] for q in fixed}
        binfo, status = s.set_border(B, Cm, D)
        assert status == 0
        a = s.solve_bordered(F[0], G[0])
        b = s.solve_bordered(F[0], G[0])
        assert all(np.array_equal(u.view(np.uint64), v.view(np.uint64)) for u, v in zip(a, b))
        ma = s.solve_bordered(F, G)
        mb = s.solve_bordered(F, G)
        assert all(np.array_equal(u.view(np.uint64), v.view(np.uint64)) for u, v in zip(ma, mb))
        assert s.counter("bordered_blocks") == 1 and s.counter("border_columns") == k
        # the device forms: the bits of the host forms
        d_B, d_C, d_D = (s.dev_alloc(8 * v.size) for v in (B, Cm, D))
        d_x, d_z, d_f, d_g = s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * k * nrhs), s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * k * nrhs)
        ptrs += [d_B, d_C, d_D, d_x, d_z, d_f, d_g]
        s.h2d(d_B, np.asfortranarray(B).T), s.h2d(d_C, np.asfortranarray(Cm).T), s.h2d(d_D, np.asfortranarray(D).T)
        s.h2d(d_f, F), s.h2d(d_g, G)
        binfo_d, status_d = s.set_border_device(k, d_B, d_C, d_D)
        assert status_d == 0 and np.array_equal(binfo_d, binfo)
        info_d = s.solve_bordered_device(d_x, d_z, d_f, d_g, nrhs, ldz=k)
        xd, zd = np.zeros((nrhs, n)), np.zeros((nrhs, k))
        s.d2h(xd, d_x), s.d2h(zd, d_z)
        assert np.array_equal(xd.view(np.uint64), ma[0].view(np.uint64)) and np.array_equal(zd.view(np.uint64), ma[1].view(np.uint64)) and np.array_equal(info_d, ma[2])
        # nothing of the ordinary solves has moved
        assert [s.counter(c) for c in TR_COUNTERS] + [s.stats()["refinement_steps"]] == keep_b
        assert {q: s.stats()[q] for q in fixed} == st_b
        x1, t1, m1 = s.solve(F[0]), s.solve_transpose(F[0]), s.solve_many(F)
        for u, v in ((x0, x1), (t0, t1), (m0, m1), (x0, x0b), (t0, t0b), (m0, m0b)):
            assert np.array_equal(u.view(np.uint64), v.view(np.uint64))
        # ... and these solves move the counters and statistics exactly as the same solves did before the bordered calls (a value of
        # the last call stays, a running count grows by the same amount)
        assert [s.counter(c) for c in TR_COUNTERS] + [s.stats()["refinement_steps"]] == [kb + (kb - ka) for ka, kb in zip(keep, keep_b)]
        assert {q: s.stats()[q] for q in fixed} == {q: st_b[q] + (st_b[q] - st[q]) for q in fixed}
    finally:
        for q in ptrs:
            s.dev_free(q)
        s.close()


# ---- case 8: exports ----

def check_exports(lib_path):
    from russell_amd import _capi

    raw = C.CDLL(lib_path or _capi.DEFAULT_LIB)
    names = ("solver_hipmf_set_border", "solver_hipmf_set_border_device", "solver_hipmf_solve_bordered", "solver_hipmf_solve_bordered_device")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "russell_hipmf.h")).read()
    for name in names:
        assert hasattr(raw, name), name
        assert name in _capi.SYMBOLS and name + "(" in header, name
    assert "#define HIPMF_BORDER_MAX 64" in header
    for name, num in (("BORDER_COLUMNS", 44), ("BORDERED_STEPS", 45), ("BORDERED_BLOCKS", 46)):
        assert "#define HIPMF_COUNTER_%s %d" % (name, num) in header
        assert Hipmf.COUNTERS[name.lower()] == num
