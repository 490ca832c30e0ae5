"""Cases of the extra-precise iterative refinement (solver_hipmf_solve_extra_precise and its siblings, kernels_refine_extra.hpp), shared by
tests/test_extra_precise_cpu.py (the CPU emulator of the HIP kernels) and tests/test_extra_precise_gpu.py (lib None = the product build).

How the error is measured: exactly, not against a second floating-point solve.  forward_error(A, b, x, tail) forms b - A (x + tail) in
fractions.Fraction, rounds it once, and solves for the error with SuperLU plus one correction.  That needs only two digits of the error; its
premise cond_inf(A) eps <= 1e-3, the condition number computed by NumPy, is asserted per case (graded257: of the tridiagonal before scaling --
row and column scalings by powers of ten change neither the pivots' order of magnitude relative to their rows nor the digits of the solve).

The NumPy restatement (reference): the same loop with SuperLU as the pass pair and the same Dot2 residual (TwoProduct by Dekker's splitting,
NumPy has no FMA; TwoSum).  Step counts are compared with it by the project's rule, steps <= reference steps + 1.  The kernel sums the
compensation's own rounding errors in a third word, the restatement stays the plain Dot2: with the pair alone the kernel's error with a tail
was 3.4e-25 on biharm300_lower (emulator) against the restatement's 1.3e-26 -- equal noise per row of the residual, amplified by chance --
and missed the factor 16 below; with the third word it is 4e-33.

Bounds asserted, none of them tuned: without a tail the forward errors against info[2] / info[4] (the solver's own bounds), and
info[2] == max(10, sqrt(n)) eps once converged (dn <= eps and rho_max <= 1/2 give dn / (1 - rho_max) <= 2 eps, below the floor).  With a
tail, eps / 4: the worst case n cond eps^2 lies below it by the premise n cond eps <= 1/4, and no plain double can do better; and 16 x the
error of the restatement with a tail -- the pass pairs differ in ordering and scaling while both floors are governed by cond eps^2."""
import ctypes as C
import functools
import os
from fractions import Fraction

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from russell_amd import problems as P
from russell_amd._capi import load
from russell_amd.backend import Hipmf
from test_solve_updated_cpu import chain
from test_transpose_solve_cpu import ERROR_HIPMF_INVALID_VALUE, ERROR_NEED_FACTORIZATION, ERROR_NULL_POINTER, mumps_5x5
from test_transpose_solve_gpu import _golden, _pm1

EPS = float(np.finfo(float).eps)
ERROR_NEED_INITIALIZATION = 500000
NOT_CONVERGED = 2
SENTINEL = -7.25
TR_COUNTERS = ("krylov_iterations", "transposed_solves", "transposed_blocks", "transposed_krylov_iterations", "updated_basis_bytes")  # of test_solve_updated_transpose_cpu.py


def _new(lib):
    return Hipmf(lib) if lib else Hipmf()


def floor_bound(n):
    return max(10.0, np.sqrt(n)) * EPS


# ---- matrices ----

def laplacian(nx, ny):
    T = lambda m: sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    return sp.csr_matrix(sp.kron(sp.identity(ny), T(nx)) + sp.kron(T(ny), sp.identity(nx)))


@functools.lru_cache(None)
def lambda200():
    return float(np.linalg.eigvalsh(laplacian(23, 21).toarray())[200])


def shifted(delta):
    A = sp.csr_matrix(laplacian(23, 21) - (lambda200() + delta) * sp.identity(483))
    A.sort_indices()
    return A


def biharmonic(n):
    T = sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tocsr()
    A = sp.csr_matrix(T @ T)
    A.sort_indices()
    return A


def graded(n):
    rng = np.random.default_rng(10 * n)
    A = sp.csr_matrix(sp.diags(10.0 ** rng.uniform(-8, 8, n)) @ chain(n) @ sp.diags(10.0 ** rng.uniform(-4, 4, n)))
    A.sort_indices()
    return A


def bordered():
    A0 = shifted(1e-10)
    n = A0.shape[0]
    rng = np.random.default_rng(484)
    col, row = rng.uniform(-1, 1, (n, 1)), rng.uniform(-1, 1, (1, n))
    A = sp.csr_matrix(sp.bmat([[A0, sp.csr_matrix(col)], [sp.csr_matrix(row), sp.csr_matrix([[3.0]])]]))
    A.sort_indices()
    return A


def arrow(n):
    """a well-conditioned chain bordered by a dense last row and column: the last row holds n > 1024 entries, more than a workgroup of the
    residual kernel stages (SPMV_CAP of kernels_vector.hpp) -- the only shape that takes its strided path"""
    rng = np.random.default_rng(n)
    col, row = rng.uniform(-1, 1, (n - 1, 1)) / n, rng.uniform(-1, 1, (1, n - 1))
    A = sp.csr_matrix(sp.bmat([[chain(n - 1), sp.csr_matrix(col)], [sp.csr_matrix(row), sp.csr_matrix([[3.0]])]]))
    A.sort_indices()
    return A


def _general(A, b):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return ((A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32)), dict(values=A.data.astype(float)), A.data.astype(float), A, b)


def _rhs(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


@functools.lru_cache(None)
def matrices():
    """name -> (initialize arguments, keyword arguments, values in the handle's CSR order, the full matrix (scipy CSR), b)"""
    out = {}
    out["shift1e-8"] = _general(shifted(1e-8), _rhs(483, 1))
    out["shift1e-10"] = _general(shifted(1e-10), _rhs(483, 2))
    B = biharmonic(300)
    out["biharm300"] = _general(B, _rhs(300, 3))
    lrp, lci, lv = P.lower_triangle(300, B.indptr.astype(np.int32), B.indices.astype(np.int32), B.data.astype(float))
    out["biharm300_lower"] = ((300, lrp, lci), dict(general_symmetric=True), lv, B, _rhs(300, 3))
    G = graded(257)
    out["graded257"] = _general(G, G @ np.random.default_rng(257).uniform(0.5, 1.5, 257))
    out["bordered484"] = _general(bordered(), _rhs(484, 4))
    out["chain4097"] = _general(chain(4097), _rhs(4097, 5))
    out["arrow1100"] = _general(arrow(1100), _rhs(1100, 11))
    (n, rp, ci, v), b5 = mumps_5x5()
    out["mumps5"] = _general(sp.csr_matrix((np.array(v, float), ci, rp), shape=(n, n)), b5)
    out["bfwb62"] = _general(_golden("bfwb62"), _rhs(62, 6))
    return out


ILL = ["shift1e-8", "shift1e-10", "biharm300", "biharm300_lower", "graded257"]
ALL = ILL + ["bordered484", "chain4097", "arrow1100", "mumps5", "bfwb62"]
TAILED = ["shift1e-10", "biharm300_lower"]


@functools.lru_cache(None)
def cond_inf(name):
    """cond_inf by NumPy (graded257: of the tridiagonal before scaling)"""
    A = chain(257) if name == "graded257" else (many_matrix() if name == "many" else (two_blocks() if name == "two_blocks" else matrices()[name][3]))
    return float(np.linalg.cond(A.toarray(), np.inf))


def handle(lib, init, kw, values, nstep=0):
    s = _new(lib)
    assert s.initialize(*init, refinement_nstep=nstep, **kw) == 0
    assert s.factorize(values) == 0
    return s


# ---- the exact error ----

def exact_residual(A, b, x, tail=None):
    """b - A (x + tail) in rational arithmetic, rounded once"""
    A = sp.csr_matrix(A)
    xs = [Fraction(float(v)) for v in x] if tail is None else [Fraction(float(v)) + Fraction(float(t)) for v, t in zip(x, tail)]
    r = np.zeros(A.shape[0])
    for i in range(A.shape[0]):
        acc = Fraction(float(b[i]))
        for e in range(A.indptr[i], A.indptr[i + 1]):
            acc -= Fraction(float(A.data[e])) * xs[A.indices[e]]
        r[i] = float(acc)
    return r


@functools.lru_cache(None)
def _lu(key):
    return spla.splu(sp.csc_matrix(_LU_MATS[key]))


_LU_MATS = {}


def lu_of(A, key):
    _LU_MATS[key] = A
    return _lu(key)


def forward_error(A, b, x, tail, key):
    """(normwise, componentwise) error of x + tail against the exact solution, and that solution (to the digits of a double)"""
    lu = lu_of(A, key)
    r = exact_residual(A, b, x, tail)
    e = lu.solve(r)
    e = e + lu.solve(r - A @ e)
    xe = (x if tail is None else x + tail) + e
    assert np.all(np.isfinite(e))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(e == 0.0, 0.0, np.abs(e) / np.abs(xe))
    return float(np.max(np.abs(e)) / np.max(np.abs(xe))), float(np.max(q)), xe


def pair_moduli(v):
    return np.hypot(v[0::2], v[1::2])


def forward_error_pairs(A, b, x, tail, key):
    """the same for interleaved complex vectors of a real-equivalent system: moduli of the complex components"""
    lu = lu_of(A, key)
    r = exact_residual(A, b, x, tail)
    e = lu.solve(r)
    e = e + lu.solve(r - A @ e)
    xe = (x if tail is None else x + tail) + e
    me, mx = pair_moduli(e), pair_moduli(xe)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(me == 0.0, 0.0, me / mx)
    return float(np.max(me) / np.max(mx)), float(np.max(q)), xe


# ---- the NumPy restatement ----

_SPLIT = 134217729.0  # 2^27 + 1


def _two_prod(a, b):
    p = a * b
    t = _SPLIT * a
    ah = t - (t - a)
    al = a - ah
    t = _SPLIT * b
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def dot2_residual(A, b, x, tail=None):
    """b - A (x + tail): every product by TwoProduct, every sum by TwoSum into (s, c), rounded once (entries in stored order)"""
    A = sp.csr_matrix(A)
    ip, ix, av = A.indptr.tolist(), A.indices.tolist(), A.data.tolist()
    xl = [float(v) for v in x]
    tl = None if tail is None else [float(v) for v in tail]
    r = np.zeros(A.shape[0])
    for i in range(A.shape[0]):
        s, c = float(b[i]), 0.0
        for e in range(ip[i], ip[i + 1]):
            for vec in ((xl,) if tl is None else (xl, tl)):
                p, pe = _two_prod(-av[e], vec[ix[e]])
                t = s + p
                bb = t - s
                c += ((s - (t - bb)) + (p - bb)) + pe
                s = t
        r[i] = s + c
    return r


def reference(A, b, key, tail=False, dx_tol=0.0, max_steps=0, pairs=False):
    """the iteration of the issue in NumPy: (x, tail or None, steps, state)"""
    lu = lu_of(A, key)
    tol = dx_tol if dx_tol > 0 else EPS
    limit = max_steps if max_steps > 0 else 10
    mod = pair_moduli if pairs else np.abs
    x = lu.solve(b)
    t = np.zeros_like(x) if tail else None
    if not np.any(b):
        return np.zeros_like(x), t, 0, 0
    dn_prev, steps, state = np.inf, 0, 2
    while steps < limit:
        dx = lu.solve(dot2_residual(A, b, x, t))
        steps += 1
        mdx, mx = float(np.max(mod(dx))), float(np.max(mod(x)))
        dn = 0.0 if mdx == 0.0 else (mdx / mx if mx > 0 else np.inf)
        if not np.all(np.isfinite(dx)) or dn > dn_prev:
            state = 1
            break
        if t is None:
            x = x + dx
        else:
            s = x + dx
            bb = s - x
            err = (x - (s - bb)) + (dx - bb)
            tt = err + t
            x = s + tt
            t = tt - (x - s)
        first, dn_prev_old, dn_prev = steps == 1, dn_prev, dn
        if dn <= tol:
            state = 0
            break
        if not first and dn > 0.5 * dn_prev_old:
            state = 1
            break
    return x, t, steps, state


# ---- item 1: without a tail ----

def check_column(name, A, b, x, info, key, n_floor, ref_steps, pairs=False):
    """item 1 of the issue for one column"""
    print("%s: steps %d (reference %d), dn %.3e, bound %.3e, dc %.3e, bound %.3e, rho_max %.3e, state %d" %
          (name, info[0], ref_steps, info[1], info[2], info[3], info[4], info[5], info[6]))
    assert info[6] == 0 and info[7] == 0
    nerr, cerr, xe = (forward_error_pairs if pairs else forward_error)(A, b, x, None, key)
    print("%s: forward error %.3e normwise, %.3e componentwise" % (name, nerr, cerr))
    assert nerr <= info[2], (nerr, info[2])
    assert info[2] == floor_bound(n_floor), (info[2], floor_bound(n_floor))
    assert np.all((pair_moduli(xe) if pairs else np.abs(xe)) > 0.0)
    assert cerr <= info[4], (cerr, info[4])
    assert 1 <= info[0] <= ref_steps + 1, (info[0], ref_steps)
    return nerr, cerr


def run_plain(lib, name):
    init, kw, values, A, b = matrices()[name]
    n = init[0]
    cond = cond_inf(name)
    print("%s: n %d, cond_inf %.3e" % (name, n, cond))
    assert cond * EPS <= 1e-3  # (the premise of forward_error)
    if name in ILL:
        # (an ordinary solve cannot be expected to meet the bound asserted below; graded257: the condition number of the matrix as it is solved)
        hard = float(np.linalg.cond(A.toarray(), np.inf)) if name == "graded257" else cond
        print("%s: cond_inf of the matrix itself %.3e" % (name, hard))
        assert hard * EPS >= 1e3 * floor_bound(n)
    _, _, ref_steps, ref_state = reference(A, b, name)
    assert ref_state == 0
    s = handle(lib, init, kw, values)
    try:
        x, t, info, status = s.solve_extra_precise(b)
        assert status == 0 and t is None
        check_column(name, A, b, x, info, name, n, ref_steps)
        assert s.counter("extra_precise_steps") == info[0] and s.counter("extra_precise_blocks") == 1
    finally:
        s.close()


# ---- item 2: with a tail ----

def run_tail(lib, name):
    init, kw, values, A, b = matrices()[name]
    n = init[0]
    cond = cond_inf(name)
    assert n * cond * EPS <= 0.25, (n, cond)
    xr, tr, ref_steps, _ = reference(A, b, name, tail=True, dx_tol=1e-24)
    ref_err, _, _ = forward_error(A, b, xr, tr, name)
    s = handle(lib, init, kw, values)
    try:
        x, t, info, status = s.solve_extra_precise(b, tail=True, dx_tol=1e-24)
        err, cerr, _ = forward_error(A, b, x, t, name)
        print("%s with a tail: error %.3e normwise, %.3e componentwise (restatement %.3e) after %d steps (restatement %d), state %d, status %d" %
              (name, err, cerr, ref_err, info[0], ref_steps, info[6], status))
        assert info[7] == 1 and status in (0, NOT_CONVERGED)
        assert err <= EPS / 4, err
        assert err <= 16 * ref_err, (err, ref_err)
        assert np.all(np.abs(t) <= EPS * np.abs(x))  # (x is the nearest double of x + tail, up to the last renormalisation)
        return err
    finally:
        s.close()


# ---- the complex handle ----

class ZHandle:
    def __init__(self, lib_path, A):
        self.lib = load(lib_path)
        self.h = self.lib.complex_solver_hipmf_new()
        assert self.h
        S = sp.csr_matrix(A).astype(np.complex128)
        S.sort_indices()
        self.n = S.shape[0]
        zv = np.ascontiguousarray(np.column_stack([S.data.real, S.data.imag]).ravel())
        rp, ci = S.indptr.astype(np.int32), S.indices.astype(np.int32)
        assert self.lib.complex_solver_hipmf_initialize(self.h, 0, 1, -1.0, 0, 0, 0, self.n, rp, ci, zv.ctypes.data) == 0
        assert self.lib.complex_solver_hipmf_factorize(self.h, None, None, None, None, None, None, None, 0, 0, zv) == 0

    def solve_extra_precise(self, b, tail=False, dx_tol=0.0, max_steps=0):
        x, info = np.zeros(2 * self.n), np.zeros(8)
        t = np.zeros(2 * self.n) if tail else None
        code = self.lib.complex_solver_hipmf_solve_extra_precise(self.h, x, None if t is None else t.ctypes.data, np.ascontiguousarray(b), float(dx_tol), int(max_steps),
                                                                 info.ctypes.data, 0)
        assert code in (0, NOT_CONVERGED), code
        return x, t, info, code

    def counter(self, which):
        return int(self.lib.complex_solver_hipmf_get_counter(self.h, which))

    def close(self):
        if self.h:
            self.lib.complex_solver_hipmf_drop(self.h)
            self.h = None


@functools.lru_cache(None)
def complex_case():
    """(the complex matrix, its real-equivalent form on interleaved vectors, the interleaved b)"""
    Az = sp.csr_matrix(laplacian(23, 21) - lambda200() * sp.identity(483) + 1e-8j * sp.identity(483))
    Are = sp.csr_matrix(sp.kron(Az.real, sp.identity(2)) + sp.kron(Az.imag, sp.csr_matrix([[0.0, -1.0], [1.0, 0.0]])))
    Are.sort_indices()
    return Az, Are, _rhs(966, 7)


def run_complex(lib):
    Az, Are, b = complex_case()
    n = Az.shape[0]
    cond = float(np.real(np.linalg.cond(Az.toarray(), np.inf)))
    print("complex: n %d, cond_inf %.3e" % (n, cond))
    assert cond * EPS <= 1e-3 and cond * EPS >= 1e3 * floor_bound(n) and n * cond * EPS <= 0.25
    _, _, ref_steps, ref_state = reference(Are, b, "complex", pairs=True)
    assert ref_state == 0
    xr, tr, _, _ = reference(Are, b, "complex", tail=True, dx_tol=1e-24, pairs=True)
    ref_err, _, _ = forward_error_pairs(Are, b, xr, tr, "complex")
    s = ZHandle(lib, Az)
    try:
        assert s.counter(39) == 0 and s.counter(40) == 0
        x, t, info, status = s.solve_extra_precise(b)
        assert status == 0 and t is None
        check_column("complex", Are, b, x, info, "complex", n, ref_steps, pairs=True)
        assert s.counter(39) == info[0] and s.counter(40) == 1
        x, t, info, status = s.solve_extra_precise(b, tail=True, dx_tol=1e-24)
        err, _, _ = forward_error_pairs(Are, b, x, t, "complex")
        print("complex with a tail: error %.3e (restatement %.3e) after %d steps, state %d" % (err, ref_err, info[0], info[6]))
        assert info[7] == 1
        assert err <= EPS / 4 and err <= 16 * ref_err, (err, ref_err)
        z = np.zeros(2 * n)
        x, t, info, status = s.solve_extra_precise(z, tail=True)
        assert status == 0 and not x.any() and not t.any() and not info.any()
        return err
    finally:
        s.close()


# ---- items 3 and 4: zeros ----

def run_zero_rhs(lib, name):
    init, kw, values, A, b = matrices()[name]
    s = handle(lib, init, kw, values)
    try:
        for tail in (False, True):
            x, t, info, status = s.solve_extra_precise(np.zeros(init[0]), tail=tail)
            assert status == 0 and not x.any() and not info.any() and not np.isnan(x).any()
            assert t is None or (not t.any() and not np.isnan(t).any())
            assert s.counter("extra_precise_steps") == 0
    finally:
        s.close()


@functools.lru_cache(None)
def two_blocks():
    A = sp.csr_matrix(sp.block_diag([chain(257), chain(130)]))
    A.sort_indices()
    return A


def run_zeros_in_solution(lib):
    A = two_blocks()
    n = A.shape[0]
    b = np.concatenate([_rhs(257, 8), np.zeros(130)])
    init, kw, values, _, _ = _general(A, b)
    assert cond_inf("two_blocks") * EPS <= 1e-3
    s = handle(lib, init, kw, values)
    try:
        x, _, info, status = s.solve_extra_precise(b)
        print("zeros in the solution: info", info)
        assert status == 0 and info[6] == 0 and np.isfinite(info[3]) and np.isfinite(info[4])
        assert not x[257:].any()
        nerr, _, _ = forward_error(A, b, x, None, "two_blocks")
        assert nerr <= info[2]
    finally:
        s.close()


# ---- item 5: many right-hand sides ----

@functools.lru_cache(None)
def many_matrix():
    """one matrix with a hard and an easy part on the diagonal: the shifted Laplacian with delta = 3e-12 (cond_inf 2.3e12, still within the
    premise of forward_error; a correction contracts by about cond eps = 5e-4 at worst, so the hard column cannot be done after two steps
    as it sometimes is with delta = 1e-10, where the count depends on the LU at hand) and a well-conditioned chain"""
    A = sp.csr_matrix(sp.block_diag([shifted(3e-12), chain(300)]))
    A.sort_indices()
    return A


@functools.lru_cache(None)
def many_columns():
    """the three kinds of columns and the restatement's step counts for them"""
    A = many_matrix()
    n = A.shape[0]
    hard = _rhs(n, 9)
    easy = A @ np.concatenate([np.zeros(483), np.ones(300)])
    kinds = [hard, easy, np.zeros(n)]
    refs = [reference(A, k, "many")[2:] for k in kinds]
    print("restatement: (steps, state) per kind", refs)
    assert refs[0][1] == 0 and refs[1][1] == 0 and refs[2] == (0, 0)
    assert refs[0][0] > refs[1][0] >= 1  # (the step counts differ between the columns)
    return kinds, [r[0] for r in refs]


def run_many(lib, nrhs):
    A = many_matrix()
    n = A.shape[0]
    ld = n + 3
    cond = cond_inf("many")
    assert cond * EPS <= 1e-3
    kinds, ref_steps = many_columns()
    B = np.full((nrhs, ld), SENTINEL)
    for c in range(nrhs):
        B[c, :n] = kinds[c % 3]
    init, kw, values, _, _ = _general(A, kinds[0])
    s = handle(lib, init, kw, values)
    ptrs = []
    try:
        X = np.full((nrhs, ld), SENTINEL)
        x, t, info, status = s.solve_extra_precise_many(B, ld=ld, x=X)
        assert status == 0 and t is None and np.all(x[:, n:] == SENTINEL)
        assert s.counter("extra_precise_blocks") == (nrhs + 15) // 16
        steps = set()
        for c in range(nrhs):
            if c % 3 == 2:
                assert not x[c, :n].any() and not info[c].any()
                continue
            if c % 3 == 1:
                # (the easy column's solution is zero on the hard block: item 4's rule for dc; its error there is exactly zero)
                assert not x[c, :483].any()
                nerr, _, _ = forward_error(A, B[c, :n], x[c, :n], None, "many")
                assert info[c][6] == 0 and nerr <= info[c][2] == floor_bound(n) and 1 <= info[c][0] <= ref_steps[1] + 1
            else:
                check_column("many[%d]" % c, A, B[c, :n], x[c, :n], info[c], "many", n, ref_steps[0])
            steps.add(int(info[c][0]))
        if nrhs >= 2:
            assert len(steps) >= 2, steps
        # with a tail: the padding of x and of the tail stays
        X2, T2 = np.full((nrhs, ld), SENTINEL), np.full((nrhs, ld), SENTINEL)
        x2, t2, info2, _ = s.solve_extra_precise_many(B, ld=ld, x=X2, x_tail=T2)
        assert np.all(x2[:, n:] == SENTINEL) and np.all(t2[:, n:] == SENTINEL)
        assert all(info2[c][7] == (0 if c % 3 == 2 else 1) for c in range(nrhs))
        assert all(not t2[c, :n].any() and not x2[c, :n].any() for c in range(2, nrhs, 3))
        # the device form: the bits of the host form
        d_x, d_b = s.dev_alloc(8 * ld * nrhs), s.dev_alloc(8 * ld * nrhs)
        ptrs += [d_x, d_b]
        s.h2d(d_b, B)
        s.h2d(d_x, np.full((nrhs, ld), SENTINEL))
        info_d, status_d = s.solve_extra_precise_device(d_x, None, d_b, nrhs, ld=ld)
        xd = np.zeros((nrhs, ld))
        s.d2h(xd, d_x)
        assert status_d == status and np.array_equal(info_d, info)
        assert np.array_equal(xd.view(np.uint64), x.view(np.uint64))
    finally:
        for p in ptrs:
            s.dev_free(p)
        s.close()


# ---- item 6: reproducibility and side effects ----

def run_side_effects(lib, name):
    init, kw, values, A, b = matrices()[name]
    n = init[0]
    s = handle(lib, init, kw, values, nstep=-1)  # (the default refinement of the ordinary solves)
    try:
        assert s.counter("extra_precise_steps") == 0 and s.counter("extra_precise_blocks") == 0
        x0 = s.solve(b)
        keep = [s.counter(k) for k in TR_COUNTERS] + [s.stats()["refinement_steps"]]
        fixed = ("n_perturbed", "factor_launches", "solve_launches", "acc_factor_count", "acc_tri_count", "residual_inf")
        st = {k: s.stats()[k] for k in fixed}
        a = s.solve_extra_precise(b)
        c = s.solve_extra_precise(b)
        assert a[3] == c[3] and np.array_equal(a[0].view(np.uint64), c[0].view(np.uint64)) and np.array_equal(a[2], c[2])
        at = s.solve_extra_precise(b, tail=True, dx_tol=1e-24)
        ct = s.solve_extra_precise(b, tail=True, dx_tol=1e-24)
        assert np.array_equal(at[0].view(np.uint64), ct[0].view(np.uint64)) and np.array_equal(at[1].view(np.uint64), ct[1].view(np.uint64))
        B = np.tile(b, (3, 1))
        m = s.solve_extra_precise_many(B)
        m2 = s.solve_extra_precise_many(B)
        assert np.array_equal(m[0].view(np.uint64), m2[0].view(np.uint64))
        assert s.counter("extra_precise_steps") > 0 and s.counter("extra_precise_blocks") == 1
        assert [s.counter(k) for k in TR_COUNTERS] + [s.stats()["refinement_steps"]] == keep
        assert {k: s.stats()[k] for k in fixed} == st
        x1 = s.solve(b)
        assert np.array_equal(x0.view(np.uint64), x1.view(np.uint64))
    finally:
        s.close()


# ---- item 7: replaced pivots ----

def run_perturbed(lib, monkeypatch):
    """The start iterate alone comes from a handle without refinement and, through HIPMF_KRYLOV=0 (read at initialize), without the Krylov
    rescue: its solve is the sequence k_perm_in, run_triangular, k_perm_out of the start."""
    A = _pm1(400, 4, np.random.default_rng(3))
    n, rp, ci, v = A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
    b = _rhs(n, 10)
    print("+-1 matrix: cond_inf %.3e" % np.linalg.cond(A.toarray(), np.inf))
    monkeypatch.setenv("HIPMF_KRYLOV", "0")
    s0 = _new(lib)
    try:
        # (status 1 is allowed here: without the rescue the probe solve behind factorize's verdict on the replaced pivots cannot finish; the factor is the same)
        assert s0.initialize(n, rp, ci, values=v, refinement_nstep=0) == 0 and s0.factorize(v) in (0, 1)
        xstart = s0.solve(b)
    finally:
        s0.close()
    monkeypatch.delenv("HIPMF_KRYLOV")
    s = _new(lib)
    try:
        assert s.initialize(n, rp, ci, values=v) == 0 and s.factorize(v) == 0
        assert s.num_perturbed > 0
        x, _, info, status = s.solve_extra_precise(b)
        e0, _, _ = forward_error(A, b, xstart, None, "pm1")
        e1, _, _ = forward_error(A, b, x, None, "pm1")
        print("%d replaced pivots: status %d, state %d after %d steps, error %.3e (start alone %.3e)" % (s.num_perturbed, status, info[6], info[0], e1, e0))
        assert status in (0, NOT_CONVERGED)
        assert info[6] in ((0,) if status == 0 else (1, 2))
        assert e1 <= e0, (e1, e0)
        x1, _, info1, _ = s.solve_extra_precise(b, max_steps=1)
        assert info1[0] == 1
    finally:
        s.close()


# ---- items 8 and 9 ----

def run_status_codes(lib):
    (n, rp, ci, v), b = mumps_5x5()
    v = np.array(v, float)
    s = _new(lib)
    try:
        x, info = np.zeros(n), np.zeros(8)
        one, many, dev = s.lib.solver_hipmf_solve_extra_precise, s.lib.solver_hipmf_solve_extra_precise_many, s.lib.solver_hipmf_solve_extra_precise_device
        assert one(s.h, x, None, b, 0.0, 0, None, 0) == ERROR_NEED_INITIALIZATION
        assert many(s.h, x, None, b, 1, n, 0.0, 0, None, 0) == ERROR_NEED_INITIALIZATION
        assert s.initialize(n, rp, ci) == 0
        assert one(s.h, x, None, b, 0.0, 0, None, 0) == ERROR_NEED_FACTORIZATION
        assert many(s.h, x, None, b, 1, n, 0.0, 0, None, 0) == ERROR_NEED_FACTORIZATION
        assert dev(s.h, C.c_void_p(8), None, C.c_void_p(8), 1, n, 0.0, 0, None) == ERROR_NEED_FACTORIZATION
        assert s.factorize(v) == 0
        assert one(s.h, x, None, b, 0.0, 0, None, 0) == 0  # (x_tail and info may be NULL)
        assert many(s.h, x, None, b, 0, n, 0.0, 0, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert many(s.h, x, None, b, 1, n - 1, 0.0, 0, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert dev(s.h, C.c_void_p(8), None, C.c_void_p(8), 0, n, 0.0, 0, None) == ERROR_HIPMF_INVALID_VALUE
        assert dev(s.h, C.c_void_p(8), None, C.c_void_p(8), 1, n - 1, 0.0, 0, None) == ERROR_HIPMF_INVALID_VALUE
        raw = C.CDLL(s.lib._name)  # (untyped bindings: NULL pointers pass)
        raw.solver_hipmf_solve_extra_precise.restype = C.c_int32
        raw.solver_hipmf_solve_extra_precise.argtypes = [C.c_void_p] * 4 + [C.c_double, C.c_int32, C.c_void_p, C.c_int32]
        h, xp, bp = C.c_void_p(s.h), x.ctypes.data_as(C.c_void_p), np.ascontiguousarray(b).ctypes.data_as(C.c_void_p)
        for args in ((None, xp, None, bp), (h, None, None, bp), (h, xp, None, None)):
            assert raw.solver_hipmf_solve_extra_precise(*args, 0.0, 0, None, 0) == ERROR_NULL_POINTER
        raw.complex_solver_hipmf_solve_extra_precise.restype = C.c_int32
        raw.complex_solver_hipmf_solve_extra_precise.argtypes = raw.solver_hipmf_solve_extra_precise.argtypes
        assert raw.complex_solver_hipmf_solve_extra_precise(None, xp, None, bp, 0.0, 0, None, 0) == ERROR_NULL_POINTER
        zh = s.lib.complex_solver_hipmf_new()
        try:
            assert raw.complex_solver_hipmf_solve_extra_precise(C.c_void_p(zh), xp, None, bp, 0.0, 0, None, 0) == ERROR_NEED_INITIALIZATION
        finally:
            s.lib.complex_solver_hipmf_drop(zh)
        # the defaults: dx_tol <= 0 is eps, max_steps <= 0 is 10
        xa, _, ia, _ = s.solve_extra_precise(b, dx_tol=-1.0, max_steps=-3)
        xb, _, ib, _ = s.solve_extra_precise(b, dx_tol=EPS, max_steps=10)
        assert np.array_equal(xa, xb) and np.array_equal(ia, ib)
    finally:
        s.close()


def check_exports(lib_path):
    from russell_amd import _capi

    raw = C.CDLL(lib_path or _capi.DEFAULT_LIB)
    names = ("solver_hipmf_solve_extra_precise", "solver_hipmf_solve_extra_precise_many", "solver_hipmf_solve_extra_precise_device",
             "complex_solver_hipmf_solve_extra_precise")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "russell_hipmf.h")).read()
    for name in names:
        assert hasattr(raw, name), name
        assert name in _capi.SYMBOLS and name + "(" in header, name
    for name, num in (("EXTRA_PRECISE_STEPS", 39), ("EXTRA_PRECISE_BLOCKS", 40)):
        assert "#define HIPMF_COUNTER_%s %d" % (name, num) in header
        assert Hipmf.COUNTERS[name.lower()] == num
