"""Solve with new complex values on a kept factor (complex_solver_hipmf_solve_updated / _device, kernels_krylov_complex.hpp) on the CPU
emulator of the HIP kernels.  tests/test_solve_updated_complex_gpu.py repeats the run_* cases on the device (lib None = the product build).

The reference is a short NumPy right-preconditioned flexible GMRES (fgmres_reference): dense LU of A_old as M^{-1}, np.vdot inner
products, modified Gram-Schmidt, Givens rotations with a real cosine.  It runs twice: in complex arithmetic on the complex matrices, and
-- the same routine -- in real arithmetic on their real-equivalent forms of order 2 n ([a -b; b a] per entry, vectors interleaved).  The
second is what an implementation that merely handed the 2 n system to the real iteration would do: its Krylov space is a subset of the
complex one.  Step counts are compared with both: steps <= complex + 1 and steps <= real-equivalent - 2, where the test first asserts
that its inputs separate the two by at least 3 steps.

The accuracy rule is that of tests/test_solve_updated_cpu.py in complex (nothing is a tuned number).  With rel_tol = 1e-10 the test's own
|b - A_new x|_2 / |b|_2, recomputed in np.clongdouble, must be <= 2 rel_tol; the rounding bound of that recomputation is asserted to be below
rel_tol first, which covers the factor 2.  The bound is written for the real-equivalent system, whose arithmetic a complex residual is
(a complex multiply-add is two real dot-product steps of two terms each): 2 n eps | |A_re| |x_re| |_2 / |b|_2 with the eps of the extended
format.  The solver's own relres (double, on the device, on the real-equivalent CSR) must agree with the recomputation within that bound
plus the same bound with the eps of double.  Forward error against np.linalg.solve(A_new, b): <= cond_2(A_new) * 2 rel_tol."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

from russell_amd._capi import load
from test_complex_error_analysis_cpu import as_complex, interleave
from test_complex_pairs_cpu import _helmholtz2d, _random_complex

EPS = np.finfo(float).eps
CLD, LD = np.clongdouble, np.longdouble
EPS_LD = float(np.finfo(LD).eps)
assert EPS_LD < EPS / 1000  # (an extended format is needed for the premise of the accuracy rule)
ERROR_NULL_POINTER, ERROR_NEED_INITIALIZATION, ERROR_NEED_FACTORIZATION, ERROR_HIPMF_INVALID_VALUE = 100000, 500000, 600000, 803
NOT_CONVERGED = 2
TOL = 1e-10
ZPASSV = 5  # ZKRY_PASSV of kernels_krylov_complex.hpp: basis vectors per pass of k_zkry_dots
ALPHA, BETA = 2.6811, 3.0504  # Radau5's complex eigenvalue pair (the matrix is (alpha + i beta) / h M - J)
COUNTERS = dict(krylov_iterations=19, transposed_solves=20, analysis_solves=21, fused_fallbacks=2, updated_steps=28, updated_cycles=29,
                updated_basis_bytes=30, updated_complex_arithmetic=37)


class ZError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("%d: %s" % (code, message))
        self.code = code


class ZH:
    """a complex_solver_hipmf handle on the CSR structure (n, rp, ci), factorised with the interleaved values zv0; lower: the structure is
    the lower triangle of a complex-symmetric matrix; env: environment variables in force during initialize and factorize; nstep: the
    refinement steps of the ordinary solves (-1: the default)"""

    def __init__(self, lib_path, n, rp, ci, v0, lower=False, env=None, pivot_epsilon=-1.0, ordering=0, factorize=True, nstep=0):
        self.lib = load(lib_path)
        self.h = self.lib.complex_solver_hipmf_new()
        assert self.h
        self.n, self.rp, self.ci = n, np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
        zv = interleave(v0)
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            code = self.lib.complex_solver_hipmf_initialize(self.h, ordering, 1, pivot_epsilon, nstep, 0, int(lower), n, self.rp, self.ci, zv.ctypes.data)
            assert code == 0, code
            self.num_perturbed = None
            if factorize:
                npert = C.c_int32()
                code = self.lib.complex_solver_hipmf_factorize(self.h, None, None, C.byref(npert), None, None, None, None, 0, 0, zv)
                assert code == 0, code
                self.num_perturbed = npert.value
        finally:
            for k, val in old.items():
                if val is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = val

    def error(self, code):
        return ZError(code, self.lib.complex_solver_hipmf_last_error(self.h).decode())

    def solve_updated(self, b, v, mapped=False, rel_tol=0.0, max_steps=0):
        """(x as a complex vector, steps, relres, status); status 0 or 2, anything else raises ZError"""
        x = np.zeros(2 * self.n)
        steps, relres = C.c_int32(-1), C.c_double(-1.0)
        code = self.lib.complex_solver_hipmf_solve_updated(self.h, x, interleave(b), interleave(v), int(bool(mapped)), float(rel_tol), int(max_steps), C.byref(steps),
                                                           C.byref(relres), 0)
        if code not in (0, NOT_CONVERGED):
            raise self.error(code)
        return as_complex(x), steps.value, relres.value, code

    def solve_updated_device(self, d_x, d_b, d_v, mapped=False, rel_tol=0.0, max_steps=0):
        steps, relres = C.c_int32(-1), C.c_double(-1.0)
        code = self.lib.complex_solver_hipmf_solve_updated_device(self.h, d_x, d_b, d_v, int(bool(mapped)), float(rel_tol), int(max_steps), C.byref(steps), C.byref(relres))
        if code not in (0, NOT_CONVERGED):
            raise self.error(code)
        return steps.value, relres.value, code

    def solve(self, b):
        x = np.zeros(2 * self.n)
        assert self.lib.complex_solver_hipmf_solve(self.h, x, interleave(b), 0) == 0
        return x

    def set_value_map(self, seg_ptr, seg_idx):
        sp_, si = np.ascontiguousarray(seg_ptr, np.int32), np.ascontiguousarray(seg_idx, np.int32)
        return self.lib.complex_solver_hipmf_set_value_map(self.h, si.size, sp_, si)

    def factorize_mapped(self, inputs):
        return self.lib.complex_solver_hipmf_factorize_mapped(self.h, None, None, None, None, 0, interleave(inputs))

    def stats(self):
        i, d = np.zeros(16, np.int64), np.zeros(16)
        assert self.lib.complex_solver_hipmf_get_stats(self.h, i, d) == 0
        return i, d

    def determinant(self):
        g = (C.c_double(), C.c_double(), C.c_double())
        assert self.lib.complex_solver_hipmf_get_determinant(self.h, C.byref(g[0]), C.byref(g[1]), C.byref(g[2])) == 0
        return tuple(q.value for q in g)

    def counter(self, name):
        return int(self.lib.complex_solver_hipmf_get_counter(self.h, COUNTERS[name]))

    def dev_alloc(self, nbytes):
        p = self.lib.hipmf_device_malloc(nbytes)
        assert p
        return p

    def dev_free(self, p):
        self.lib.hipmf_device_free(p)

    def h2d(self, d, a):
        a = np.ascontiguousarray(a)
        assert self.lib.hipmf_memcpy_h2d(d, a.ctypes.data_as(C.c_void_p), a.nbytes) == 0

    def d2h(self, a, d):
        assert self.lib.hipmf_memcpy_d2h(a.ctypes.data_as(C.c_void_p), d, a.nbytes) == 0

    def close(self):
        if self.h:
            self.lib.complex_solver_hipmf_drop(self.h)
            self.h = None


# ---- matrices: a case is (n, rp, ci, v0) with complex values in CSR order, plus keywords of ZH ----

def structure(A, lower=False):
    S = sp.csr_matrix(sp.tril(A) if lower else A).astype(np.complex128)
    S.sort_indices()
    return S.shape[0], S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.copy()


def full(n, rp, ci, v, lower=False):
    """the full matrix (scipy CSR) of a handle's structure and values"""
    M = sp.csr_matrix((np.asarray(v, np.complex128), ci, rp), shape=(n, n))
    if lower:
        M = M + sp.tril(M, -1).T
    return sp.csr_matrix(M)


def laplacian(nx, ny):
    """the unit-spacing 5-point Laplacian (Dirichlet) on an nx x ny grid"""
    T = lambda m: sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    return sp.csr_matrix(sp.kron(sp.identity(ny), T(nx)) + sp.kron(T(ny), sp.identity(nx)))


def shifted_grid(nx, ny, unsym=False):
    """(n, rp, ci, h -> values of K(h) = (alpha + i beta) / h I + L in CSR order); unsym: every entry of L scaled by 1 + 0.3 U(-1, 1)"""
    L = laplacian(nx, ny)
    L.sort_indices()
    n, rp, ci, lv = structure(L)
    if unsym:
        lv = lv * (1.0 + 0.3 * np.random.default_rng(24).uniform(-1.0, 1.0, lv.size))
    diag = np.repeat(np.arange(n), np.diff(rp)) == ci
    return n, rp, ci, lambda h: lv + (ALPHA + 1j * BETA) / h * diag


def zchain(n):
    """complex diagonally dominant tridiagonal matrix (unsymmetric, diagonal entries of any phase in the right half plane)"""
    rng = np.random.default_rng(n)
    cz = lambda lo, hi, m: rng.uniform(lo, hi, m) * np.exp(1j * rng.uniform(-1.2, 1.2, m))
    return sp.diags([-cz(0.5, 1.0, n - 1), cz(3.0, 4.0, n), -cz(0.5, 1.0, n - 1)], [-1, 0, 1]).tocsr()


def reference_5x5():
    """the 5 x 5 matrix of the reference's own complex test (tests/test_complex_pairs_cpu.py::test_reference_known_answer)"""
    A = np.zeros((5, 5), dtype=complex)
    A[0, 0], A[0, 1] = 2 + 1j, 3 + 1j
    A[1, 0], A[1, 2], A[1, 4] = 3 - 1j, 4 + 2j, 6 + 3j
    A[2, 1], A[2, 2], A[2, 3] = -1 + 1j, -3 - 1j, 2 + 2j
    A[3, 2] = 1
    A[4, 1], A[4, 2], A[4, 4] = 4, 2, 1 + 1j
    return sp.csr_matrix(A)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """name -> ((n, rp, ci, v0), keywords of ZH)"""
    if name == "ref5":
        return structure(reference_5x5()), {}
    if name == "weak300":  # diagonal entries of modulus 0.005, every seventh purely imaginary: the matching on the moduli permutes complex rows
        return structure(_random_complex(300, 0.03, seed=305, diag=0.005)), {}
    if name == "random200":
        return structure(_random_complex(200, 0.03, seed=600, diag=4.0)), {}
    if name == "symlower":  # complex symmetric, handed over as its lower triangle (mirrored inside the handle)
        A = _helmholtz2d(18, 17)
        return structure(sp.csr_matrix((A + A.T) * 0.5), lower=True), dict(lower=True)
    if name.startswith("zchain"):
        return structure(zchain(int(name[6:]))), {}
    raise KeyError(name)


def real_equivalent(A):
    """[a -b; b a] per entry, unknowns (re, im) interleaved: the matrix the handle factorises"""
    A = np.asarray(A)
    return np.kron(A.real, np.eye(2)) + np.kron(A.imag, np.array([[0.0, -1.0], [1.0, 0.0]]))


def fgmres_reference(A_new, A_old, b, tol, restart, max_steps):
    """right-preconditioned flexible GMRES from x = 0 in the arithmetic of its arguments (complex, or real for the real-equivalent
    matrices); returns (x, steps, relres)"""
    n = b.size
    lu = sla.lu_factor(A_old)
    dt = np.result_type(A_new.dtype, b.dtype)
    m = max(4, min(restart, n))
    x, steps = np.zeros(n, dt), 0
    bnorm = np.linalg.norm(b)
    r = b.astype(dt)
    rnorm = np.linalg.norm(r)
    while rnorm > tol * bnorm and steps < max_steps:
        V, Z = [r / rnorm], []
        H = np.zeros((m + 1, m), dt)
        g = np.zeros(m + 1, dt)
        g[0] = rnorm
        cs, sn = np.zeros(m), np.zeros(m, dt)
        k = 0
        while k < m and steps < max_steps:
            Z.append(sla.lu_solve(lu, V[k]))
            w = A_new @ Z[k]
            steps += 1
            for j in range(k + 1):
                H[j, k] = np.vdot(V[j], w)
                w = w - H[j, k] * V[j]
            hn = np.linalg.norm(w)
            H[k + 1, k] = hn
            for j in range(k):  # rotations [c s; -conj(s) c], c real
                H[j, k], H[j + 1, k] = cs[j] * H[j, k] + sn[j] * H[j + 1, k], -np.conj(sn[j]) * H[j, k] + cs[j] * H[j + 1, k]
            a = H[k, k]
            d = np.hypot(abs(a), hn)
            phase = a / abs(a) if abs(a) > 0 else 1.0
            cs[k], sn[k] = (abs(a) / d, phase * hn / d) if d > 0 else (1.0, 0.0)
            H[k, k], H[k + 1, k] = phase * d, 0.0
            g[k + 1], g[k] = -np.conj(sn[k]) * g[k], cs[k] * g[k]
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


def both_references(A_new, A_old, b, restart=30, max_steps=None, real_too=True):
    """(steps of the complex reference, steps of the real-equivalent reference or None); both must have converged"""
    A_new, A_old = np.asarray(A_new.todense() if sp.issparse(A_new) else A_new), np.asarray(A_old.todense() if sp.issparse(A_old) else A_old)
    max_steps = max_steps or 4 * restart
    _, zsteps, zrel = fgmres_reference(A_new, A_old, b, TOL, restart, max_steps)
    if not real_too:
        print("reference: complex %d steps (relres %.3e)" % (zsteps, zrel))
        assert zrel <= TOL
        return zsteps, None
    _, rsteps, rrel = fgmres_reference(real_equivalent(A_new), real_equivalent(A_old), interleave(b), TOL, restart, max_steps)
    print("reference: complex %d steps (relres %.3e), real-equivalent %d steps (relres %.3e)" % (zsteps, zrel, rsteps, rrel))
    assert zrel <= TOL and rrel <= TOL
    return zsteps, rsteps


def own_relres(A_new, x, b):
    """(|b - A_new x|_2 / |b|_2 recomputed in extended precision on the sparse matrix, the rounding bound of that recomputation, the same
    bound for double); the bounds are those of the real-equivalent system of order 2 n"""
    M = sp.coo_matrix(A_new)
    n = b.size
    ax = np.zeros(n, CLD)
    np.add.at(ax, M.row, M.data.astype(CLD) * x.astype(CLD)[M.col])
    r = b.astype(CLD) - ax
    bnorm = float(np.sqrt(np.sum(np.abs(b.astype(CLD)) ** 2)))
    ar, ai, xr, xi = np.abs(M.data.real), np.abs(M.data.imag), np.abs(x.real)[M.col], np.abs(x.imag)[M.col]
    top, bottom = np.bincount(M.row, ar * xr + ai * xi, n), np.bincount(M.row, ai * xr + ar * xi, n)
    scale = float(np.sqrt(np.sum(top ** 2) + np.sum(bottom ** 2))) / bnorm
    return float(np.sqrt(np.sum(np.abs(r) ** 2))) / bnorm, 2 * n * EPS_LD * scale, 2 * n * EPS * scale


def check_accuracy(A_new, x, b, relres=None, cond=None, xd=None):
    """the accuracy rule of the module docstring; cond / xd: the condition number and the dense solution when the caller has them"""
    own, bound, bound_double = own_relres(A_new, x, b)
    print("own relres %.3e, rounding bound of it %.3e, reported %s" % (own, bound, relres))
    assert bound < TOL, bound
    assert own <= 2 * TOL, own
    if relres is not None:
        assert relres <= TOL and abs(relres - own) <= bound + bound_double
    if xd is None or cond is None:
        D = sp.csr_matrix(A_new).toarray()
        xd = np.linalg.solve(D, b) if xd is None else xd
        cond = np.linalg.cond(D) if cond is None else cond
    err = np.linalg.norm(x - xd) / np.linalg.norm(xd)
    print("forward error %.3e, cond_2 %.3e" % (err, cond))
    assert err <= cond * 2 * TOL, (err, cond)


def rhs_for(n, seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def redraw_rows(case, nrows=3, seed=7):
    """all entries of `nrows` rows redrawn (scaled by complex factors of modulus in [0.5, 1.5] and phase in [-0.5, 0.5]: the matrices stay
    well conditioned): a change of rank `nrows`"""
    n, rp, ci, v0 = case
    rng = np.random.default_rng(seed)
    rows = rng.choice(n, size=min(nrows, n), replace=False)
    v = np.array(v0, np.complex128)
    for i in rows:
        m = rp[i + 1] - rp[i]
        v[rp[i]:rp[i + 1]] *= rng.uniform(0.5, 1.5, m) * np.exp(1j * rng.uniform(-0.5, 0.5, m))
    return v


@functools.lru_cache(maxsize=None)
def shift_case(h1, unsym=False, restart=30, max_steps=0, real_too=True, seed=3):
    """the Radau5 step-size change on the 24 x 20 grid, K(1) -> K(h1): (structure, v0, v1, b, the steps of the complex reference and, with
    real_too, of the real-equivalent one), computed once"""
    n, rp, ci, vals = shifted_grid(24, 20, unsym)
    v0, v1 = vals(1.0), vals(h1)
    b = rhs_for(n, seed)
    zsteps, rsteps = both_references(full(n, rp, ci, v1), full(n, rp, ci, v0), b, restart, max_steps or 4 * restart, real_too)
    return (n, rp, ci), v0, v1, b, zsteps, rsteps


@functools.lru_cache(maxsize=None)
def rank_case(name):
    """three rows of matrix `name` redrawn: (case, keywords, v1, b, complex reference steps, cond_2(A_new), the dense solution), computed once"""
    case, kw = matrix(name)
    n, rp, ci, v0 = case
    v1 = redraw_rows(case)
    A0, A1 = full(n, rp, ci, v0).toarray(), full(n, rp, ci, v1).toarray()
    b = rhs_for(n, 2)
    _, zsteps, zrel = fgmres_reference(A1, A0, b, TOL, 30, 120)
    print("reference: %d steps, relres %.3e" % (zsteps, zrel))
    assert zsteps <= 5 and zrel <= TOL  # (A_new M^{-1} = I + a matrix of rank 3: at most 4 steps in exact arithmetic)
    return case, kw, v1, b, zsteps, float(np.linalg.cond(A1)), np.linalg.solve(A1, b)


# ---- the run functions (lib: the emulator's path, or None for the product build) ----

def run_shift(lib, h1, unsym=False, restart=None, max_steps=0, monkeypatch=None, real_too=True):
    """the step-size change against the complex reference and, with real_too, against the real-equivalent one (complex arithmetic is
    really used); returns (steps, complex reference steps, cycles)"""
    if restart is not None:
        monkeypatch.setenv("HIPMF_UPDATED_RESTART", str(restart))
    m = restart or 30
    (n, rp, ci), v0, v1, b, zsteps, rsteps = shift_case(h1, unsym, m, max_steps, real_too)
    if real_too:
        assert rsteps >= zsteps + 3, (zsteps, rsteps)  # the premise: these inputs tell the two iterations apart
    s = ZH(lib, n, rp, ci, v0)
    try:
        assert s.counter("updated_complex_arithmetic") == 0
        x, steps, relres, status = s.solve_updated(b, v1, rel_tol=TOL, max_steps=max_steps)
        cycles = s.counter("updated_cycles")
        print("device: %d steps in %d cycles, relres %.3e" % (steps, cycles, relres))
        assert status == 0
        assert steps <= zsteps + 1, (steps, zsteps)
        if real_too:
            assert steps <= rsteps - 2, (steps, rsteps)
        assert s.counter("updated_complex_arithmetic") == 1 and s.counter("updated_steps") == steps
        assert cycles >= (steps + m - 1) // m
        check_accuracy(full(n, rp, ci, v1), x, b, relres)
        return steps, zsteps, cycles
    finally:
        s.close()


def run_unchanged(lib, name):
    case, kw = matrix(name)
    n, rp, ci, v0 = case
    A = full(n, rp, ci, v0, kw.get("lower", False))
    b = rhs_for(n)
    s = ZH(lib, *case, **kw)
    try:
        if name == "weak300":
            assert s.stats()[0][14] == 1  # matched
        x, steps, relres, status = s.solve_updated(b, v0, rel_tol=TOL)
        assert (steps, status) == (1, 0), (steps, status, relres)
        assert s.counter("updated_steps") == 1 and s.counter("updated_cycles") == 1 and s.counter("updated_complex_arithmetic") == 1
        m = max(4, min(30, n))
        assert s.counter("updated_basis_bytes") == (2 * m + 1) * 2 * n * 8
        check_accuracy(A, x, b, relres)
    finally:
        s.close()


def run_rank_change(lib, name):
    """cases 3 and 4"""
    case, kw, v1, b, zsteps, cond, xd = rank_case(name)
    n, rp, ci, v0 = case
    s = ZH(lib, *case, **kw)
    try:
        x, steps, relres, status = s.solve_updated(b, v1, rel_tol=TOL)
        print("device: %d steps, relres %.3e" % (steps, relres))
        assert status == 0 and steps <= zsteps + 1
        check_accuracy(full(n, rp, ci, v1), x, b, relres, cond, xd)
    finally:
        s.close()


def run_not_converged(lib):
    (n, rp, ci), v0, v1, b, zsteps, _ = shift_case(0.1)
    assert zsteps > 3
    s = ZH(lib, n, rp, ci, v0)
    try:
        x, steps, relres, status = s.solve_updated(b, v1, rel_tol=TOL, max_steps=3)
        assert (status, steps) == (NOT_CONVERGED, 3)
        assert TOL < relres < 1.0
        own, bound, bound_double = own_relres(full(n, rp, ci, v1), x, b)
        print("reported %.6e, own %.6e, rounding bounds %.3e (own) %.3e (double)" % (relres, own, bound, bound_double))
        assert bound < TOL and abs(relres - own) <= bound + bound_double
        x0, steps, relres, status = s.solve_updated(np.zeros(n, complex), v1, rel_tol=TOL)
        assert (steps, relres, status) == (0, 0.0, 0) and not x0.any()
        bad = b.copy()
        bad[n // 2] = complex(1.0, np.nan)
        _, steps, relres, status = s.solve_updated(bad, v1, rel_tol=TOL)
        assert (steps, status) == (0, NOT_CONVERGED) and np.isnan(relres)
        x, steps, relres, status = s.solve_updated(b, v0)  # the defaults after all that: 1e-12, 4 x restart
        assert (steps, status) == (1, 0) and relres <= 1e-12
    finally:
        s.close()


def run_mapped(lib, name):
    """every CSR entry is the sum of two triplets, handed over in a shuffled order: the bits of mapped = 0, on the summed values, of an
    identically set-up handle without the triplet map; both mismatches of `mapped`"""
    case, kw = matrix(name)
    n, rp, ci, v0 = case
    nnz = v0.size
    rng = np.random.default_rng(11)
    v1 = redraw_rows(case)
    parts = np.concatenate([v1 * rng.uniform(0.2, 0.8, nnz), np.zeros(nnz, complex)])
    parts[nnz:] = v1 - parts[:nnz]
    order = rng.permutation(2 * nnz)  # input k holds part order[k]
    where = np.argsort(order)  # part q is input where[q]
    seg_ptr = 2 * np.arange(nnz + 1)
    seg_idx = np.empty(2 * nnz, np.int64)
    seg_idx[0::2], seg_idx[1::2] = where[:nnz], where[nnz:]
    inputs = parts[order]
    summed = (0.0 + inputs[seg_idx[0::2]]) + inputs[seg_idx[1::2]]  # (the order of the device's gather, real and imaginary parts apart)
    b = rhs_for(n, 4)
    plain, s = ZH(lib, *case, **kw), ZH(lib, *case, **kw)
    try:
        with pytest.raises(ZError) as e:
            s.solve_updated(b, inputs, mapped=True, rel_tol=TOL)
        assert e.value.code == ERROR_HIPMF_INVALID_VALUE and "no triplet map" in str(e.value)
        assert s.set_value_map(seg_ptr, seg_idx) == 0
        with pytest.raises(ZError) as e:
            s.solve_updated(b, summed, mapped=False, rel_tol=TOL)
        assert e.value.code == ERROR_HIPMF_INVALID_VALUE and "triplet map" in str(e.value)
        xm, steps_m, rel_m, st_m = s.solve_updated(b, inputs, mapped=True, rel_tol=TOL)
        x0, steps_0, rel_0, st_0 = plain.solve_updated(b, summed, mapped=False, rel_tol=TOL)
        assert (steps_m, st_m) == (steps_0, st_0) and st_0 == 0 and rel_m == rel_0
        assert np.array_equal(interleave(xm).view(np.uint64), interleave(x0).view(np.uint64))
        check_accuracy(full(n, rp, ci, summed, kw.get("lower", False)), xm, b, rel_m)
        assert s.factorize_mapped(inputs) == 0  # the triplet map is still the one in force
        xf = as_complex(s.solve(b))
        assert np.linalg.norm(xf - xm) <= 1e-6 * np.linalg.norm(xm)
    finally:
        s.close()
        plain.close()


def run_status_codes(lib):
    """the order of the contract: NULL pointers, initialize, factorize, then invalid values"""
    case, _ = matrix("ref5")
    n, rp, ci, v0 = case
    zv, b, x = interleave(v0), interleave(rhs_for(n)), np.zeros(2 * n)
    s = ZH(lib, *case, factorize=False)
    fresh = load(lib).complex_solver_hipmf_new()
    try:
        call = s.lib.complex_solver_hipmf_solve_updated
        assert call(fresh, x, b, zv, 0, TOL, 0, None, None, 0) == ERROR_NEED_INITIALIZATION
        assert call(s.h, x, b, zv, 0, TOL, 0, None, None, 0) == ERROR_NEED_FACTORIZATION
        assert call(s.h, x, b, zv, 1, float("nan"), 0, None, None, 0) == ERROR_NEED_FACTORIZATION  # (before the invalid values)
        assert s.lib.complex_solver_hipmf_solve_updated_device(s.h, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), 0, TOL, 0, None, None) == ERROR_NEED_FACTORIZATION
        assert s.lib.complex_solver_hipmf_factorize(s.h, None, None, None, None, None, None, None, 0, 0, zv) == 0
        assert call(s.h, x, b, zv, 0, TOL, 0, None, None, 0) == 0  # (steps and relres may be NULL)
        assert call(s.h, x, b, zv, 0, float("nan"), 0, None, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert call(s.h, x, b, zv, 0, float("inf"), 0, None, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert call(s.h, x, b, zv, 1, TOL, 0, None, None, 0) == ERROR_HIPMF_INVALID_VALUE  # mapped without a triplet map
        raw = C.CDLL(s.lib._name)  # (untyped bindings: NULL pointers pass)
        raw.complex_solver_hipmf_solve_updated.restype = C.c_int32
        raw.complex_solver_hipmf_solve_updated.argtypes = [C.c_void_p] * 4 + [C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
        h, xp, bp, vp = C.c_void_p(s.h), x.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), zv.ctypes.data_as(C.c_void_p)
        for args in ((None, xp, bp, vp), (h, None, bp, vp), (h, xp, None, vp), (h, xp, bp, None)):
            assert raw.complex_solver_hipmf_solve_updated(*args, 0, TOL, 0, None, None, 0) == ERROR_NULL_POINTER
        assert raw.complex_solver_hipmf_solve_updated(C.c_void_p(fresh), None, bp, vp, 0, TOL, 0, None, None, 0) == ERROR_NULL_POINTER  # (before initialize)
    finally:
        s.lib.complex_solver_hipmf_drop(fresh)
        s.close()


def run_no_side_effects(lib, name):
    """around a call: the bits of the ordinary solve, get_stats, the counters of the ordinary solves and the determinant"""
    case, kw = matrix(name)
    n, rp, ci, v0 = case
    v1 = redraw_rows(case)
    b = rhs_for(n, 5)
    s = ZH(lib, *case, nstep=-1, **kw)
    try:
        def snapshot():
            x = s.solve(b)
            i, d = s.stats()
            keep = np.concatenate([i[:11], i[13:]])  # (without the launch counts and timers, which every solve moves)
            return (x.view(np.uint64).copy(), keep, d[:4].copy(), d[9], np.array(s.determinant()), s.counter("krylov_iterations"), s.counter("transposed_solves"),
                    s.counter("analysis_solves"), s.counter("fused_fallbacks"))
        before = snapshot()
        i0, d0 = s.stats()
        det0 = s.determinant()
        x, steps, relres, status = s.solve_updated(b, v1, rel_tol=TOL)
        assert status == 0 and steps > 1
        i1, d1 = s.stats()
        assert np.array_equal(i0, i1) and np.array_equal(d0.view(np.uint64), d1.view(np.uint64))  # every statistic, the timers included
        assert s.determinant() == det0
        after = snapshot()
        for a, c in zip(before, after):
            assert np.array_equal(a, c)
        check_accuracy(full(n, rp, ci, v1, kw.get("lower", False)), x, b, relres)
    finally:
        s.close()


def run_reproducible(lib, name, env=None):
    """two calls give the same bits; env: e.g. HIPMF_COMPLEX_PAIRS=0, the plain real-equivalent factorisation as preconditioner"""
    case, kw = matrix(name)
    n, rp, ci, v0 = case
    v1 = redraw_rows(case)
    b = rhs_for(n, 6)
    s = ZH(lib, *case, env=env, **kw)
    try:
        x1, st1, r1, c1 = s.solve_updated(b, v1, rel_tol=TOL)
        x2, st2, r2, c2 = s.solve_updated(b, v1, rel_tol=TOL)
        assert (st1, c1) == (st2, c2) and c1 == 0 and r1 == r2 and np.array_equal(interleave(x1).view(np.uint64), interleave(x2).view(np.uint64))
        check_accuracy(full(n, rp, ci, v1, kw.get("lower", False)), x1, b, r1)
    finally:
        s.close()


def perturbed_matrix(p=3, m=20, seed=1):
    """Natural order, no matching: a leaf supernode of p complex columns whose diagonal block is ZERO, a second leaf with a strong one,
    both coupled densely to the m rows / columns of the root.  The pivot searches stay inside a pivot block, so the p complex pivots of
    the first leaf are replaced by the (tiny) pivot_epsilon; the matrix itself is well conditioned"""
    rng = np.random.default_rng(seed)
    n = 2 * p + m
    cz = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    A = np.zeros((n, n), dtype=complex)
    A[p:2 * p, p:2 * p] = cz(p, p) * 0.3 + 4.0 * np.eye(p)
    for a0 in (0, p):
        A[a0:a0 + p, 2 * p:] = cz(p, m) * 0.3
        A[2 * p:, a0:a0 + p] = cz(m, p) * 0.3
    A[2 * p:, 2 * p:] = np.diag((4.0 + rng.random(m)) * np.exp(2j * np.pi * rng.random(m))) + np.diag(cz(m - 1) * 0.2, 1) + np.diag(cz(m - 1) * 0.2, -1)
    return sp.csr_matrix(A)


def run_perturbed(lib):
    """a factor with replaced pivots is only a weaker preconditioner: converged, or status 2 with a truthful relres"""
    A = perturbed_matrix()
    case = structure(A)
    n = case[0]
    s = ZH(lib, *case, env={"HIPMF_MATCHING": "0"}, pivot_epsilon=1e-13, ordering=2)
    try:
        assert s.num_perturbed > 0
        b = rhs_for(n, 8)
        x, steps, relres, status = s.solve_updated(b, case[3], rel_tol=TOL, max_steps=60)
        print("%d replaced pivots: status %d, %d steps, relres %.3e" % (s.num_perturbed, status, steps, relres))
        assert steps >= 1 and status in (0, NOT_CONVERGED)
        own, bound, bound_double = own_relres(A, x, b)
        assert bound < TOL and abs(relres - own) <= bound + bound_double
        assert (relres <= TOL) == (status == 0)
    finally:
        s.close()


def run_device_entry(lib, name):
    """the _device entry point gives the bits of the host entry point"""
    case, kw = matrix(name)
    n = case[0]
    v1 = redraw_rows(case)
    b = rhs_for(n, 9)
    s = ZH(lib, *case, **kw)
    ptrs = []
    try:
        xh, steps, relres, status = s.solve_updated(b, v1, rel_tol=TOL)
        d_x, d_b, d_v = s.dev_alloc(16 * n), s.dev_alloc(16 * n), s.dev_alloc(16 * v1.size)
        ptrs += [d_x, d_b, d_v]
        s.h2d(d_b, interleave(b))
        s.h2d(d_v, interleave(v1))
        assert s.solve_updated_device(d_x, d_b, d_v, rel_tol=TOL) == (steps, relres, status)
        xd = np.zeros(2 * n)
        s.d2h(xd, d_x)
        assert np.array_equal(xd.view(np.uint64), interleave(xh).view(np.uint64))
    finally:
        for p in ptrs:
            s.dev_free(p)
        s.close()


def run_host_mirror(lib):
    """ComplexLinSolver.solve_updated of russell_amd.sparse: triplets in the order of the factorisation (the triplet map) and in another
    order (summed on the host, handed over through the same map), the error string of status 2, a changed pattern"""
    from russell_amd import sparse as S

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    product = os.path.join(root, "russell_amd", "lib", "librussell_hipmf.so")
    S._L().rh_set_hipmf_library((lib or product).encode())
    try:
        n, rp, ci, vals = shifted_grid(12, 10)
        rows = np.repeat(np.arange(n), np.diff(rp)).astype(np.int32)

        def coo(v, order=None):
            order = np.arange(v.size) if order is None else order
            mat = S.ComplexCooMatrix(n, n, v.size)
            mat.put_many(rows[order], ci[order], v[order])
            return mat
        v0, v1 = vals(1.0), vals(0.5)
        b = rhs_for(n, 10)
        solver = S.ComplexLinSolver(S.Genie.Hipmf)
        with pytest.raises(S.StrError, match="factorize must be called"):
            solver.solve_updated(coo(v1), b)
        solver.actual.factorize(coo(v0))
        x, steps, relres = solver.solve_updated(coo(v1), b, rel_tol=TOL)
        assert 1 < steps <= 30
        check_accuracy(full(n, rp, ci, v1), x, b, relres)
        pi = np.random.default_rng(1).permutation(v1.size)
        xp, steps_p, relres_p = solver.solve_updated(coo(v1, pi), b, rel_tol=TOL)
        assert steps_p == steps and np.array_equal(interleave(xp).view(np.uint64), interleave(x).view(np.uint64))
        with pytest.raises(S.StrError, match=r"Error\(2\): the iteration on the kept factorization did not converge"):
            solver.solve_updated(coo(vals(0.01)), b, rel_tol=TOL, max_steps=2)
        moved = ci.copy()
        k = int(np.flatnonzero(rows == ci + 1)[0])  # a sub-diagonal entry moves to the (empty) corner of its row
        moved[k] = n - 1
        bad = S.ComplexCooMatrix(n, n, v1.size)
        bad.put_many(rows, moved, v1)
        with pytest.raises(S.StrError, match="sparsity pattern differs"):
            solver.solve_updated(bad, b)
        with pytest.raises(S.StrError, match="right-hand side vector is incorrect"):
            solver.solve_updated(coo(v1), b[:-1])
        solver.actual.factorize(coo(v1))  # the handle's map is still the one of the factorisation
        xf = solver.actual.solve(b)
        assert np.linalg.norm(xf - x) <= 1e-6 * np.linalg.norm(x)
    finally:
        S._L().rh_set_hipmf_library(product.encode())


# ---- the tests on the emulator ----

def test_exports(emu_lib):
    """the two entry points and the counter exist (they do not on the parent commit)"""
    raw = C.CDLL(emu_lib)
    for name in ("complex_solver_hipmf_solve_updated", "complex_solver_hipmf_solve_updated_device"):
        assert hasattr(raw, name), name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "russell_hipmf.h")).read()
    assert "#define HIPMF_COUNTER_UPDATED_COMPLEX_ARITHMETIC 37" in header
    kernels = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "russell_amd", "csrc", "kernels_krylov_complex.hpp")).read()
    assert "constexpr int ZKRY_PASSV = %d;" % ZPASSV in kernels
    s = ZH(emu_lib, *matrix("ref5")[0])
    try:
        assert [s.counter(k) for k in ("updated_steps", "updated_cycles", "updated_basis_bytes", "updated_complex_arithmetic")] == [0, 0, 0, 0]
    finally:
        s.close()


@pytest.mark.parametrize("h1", [0.5, 2.0, 0.1])
def test_complex_arithmetic_is_used(emu_lib, h1):
    run_shift(emu_lib, h1)


def test_complex_arithmetic_is_used_unsymmetric(emu_lib):
    run_shift(emu_lib, 0.1, unsym=True)


@pytest.mark.parametrize("name", ["ref5", "weak300", "symlower"])
def test_unchanged_values_take_one_step(emu_lib, name):
    run_unchanged(emu_lib, name)


@pytest.mark.parametrize("name", ["ref5", "random200"])
def test_rank_three_change(emu_lib, name):
    run_rank_change(emu_lib, name)


@pytest.mark.parametrize("n", [512, 513, 2049])
def test_tile_edges(emu_lib, n):
    """2 n doubles: exactly one workgroup tile, one pair past it, one pair past four tiles"""
    run_rank_change(emu_lib, "zchain%d" % n)


@pytest.mark.parametrize("restart", [ZPASSV, ZPASSV - 1])
def test_basis_count_edges(emu_lib, monkeypatch, restart):
    """the restart length at the number of vectors per pass and one below it: a full group, a partial group, a restart"""
    steps, zsteps, cycles = run_shift(emu_lib, 0.5, restart=restart, max_steps=200, monkeypatch=monkeypatch, real_too=False)
    assert zsteps >= ZPASSV + 2 and steps > restart and cycles >= 2


def test_restart_four_many_cycles(emu_lib, monkeypatch):
    steps, zsteps, cycles = run_shift(emu_lib, 10.0, restart=4, max_steps=400, monkeypatch=monkeypatch, real_too=False)
    assert steps > 8 and cycles > 2


def test_not_converged_zero_and_nan(emu_lib):
    run_not_converged(emu_lib)


@pytest.mark.parametrize("name", ["random200", "symlower"])
def test_mapped_values(emu_lib, name):
    run_mapped(emu_lib, name)


def test_status_codes(emu_lib):
    run_status_codes(emu_lib)


@pytest.mark.parametrize("name", ["random200", "weak300", "symlower"])
def test_no_side_effects(emu_lib, name):
    run_no_side_effects(emu_lib, name)


@pytest.mark.parametrize("name", ["random200", "symlower"])
def test_reproducible(emu_lib, name):
    run_reproducible(emu_lib, name)


def test_plain_real_equivalent_factor(emu_lib):
    run_reproducible(emu_lib, "random200", env={"HIPMF_COMPLEX_PAIRS": "0"})


def test_perturbed_factor(emu_lib):
    run_perturbed(emu_lib)


def test_device_entry_point(emu_lib):
    run_device_entry(emu_lib, "random200")


def test_host_mirror(emu_lib):
    run_host_mirror(emu_lib)
