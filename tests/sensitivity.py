"""Tangent and adjoint sensitivities of the solve with respect to the matrix values: solver_hipmf_values_outer / _solve_tangent /
_solve_adjoint, their _device forms and the complex twin's three calls (kernels_sensitivity.hpp).  The cases and checks;
tests/test_sensitivity_cpu.py runs them on the CPU emulator of the HIP kernels, tests/test_sensitivity_gpu.py on the device (lib None).

Every case knows, for every value t the CALLER hands over, the matrix positions it stands for (`positions`): one for a general CSR entry,
two for an off-diagonal entry of symmetric-lower storage (also when the handle expands the matrix inside), the position of its CSR entry
for a COO triplet of a value map (duplicates of an entry all receive the entry's gradient).  The checks never look at the handle's own
storage.

Rules (none is a tuned number):
  outer     every value of grad against the sum over its positions and the columns, exact: the terms in integer arithmetic (a double is
            an integer times a power of two; exact_ints), the value as a fractions.Fraction, a sample of values per case also with one
            Fraction per term.  The kernel sums the columns of
            a position by ONE chain of fused multiply-adds, so with M = sum over positions and columns of |u_i| |w_j|
                |got - exact| <= (ncols + npos - 1) eps |alpha| M        (one eps M per extra addition between positions)
            and, when a second call accumulates into the first (beta = 1), one more rounding of the sum: + eps (|prior| + |alpha| M).
            Complex values: the same bound for the real and for the imaginary part (two fused multiply-adds per column and part,
            eps = 2 u).  alpha = +-1 and beta = 0, 1 are exact factors.
  solves    the exact componentwise backward error of EVERY column of dx (against A) and lambda (against A^T, complex: A^H), residual
            exact and rounded once (exact_residuals; its first column against exact_residual's Fractions): row i at most (p_i + 2) eps (|A| |y| + |rhs|)_i, p_i the entries of the row -- the measurement of
            tests/bordered.py.  The tangent's right-hand side db - dA x is formed on the device in double: x, dvalues and db are
            integers here, so that it is exact in any order and the test can restate it exactly; db is large enough that no entry of it
            is exactly zero (run_solves says why).
  gradient  grad_values by the outer rule against the RETURNED lambda and the given x.
  identity  |sum_c <g_c, dx_c> - <grad, dvalues> - sum_c <lambda_c, db_c>| <= 10 cond_2(A) eps sum_c |g_c|_2 |dx_c|_2 (complex: real
            parts), the inner products in extended precision, cond_2 by NumPy (matrix_and_cond: once per matrix and session).
  finite differences (mumps5): central differences of J = <c, A^{-1} b> with np.linalg.solve, h = 1e-6: truncation ~ h^2 and rounding
            ~ eps / h are both far below the 1e-6 (relative to max |grad|) asked for."""
import ctypes as C
import functools
import os
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

import test_solve_updated_cpu as SU
from russell_amd import problems as P
from extra_precise import EPS, SENTINEL, exact_residual, laplacian
from russell_amd.backend import ComplexHipmf, Hipmf
from test_transpose_solve_cpu import ERROR_HIPMF_INVALID_VALUE, ERROR_NEED_FACTORIZATION, ERROR_NULL_POINTER

ERROR_NEED_INITIALIZATION = 500000
LD = np.longdouble
NRHS = [1, 16, 17, 33]
PAD = 3  # ld = ndim + PAD, the padding filled with SENTINEL
REAL_CASES = ["mumps5", "chain257", "chain4097", "poisson", "poisson_lower", "saddle", "arrow300", "coo_dup", "saddle_mapped"]
COMPLEX_CASES = ["zgrid", "zgrid_mapped", "zgrid_lower"]
# Every matrix meets every check at every column count.  One exception, on the CPU emulator only, where a blocked solve of a long matrix
# takes seconds: there the SOLVE checks of the long matrices take 1 (the single-column paths) and 17 columns (a full block of sixteen
# and a block of one); the device file runs the full product.  The outer-product check runs the full product everywhere.
SHORT = ("mumps5", "chain257", "arrow300", "coo_dup", "zgrid_mapped")
CASE_COLUMNS = [(name, c) for name in REAL_CASES + COMPLEX_CASES for c in NRHS]
CASE_COLUMNS_EMULATED_SOLVES = [(name, c) for name, c in CASE_COLUMNS if name in SHORT or c in (1, 17)]
OLD_COUNTERS = [k for k, v in Hipmf.COUNTERS.items() if v <= 46]


class Case:
    """name, complex?, initialize arguments, the values the handle is factorised with (in the caller's order), whether they are the inputs
    of a value map, positions[t] = the (i, j) value t stands for, and A(values) -> the dense matrix"""

    def __init__(self, name, init, kw, values, positions, value_map=None):
        self.name, self.init, self.kw, self.values, self.positions, self.value_map = name, init, kw, values, positions, value_map
        self.n = init[0]
        self.complex = np.iscomplexobj(values)
        self.mapped = value_map is not None

    def dense(self, values):
        A = np.zeros((self.n, self.n), np.complex128 if self.complex else np.float64)
        t, ij = np.repeat(np.arange(len(self.positions)), [len(p) for p in self.positions]), np.array([q for p in self.positions for q in p])
        np.add.at(A, (ij[:, 0], ij[:, 1]), np.asarray(values)[t])
        return A

    def handle(self, lib, nstep=-1, factorize=True):
        s = (ComplexHipmf if self.complex else Hipmf)(lib) if lib else (ComplexHipmf if self.complex else Hipmf)()
        kw = dict(self.kw)
        if self.mapped:  # (the analysis sees the assembled entries, the factorisation the triplets)
            kw["values"] = self.csr_values(self.values)
        assert s.initialize(*self.init, refinement_nstep=nstep, **kw) == 0
        if self.mapped:
            assert s.set_value_map(*self.value_map) == 0
        if factorize:
            assert (s.factorize_mapped(self.values) if self.mapped else s.factorize(self.values)) == 0
        return s

    def csr_values(self, inputs):
        sp_, si = self.value_map
        return np.array([sum(inputs[si[q]] for q in range(sp_[k], sp_[k + 1])) for k in range(len(sp_) - 1)])


def _csr_positions(n, rp, ci, symmetric):
    out = []
    for i in range(n):
        for k in range(rp[i], rp[i + 1]):
            j = int(ci[k])
            out.append([(i, j)] if (not symmetric or i == j) else [(i, j), (j, i)])
    return out


def _triplets(n, rp, ci, values, seed):
    """the CSR entries as COO triplets with duplicates (one to three per entry, in shuffled order) whose sums are `values`"""
    rng = np.random.default_rng(seed)
    nnz = int(rp[n])
    count = rng.integers(1, 4, nnz)
    owner = rng.permutation(np.repeat(np.arange(nnz), count))  # triplet t belongs to CSR entry owner[t]
    order = np.argsort(owner, kind="stable")
    seg_ptr = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    seg_idx = order.astype(np.int32)
    inputs = np.zeros(owner.size, values.dtype)
    for k in range(nnz):
        ts = seg_idx[seg_ptr[k]:seg_ptr[k + 1]]
        parts = rng.uniform(0.2, 1.0, ts.size)
        inputs[ts] = values[k] * parts / parts.sum()
    rows = np.repeat(np.arange(n), np.diff(rp))
    positions = [[(int(rows[owner[t]]), int(ci[owner[t]]))] for t in range(owner.size)]
    return inputs, (seg_ptr, seg_idx), positions


def _zgrid(nx, ny, symmetric, seed=3):
    """a complex shifted grid, (alpha + i beta) I - J on a 2D mesh: J the 5-point stencil with complex couplings (symmetric: A = A^T)"""
    rng = np.random.default_rng(seed)
    L = sp.csr_matrix(laplacian(nx, ny)).astype(np.complex128)
    L.data = L.data * (1.0 + 0.2 * rng.uniform(-1, 1, L.nnz) + 0.2j * rng.uniform(-1, 1, L.nnz))
    if symmetric:
        L = sp.csr_matrix(sp.tril(L) + sp.tril(L, -1).T)
    A = sp.csr_matrix(L + (2.6811 + 3.0504j) * sp.identity(nx * ny))
    A.sort_indices()
    return A


@functools.lru_cache(None)
def cases():
    out = {}
    for name, (init, kw, values) in SU.matrices().items():
        if name in REAL_CASES:
            out[name] = Case(name, init, kw, np.array(values, float), _csr_positions(*init, bool(kw.get("general_symmetric"))))
    n = 300  # an arrow: the last row and the last column are full
    rng = np.random.default_rng(300)
    A = sp.lil_matrix((n, n))
    A.setdiag(rng.uniform(3.0, 4.0, n))
    A[n - 1, :] = rng.uniform(-1, 1, n) / 20
    A[:, n - 1] = rng.uniform(-1, 1, (n, 1)) / 20
    A[n - 1, n - 1] = 4.0
    A = sp.csr_matrix(A)
    A.sort_indices()
    init = (n, A.indptr.astype(np.int32), A.indices.astype(np.int32))
    out["arrow300"] = Case("arrow300", init, dict(values=A.data.copy()), A.data.copy(), _csr_positions(*init, False))
    # the saddle-point matrix as COO triplets of its lower triangle, with duplicates: the handle expands it inside, so that every
    # off-diagonal triplet feeds two slots of the handle's storage
    init, kw, values = SU.matrices()["saddle"]
    inputs, vmap, positions = _triplets(*init, np.array(values, float), seed=23)
    out["saddle_mapped"] = Case("saddle_mapped", init, dict(general_symmetric=True), inputs,
                                [p if p[0][0] == p[0][1] else [p[0], p[0][::-1]] for p in positions], vmap)
    n, rp, ci, v = P.poisson2d(12, 11)
    v = v * (1.0 + 0.1 * np.random.default_rng(12).uniform(-1, 1, v.size))
    inputs, vmap, positions = _triplets(n, rp, ci, v, seed=21)
    out["coo_dup"] = Case("coo_dup", (n, rp, ci), {}, inputs, positions, vmap)
    A = _zgrid(24, 22, False)
    init = (A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32))
    out["zgrid"] = Case("zgrid", init, dict(values=A.data.copy()), A.data.copy(), _csr_positions(*init, False))
    A = _zgrid(12, 11, False, seed=4)
    init = (A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32))
    inputs, vmap, positions = _triplets(*init, A.data, seed=22)
    out["zgrid_mapped"] = Case("zgrid_mapped", init, {}, inputs, positions, vmap)
    Lw = sp.csr_matrix(sp.tril(_zgrid(24, 22, True)))
    Lw.sort_indices()
    init = (Lw.shape[0], Lw.indptr.astype(np.int32), Lw.indices.astype(np.int32))
    out["zgrid_lower"] = Case("zgrid_lower", init, dict(general_symmetric=True, values=Lw.data.copy()), Lw.data.copy(), _csr_positions(*init, True))
    return out


@functools.lru_cache(None)
def matrix_and_cond(name):
    """(A, cond_2(A)); cond_2 = sqrt(lambda_max / lambda_min) of A^H A by np.linalg.eigvalsh: np.linalg.cond's number to a relative
    eps cond_2^2 (at most 1e-6 here, against the factor 10 of the rule) in a third of the time of its SVD"""
    A = cases()[name].dense(cases()[name].values)
    w = np.linalg.eigvalsh(A.conj().T @ A)
    return A, float(np.sqrt(w[-1] / w[0]))


# ---- operands ----

def padded(cols, n):
    """(ncols, n + PAD) with the columns in the first n places and SENTINEL behind them"""
    out = np.full((cols.shape[0], n + PAD), SENTINEL, cols.dtype)
    out[:, :n] = cols
    return out


def random_columns(case, ncols, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((ncols, case.n))
    return padded(c + 1j * rng.standard_normal((ncols, case.n)) if case.complex else c, case.n)


def cancelling_columns(case, ncols, seed):
    """u_c = a_c p, w_c = q with a = 1e8, 1, -1e8, -1, ...: the sum over the columns cancels to (nearly) nothing of its terms"""
    rng = np.random.default_rng(seed)
    a = np.array([[1e8, 1.0, -1e8, -1.0][c % 4] for c in range(ncols)])
    p, q = rng.uniform(0.5, 1.5, case.n), rng.uniform(0.5, 1.5, case.n)
    if case.complex:
        p, q = p * np.exp(2j * np.pi * rng.random(case.n)), q * np.exp(2j * np.pi * rng.random(case.n))
    return padded(a[:, None] * p[None, :], case.n), padded(np.repeat(q[None, :], ncols, 0), case.n)


def integer_columns(case, ncols, seed, span=4, offset=0):
    """small integers; with an offset every entry (complex: either part) is at least offset - span in magnitude, of either sign"""
    rng = np.random.default_rng(seed)
    draw = lambda: (rng.integers(-span, span + 1, (ncols, case.n)) + offset * rng.choice([-1, 1], (ncols, case.n))).astype(float)
    c = draw()
    return padded(c + 1j * draw() if case.complex else c, case.n)


def integer_values(case, seed, span=3):
    rng = np.random.default_rng(seed)
    v = rng.integers(-span, span + 1, case.values.size).astype(float)
    return v + 1j * rng.integers(-span, span + 1, case.values.size) if case.complex else v


# ---- the exact outer product ----
# Exact arithmetic without a Fraction per term: a double is an integer times a power of two, so an array of doubles is an array of
# Python integers (NumPy object arrays: exact, unbounded) times ONE power of two, products and sums of such arrays are exact, and a
# Fraction is made once per VALUE, for the comparison.

def exact_ints(a):
    """(object array m of Python ints, e) with a == m * 2**e exactly, elementwise"""
    a = np.asarray(a, np.float64)
    mant, ex = np.frexp(a)
    m53 = (mant * 2.0 ** 53).astype(np.int64)  # (|mant| < 1 has 53 bits: exact)
    e = int(ex[a != 0].min()) - 53 if np.any(a != 0) else 0
    shift = np.where(a != 0, ex - 53 - e, 0)
    out = m53.astype(object)
    big = shift > 0
    if np.any(big):
        out[big] = out[big] * (2 ** shift[big].astype(object))
    return out, e


def scaled_fraction(m, e):
    return Fraction(int(m)) * Fraction(2) ** e


def exact_outer(case, U, W, conjugate_w=False):
    """per caller value: the exact sum over its positions and the columns -- integer arrays (re, im) and their power of two --, M = the
    same sum of |u_i| |w_j| (extended precision, nudged up: never below the exact sum), and the number of positions"""
    n = case.n
    npos = np.array([len(p) for p in case.positions])
    first = np.array([p[0] for p in case.positions])
    second = np.array([p[1] if len(p) > 1 else p[0] for p in case.positions])
    assert npos.max() <= 2
    Uc, Wc = U[:, :n], (np.conj(W[:, :n]) if conjugate_w else W[:, :n])
    ui, eu = exact_ints(np.stack([Uc.real, Uc.imag]))
    wi, ew = exact_ints(np.stack([Wc.real, Wc.imag]))
    au, aw = np.abs(Uc).astype(LD), np.abs(Wc).astype(LD)
    re, im, M = np.zeros(npos.size, object), np.zeros(npos.size, object), np.zeros(npos.size, LD)
    for pos, sel in ((first, npos > 0), (second, npos > 1)):
        I, J = pos[sel, 0], pos[sel, 1]
        re[sel] += (ui[0][:, I] * wi[0][:, J] - ui[1][:, I] * wi[1][:, J]).sum(0)
        if case.complex:
            im[sel] += (ui[0][:, I] * wi[1][:, J] + ui[1][:, I] * wi[0][:, J]).sum(0)
        M[sel] += (au[:, I] * aw[:, J]).sum(0)
    return re, im, eu + ew, M.astype(np.float64) * (1.0 + 1e-15), npos


def check_outer(case, got, exact, ncols, alpha, prior=None, label=""):
    """the outer rule; prior: the array the call accumulated into with beta = 1 (None: beta = 0)"""
    assert np.all(np.isfinite(got)), label
    re, im, e, M, npos = exact
    worst = 0.0
    fa = Fraction(alpha)
    for part, ex in ((np.real, re), (np.imag, im)) if case.complex else ((np.real, re),):
        g = part(got)
        pr = None if prior is None else part(prior)
        for t in range(g.size):
            want = fa * scaled_fraction(ex[t], e)
            b = (ncols + npos[t] - 1) * EPS * abs(alpha) * M[t]
            if pr is not None:
                want += Fraction(float(pr[t]))
                b += EPS * (abs(float(pr[t])) + abs(alpha) * M[t])
            err = abs(float(Fraction(float(g[t])) - want))
            assert err <= b, (label, t, err, b)
            worst = max(worst, err / b if b > 0 else 0.0)
    print("%s %s ncols=%d: worst error / bound = %.3f" % (case.name, label, ncols, worst))


def exact_outer_by_fractions(case, U, W, t):
    """value t of exact_outer the slow way, one Fraction per term: (re, im)"""
    f = lambda v: Fraction(float(v))
    re = im = Fraction(0)
    for i, j in case.positions[t]:
        for c in range(U.shape[0]):
            u, w = complex(U[c, i]), complex(W[c, j])
            re += f(u.real) * f(w.real) - f(u.imag) * f(w.imag)
            im += f(u.real) * f(w.imag) + f(u.imag) * f(w.real)
    return re, im


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- check 2: the outer product against exact arithmetic ----

def run_outer(lib, name, ncols):
    case = cases()[name]
    s = case.handle(lib, factorize=False)  # (the primitive needs initialize only)
    kind = dict(mapped=case.mapped)
    try:
        nan = np.full(case.values.size, np.nan, case.values.dtype)
        U, W = random_columns(case, ncols, 1), random_columns(case, ncols, 2)
        ex = exact_outer(case, U, W)
        g1 = s.values_outer(U, W, grad=nan.copy(), **kind)  # beta = 0: the NaNs are not read
        check_outer(case, g1, ex, ncols, 1.0, label="random")
        for t in sorted(set(np.random.default_rng(ncols).integers(0, case.values.size, 4)) | {case.values.size - 1}):  # the reference against Fractions per term
            assert (scaled_fraction(ex[0][t], ex[2]), scaled_fraction(ex[1][t], ex[2])) == exact_outer_by_fractions(case, U, W, t)
        Uc, Wc = cancelling_columns(case, ncols, 3)
        exc = exact_outer(case, Uc, Wc)
        g2 = s.values_outer(Uc, Wc, alpha=-1.0, grad=nan.copy(), **kind)
        check_outer(case, g2, exc, ncols, -1.0, label="cancelling, alpha = -1")
        g3 = s.values_outer(Uc, Wc, alpha=-1.0, beta=1.0, grad=g1.copy(), **kind)  # beta = 1: accumulated into the first call's result
        check_outer(case, g3, exc, ncols, -1.0, prior=g1, label="accumulated")
        if case.complex:
            g4 = s.values_outer(U, W, grad=nan.copy(), conjugate_w=True, **kind)
            check_outer(case, g4, exact_outer(case, U, W, conjugate_w=True), ncols, 1.0, label="conjugated w")
        assert bits_equal(U[:, case.n:], np.full((ncols, PAD), SENTINEL, U.dtype)) and s.counter("sens_outer_columns") == (4 if case.complex else 3) * ncols
    finally:
        s.close()


# ---- check 3: the same bits ----

class DeviceArrays:
    def __init__(self, s):
        self.s, self.ptrs = s, []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.s.dev_alloc(max(a.nbytes, 8))
        self.ptrs.append(p)
        self.s.h2d(p, a)
        return p

    def get(self, p, like):
        out = np.zeros_like(like)
        self.s.d2h(out, p)
        return out

    def free(self):
        for p in self.ptrs:
            self.s.dev_free(p)


def run_reproducible(lib, name):
    """host and device forms, two calls, and the gradient of solve_adjoint against values_outer on its own columns: the same bits"""
    case = cases()[name]
    nrhs = 17  # two blocks of the solve, one chain of the product
    # (the tangent pair and the in-place adjoint of a long matrix on the emulator, where a blocked solve takes seconds: two columns)
    nt = 2 if lib and name not in SHORT and not case.complex else nrhs
    n, ld = case.n, case.n + PAD
    s = case.handle(lib)
    dev = DeviceArrays(s) if not case.complex else None
    kind = dict(mapped=case.mapped)
    try:
        U, W = random_columns(case, nrhs, 5), random_columns(case, nrhs, 6)
        g0 = np.random.default_rng(7).standard_normal(case.values.size) * (1 + 1j if case.complex else 1)
        a = s.values_outer(U, W, alpha=0.5, beta=2.0, grad=g0.copy(), **kind)
        b = s.values_outer(U, W, alpha=0.5, beta=2.0, grad=g0.copy(), **kind)
        assert bits_equal(a, b)
        G, X = random_columns(case, nrhs, 8), random_columns(case, nrhs, 9)
        lam, gr = s.solve_adjoint(G, X, beta=1.0, grad=g0.copy(), **kind)
        if case.complex:  # (the real handles repeat the call in its device form below)
            lam2, gr2 = s.solve_adjoint(G, X, beta=1.0, grad=g0.copy(), **kind)
            assert bits_equal(lam, lam2) and bits_equal(gr, gr2)
        # the 16-column blocks of the solve do not cut the chain: ONE outer product over the returned columns gives the gradient
        again = s.values_outer(lam, X, alpha=-1.0, beta=1.0, grad=g0.copy(), conjugate_w=True, **kind) if case.complex else s.values_outer(
            lam, X, alpha=-1.0, beta=1.0, grad=g0.copy(), **kind)
        assert bits_equal(gr, again)
        DV, DB = integer_values(case, 10), integer_columns(case, nrhs, 11)
        dx = s.solve_tangent(X[:nt], DV, DB[:nt], **kind)
        if case.complex:
            assert bits_equal(dx, s.solve_tangent(X, DV, DB, **kind))
        if dev:
            d_u, d_w, d_g = dev.put(U), dev.put(W), dev.put(g0)
            s.values_outer_device(d_g, d_u, d_w, nrhs, alpha=0.5, beta=2.0, ldu=ld, ldw=ld, **kind)
            assert bits_equal(dev.get(d_g, g0), a)
            d_G, d_X, d_lam, d_gr = dev.put(G), dev.put(X), dev.put(np.full_like(G, SENTINEL)), dev.put(g0)
            s.solve_adjoint_device(d_lam, d_gr, d_X, d_G, nrhs, beta=1.0, ld=ld, **kind)
            lam_d = dev.get(d_lam, G)
            assert bits_equal(lam_d[:, :n], lam[:, :n]) and np.all(lam_d[:, n:] == SENTINEL) and bits_equal(dev.get(d_gr, g0), gr)
            s.solve_adjoint_device(d_G, None, None, d_G, nt, ld=ld)  # lambda over g, no gradient
            lam_t = lam if nt == nrhs else s.solve_adjoint(G[:nt], want_grad=False)[0]
            assert bits_equal(dev.get(d_G, G)[:nt, :n], lam_t[:, :n]) and bits_equal(dev.get(d_G, G)[nt:], G[nt:])
            d_dv, d_db, d_dx = dev.put(DV), dev.put(DB), dev.put(np.full_like(X, SENTINEL))
            s.solve_tangent_device(d_dx, d_X, d_dv, d_db, nt, ld=ld, **kind)
            dx_d = dev.get(d_dx, X)
            assert bits_equal(dx_d[:nt, :n], dx[:, :n]) and np.all(dx_d[:nt, n:] == SENTINEL) and np.all(dx_d[nt:] == SENTINEL)
    finally:
        if dev:
            dev.free()
        s.close()


# ---- check 4: the two solves ----

def real_equivalent(A):
    """[a -b; b a] per entry, rows / columns 2 k, 2 k + 1"""
    A = sp.coo_matrix(A)
    r, c, v = A.row, A.col, A.data
    return sp.csr_matrix((np.concatenate([v.real, -v.imag, v.imag, v.real]), (np.concatenate([2 * r, 2 * r, 2 * r + 1, 2 * r + 1]),
                                                                              np.concatenate([2 * c, 2 * c + 1, 2 * c, 2 * c + 1]))), shape=(2 * A.shape[0], 2 * A.shape[1]))


def as_real(v):
    """interleaved (re, im) along the last axis"""
    return np.ascontiguousarray(v).view(np.float64) if np.iscomplexobj(v) else v


def exact_residuals(M, B, Y):
    """B - Y M^T for the columns held in the rows of B and Y, exactly (integer arithmetic, see exact_ints), every entry rounded once:
    exact_residual of tests/extra_precise.py for all columns at once"""
    M = sp.csr_matrix(M)
    assert np.all(np.diff(M.indptr) > 0)
    (am, ea), (ym, ey), (bm, eb) = exact_ints(M.data), exact_ints(Y), exact_ints(B)
    e = min(eb, ea + ey)
    prod = np.add.reduceat(am[None, :] * ym[:, M.indices], M.indptr[:-1], axis=1)
    r = bm * (2 ** (eb - e)) - prod * (2 ** (ea + ey - e))
    return np.ldexp(r.astype(np.float64), e)  # (int -> double rounds once, to nearest; the power of two is exact)


def backward_error_ratios(M, B, Y):
    """per column: max over the rows of the exact componentwise backward error of M y = b over (p_i + 2) eps"""
    M = sp.csr_matrix(M)
    R = exact_residuals(M, B, Y)
    assert np.array_equal(R[0], exact_residual(M, B[0], Y[0]))  # the reference against Fractions per term
    den = np.abs(Y) @ abs(M).T + np.abs(B)
    p = np.diff(M.indptr)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(den > 0, np.abs(R) / den, np.where(np.abs(R) > 0, np.inf, 0.0))
    return np.max(q / ((p + 2) * EPS)[None, :], axis=1)


def run_solves(lib, name, nrhs):
    case = cases()[name]
    n = case.n
    A, cond = matrix_and_cond(name)
    s = case.handle(lib)
    kind = dict(mapped=case.mapped)
    try:
        # db lies above any |dA x|_i (at most 24 x the entries of a row, 300 in the arrow): no entry of the right-hand side is exactly zero.
        # A zero there, in a row whose solution entries are zero in exact arithmetic, turns the componentwise measure into 0 / 0: any
        # rounding residue of the solve counts 1 (seen on the device: the 5 x 5 matrix, one column of 33) -- the rows Arioli, Demmel & Duff
        # measure differently, and not what this check is about
        X, DB, DV = integer_columns(case, nrhs, 31), integer_columns(case, nrhs, 32, offset=10000), integer_values(case, 33)
        G = random_columns(case, nrhs, 34)
        dA = case.dense(DV)
        R = DB[:, :n] - X[:, :n] @ dA.T  # (integers: exact in double, in any order of summation)
        assert np.all(as_real(np.ascontiguousarray(R)) != 0)
        dx_out = np.full_like(X, SENTINEL)
        dx = s.solve_tangent(X, DV, DB, dx=dx_out, **kind)
        lam, grad = s.solve_adjoint(G, X, lam=np.full_like(G, SENTINEL), **kind)
        assert np.all(dx[:, n:] == SENTINEL) and np.all(lam[:, n:] == SENTINEL)
        # backward errors of EVERY column, exactly
        Ms = sp.csr_matrix(real_equivalent(A) if case.complex else A)
        MsT = sp.csr_matrix(real_equivalent(A.conj().T) if case.complex else A.T)
        wt = backward_error_ratios(Ms, as_real(np.ascontiguousarray(R)), as_real(np.ascontiguousarray(dx[:, :n])))
        wa = backward_error_ratios(MsT, as_real(np.ascontiguousarray(G[:, :n])), as_real(np.ascontiguousarray(lam[:, :n])))
        print("%s nrhs=%d: backward error / ((p + 2) eps), worst column: tangent %.3f (column %d), adjoint %.3f (column %d)" % (name, nrhs, wt.max(), wt.argmax(), wa.max(), wa.argmax()))
        assert np.all(wt <= 1.0) and np.all(wa <= 1.0), (wt, wa)
        # the gradient is the outer product of the call's own lambda with x
        check_outer(case, grad, exact_outer(case, lam, X, conjugate_w=True), nrhs, -1.0, label="gradient")
        # the adjoint identity
        dot = (lambda a, b: (np.conj(a).astype(np.clongdouble) * b.astype(np.clongdouble)).sum().real) if case.complex else (lambda a, b: (a.astype(LD) * b.astype(LD)).sum())
        lhs = dot(G[:, :n], dx[:, :n])
        rhs = dot(grad, DV) + dot(lam[:, :n], DB[:, :n])
        scale = float(sum(np.linalg.norm(G[c, :n]) * np.linalg.norm(dx[c, :n]) for c in range(nrhs)))
        print("%s nrhs=%d: identity %.17g against %.17g, difference / bound = %.3e (cond_2 %.3e)" % (name, nrhs, lhs, rhs, abs(float(lhs - rhs)) / (10 * cond * EPS * scale), cond))
        assert abs(float(lhs - rhs)) <= 10 * cond * EPS * scale
        if nrhs > 1:
            return
        # db = None is db = 0
        dx0 = s.solve_tangent(X, DV, None, **kind)
        dxz = s.solve_tangent(X, DV, np.zeros_like(DB), **kind)
        assert bits_equal(dx0, dxz)
    finally:
        s.close()


def run_finite_differences(lib):
    case = cases()["mumps5"]
    n, h = case.n, 1e-6
    rng = np.random.default_rng(41)
    b, c = rng.standard_normal(n), rng.standard_normal(n)
    s = case.handle(lib)
    try:
        x = s.solve(b)
        lam, grad = s.solve_adjoint(c, x)
        J = lambda v, rhs: float(c @ np.linalg.solve(case.dense(v), rhs))
        fd = np.zeros(case.values.size)
        for t in range(fd.size):
            e = np.zeros(fd.size)
            e[t] = h
            fd[t] = (J(case.values + e, b) - J(case.values - e, b)) / (2 * h)
        fdb = np.array([(J(case.values, b + h * np.eye(n)[i]) - J(case.values, b - h * np.eye(n)[i])) / (2 * h) for i in range(n)])
        print("finite differences: grad %.3e, lambda %.3e (relative)" % (np.max(np.abs(fd - grad)) / np.max(np.abs(grad)), np.max(np.abs(fdb - lam)) / np.max(np.abs(lam))))
        assert np.max(np.abs(fd - grad)) <= 1e-6 * np.max(np.abs(grad))
        assert np.max(np.abs(fdb - lam)) <= 1e-6 * np.max(np.abs(lam))
        # the tangent against the same differences: dJ along (dvalues, db)
        dv, db = rng.standard_normal(fd.size), rng.standard_normal(n)
        dx = s.solve_tangent(x, dv, db)
        assert abs(c @ dx - (fd @ dv + fdb @ db)) <= 1e-6 * (np.max(np.abs(grad)) * np.abs(dv).sum() + np.max(np.abs(lam)) * np.abs(db).sum())
    finally:
        s.close()


# ---- check 5: life cycle and side effects ----

def determinant_state(s, case):
    """what the determinant is made of: the complex handle's determinant; the real handle's pivots (the fourth factor buffer), whose
    product it is, bit for bit"""
    if case.complex:
        return np.array(s.determinant())
    ptr, nbytes = s.factor_buffers()[3]
    piv = np.zeros(nbytes // 8)
    s.d2h(piv, ptr)
    return piv


def run_side_effects(lib, name, nrhs=3):
    case = cases()[name]
    n = case.n
    s = case.handle(lib)
    kind = dict(mapped=case.mapped)
    try:
        F = random_columns(case, nrhs, 51)[:, :n].copy()
        X, G, DV = random_columns(case, nrhs, 52), random_columns(case, nrhs, 53), integer_values(case, 54)
        # (the complex wrapper has no solve_many and no statistics)
        solves = (lambda: (s.solve(F[0]), s.solve_transpose(F[0]), s.solve_transpose(F[0], conjugate=False))) if case.complex else (
            lambda: (s.solve(F[0]), s.solve_transpose(F[0]), s.solve_many(F)))
        det0 = determinant_state(s, case)
        fixed = () if case.complex else ("n_perturbed", "factor_launches", "solve_launches", "acc_factor_count", "acc_tri_count", "residual_inf", "refinement_steps")
        snapshot = lambda: ([s.counter(k) for k in OLD_COUNTERS], {q: s.stats()[q] for q in fixed})
        assert s.counter("sens_outer_columns") == 0 and s.counter("sens_outer_us") == 0
        r0, k0 = solves(), snapshot()
        r1, k1 = solves(), snapshot()  # (what a repetition without sensitivity calls changes)
        s.values_outer(X, G, **kind)
        assert s.counter("sens_outer_columns") == nrhs and s.counter("sens_outer_us") >= 0
        dx = s.solve_tangent(X, DV, None, **kind)
        lam, grad = s.solve_adjoint(G, X, **kind)
        assert s.counter("sens_outer_columns") == 2 * nrhs
        # lambda over g; the solve alone
        buf = G.copy()
        lam_in_place, none = s.solve_adjoint(buf, want_grad=False, lam=buf)
        assert none is None and lam_in_place is buf and bits_equal(buf[:, :n], lam[:, :n]) and np.all(buf[:, n:] == SENTINEL) and s.counter("sens_outer_columns") == 2 * nrhs
        lam1, grad1 = s.solve_adjoint(G[0], X[0], **kind)  # one column: the single transposed solve
        assert lam1.shape == (n + PAD,) and np.all(np.isfinite(grad1))
        assert snapshot() == k1  # nothing of the ordinary or of the transposed solves has moved
        assert bits_equal(determinant_state(s, case), det0)
        r2, k2 = solves(), snapshot()
        for u, v in zip(r0 + r0, r1 + r2):
            assert bits_equal(u, v)
        (c0, s0), (c1, s1) = k0, k1
        assert k2 == ([b + (b - a) for a, b in zip(c0, c1)], {q: s1[q] + (s1[q] - s0[q]) for q in fixed})
    finally:
        s.close()


def run_status_codes(lib):
    case = cases()["coo_dup"]
    n, nnz_in = case.n, case.values.size
    s = Hipmf(lib) if lib else Hipmf()
    L = s.lib
    u, g = np.ones((2, n)), np.zeros(nnz_in)
    p = lambda a: a.ctypes.data
    try:
        outer = lambda h, gr, uu, ww, nc=2, lu=n, lw=n, mapped=0: L.solver_hipmf_values_outer(h, gr, uu, ww, nc, lu, lw, 1.0, 0.0, mapped)
        tangent = lambda h, dx, x, dv, nr=2, ld=n, mapped=0: L.solver_hipmf_solve_tangent(h, dx, x, dv, None, nr, ld, mapped)
        adjoint = lambda h, lam, gr, x, gg, nr=2, ld=n, mapped=0: L.solver_hipmf_solve_adjoint(h, lam, gr, x, gg, nr, ld, 0.0, mapped)
        assert outer(None, p(g), p(u), p(u)) == ERROR_NULL_POINTER and outer(s.h, None, p(u), p(u)) == ERROR_NULL_POINTER
        assert outer(s.h, p(g), None, p(u)) == ERROR_NULL_POINTER and outer(s.h, p(g), p(u), None) == ERROR_NULL_POINTER
        assert outer(s.h, p(g), p(u), p(u)) == ERROR_NEED_INITIALIZATION
        assert tangent(s.h, p(u), p(u), p(g)) == ERROR_NEED_INITIALIZATION and adjoint(s.h, p(u), p(g), p(u), p(u)) == ERROR_NEED_INITIALIZATION
        assert L.solver_hipmf_values_outer_device(s.h, None, None, None, 1, n, n, 1.0, 0.0, 0) == ERROR_NULL_POINTER
        assert s.initialize(*case.init, values=case.csr_values(case.values)) == 0
        gc = np.zeros(s.nnz)
        assert outer(s.h, p(gc), p(u), p(u)) == 0  # initialize is enough for the primitive
        assert outer(s.h, p(g), p(u), p(u), mapped=1) == ERROR_HIPMF_INVALID_VALUE  # no map yet
        assert tangent(s.h, p(u), p(u), p(gc)) == ERROR_NEED_FACTORIZATION and adjoint(s.h, p(u), p(gc), p(u), p(u)) == ERROR_NEED_FACTORIZATION
        assert L.solver_hipmf_solve_tangent_device(s.h, p(u), p(u), p(gc), None, 2, n, 0) == ERROR_NEED_FACTORIZATION
        assert L.solver_hipmf_solve_adjoint_device(s.h, p(u), None, None, p(u), 2, n, 0.0, 0) == ERROR_NEED_FACTORIZATION
        assert s.factorize(case.csr_values(case.values)) == 0
        assert tangent(s.h, p(u), p(u), p(g), mapped=1) == ERROR_HIPMF_INVALID_VALUE and adjoint(s.h, p(u), p(g), p(u), p(u), mapped=1) == ERROR_HIPMF_INVALID_VALUE
        assert s.set_value_map(*case.value_map) == 0
        out = np.zeros((2, n))
        assert outer(s.h, p(g), p(u), p(u), mapped=1) == 0 and tangent(s.h, p(out), p(u), p(g), mapped=1) == 0
        for bad in (dict(nc=0), dict(lu=n - 1), dict(lw=n - 1)):
            assert outer(s.h, p(gc), p(u), p(u), **bad) == ERROR_HIPMF_INVALID_VALUE, bad
        for bad in (dict(nr=0), dict(ld=n - 1)):
            assert tangent(s.h, p(u), p(u), p(gc), **bad) == ERROR_HIPMF_INVALID_VALUE, bad
            assert adjoint(s.h, p(u), p(gc), p(u), p(u), **bad) == ERROR_HIPMF_INVALID_VALUE, bad
        assert tangent(s.h, None, p(u), p(gc)) == ERROR_NULL_POINTER and tangent(s.h, p(u), None, p(gc)) == ERROR_NULL_POINTER
        assert tangent(s.h, p(u), p(u), None) == ERROR_NULL_POINTER and tangent(None, p(u), p(u), p(gc)) == ERROR_NULL_POINTER
        assert adjoint(s.h, None, p(gc), p(u), p(u)) == ERROR_NULL_POINTER and adjoint(s.h, p(u), p(gc), p(u), None) == ERROR_NULL_POINTER
        assert adjoint(s.h, p(u), p(gc), None, p(u)) == ERROR_NULL_POINTER  # a gradient needs x
        assert adjoint(s.h, p(out), None, None, p(u)) == 0  # ... the solve alone does not
        # a second map replaces the first: the gradient follows it
        ident = (np.arange(s.nnz + 1, dtype=np.int32), np.arange(s.nnz, dtype=np.int32))
        assert s.set_value_map(*ident) == 0
        a = s.values_outer(u, u, mapped=True)
        assert a.size == s.nnz and bits_equal(a, s.values_outer(u, u))
    finally:
        s.close()
    # the complex handle
    zc = cases()["zgrid_mapped"]
    z = ComplexHipmf(lib) if lib else ComplexHipmf()
    L = z.lib
    n = zc.n
    uz, gz = np.ones((2, n), np.complex128), np.zeros(zc.values.size, np.complex128)
    try:
        zouter = lambda h, gr, uu, ww, nc=2, lu=n, lw=n, mapped=0, cj=0: L.complex_solver_hipmf_values_outer(h, gr, uu, ww, nc, lu, lw, 1.0, 0.0, mapped, cj)
        ztangent = lambda h, dx, x, dv, nr=2, ld=n, mapped=0: L.complex_solver_hipmf_solve_tangent(h, dx, x, dv, None, nr, ld, mapped)
        zadjoint = lambda h, lam, gr, x, gg, nr=2, ld=n, mapped=0: L.complex_solver_hipmf_solve_adjoint(h, lam, gr, x, gg, nr, ld, 0.0, mapped)
        assert zouter(None, p(gz), p(uz), p(uz)) == ERROR_NULL_POINTER and zouter(z.h, p(gz), None, p(uz)) == ERROR_NULL_POINTER
        assert zouter(z.h, p(gz), p(uz), p(uz)) == ERROR_NEED_INITIALIZATION and ztangent(z.h, p(uz), p(uz), p(gz)) == ERROR_NEED_INITIALIZATION
        assert zadjoint(z.h, p(uz), p(gz), p(uz), p(uz)) == ERROR_NEED_INITIALIZATION
        assert z.initialize(*zc.init, values=zc.csr_values(zc.values)) == 0
        gzc = np.zeros(z.nnz, np.complex128)
        assert zouter(z.h, p(gzc), p(uz), p(uz)) == 0
        assert zouter(z.h, p(gz), p(uz), p(uz), mapped=1) == ERROR_HIPMF_INVALID_VALUE  # mapped has to name the map in force
        assert zouter(z.h, p(gzc), p(uz), p(uz), cj=2) == ERROR_HIPMF_INVALID_VALUE and zouter(z.h, p(gzc), p(uz), p(uz), nc=0) == ERROR_HIPMF_INVALID_VALUE
        assert zouter(z.h, p(gzc), p(uz), p(uz), lu=n - 1) == ERROR_HIPMF_INVALID_VALUE
        assert ztangent(z.h, p(uz), p(uz), p(gzc)) == ERROR_NEED_FACTORIZATION and zadjoint(z.h, p(uz), p(gzc), p(uz), p(uz)) == ERROR_NEED_FACTORIZATION
        assert z.set_value_map(*zc.value_map) == 0 and z.factorize_mapped(zc.values) == 0
        assert zouter(z.h, p(gzc), p(uz), p(uz)) == ERROR_HIPMF_INVALID_VALUE and zouter(z.h, p(gz), p(uz), p(uz), mapped=1) == 0
        outz = np.zeros((2, n), np.complex128)
        assert ztangent(z.h, p(outz), p(uz), p(gz), mapped=1) == 0 and ztangent(z.h, p(uz), p(uz), p(gz), mapped=0) == ERROR_HIPMF_INVALID_VALUE
        assert ztangent(z.h, p(uz), p(uz), p(gz), nr=0, mapped=1) == ERROR_HIPMF_INVALID_VALUE and zadjoint(z.h, p(uz), p(gz), p(uz), p(uz), ld=n - 1, mapped=1) == ERROR_HIPMF_INVALID_VALUE
        assert zadjoint(z.h, p(outz), None, None, p(uz)) == 0 and zadjoint(z.h, p(uz), p(gz), None, p(uz), mapped=1) == ERROR_NULL_POINTER
        assert z.counter("sens_outer_columns") == 4
    finally:
        z.close()


# ---- check 1: exports ----

def check_exports(lib_path):
    from russell_amd import _capi

    raw = C.CDLL(lib_path or _capi.DEFAULT_LIB)
    names = ("solver_hipmf_values_outer", "solver_hipmf_values_outer_device", "solver_hipmf_solve_tangent", "solver_hipmf_solve_tangent_device",
             "solver_hipmf_solve_adjoint", "solver_hipmf_solve_adjoint_device", "complex_solver_hipmf_values_outer", "complex_solver_hipmf_solve_tangent",
             "complex_solver_hipmf_solve_adjoint")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "russell_hipmf.h")).read()
    for name in names:
        assert hasattr(raw, name), name
        assert name in _capi.SYMBOLS and name + "(" in header, name
    for name, num in (("SENS_OUTER_COLUMNS", 47), ("SENS_OUTER_US", 48)):
        assert "#define HIPMF_COUNTER_%s %d" % (name, num) in header
        assert Hipmf.COUNTERS[name.lower()] == num
