"""Cases of the transposed bordered solve on the kept factor (solver_hipmf_solve_bordered_transpose and its _device form,
kernels_border.hpp), shared by tests/test_bordered_transpose_cpu.py (the CPU emulator of the HIP kernels) and
tests/test_bordered_transpose_gpu.py (lib None = the product build).

    [ A^T  C   ] [y]   [p]
    [ B^T  D^T ] [w] = [q]      M^T, M = the assembled (n + k) matrix of tests/bordered.py

The borders, the right-hand sides, the assembled matrix, the comparison solution (SuperLU on the assembled matrix plus one step) and the
exact measurement (fractions.Fraction, rounded once) are those of tests/bordered.py and tests/extra_precise.py, imported.  The bounds per
column are check_column's of the plain form, on M^T: state 0, steps <= the restatement's + 1, exact componentwise backward error of row i
<= (p_i + 2) eps, forward error <= max(10 x the comparison's, max(10, sqrt(n + k)) eps) under the asserted premise cond(M^T) eps <= 1e-3.

The matrices are UNSYMMETRIC, or M^T could not be told from M: R A Cc with R = diag(r), Cc = diag(c), r and c seeded and uniform in
(0.5, 2), on the matrices of tests/bordered.py (the scalings keep the folds singular to the same order); "upat483" also drops seeded
strict upper entries of every third row, so the pattern of A^T is not a relabelling of A's.  "biharm300_lower" is taken as it is: the
handle where A^T = A, with B != C.  border() and right_hand_sides() depend on the matrix through n alone and are called with the name of
the unscaled matrix (BASE).

The NumPy restatement (RestatementT): SuperLU of A with trans='T' as the pass pair, V = A^{-T} C, S^T = D^T - B^T V, the same stopping
rule.  With exact=True its residual is the Fraction one rounded once -- what the kernels compute.

"State 0 for every column" is a condition on the inputs.  Before the seeds of the scalings (SCALING_SEED) were fixed, the restatement
with the exact residual (RestatementT.solve(..., exact=True)) ran on the CPU on every (matrix, k, column) the tests below use, q = NULL
variants included: 178 columns.  All of them end in state 0 within four steps (at most two were needed) with the first seeds tried,
1 .. 5 in the order of SCALING_SEED: 0 candidates were discarded."""
import ctypes as C
import functools
import os

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import bordered as B
from bordered import assembled, border, comparison, exact_errors, right_hand_sides
from extra_precise import EPS, ERROR_NEED_INITIALIZATION, SENTINEL, TR_COUNTERS, _new, exact_residual, floor_bound, handle, lu_of
from russell_amd.backend import Hipmf
from test_transpose_solve_cpu import ERROR_HIPMF_INVALID_VALUE, ERROR_NEED_FACTORIZATION, ERROR_NULL_POINTER

K_SHAPES = [1, 3, 15, 16, 17, 33, 64]
NRHS_SHAPES = [1, 3, 4, 5, 15, 16, 17, 33]  # (3, 4, 5: around the four-column tile of k_border_residual_nt)
BASE = {"ulap483": "lap483", "ulap4087": "lap4087", "ufold1e-6": "fold1e-6", "ufold1e-10": "fold1e-10", "upat483": "lap483", "biharm300_lower": "biharm300_lower"}
SCALING_SEED = {"ulap483": 1, "ulap4087": 2, "ufold1e-6": 3, "ufold1e-10": 4, "upat483": 5}
BORDER_COUNTERS = ("border_columns", "bordered_steps", "bordered_blocks")
T_COUNTERS = ("bordered_transposed_steps", "bordered_transposed_blocks", "border_transposed_bytes")


# ---- matrices ----

@functools.lru_cache(None)
def matrix(name):
    """name -> (initialize arguments, keyword arguments, values in the handle's CSR order, the full matrix (scipy CSR))"""
    if name == "biharm300_lower":
        return B.matrix(name)
    A0 = B.matrix(BASE[name])[3]
    n = A0.shape[0]
    rng = np.random.default_rng(SCALING_SEED[name])
    r, c = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n)
    A = sp.csr_matrix(sp.diags(r) @ A0 @ sp.diags(c))
    if name == "upat483":
        A = A.tocoo()
        drop = (A.row % 3 == 0) & (A.col > A.row) & (rng.uniform(0, 1, A.nnz) < 0.5)
        assert drop.any()
        A = sp.csr_matrix((A.data[~drop], (A.row[~drop], A.col[~drop])), shape=(n, n))
        assert (abs(A) > 0).astype(int).T.tocsr().nnz == A.nnz and ((abs(A) > 0) != (abs(A) > 0).T).nnz > 0  # (an unsymmetric pattern)
    A.sort_indices()
    assert abs(A - A.T).max() > 0.1
    return (n, A.indptr.astype(np.int32), A.indices.astype(np.int32)), dict(values=A.data.astype(float)), A.data.astype(float), A


def border_of(name, k):
    return border(BASE[name], k)


def rhs_of(name, k, nrhs):
    """(P, Q): the rows are the right-hand sides of the first n and of the last k rows"""
    return right_hand_sides(BASE[name], k, nrhs)


@functools.lru_cache(None)
def assembled_t(name, k):
    Bm, Cm, D = border_of(name, k)
    Mt = sp.csr_matrix(assembled(matrix(name)[3], Bm, Cm, D).T)
    Mt.sort_indices()
    return Mt


# ---- the NumPy restatement, transposed ----

class RestatementT:
    def __init__(self, A, Bm, Cm, D, key):
        self.At, self.B, self.C, self.Dt = sp.csr_matrix(A.T), Bm, Cm, np.ascontiguousarray(D.T)
        self.lu = lu_of(A, key)
        self.V = self.lu.solve(Cm, trans="T")
        self.St = self.Dt - Bm.T @ self.V
        self.luSt = sla.lu_factor(self.St)
        self.Mt = sp.csr_matrix(assembled(A, Bm, Cm, D).T)

    def eliminate(self, rp, rq):
        y0 = self.lu.solve(rp, trans="T")
        w = sla.lu_solve(self.luSt, rq - self.B.T @ y0)
        return y0 - self.V @ w, w

    def measure(self, p, q, y, w, exact):
        """omega over the n + k rows of M^T as solve defines it, and the residual (exact: Fraction, rounded once)"""
        n = p.size
        omega, rp, rq = B.omega_of(self.At, self.C, self.B, self.Dt, p, q, y, w)
        if not exact:
            return omega, rp, rq
        rhs, sol = np.concatenate([p, q]), np.concatenate([y, w])
        r = exact_residual(self.Mt, rhs, sol)
        den = abs(self.Mt) @ np.abs(sol) + np.abs(rhs)
        with np.errstate(divide="ignore", invalid="ignore"):
            qq = np.where(den > 0, np.abs(r) / den, np.where(np.abs(r) > 0, 1.0, 0.0))
        return float(np.max(qq)), r[:n], r[n:]

    def solve(self, p, q, max_steps=0, exact=False):
        """(y, w, steps, state, omega before the first step)"""
        limit = max_steps if max_steps > 0 else 4
        y, w = self.eliminate(p, q)
        prev, steps, omega0 = np.inf, 0, None
        while True:
            omega, rp, rq = self.measure(p, q, y, w, exact)
            if steps == 0:
                omega0 = omega
            if steps > 0 and not omega < prev:
                return ys, ws, steps, 1, omega0
            if omega <= EPS:
                return y, w, steps, 0, omega0
            if steps > 0 and omega > 0.5 * prev:
                return y, w, steps, 1, omega0
            if steps >= limit:
                return y, w, steps, 2, omega0
            prev, ys, ws = omega, y, w
            dy, dw = self.eliminate(rp, rq)
            y, w, steps = y + dy, w + dw, steps + 1


@functools.lru_cache(None)
def restatement_t(name, k):
    Bm, Cm, D = border_of(name, k)
    return RestatementT(matrix(name)[3], Bm, Cm, D, "At:" + name)


@functools.lru_cache(None)
def cond_assembled_t(name, k):
    return float(np.linalg.cond(assembled_t(name, k).toarray(), np.inf))


def check_column(label, name, k, p, q, y, w, info, unstable=False):
    """check_column of tests/bordered.py on M^T; unstable: the assertions of the fold case beside them"""
    A = matrix(name)[3]
    n = A.shape[0]
    Mt = assembled_t(name, k)
    assert np.all(np.diff(Mt.indptr)[:n] == np.diff(sp.csr_matrix(A.T).indptr) + k) and np.all(np.diff(Mt.indptr)[n:] == n + k)  # (dense border entries included)
    key = "Mt:%s:%d" % (name, k)
    assert cond_assembled_t(name, k) * EPS <= 1e-3  # (the premise of the forward error)
    rhs, sol = np.concatenate([p, q]), np.concatenate([y, w])
    _, _, ref_steps, ref_state, ref_omega0 = restatement_t(name, k).solve(p, q)
    back, fe = exact_errors(Mt, rhs, sol, key)
    _, fe_cmp = exact_errors(Mt, rhs, comparison(Mt, rhs, key), key)
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


def bordered_handle(lib, name, k, nstep=0):
    init, kw, values, _ = matrix(name)
    s = handle(lib, init, kw, values, nstep=nstep)
    binfo, status = s.set_border(*border_of(name, k))
    assert status == 0, status
    return s, binfo


def same_bits(a, b):
    return all((u is None and v is None) or np.array_equal(u.view(np.uint64), v.view(np.uint64)) for u, v in zip(a, b))


# ---- case 1: exports ----

def check_exports(lib_path):
    from russell_amd import _capi

    raw = C.CDLL(lib_path or _capi.DEFAULT_LIB)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "russell_hipmf.h")).read()
    for name in ("solver_hipmf_solve_bordered_transpose", "solver_hipmf_solve_bordered_transpose_device"):
        assert hasattr(raw, name), name
        assert name in _capi.SYMBOLS and name + "(" in header, name
    for name, num in (("BORDERED_TRANSPOSED_STEPS", 49), ("BORDERED_TRANSPOSED_BLOCKS", 50), ("BORDER_TRANSPOSED_BYTES", 51)):
        assert "#define HIPMF_COUNTER_%s %d" % (name, num) in header
        assert Hipmf.COUNTERS[name.lower()] == num
    assert hasattr(Hipmf, "solve_bordered_transpose") and hasattr(Hipmf, "solve_bordered_transpose_device")


# ---- cases 2, 3, 10: shapes, with the padding sentinels ----

def run_shape(lib, name, k, nrhs, variants=False):
    n = matrix(name)[0][0]
    Pm, Qm = rhs_of(name, k, nrhs)
    ldx, ldz = n + 5, k + 2
    s, binfo = bordered_handle(lib, name, k)
    try:
        assert s.counter("border_transposed_bytes") == 0  # (nothing is held for the transposed side before the first call)
        Pp, Qp = np.full((nrhs, ldx), SENTINEL), np.full((nrhs, ldz), SENTINEL)
        Pp[:, :n], Qp[:, :k] = Pm, Qm
        Y, W = np.full((nrhs, ldx), SENTINEL), np.full((nrhs, ldz), SENTINEL)
        y, w, info = s.solve_bordered_transpose(Pp, Qp, ldx=ldx, ldz=ldz, y=Y, w=W)
        assert np.all(y[:, n:] == SENTINEL) and np.all(w[:, k:] == SENTINEL)  # (entries beyond n and k are not touched)
        kp = (k + 15) // 16 * 16
        assert s.counter("bordered_transposed_blocks") == (nrhs + 15) // 16 and s.counter("border_transposed_bytes") == 8 * (n * kp + kp * kp)
        assert [s.counter(c) for c in BORDER_COUNTERS] == [k, 0, 0]
        for c in range(nrhs):
            check_column("%s k %d column %d of %d" % (name, k, c, nrhs), name, k, Pm[c], Qm[c], y[c, :n], w[c, :k], info[c])
        if variants:
            # w = NULL: the same y, bit for bit
            Y2 = np.full((nrhs, ldx), SENTINEL)
            y2, w2, info2 = s.solve_bordered_transpose(Pp, Qp, ldx=ldx, ldz=ldz, y=Y2, want_w=False)
            assert w2 is None and np.array_equal(y2.view(np.uint64), y.view(np.uint64)) and np.array_equal(info2, info)
            # q = NULL: q = 0
            Y3, W3 = np.full((nrhs, ldx), SENTINEL), np.full((nrhs, ldz), SENTINEL)
            y3, w3, info3 = s.solve_bordered_transpose(Pp, None, ldx=ldx, ldz=ldz, y=Y3, w=W3)
            assert np.all(y3[:, n:] == SENTINEL) and np.all(w3[:, k:] == SENTINEL)
            for c in range(nrhs):
                check_column("%s k %d column %d, q = NULL" % (name, k, c), name, k, Pm[c], np.zeros(k), y3[c, :n], w3[c, :k], info3[c])
    finally:
        s.close()


# ---- case 4: near a fold ----

def run_fold(lib, name, k):
    condA = float(np.linalg.cond(matrix(name)[3].toarray(), np.inf))
    print("%s: cond_inf(A) %.3e, cond_inf(M^T) %.3e" % (name, condA, cond_assembled_t(name, k)))
    Pm, Qm = rhs_of(name, k, 1)
    s, _ = bordered_handle(lib, name, k)
    try:
        y, w, info = s.solve_bordered_transpose(Pm[0], Qm[0])
        check_column("%s k %d" % (name, k), name, k, Pm[0], Qm[0], y, w, info, unstable=True)
        assert s.counter("bordered_transposed_steps") == info[0]
    finally:
        s.close()


# ---- case 5: the handle where A^T = A ----

def run_symmetric(lib, k):
    name = "biharm300_lower"
    Pm, Qm = rhs_of(name, k, 1)
    s, _ = bordered_handle(lib, name, k)
    try:
        Bm, Cm, _ = border_of(name, k)
        assert np.max(np.abs(Bm - Cm)) > 0.1  # (M^T != M although A^T = A)
        blocks = s.counter("transposed_blocks")
        y, w, info = s.solve_bordered_transpose(Pm[0], Qm[0])
        check_column("%s k %d" % (name, k), name, k, Pm[0], Qm[0], y, w, info)
        assert s.counter("symmetric_ldlt") == 1 and s.counter("transposed_blocks") == blocks
    finally:
        s.close()


# ---- case 6: against the plain form ----

def run_adjoint_identity(lib, name, k):
    """<y, f> + <w, g> = <x, p> + <z, q> for M (x; z) = (f; g) and M^T (y; w) = (p; q), in rational arithmetic, to within the sum of
    the two forward-error bounds of check_column applied to the exact products' magnitudes"""
    from fractions import Fraction

    n = matrix(name)[0][0]
    F, G = right_hand_sides(BASE[name], k, 2)
    f, g, p, q = F[0], G[0], F[1], G[1]
    s, _ = bordered_handle(lib, name, k)
    try:
        x, z, info = s.solve_bordered(f, g)
        y, w, info_t = s.solve_bordered_transpose(p, q)
        assert info[3] == 0 and info_t[3] == 0
        Mt = assembled_t(name, k)
        M = sp.csr_matrix(Mt.T)
        M.sort_indices()
        xz, yw, fg, pq = np.concatenate([x, z]), np.concatenate([y, w]), np.concatenate([f, g]), np.concatenate([p, q])
        key, key_t = "M:%s:%d" % (name, k), "Mt:%s:%d" % (name, k)
        _, fe = exact_errors(M, fg, xz, key)
        _, fe_t = exact_errors(Mt, pq, yw, key_t)
        bound = max(10.0 * exact_errors(M, fg, comparison(M, fg, key), key)[1], floor_bound(n + k))  # (check_column's, of either form)
        bound_t = max(10.0 * exact_errors(Mt, pq, comparison(Mt, pq, key_t), key_t)[1], floor_bound(n + k))
        assert fe <= bound and fe_t <= bound_t
        dot = lambda a, b: sum((Fraction(float(u)) * Fraction(float(v)) for u, v in zip(a, b)), Fraction(0))
        gap = abs(float(dot(yw, fg) - dot(xz, pq)))
        # <yw, fg> = <yw_exact, fg> + <e_t, fg> and <xz, pq> likewise, the exact products agree: the gap is at most |e_t|_inf |fg|_1 +
        # |e|_inf |pq|_1, the errors relative to the exact solutions' largest entries (the computed ones' within a factor 1 + bound)
        slack = bound_t * (1.0 + bound_t) * np.max(np.abs(yw)) * np.abs(fg).sum() + bound * (1.0 + bound) * np.max(np.abs(xz)) * np.abs(pq).sum()
        print("adjoint identity %s k %d: gap %.3e, sum of the forward-error bounds %.3e (forward errors %.3e, %.3e)" % (name, k, gap, slack, fe, fe_t))
        assert gap <= slack
    finally:
        s.close()


def run_interleaved(lib, name, k, nrhs):
    """plain, transposed, plain, transposed on one handle: the bits of two fresh handles that run one form each"""
    F, G = rhs_of(name, k, nrhs)
    s, _ = bordered_handle(lib, name, k)
    s1, _ = bordered_handle(lib, name, k)
    s2, _ = bordered_handle(lib, name, k)
    try:
        a1, t1, a2, t2 = s.solve_bordered(F, G), s.solve_bordered_transpose(F, G), s.solve_bordered(F, G), s.solve_bordered_transpose(F, G)
        ra, rt = s1.solve_bordered(F, G), s2.solve_bordered_transpose(F, G)
        assert same_bits(a1, ra) and same_bits(a2, ra) and same_bits(t1, rt) and same_bits(t2, rt)
        assert not np.array_equal(ra[0], rt[0])
        assert s1.counter("border_transposed_bytes") == 0 and s2.counter("border_transposed_bytes") > 0
    finally:
        s.close(), s1.close(), s2.close()


# ---- case 7: composed with the sensitivities ----

def run_sensitivity(lib):
    """J = <c, x> + <d, z> with M (x; z) = (f; g): dJ/da = -lambda_i x_j on the pattern with M^T (lambda; mu) = (c; d) -- values_outer
    with u = lambda, w = x, alpha = -1 -- against central differences in eight seeded stored values (h and the relative agreement of
    tests/sensitivity.py's run_finite_differences: 1e-6 of max |grad|)"""
    name, k, h = "ulap483", 3, 1e-6
    init, kw, values, A = matrix(name)
    n = init[0]
    Bm, Cm, D = border_of(name, k)
    F, G = rhs_of(name, k, 2)
    f, g, c, d = F[0], G[0], F[1], G[1]
    s, _ = bordered_handle(lib, name, k)
    try:
        x, z, info = s.solve_bordered(f, g)
        lam, mu, info_t = s.solve_bordered_transpose(c, d)
        assert info[3] == 0 and info_t[3] == 0
        grad = s.values_outer(lam, x, alpha=-1.0)
        assert grad.shape == values.shape
        rhs, cd = np.concatenate([f, g]), np.concatenate([c, d])

        def J(v):
            Av = sp.csr_matrix((v, A.indices, A.indptr), shape=A.shape)
            return float(cd @ np.linalg.solve(assembled(Av, Bm, Cm, D).toarray(), rhs))

        picks = np.random.default_rng(8).choice(values.size, 8, replace=False)
        fd = np.zeros(8)
        for t, e in enumerate(picks):
            dv = np.zeros(values.size)
            dv[e] = h
            fd[t] = (J(values + dv) - J(values - dv)) / (2 * h)
        print("sensitivity composition: max |fd - grad| / max |grad| = %.3e" % (np.max(np.abs(fd - grad[picks])) / np.max(np.abs(grad))))
        assert np.max(np.abs(fd - grad[picks])) <= 1e-6 * np.max(np.abs(grad))
    finally:
        s.close()


# ---- case 8: life cycle and status codes ----

def run_status_codes(lib):
    name, k = "ulap483", 3
    init, kw, values, A = matrix(name)
    n = init[0]
    Bm, Cm, D = (np.asfortranarray(a) for a in border_of(name, k))
    Pm, Qm = rhs_of(name, k, 1)
    f, g = np.ascontiguousarray(Pm[0]), np.ascontiguousarray(Qm[0])
    s = _new(lib)
    try:
        x, z = np.zeros(n), np.zeros(k)
        setb, solve, solved = s.lib.solver_hipmf_set_border, s.lib.solver_hipmf_solve_bordered_transpose, s.lib.solver_hipmf_solve_bordered_transpose_device
        p = lambda a: a.ctypes.data
        border_args = (k, p(Bm), n, p(Cm), n, p(D), k, None, 0)
        solve_args = (p(x), p(z), p(f), p(g), 1, n, k, 0, None, 0)
        # NULL pointers first
        assert solve(None, *solve_args) == ERROR_NULL_POINTER and solved(None, *solve_args) == ERROR_NULL_POINTER
        assert solve(s.h, None, p(z), p(f), p(g), 1, n, k, 0, None, 0) == ERROR_NULL_POINTER
        assert solve(s.h, p(x), p(z), None, p(g), 1, n, k, 0, None, 0) == ERROR_NULL_POINTER
        # then the state of the handle
        assert solve(s.h, *solve_args) == ERROR_NEED_INITIALIZATION
        assert s.initialize(*init, **kw) == 0
        assert solve(s.h, *solve_args) == ERROR_NEED_FACTORIZATION
        assert solved(s.h, C.c_void_p(8), None, C.c_void_p(8), None, 1, n, k, 0, None, 0) == ERROR_NEED_FACTORIZATION
        assert s.factorize(values) == 0
        # then the values
        assert solve(s.h, *solve_args) == ERROR_HIPMF_INVALID_VALUE  # (no border was set)
        assert setb(s.h, *border_args) == 0 and s.counter("border_columns") == k and s.counter("border_transposed_bytes") == 0
        assert solve(s.h, *solve_args) == 0  # (info may be NULL)
        held = s.counter("border_transposed_bytes")
        assert held == 8 * (n * 16 + 16 * 16)
        x0, z0 = x.copy(), z.copy()
        assert solve(s.h, p(x), p(z), p(f), p(g), 0, n, k, 0, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert solve(s.h, p(x), p(z), p(f), p(g), 1, n - 1, k, 0, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert solve(s.h, p(x), p(z), p(f), p(g), 1, n, k - 1, 0, None, 0) == ERROR_HIPMF_INVALID_VALUE
        # max_steps <= 0 selects 4
        info_a, info_b = np.zeros(4), np.zeros(4)
        xa, xb = np.zeros(n), np.zeros(n)
        assert solve(s.h, p(xa), None, p(f), p(g), 1, n, k, -3, p(info_a), 0) == 0 and solve(s.h, p(xb), None, p(f), p(g), 1, n, k, 4, p(info_b), 0) == 0
        assert np.array_equal(xa, xb) and np.array_equal(info_a, info_b) and np.array_equal(xa, x0)
        # a second factorize -- of other values -- drops the border until set_border is called again; V is then built anew
        assert s.factorize(2.0 * values) == 0
        assert s.counter("border_columns") == 0
        assert solve(s.h, *solve_args) == ERROR_HIPMF_INVALID_VALUE
        assert setb(s.h, *border_args) == 0 and s.counter("border_transposed_bytes") == 0
        assert solve(s.h, *solve_args) == 0 and not np.array_equal(x, x0)  # (another matrix: a V kept from the first one would not do)
        R2 = RestatementT(sp.csr_matrix(2.0 * A), Bm, Cm, D, "At2:" + name)
        y2, w2, _, state2, _ = R2.solve(f, g)
        assert state2 in (0, 1) and np.max(np.abs(x - y2)) <= 1e-10 * np.max(np.abs(y2)) and np.max(np.abs(z - w2)) <= 1e-10 * np.max(np.abs(w2))
        assert s.factorize(values) == 0 and setb(s.h, *border_args) == 0
        assert solve(s.h, *solve_args) == 0 and np.array_equal(x, x0) and np.array_equal(z, z0)  # (the same bits as before)
        # k = 0 frees the border (the pointers may be NULL)
        assert s.counter("border_transposed_bytes") == held
        assert setb(s.h, 0, None, 0, None, 0, None, 0, None, 0) == 0
        assert s.counter("border_columns") == 0 and s.counter("border_transposed_bytes") == 0
        assert solve(s.h, *solve_args) == ERROR_HIPMF_INVALID_VALUE
    finally:
        s.close()


# ---- case 9: reproducible and without side effects ----

def run_side_effects(lib, name):
    k, nrhs = 3, 3
    init, kw, values, A = matrix(name)
    n = init[0]
    Bm, Cm, D = border_of(name, k)
    F, G = rhs_of(name, k, nrhs)
    s = handle(lib, init, kw, values, nstep=-1)  # (the default refinement of the ordinary solves)
    ptrs = []
    try:
        assert all(s.counter(c) == 0 for c in T_COUNTERS)
        binfo, status = s.set_border(Bm, Cm, D)
        assert status == 0
        kp = 16
        # what set_border reports is the plain side alone: three packed n x kp arrays, D and the LU of S, the partial sums, the record, the pivots
        nch = (n + 1023) // 1024
        assert binfo[3] == 8 * (3 * n * kp + 2 * kp * kp + 4 * nch * kp * 16 + 8) + 4 * kp
        x0, t0, m0, b0 = s.solve(F[0]), s.solve_transpose(F[0]), s.solve_many(F), s.solve_bordered(F, G)
        watched = TR_COUNTERS + BORDER_COUNTERS
        keep = [s.counter(c) for c in watched] + [s.stats()["refinement_steps"]]
        fixed = ("n_perturbed", "factor_launches", "solve_launches", "acc_factor_count", "acc_tri_count", "residual_inf")
        st = {q: s.stats()[q] for q in fixed}
        x0b, t0b, m0b, b0b = s.solve(F[0]), s.solve_transpose(F[0]), s.solve_many(F), s.solve_bordered(F, G)  # (what a repetition without transposed calls changes)
        keep_b = [s.counter(c) for c in watched] + [s.stats()["refinement_steps"]]
        st_b = {q: s.stats()[q] for q in fixed}
        assert s.counter("border_transposed_bytes") == 0
        a = s.solve_bordered_transpose(F[0], G[0])
        b = s.solve_bordered_transpose(F[0], G[0])
        assert same_bits(a, b)
        ma = s.solve_bordered_transpose(F, G)
        mb = s.solve_bordered_transpose(F, G)
        assert same_bits(ma, mb)
        assert s.counter("bordered_transposed_blocks") == 1 and s.counter("border_transposed_bytes") == 8 * (n * kp + kp * kp)
        # the device form: the bits of the host form
        d_y, d_w, d_p, d_q = s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * k * nrhs), s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * k * nrhs)
        ptrs += [d_y, d_w, d_p, d_q]
        s.h2d(d_p, F), s.h2d(d_q, G)
        info_d = s.solve_bordered_transpose_device(d_y, d_w, d_p, d_q, nrhs, ldz=k)
        yd, wd = np.zeros((nrhs, n)), np.zeros((nrhs, k))
        s.d2h(yd, d_y), s.d2h(wd, d_w)
        assert same_bits((yd, wd, info_d), ma)
        # nothing of the other solves has moved
        assert [s.counter(c) for c in watched] + [s.stats()["refinement_steps"]] == keep_b
        assert {q: s.stats()[q] for q in fixed} == st_b
        x1, t1, m1, b1 = s.solve(F[0]), s.solve_transpose(F[0]), s.solve_many(F), s.solve_bordered(F, G)
        for u, v in ((x0, x1), (t0, t1), (m0, m1), (x0, x0b), (t0, t0b), (m0, m0b)):
            assert np.array_equal(u.view(np.uint64), v.view(np.uint64))
        assert same_bits(b0, b1) and same_bits(b0, b0b)
        # ... and these solves move the counters and statistics exactly as the same solves did before the transposed calls
        assert [s.counter(c) for c in watched] + [s.stats()["refinement_steps"]] == [kb + (kb - ka) for ka, kb in zip(keep, keep_b)]
        assert {q: s.stats()[q] for q in fixed} == {q: st_b[q] + (st_b[q] - st[q]) for q in fixed}
    finally:
        for q in ptrs:
            s.dev_free(q)
        s.close()
