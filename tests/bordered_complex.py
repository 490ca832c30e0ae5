"""Cases of the bordered solves of the COMPLEX handle on the kept factor (complex_solver_hipmf_set_border, _solve_bordered,
_solve_bordered_transpose and their _device forms; kernels_border_complex.hpp), shared by tests/test_bordered_complex_cpu.py (the CPU
emulator of the HIP kernels) and tests/test_bordered_complex_gpu.py (lib None = the product build).

    [ A   B ] [x]   [f]
    [ C^T D ] [z] = [g]      M = the assembled complex (n + k) matrix, C^T the plain transpose

Matrices: zlap483 / zlap4087 = laplacian + (1 + 0.5i) I (real-equivalent order 966 / 8174: eight 1024-row chunks of the Gram and
border-row kernels, the last ragged), zhopf1e-6 / zhopf1e-10 = laplacian(23, 21) - lambda200 I + i delta I (cond_inf 6.9e6 / 6.9e10).
Borders: real and imaginary parts uniform in (-1, 1) from default_rng(1000 k + n) -- a C whose imaginary part matters, so that C^T taken
as C^H, or the real-equivalent form of C transposed where that of conj(C) belongs, fails every case.  Right-hand sides: complex standard
normal.

The NumPy restatement is tests/bordered.py's Restatement (tests/bordered_transpose.py's RestatementT) on complex arrays: complex SuperLU
of A as the pass pair, W = A^{-1} B, the complex S, a working-precision residual, omega on complex moduli (numpy's abs).  M^H is restated
as M^T on conjugated data: every modulus, and so every omega and step count, is the same.  Only its step counts are asserted against
(steps <= restatement's + 1): on zlap4087 it ends columns itself as "no progress" at omega = 2.2e-16 .. 3.2e-16, the noise of a
working-precision residual that the kernels' compensated residual does not have.

The error is measured exactly: exact_residual (tests/extra_precise.py, fractions.Fraction, rounded once) on the REAL-EQUIVALENT assembled
matrix, then pair moduli.  Per column: state 0; steps as above; componentwise backward error of complex row i <= (p_i + 2) eps, p_i the
entries of row i of M, dense border entries included; forward error of the stacked (x; z) in the infinity norm, on moduli, <=
max(10 x the comparison's, floor_bound(n + k)), the comparison being complex SuperLU on M plus one refinement step -- evaluated only
where the error exceeds the floor, since below it the bound holds whatever the comparison gives.  The premise cond_inf(M) eps <= 1e-3 of
the forward-error measurement is asserted: by numpy.linalg.cond on the 483-row matrices, by |M|_inf times Hager's estimate of
|M^{-1}|_inf (scipy's onenormest on SuperLU's solves; a lower bound within a small factor, against a premise with decades to spare) on
the 4087-row ones."""
import ctypes as C
import functools
import os

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import bordered as B
from bordered import assembled, comparison
from bordered_transpose import RestatementT
from extra_precise import EPS, ERROR_NEED_INITIALIZATION, SENTINEL, TR_COUNTERS, exact_residual, floor_bound, laplacian, lambda200, lu_of, pair_moduli
from russell_amd.backend import ComplexHipmf, Hipmf
from test_transpose_solve_cpu import ERROR_HIPMF_INVALID_VALUE, ERROR_NEED_FACTORIZATION, ERROR_NULL_POINTER

WARNING_SINGULAR_MATRIX = 1
K_SHAPES = [1, 3, 8, 9, 16, 17, 31, 32]  # (the real-equivalent width crosses 16 at 8 | 9 and 32 at 16 | 17, and fills 64 at 32)
NRHS_SHAPES = [1, 15, 16, 17, 33]
PLAIN_COUNTERS = ("complex_bordered_steps", "complex_bordered_blocks")
T_COUNTERS = ("complex_bordered_transposed_steps", "complex_bordered_transposed_blocks")
SENT = complex(SENTINEL, SENTINEL)


# ---- matrices, borders, right-hand sides ----

@functools.lru_cache(None)
def matrix(name):
    """the complex matrix (scipy CSR, sorted)"""
    if name == "zlap483":
        A = laplacian(23, 21) + (1 + 0.5j) * sp.identity(483)
    elif name == "zlap4087":
        A = laplacian(67, 61) + (1 + 0.5j) * sp.identity(4087)
    elif name in ("zhopf1e-6", "zhopf1e-10"):
        A = laplacian(23, 21) - lambda200() * sp.identity(483) + 1j * float(name[5:]) * sp.identity(483)
    else:
        raise KeyError(name)
    A = sp.csr_matrix(A).astype(np.complex128)
    A.sort_indices()
    return A


@functools.lru_cache(None)
def border(name, k):
    n = matrix(name).shape[0]
    rng = np.random.default_rng(1000 * k + n)
    draw = lambda *shape: rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)
    return draw(n, k), draw(n, k), draw(k, k)


@functools.lru_cache(None)
def right_hand_sides(name, k, nrhs):
    """(F, G): the rows are the right-hand sides of the first n and of the last k rows"""
    n = matrix(name).shape[0]
    rng = np.random.default_rng(7 * n + 13 * k + nrhs)
    draw = lambda *shape: rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    return draw(nrhs, n), draw(nrhs, k)


@functools.lru_cache(None)
def assembled_of(name, k, trans=0):
    """M (trans 0), M^T (1) or M^H (2) as a sorted complex CSR matrix"""
    Bm, Cm, D = border(name, k)
    M = assembled(matrix(name), Bm, Cm, D)
    M = sp.csr_matrix(M if trans == 0 else (M.T if trans == 1 else M.conj().T))
    M.sort_indices()
    return M


def real_equivalent(Mz):
    """a + i b -> [a -b; b a] at rows 2i, 2i+1 / columns 2j, 2j+1: the matrix of the interleaved vectors"""
    R = sp.csr_matrix(sp.kron(Mz.real, sp.identity(2)) + sp.kron(Mz.imag, sp.csr_matrix([[0.0, -1.0], [1.0, 0.0]])))
    R.sort_indices()
    return R


def interleaved(v):
    return np.ascontiguousarray(v, dtype=np.complex128).view(np.float64)


def handle(lib, name, nstep=0):
    A = matrix(name)
    s = ComplexHipmf(lib) if lib else ComplexHipmf()
    assert s.initialize(A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32), refinement_nstep=nstep, values=A.data) == 0
    assert s.factorize(A.data) == 0
    return s


def bordered_handle(lib, name, k, nstep=0):
    s = handle(lib, name, nstep)
    binfo, status = s.set_border(*border(name, k))
    assert status == 0, status
    return s, binfo


def same_bits(a, b):
    return all((u is None and v is None) or np.array_equal(np.asarray(u).view(np.uint64), np.asarray(v).view(np.uint64)) for u, v in zip(a, b))


# ---- the restatement's step counts, the premise and the exact measurement ----

@functools.lru_cache(None)
def restatement(name, k):
    return B.Restatement(matrix(name), *border(name, k), "zA:" + name)


@functools.lru_cache(None)
def restatement_t(name, k):
    return RestatementT(matrix(name), *border(name, k), "zA:" + name)


def reference_steps(name, k, trans, f, g):
    """(steps, state, omega before the first step) of the NumPy restatement; M^H: M^T on conjugated data"""
    if trans == 0:
        return restatement(name, k).solve(f, g)[2:]
    return restatement_t(name, k).solve(np.conj(f) if trans == 2 else f, np.conj(g) if trans == 2 else g)[2:]


@functools.lru_cache(None)
def cond_assembled(name, k, trans=0):
    M = assembled_of(name, k, trans)
    if M.shape[0] < 1000:
        return float(np.real(np.linalg.cond(M.toarray(), np.inf)))
    lu = lu_of(M, "zM:%s:%d:%d" % (name, k, trans))
    n = M.shape[0]
    inv_h = spla.LinearOperator((n, n), dtype=np.complex128, matvec=lambda v: lu.solve(np.asarray(v, np.complex128).ravel(), trans="H"),
                                rmatvec=lambda v: lu.solve(np.asarray(v, np.complex128).ravel()))
    return float(abs(M).sum(axis=1).max() * spla.onenormest(inv_h))  # |M^{-1}|_inf = |M^{-H}|_1


@functools.lru_cache(None)
def real_equivalent_of(name, k, trans):
    return real_equivalent(assembled_of(name, k, trans))


def exact_errors(M, Mre, rhs, y, key):
    """(max over the complex rows of the exact componentwise backward error / ((p_i + 2) eps), forward error of y in the infinity norm on
    moduli, relative): the residual in fractions.Fraction on the real-equivalent matrix, rounded once, then complex SuperLU of M plus
    one correction"""
    r = exact_residual(Mre, interleaved(rhs), interleaved(y))
    den = abs(M) @ np.abs(y) + np.abs(rhs)
    p = np.diff(M.indptr)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(den > 0, pair_moduli(r) / den, np.where(pair_moduli(r) > 0, np.inf, 0.0))
    lu = lu_of(M, key)
    rz = r[0::2] + 1j * r[1::2]
    e = lu.solve(rz)
    e = e + lu.solve(rz - M @ e)
    assert np.all(np.isfinite(e))
    return float(np.max(q / ((p + 2) * EPS))), float(np.max(np.abs(e)) / np.max(np.abs(y + e)))


def check_column(label, name, k, trans, f, g, x, z, info):
    """the acceptance rules for one column of M (trans 0), M^T (1) or M^H (2)"""
    n = matrix(name).shape[0]
    M = assembled_of(name, k, trans)
    assert np.all(np.diff(M.indptr)[:n] == np.diff(matrix(name).indptr) + k) and np.all(np.diff(M.indptr)[n:] == n + k)  # (dense border entries included; A's pattern is symmetric)
    key = "zM:%s:%d:%d" % (name, k, trans)
    assert cond_assembled(name, k, trans) * EPS <= 1e-3  # (the premise of the forward error)
    rhs, y = np.concatenate([f, g]), np.concatenate([x, z])
    ref_steps, ref_state, ref_omega0 = reference_steps(name, k, trans, f, g)
    Mre = real_equivalent_of(name, k, trans)
    back, fe = exact_errors(M, Mre, rhs, y, key)
    floor = floor_bound(n + k)
    fe_cmp = exact_errors(M, Mre, rhs, comparison(M, rhs, key), key)[1] if fe > floor else float("nan")  # (below the floor the bound holds whatever the comparison gives)
    print("%s: steps %d (restatement %d, state %d), omega %.3e, before %.3e (restatement %.3e), state %d; exact backward error / ((p + 2) eps) %.3f, "
          "forward error %.3e (comparison %.3e, floor %.3e)" % (label, info[0], ref_steps, ref_state, info[1], info[2], ref_omega0, info[3], back, fe, fe_cmp, floor))
    assert info[3] == 0, info
    assert info[0] <= ref_steps + 1, (info[0], ref_steps)
    assert back <= 1.0, back
    assert fe <= floor or fe <= 10.0 * fe_cmp, (fe, fe_cmp)


# ---- case 1: exports ----

def check_exports(lib_path):
    from russell_amd import _capi

    raw = C.CDLL(lib_path or _capi.DEFAULT_LIB)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "russell_hipmf.h")).read()
    for name in ("set_border", "set_border_device", "solve_bordered", "solve_bordered_device", "solve_bordered_transpose", "solve_bordered_transpose_device"):
        assert hasattr(raw, "complex_solver_hipmf_" + name), name
        assert "complex_solver_hipmf_" + name in _capi.SYMBOLS and "complex_solver_hipmf_" + name + "(" in header, name
        assert hasattr(ComplexHipmf, name), name
    assert "#define HIPMF_COMPLEX_BORDER_MAX 32" in header
    for name, num in (("COMPLEX_BORDER_COLUMNS", 52), ("COMPLEX_BORDERED_STEPS", 53), ("COMPLEX_BORDERED_BLOCKS", 54), ("COMPLEX_BORDERED_TRANSPOSED_STEPS", 55),
                      ("COMPLEX_BORDERED_TRANSPOSED_BLOCKS", 56), ("COMPLEX_BORDER_TRANSPOSED_BYTES", 57)):
        assert "#define HIPMF_COUNTER_%s %d" % (name, num) in header
        assert Hipmf.COUNTERS[name.lower()] == num


# ---- cases 2 and 3: border widths and column counts, with the padding sentinels ----

def padded(V, ld):
    out = np.full((V.shape[0], ld), SENT)
    out[:, :V.shape[1]] = V
    return out


def run_shape(lib, name, k, nrhs, variants=False):
    n = matrix(name).shape[0]
    F, G = right_hand_sides(name, k, nrhs)
    ldx, ldz = n + 5, k + 2
    s, _ = bordered_handle(lib, name, k)
    ptrs = []
    try:
        Fp, Gp = padded(F, ldx), padded(G, ldz)
        X, Z = np.full((nrhs, ldx), SENT), np.full((nrhs, ldz), SENT)
        x, z, info = s.solve_bordered(Fp, Gp, ldx=ldx, ldz=ldz, x=X, z=Z)
        assert np.all(x[:, n:] == SENT) and np.all(z[:, k:] == SENT)  # (entries beyond n and k are not touched)
        assert s.counter("complex_bordered_blocks") == (nrhs + 15) // 16 and s.counter("complex_border_columns") == k
        assert s.counter("complex_border_transposed_bytes") == 0  # (nothing is built for the transposed side by a handle that does not ask)
        for c in range(nrhs):
            check_column("%s k %d column %d of %d" % (name, k, c, nrhs), name, k, 0, F[c], G[c], x[c, :n], z[c, :k], info[c])
        if variants:
            # z = NULL: the same x, bit for bit
            x2, z2, info2 = s.solve_bordered(Fp, Gp, ldx=ldx, ldz=ldz, x=np.full((nrhs, ldx), SENT), want_z=False)
            assert z2 is None and same_bits([x2], [x]) and np.array_equal(info2, info)
            # g = NULL: g = 0
            x3, z3, info3 = s.solve_bordered(Fp, None, ldx=ldx, ldz=ldz, x=np.full((nrhs, ldx), SENT), z=np.full((nrhs, ldz), SENT))
            assert np.all(x3[:, n:] == SENT) and np.all(z3[:, k:] == SENT)
            for c in range(nrhs):
                check_column("%s k %d column %d, g = NULL" % (name, k, c), name, k, 0, F[c], np.zeros(k, complex), x3[c, :n], z3[c, :k], info3[c])
            # the _device forms, padded too: the bits of the host forms
            Bm, Cm, D = border(name, k)
            d_B, d_C, d_D = (s.dev_alloc(16 * v.size) for v in (Bm, Cm, D))
            d_x, d_z, d_f, d_g = s.dev_alloc(16 * ldx * nrhs), s.dev_alloc(16 * ldz * nrhs), s.dev_alloc(16 * ldx * nrhs), s.dev_alloc(16 * ldz * nrhs)
            ptrs += [d_B, d_C, d_D, d_x, d_z, d_f, d_g]
            s.h2d(d_B, np.asfortranarray(Bm).T), s.h2d(d_C, np.asfortranarray(Cm).T), s.h2d(d_D, np.asfortranarray(D).T)
            s.h2d(d_f, Fp), s.h2d(d_g, Gp), s.h2d(d_x, np.full((nrhs, ldx), SENT)), s.h2d(d_z, np.full((nrhs, ldz), SENT))
            binfo_h = s.set_border(Bm, Cm, D)[0]
            binfo_d, status_d = s.set_border_device(k, d_B, d_C, d_D)
            assert status_d == 0 and np.array_equal(binfo_d, binfo_h)
            info_d = s.solve_bordered_device(d_x, d_z, d_f, d_g, nrhs, ldx=ldx, ldz=ldz)
            xd, zd = np.zeros((nrhs, ldx), complex), np.zeros((nrhs, ldz), complex)
            s.d2h(xd, d_x), s.d2h(zd, d_z)
            assert same_bits([xd, zd], [x, z]) and np.array_equal(info_d, info)
    finally:
        for q in ptrs:
            s.dev_free(q)
        s.close()


# ---- case 4: near a fold / Hopf point ----

def run_hopf(lib, name, k):
    F, G = right_hand_sides(name, k, 1)
    s, _ = bordered_handle(lib, name, k)
    try:
        x, z, info = s.solve_bordered(F[0], G[0])
        check_column("%s k %d" % (name, k), name, k, 0, F[0], G[0], x, z, info)
        assert s.counter("complex_bordered_steps") == info[0]
    finally:
        s.close()


# ---- case 5: both transposed forms ----

def run_transposed(lib, name, k, nrhs, conjugate):
    n = matrix(name).shape[0]
    trans = 2 if conjugate else 1
    Pm, Qm = right_hand_sides(name, k, nrhs)
    ldx, ldz = n + 5, k + 2
    s, _ = bordered_handle(lib, name, k)
    ptrs = []
    try:
        x0 = s.solve_bordered(Pm[0], Qm[0])
        plain = [s.counter(c) for c in PLAIN_COUNTERS]
        assert [s.counter(c) for c in T_COUNTERS] == [0, 0] and s.counter("complex_border_transposed_bytes") == 0
        Pp, Qp = padded(Pm, ldx), padded(Qm, ldz)
        y, w, info = s.solve_bordered_transpose(Pp, Qp, conjugate=conjugate, ldx=ldx, ldz=ldz, y=np.full((nrhs, ldx), SENT), w=np.full((nrhs, ldz), SENT))
        assert np.all(y[:, n:] == SENT) and np.all(w[:, k:] == SENT)
        kp = (2 * k + 15) // 16 * 16  # (V packed, D^H, and the LU of the transposed side's own Schur complement with its pivots)
        assert s.counter("complex_bordered_transposed_blocks") == (nrhs + 15) // 16 and s.counter("complex_border_transposed_bytes") == 8 * (2 * n * kp + 2 * kp * kp) + 4 * kp
        assert [s.counter(c) for c in PLAIN_COUNTERS] == plain and s.counter("complex_border_columns") == k  # (the plain form's counters have not moved)
        for c in range(nrhs):
            check_column("%s k %d %s column %d of %d" % (name, k, "M^H" if conjugate else "M^T", c, nrhs), name, k, trans, Pm[c], Qm[c], y[c, :n], w[c, :k], info[c])
        # ... nor does a plain call move the transposed form's, or a bit of its own result
        tc = [s.counter(c) for c in T_COUNTERS]
        assert same_bits(s.solve_bordered(Pm[0], Qm[0]), x0) and [s.counter(c) for c in T_COUNTERS] == tc
        # w = NULL and a repetition: the same bits; the other conjugation is served from the same V
        y2, w2, info2 = s.solve_bordered_transpose(Pp, Qp, conjugate=conjugate, ldx=ldx, ldz=ldz, y=np.full((nrhs, ldx), SENT), want_w=False)
        assert w2 is None and same_bits([y2], [y]) and np.array_equal(info2, info)
        bytes_t = s.counter("complex_border_transposed_bytes")
        yo, wo, info_o = s.solve_bordered_transpose(Pm[0], Qm[0], conjugate=not conjugate)
        check_column("%s k %d %s" % (name, k, "M^T" if conjugate else "M^H"), name, k, 3 - trans, Pm[0], Qm[0], yo, wo, info_o)
        assert s.counter("complex_border_transposed_bytes") == bytes_t
        # the _device form: the bits of the host form
        d_y, d_w, d_p, d_q = s.dev_alloc(16 * ldx * nrhs), s.dev_alloc(16 * ldz * nrhs), s.dev_alloc(16 * ldx * nrhs), s.dev_alloc(16 * ldz * nrhs)
        ptrs += [d_y, d_w, d_p, d_q]
        s.h2d(d_p, Pp), s.h2d(d_q, Qp), s.h2d(d_y, np.full((nrhs, ldx), SENT)), s.h2d(d_w, np.full((nrhs, ldz), SENT))
        info_d = s.solve_bordered_transpose_device(d_y, d_w, d_p, d_q, nrhs, conjugate=conjugate, ldx=ldx, ldz=ldz)
        yd, wd, pd = np.zeros((nrhs, ldx), complex), np.zeros((nrhs, ldz), complex), np.zeros((nrhs, ldx), complex)
        s.d2h(yd, d_y), s.d2h(wd, d_w), s.d2h(pd, d_p)
        assert same_bits([yd, wd, pd], [y, w, Pp]) and np.array_equal(info_d, info)  # (p is not changed by the conjugation on entry)
        # the first transposed call after a new set_border rebuilds V
        assert s.set_border(*border(name, k))[1] == 0 and s.counter("complex_border_transposed_bytes") == 0
        y3, w3, info3 = s.solve_bordered_transpose(Pp, Qp, conjugate=conjugate, ldx=ldx, ldz=ldz)
        assert same_bits([y3[:, :n], w3[:, :k]], [y[:, :n], w[:, :k]]) and s.counter("complex_border_transposed_bytes") == bytes_t
    finally:
        for q in ptrs:
            s.dev_free(q)
        s.close()


# ---- case 6: Woodbury ----

def run_woodbury(lib):
    """(A + U V^T) x = b as the bordered system with D = -I, g = 0, called with g and z NULL.  The solution is measured against the exact
    one of the assembled bordered matrix M -- the same x, without the rounding of a dense A + U V^T --: forward error of x alone, and the
    exact backward error of (x; z) from the call that returns z."""
    name, k = "zlap483", 3
    A = matrix(name)
    n = A.shape[0]
    U, V, _ = border(name, k)
    D = -np.identity(k, dtype=complex)
    b = right_hand_sides(name, k, 1)[0][0]
    M = sp.csr_matrix(assembled(A, U, V, D))
    M.sort_indices()
    Mre = real_equivalent(M)
    assert float(np.real(np.linalg.cond(M.toarray(), np.inf))) * EPS <= 1e-3
    assert float(np.real(np.linalg.cond(A.toarray() + U @ V.T, np.inf))) * EPS <= 1e-3
    ref_steps, ref_state, _ = B.Restatement(A, U, V, D, "zA:" + name).solve(b, np.zeros(k, complex))[2:]
    s = handle(lib, name)
    try:
        assert s.set_border(U, V, D)[1] == 0
        x, z, info = s.solve_bordered(b, None, want_z=False)
        assert z is None
        x2, z2, _ = s.solve_bordered(b, None)  # with z returned: the same x
        assert same_bits([x2], [x])
        rhs = np.concatenate([b, np.zeros(k, complex)])
        lu = lu_of(M, "zwoodbury")

        def errors_of(y):
            r = exact_residual(Mre, interleaved(rhs), interleaved(y))
            rz = r[0::2] + 1j * r[1::2]
            e = lu.solve(rz)
            e = e + lu.solve(rz - M @ e)
            return pair_moduli(r), float(np.max(np.abs(e[:n])) / np.max(np.abs((y + e)[:n])))

        r, fe = errors_of(np.concatenate([x2, z2]))
        fe_cmp = errors_of(comparison(M, rhs, "zwoodbury"))[1]
        print("Woodbury k %d: steps %d (restatement %d, state %d), omega %.3e, state %d, forward error of x %.3e (comparison %.3e)" %
              (k, info[0], ref_steps, ref_state, info[1], info[3], fe, fe_cmp))
        assert info[3] == 0 and info[0] <= ref_steps + 1
        assert fe <= max(10.0 * fe_cmp, floor_bound(n)), (fe, fe_cmp)
        den = abs(M) @ np.abs(np.concatenate([x2, z2])) + np.abs(rhs)
        p = np.concatenate([np.diff(A.indptr) + k, np.full(k, n + k)])
        assert np.all(r <= (p + 2) * EPS * den)
        # ... and it solves the rank-k changed system: the residual of the dense A + U V^T in working precision
        Ad = A.toarray() + U @ V.T
        assert np.max(np.abs(b - Ad @ x) / (np.abs(Ad) @ np.abs(x) + np.abs(b))) <= (n + 2) * EPS
    finally:
        s.close()


# ---- case 7: what set_border returns ----

def log_distance(mant, expo, sign, logabs):
    """| log |a| - log |b| | + | a / |a| - b / |b| | for a = mant x 10^expo, b = sign exp(logabs)"""
    return abs(np.log(abs(mant)) + expo * np.log(10.0) - logabs) + abs(mant / abs(mant) - sign)


def run_border_info(lib, k):
    """The tolerances are run_border_info's of tests/bordered.py: 100 x what the restatement's own S shows against det M / det A by NumPy
    (here the distance of the complex logarithms, modulus and phase, with n eps as its least value: n logarithms are summed), a factor
    2 on the pivot ratio.  det A (complex_solver_hipmf_get_determinant) x det S against det M: both factors are LU determinants in
    double of matrices of this size, so twice that bound."""
    name = "zlap483"
    A = matrix(name)
    n = A.shape[0]
    Bm, Cm, D = border(name, k)
    s, binfo = bordered_handle(lib, name, k)
    try:
        sM, lM = np.linalg.slogdet(assembled_of(name, k).toarray())
        sA, lA = np.linalg.slogdet(A.toarray())
        Sref = restatement(name, k).S
        sS, lS = np.linalg.slogdet(Sref)
        gap = max(abs(lS - (lM - lA)) + abs(sS - sM / sA), n * EPS)
        mant = complex(binfo[1], binfo[2])
        got = log_distance(mant, binfo[3], sM / sA, lM - lA)
        print("k %d: det S = (%.15f %+.15f i) x 10^%d, off by %.3e, restatement's S off by %.3e; min / max |u_ii| %.6e" % (k, mant.real, mant.imag, binfo[3], got, gap, binfo[0]))
        assert 1.0 <= abs(mant) < 10.0 and binfo[3] == np.floor(binfo[3])
        assert got <= 100.0 * gap, (got, gap)
        u = np.abs(np.diag(sla.lu(Sref)[2]))
        ratio = float(u.min() / u.max())
        assert ratio / 2 <= binfo[0] <= 2 * ratio, (binfo[0], ratio)
        assert binfo[4] >= 16 * (3 * n * k + k * k)
        assert s.counter("complex_border_columns") == k
        dr, di, de = s.determinant()
        prod = complex(dr, di) * mant
        got_m = log_distance(prod, de + binfo[3], sM, lM)
        print("k %d: det A det S against det M: off by %.3e" % (k, got_m))
        assert got_m <= 200.0 * gap, (got_m, gap)
    finally:
        s.close()


# ---- case 8: a singular Schur complement ----

def run_singular_border(lib):
    name = "zlap483"
    n = matrix(name).shape[0]
    s = handle(lib, name)
    try:
        Cm = border(name, 1)[1]
        info, status = s.set_border(np.zeros((n, 1), complex), Cm, np.zeros((1, 1), complex))  # S = D - C^T A^{-1} 0 = 0 exactly
        assert status == WARNING_SINGULAR_MATRIX
        assert s.counter("complex_border_columns") == 0
        x = np.zeros(n, complex)
        assert s.lib.complex_solver_hipmf_solve_bordered(s.h, x.ctypes.data, None, np.ones(n, complex).ctypes.data, None, 1, n, 1, 0, None, 0) == ERROR_HIPMF_INVALID_VALUE
        # the second pivot of a 2 x 2 S: B = 0 and D = [[1, 1], [1, 1]] eliminate to an exact zero
        Bm, Cm, _ = border(name, 2)
        info, status = s.set_border(0 * Bm, Cm, np.ones((2, 2), complex))
        assert status == WARNING_SINGULAR_MATRIX and s.counter("complex_border_columns") == 0
    finally:
        s.close()


# ---- case 9: life cycle and status codes ----

def run_status_codes(lib):
    name, k = "zlap483", 3
    A = matrix(name)
    n = A.shape[0]
    Bm, Cm, D = (np.asfortranarray(a) for a in border(name, k))
    f, g = right_hand_sides(name, k, 1)
    f, g = np.ascontiguousarray(f[0]), np.ascontiguousarray(g[0])
    s = ComplexHipmf(lib) if lib else ComplexHipmf()
    try:
        x, z = np.zeros(n, complex), np.zeros(k, complex)
        L = s.lib
        setb, solve, solvet = L.complex_solver_hipmf_set_border, L.complex_solver_hipmf_solve_bordered, L.complex_solver_hipmf_solve_bordered_transpose
        setd, solved, solvetd = L.complex_solver_hipmf_set_border_device, L.complex_solver_hipmf_solve_bordered_device, L.complex_solver_hipmf_solve_bordered_transpose_device
        p = lambda a: a.ctypes.data
        border_args = (k, p(Bm), n, p(Cm), n, p(D), k, None, 0)
        solve_args = (p(x), p(z), p(f), p(g), 1, n, k, 0, None, 0)
        solvet_args = (p(x), p(z), p(f), p(g), 1, n, k, 1, 0, None, 0)
        # NULL pointers first
        assert setb(None, *border_args) == ERROR_NULL_POINTER and solve(None, *solve_args) == ERROR_NULL_POINTER and solvet(None, *solvet_args) == ERROR_NULL_POINTER
        assert solve(s.h, None, p(z), p(f), p(g), 1, n, k, 0, None, 0) == ERROR_NULL_POINTER
        assert solve(s.h, p(x), p(z), None, p(g), 1, n, k, 0, None, 0) == ERROR_NULL_POINTER
        assert solvet(s.h, None, p(z), p(f), p(g), 1, n, k, 1, 0, None, 0) == ERROR_NULL_POINTER
        assert setb(s.h, k, None, n, p(Cm), n, p(D), k, None, 0) == ERROR_NULL_POINTER
        assert solved(None, *solve_args) == ERROR_NULL_POINTER and setd(None, *border_args) == ERROR_NULL_POINTER and solvetd(None, *solvet_args) == ERROR_NULL_POINTER
        # then the state of the handle
        assert setb(s.h, *border_args) == ERROR_NEED_INITIALIZATION and solve(s.h, *solve_args) == ERROR_NEED_INITIALIZATION
        assert solvet(s.h, *solvet_args) == ERROR_NEED_INITIALIZATION
        assert s.initialize(n, A.indptr.astype(np.int32), A.indices.astype(np.int32), refinement_nstep=0, values=A.data) == 0
        assert setb(s.h, *border_args) == ERROR_NEED_FACTORIZATION and solve(s.h, *solve_args) == ERROR_NEED_FACTORIZATION
        assert solvet(s.h, *solvet_args) == ERROR_NEED_FACTORIZATION
        assert solved(s.h, C.c_void_p(8), None, C.c_void_p(8), None, 1, n, k, 0, None, 0) == ERROR_NEED_FACTORIZATION
        assert s.factorize(A.data) == 0
        # then the values
        assert solve(s.h, *solve_args) == ERROR_HIPMF_INVALID_VALUE and solvet(s.h, *solvet_args) == ERROR_HIPMF_INVALID_VALUE  # (no border was set)
        assert setb(s.h, -1, p(Bm), n, p(Cm), n, p(D), k, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert setb(s.h, 33, p(Bm), n, p(Cm), n, p(D), 33, None, 0) == ERROR_HIPMF_INVALID_VALUE  # (HIPMF_COMPLEX_BORDER_MAX = 32)
        assert setb(s.h, k, p(Bm), n - 1, p(Cm), n, p(D), k, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert setb(s.h, k, p(Bm), n, p(Cm), n - 1, p(D), k, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert setb(s.h, k, p(Bm), n, p(Cm), n, p(D), k - 1, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert s.counter("complex_border_columns") == 0
        assert setb(s.h, *border_args) == 0 and s.counter("complex_border_columns") == k
        assert solve(s.h, *solve_args) == 0  # (info may be NULL)
        x0 = x.copy()
        assert solve(s.h, p(x), p(z), p(f), p(g), 0, n, k, 0, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert solve(s.h, p(x), p(z), p(f), p(g), 1, n - 1, k, 0, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert solve(s.h, p(x), p(z), p(f), p(g), 1, n, k - 1, 0, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert solvet(s.h, p(x), p(z), p(f), p(g), 1, n, k, 2, 0, None, 0) == ERROR_HIPMF_INVALID_VALUE  # (conjugate is 0 or 1)
        assert solvet(s.h, p(x), p(z), p(f), p(g), 1, n, k - 1, 1, 0, None, 0) == ERROR_HIPMF_INVALID_VALUE
        assert np.array_equal(x, x0)
        # max_steps <= 0 selects 4
        info_a, info_b = np.zeros(4), np.zeros(4)
        xa, xb = np.zeros(n, complex), np.zeros(n, complex)
        assert solve(s.h, p(xa), None, p(f), p(g), 1, n, k, -3, p(info_a), 0) == 0 and solve(s.h, p(xb), None, p(f), p(g), 1, n, k, 4, p(info_b), 0) == 0
        assert np.array_equal(xa, xb) and np.array_equal(info_a, info_b) and np.array_equal(xa, x0)
        # a second factorize drops the border until set_border is called again
        assert s.factorize(A.data) == 0
        assert s.counter("complex_border_columns") == 0
        assert solve(s.h, *solve_args) == ERROR_HIPMF_INVALID_VALUE and solvet(s.h, *solvet_args) == ERROR_HIPMF_INVALID_VALUE
        assert setb(s.h, *border_args) == 0
        assert solve(s.h, *solve_args) == 0 and np.array_equal(x, x0)
        # ... and so does factorize_mapped, after a transposed call has built V
        assert solvet(s.h, *solvet_args) == 0 and s.counter("complex_border_transposed_bytes") > 0
        assert s.factorize_mapped(A.data) == 0
        assert s.counter("complex_border_columns") == 0
        assert solve(s.h, *solve_args) == ERROR_HIPMF_INVALID_VALUE and solvet(s.h, *solvet_args) == ERROR_HIPMF_INVALID_VALUE
        assert setb(s.h, *border_args) == 0
        assert solve(s.h, *solve_args) == 0 and np.array_equal(x, x0)
        # k = 0 frees the border (the pointers may be NULL)
        assert setb(s.h, 0, None, 0, None, 0, None, 0, None, 0) == 0
        assert s.counter("complex_border_columns") == 0 and s.counter("complex_border_transposed_bytes") == 0
        assert solve(s.h, *solve_args) == ERROR_HIPMF_INVALID_VALUE
    finally:
        s.close()


# ---- case 10: reproducible and without side effects ----

def _stats(s):
    i, d = np.zeros(16, np.int64), np.zeros(16)
    assert s.lib.complex_solver_hipmf_get_stats(s.h, i, d) == 0
    return [int(i[8]), int(i[9]), int(i[10]), int(i[11]), int(i[12]), float(d[9])]  # perturbed and zero pivots, refinement steps, launches, |r|_inf


def run_side_effects(lib):
    name, k, nrhs = "zlap483", 3, 3
    F, G = right_hand_sides(name, k, nrhs)
    s = handle(lib, name, nstep=-1)  # (the default refinement of the ordinary solves)
    try:
        assert [s.counter(c) for c in PLAIN_COUNTERS + T_COUNTERS] == [0, 0, 0, 0] and s.counter("complex_border_columns") == 0
        det0 = s.determinant()
        x0, t0 = s.solve(F[0]), s.solve_transpose(F[0])
        keep, st = [s.counter(c) for c in TR_COUNTERS], _stats(s)
        x0b, t0b = s.solve(F[0]), s.solve_transpose(F[0])  # (what a repetition without bordered calls changes)
        keep_b, st_b = [s.counter(c) for c in TR_COUNTERS], _stats(s)
        assert s.set_border(*border(name, k))[1] == 0
        a, b = s.solve_bordered(F[0], G[0]), s.solve_bordered(F[0], G[0])
        assert same_bits(a, b)
        ma, mb = s.solve_bordered(F, G), s.solve_bordered(F, G)
        assert same_bits(ma, mb)
        for conjugate in (True, False):
            ta, tb = s.solve_bordered_transpose(F, G, conjugate=conjugate), s.solve_bordered_transpose(F, G, conjugate=conjugate)
            assert same_bits(ta, tb)
        assert same_bits(s.solve_bordered(F, G), ma)  # (the transposed calls in between have changed no bit of the plain form)
        assert s.counter("complex_bordered_blocks") == 1 and s.counter("complex_border_columns") == k
        # nothing of the ordinary solves has moved: the factor and its determinant, the counters, the statistics
        assert s.determinant() == det0
        assert [s.counter(c) for c in TR_COUNTERS] == keep_b and _stats(s) == st_b
        x1, t1 = s.solve(F[0]), s.solve_transpose(F[0])
        assert same_bits([x0, t0, x0, t0], [x1, t1, x0b, t0b])
        # ... and these solves move the counters and statistics exactly as the same solves did before the bordered calls (a value of the
        # last call stays, a running count grows by the same amount)
        assert [s.counter(c) for c in TR_COUNTERS] == [kb + (kb - ka) for ka, kb in zip(keep, keep_b)]
        assert _stats(s) == [qb + (qb - qa) for qa, qb in zip(st, st_b)]
    finally:
        s.close()
