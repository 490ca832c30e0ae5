"""Matrices whose elimination tree is prescribed by hand, and the extended-precision reference they are checked against.

The suite's other matrices get whatever fronts nested dissection makes of a grid; here the natural order (HIPMF_ORDERING_NONE) and a
block pattern fix them: `two_leaves_and_root(p, m, ...)` gives leaf fronts with p pivots and m off-diagonal rows under a dense m x m
root, `chain(...)` a leaf under a middle front that still has off-diagonal rows of its own when it receives the leaf's contribution
block.  Relaxed amalgamation, the dense path of tiny matrices and supernode splitting may reshape what was asked for, so every user
asserts what `reached()` reports.

`Reference` is plain numpy: a dense LAPACK solve polished with longdouble residuals, the componentwise backward error omega and the
forward error in longdouble, and the same two figures for the unrefined float64 LAPACK solve, which is what the tolerance is set by
(`Reference.check`).  No product code in it."""
import os
from contextlib import contextmanager

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
ORDERING_NONE = 2
SMALL_F = 64       # fronts of at most this many rows: k_small_factor
MID_PMAX = 32      # one-workgroup fronts (k_front_lu): pivots at most ...
MID_MMAX = 192     # ... and off-diagonal rows at most
DENSE_N = 32       # matrices of at most this order are one dense front
RELAX_BIG = 2048   # fronts of at least this many rows absorb a child whatever its columns, if that takes (almost) no explicit zeros
STRONG, WEAK = 3.0, 0.05

# ONE margin for every assertion against the unrefined LAPACK solve (profiles/r08_front_shapes.txt)
C = 16.0


@contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, val in old.items():
            if val is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = val


class Case:
    """n, the CSR arrays handed to the solver (the lower triangle when symmetric), and the dense matrix A they stand for."""

    def __init__(self, A, symmetric):
        self.A = A
        self.n = A.shape[0]
        self.symmetric = symmetric
        M = sp.csr_matrix(np.tril(A) if symmetric else A)
        M.sort_indices()
        self.rp, self.ci, self.v = M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64)


def _block(rng, r, c, s):
    return rng.standard_normal((r, c)) * s


def _sym(B):
    return (B + B.T) / np.sqrt(2.0)


def _pivot_block(rng, p, s, weak, symmetric, group=32):
    """p x p pivot block: N(0, 1) s entries and +3 on the diagonal.  `weak`: +0.05 on the diagonal instead, and the +3 of row i one
    column further (cyclically inside its group of `group` pivots, the rows one diagonal tile of the tiled path searches): every pivot
    search has to interchange rows, none can reach outside its tile, and the block is as well conditioned as the strong one (a
    diagonal of 0.05 alone leaves cond_inf(A) above 1e4 and no pivot of any size to a leaf with a single pivot, which keeps +3)."""
    D = rng.standard_normal((p, p)) * s
    if symmetric:
        D = _sym(D)
    if not weak:
        return D + np.eye(p) * STRONG
    for g0 in range(0, p, group):
        g = min(group, p - g0)
        for i in range(g):
            D[g0 + i, g0 + i] += WEAK if g > 1 else STRONG
            if g > 1:
                D[g0 + i, g0 + (i + 1) % g] += STRONG
        # what the group's first pivot search sees: its largest candidate is not the diagonal entry (the later searches see updated
        # columns; in every original column of the group, too, the +3 sits in the row before)
        assert g == 1 or all(np.argmax(np.abs(D[g0:g0 + g, g0 + c])) == (c - 1) % g for c in range(g))
    return D


def two_leaves_and_root(p, m, seed, weak=False, symmetric=False, leaves=2, group=32, coupling=1.0):
    """`leaves` leaf supernodes of p columns, each coupled densely to the same m later rows / columns, then the dense m x m root.
    Off-diagonal entries are N(0, 1) / sqrt(p + m), so conditioning does not grow with the shape; the diagonal gets +3, or +0.05 on
    the leaves' pivot blocks when `weak` (_pivot_block: the pivot search then has to interchange rows inside the pivot block / the
    32-row diagonal tile).  m = 0: independent dense fronts.  `coupling` scales the leaves' off-diagonal blocks: with many leaves the
    root's Schur complement is the sum of that many updates, and sqrt(2 / leaves) keeps it what two leaves make it."""
    assert not (weak and symmetric)  # (L D L^T takes its pivots from the diagonal)
    rng = np.random.default_rng(seed)
    s = 1.0 / np.sqrt(p + m)
    n = leaves * p + m
    r0 = leaves * p
    A = np.zeros((n, n))
    for g in range(leaves):
        a0 = g * p
        A[a0:a0 + p, a0:a0 + p] = _pivot_block(rng, p, s, weak, symmetric, group)
        A[a0:a0 + p, r0:] = _block(rng, p, m, s * coupling)
        A[r0:, a0:a0 + p] = A[a0:a0 + p, r0:].T if symmetric else _block(rng, m, p, s * coupling)
    R = _block(rng, m, m, s)
    A[r0:, r0:] = (_sym(R) if symmetric else R) + np.eye(m) * STRONG
    return Case(A, symmetric)


def chain(p1, m1, p2, m2, seed, weak=False, symmetric=False):
    """leaf (p1 pivots, m1 off-diagonal rows) -> middle (p2 pivots, m2 off-diagonal rows) -> dense m2 x m2 root.  The leaf's
    off-diagonal rows are spread evenly over ALL rows of the middle front, its first pivot and its last off-diagonal row included,
    so the middle front receives a contribution block that reaches into its own off-diagonal rows, and its parent is the middle
    front's first column.  Two one-pivot leaves come first, one under the middle front and one under the root: a front with two
    children is not folded into its only child's supernode (with one child, middle and root would be ONE fundamental supernode)."""
    assert not (weak and symmetric) and 2 <= m1 <= p2 + m2
    rng = np.random.default_rng(seed)
    leaf0, mid0, root0 = 2, 2 + p1, 2 + p1 + p2
    n = root0 + m2
    A = np.zeros((n, n))
    s1, s2 = 1.0 / np.sqrt(p1 + m1), 1.0 / np.sqrt(p2 + m2)
    rows = np.unique(np.round(np.linspace(mid0, n - 1, m1)).astype(int))  # the leaf's off-diagonal rows
    assert rows.size == m1
    for k, parent in ((0, mid0), (1, root0)):
        A[k, k] = STRONG
        A[k, parent] = A[parent, k] = 0.25
    A[leaf0:mid0, leaf0:mid0] = _pivot_block(rng, p1, s1, weak, symmetric)
    A[leaf0:mid0, rows] = _block(rng, p1, m1, s1)
    A[rows, leaf0:mid0] = A[leaf0:mid0, rows].T if symmetric else _block(rng, m1, p1, s1)
    A[mid0:root0, mid0:root0] = _pivot_block(rng, p2, s2, weak, symmetric)
    A[mid0:root0, root0:] = _block(rng, p2, m2, s2)
    A[root0:, mid0:root0] = A[mid0:root0, root0:].T if symmetric else _block(rng, m2, p2, s2)
    R = _block(rng, m2, m2, s2)
    A[root0:, root0:] = (_sym(R) if symmetric else R) + np.eye(m2) * STRONG
    return Case(A, symmetric)


def complex_two_leaves_and_root(p, m, seed, weak=False, symmetric=False, leaves=2):
    """The complex twin: complex order p, m (real-equivalent fronts of 2p, 2m, paired pivot searches).  Returns the complex dense matrix,
    the CSR pattern and the interleaved (re, im) values; `symmetric`: complex SYMMETRIC (A = A^T, not Hermitian), lower triangle."""
    re = two_leaves_and_root(p, m, seed, weak=weak, symmetric=symmetric, leaves=leaves, group=16)  # (16 complex pivots = one 32-row tile)
    im = two_leaves_and_root(p, m, seed + 7919, weak=False, symmetric=symmetric, leaves=leaves)
    Z = re.A + 1j * (im.A - np.diag(np.diag(im.A)) * 0.5)  # (diagonal 3 + 1.5 i plus noise)
    M = sp.csr_matrix(np.tril(Z) if symmetric else Z)
    M.sort_indices()
    zv = np.ascontiguousarray(np.stack([M.data.real, M.data.imag], axis=1).ravel())
    return Z, M.indptr.astype(np.int32), M.indices.astype(np.int32), zv


def reached(s):
    """What the analysis and the plan made of the matrix: the figures every case asserts."""
    st = s.stats()
    out = {k: st[k] for k in ("nsuper", "max_front", "max_pivots")}
    out.update({k: s.counter(k) for k in ("mid_fronts", "wave_fronts", "leaf_fronts", "symmetric_ldlt")})
    return out


# ---- the reference ----------------------------------------------------------------------------------------------------------------------

def forward_error(x, x_ref):
    return float(np.max(np.abs(np.asarray(x).astype(LD) - x_ref)) / np.max(np.abs(x_ref)))


class Reference:
    """For one matrix: x_ref of any right-hand side to longdouble accuracy, and what unrefined float64 LAPACK reaches on it.  The
    longdouble copy of A and LAPACK's factor (getrf: what numpy.linalg.solve computes per call) are made once; `transposed()` is the
    reference of A^T on the same two."""

    def __init__(self, A, _shared=None):
        assert np.finfo(LD).eps < 2e-19  # x87 extended precision (x86-64)
        self.A = A
        self.trans = _shared is not None
        if _shared is None:
            self.Al = A.astype(LD)
            self._lu = sla.lu_factor(A)
            inv = np.linalg.inv(A)  # (for cond_inf only)
            self.cond, self._cond_t = float(np.linalg.norm(A, np.inf) * np.linalg.norm(inv, np.inf)), float(np.linalg.norm(A, 1) * np.linalg.norm(inv, 1))
        else:
            self.Al, self._lu, self.cond = _shared.Al, _shared._lu, _shared._cond_t
        self.M = self.Al.T if self.trans else self.Al
        self._known = {}

    def transposed(self):
        return Reference(self.A, _shared=self)

    def _lapack(self, b):
        return sla.lu_solve(self._lu, b, trans=int(self.trans))

    def omega(self, x, b):
        """max_i |b - A x|_i / (|A||x| + |b|)_i in longdouble (Oettli-Prager: the componentwise backward error)"""
        xl, bl = np.asarray(x).astype(LD), np.asarray(b).astype(LD)
        r = np.abs(bl - self.M @ xl)
        ax, d = np.abs(xl), np.abs(bl)
        for i in range(0, d.size, 1024):  # (row blocks: no second longdouble copy of a large matrix)
            d[i:i + 1024] += np.abs(self.M[i:i + 1024]) @ ax
        ok = d > 0
        assert np.all(r[~ok] == 0)
        return float(np.max(r[ok] / d[ok])) if np.any(ok) else 0.0

    def prepare(self, b):
        """(x_ref in longdouble, omega and forward error of the unrefined float64 LAPACK solve), remembered per right-hand side"""
        key = np.asarray(b).tobytes()
        if key not in self._known:
            x0 = self._lapack(np.asarray(b, dtype=np.float64))
            bl = np.asarray(b).astype(LD)
            x = x0.astype(LD)
            last = np.inf
            for _ in range(12):
                r = bl - self.M @ x
                d = self._lapack(r.astype(np.float64)).astype(LD)  # (longdouble residual, float64 correction, longdouble sum)
                x = x + d
                step = float(np.max(np.abs(d)) / np.max(np.abs(x)))
                # done below 1e-18 |x|.  A residual formed in longdouble is itself only good to eps_ld |A||x|, so the corrections of a
                # large system stop shrinking at about eps_ld cond_inf |x| (order 8 000: a few 1e-18); a correction that no longer
                # halves AND is below that floor is as far as this arithmetic goes -- still 2 000 times below eps cond_inf, the scale
                # every forward error is judged on
                if step <= 1e-18 or (step > 0.5 * last and step <= float(np.finfo(LD).eps) * self.cond):
                    break
                last = step
            else:
                raise AssertionError("the reference did not converge: cond_inf = %.3g" % self.cond)
            self._known[key] = (x, self.omega(x0, b), forward_error(x0, x))
        return self._known[key]

    def figures(self, x, b):
        """omega, omega_lapack, fe, fe_lapack of x for A x = b"""
        x_ref, om_l, fe_l = self.prepare(b)
        return self.omega(x, b), om_l, forward_error(x, x_ref), fe_l

    def check(self, x, b, what, log=None):
        om, om_l, fe, fe_l = self.figures(x, b)
        if log is not None:
            log.append("%-44s omega %.3e omega_lapack %.3e fe %.3e fe_lapack %.3e cond_inf %.3e" % (what, om, om_l, fe, fe_l, self.cond))
        assert np.all(np.isfinite(x)), what
        assert om <= C * max(om_l, EPS), (what, "omega", om, om_l)
        assert fe <= C * max(fe_l, EPS * self.cond), (what, "forward error", fe, fe_l, self.cond)
        return om, om_l, fe, fe_l


def check_determinant(A, coefficient, exponent):
    """mantissa * 10^exponent against slogdet of the dense matrix (the bound of tests/test_mid_fronts_cpu.py)"""
    sign, logdet = np.linalg.slogdet(A)
    assert np.sign(coefficient) == sign and abs(np.log10(abs(coefficient)) + exponent - logdet / np.log(10.0)) < 1e-9


# ---- what a two-leaf / chain case must turn into ---------------------------------------------------------------------------------------

def kind(p, m):
    """the factorisation kernel of a front with p pivots and m off-diagonal rows on the default schedule"""
    if p + m <= SMALL_F:
        return "small"
    return "one-workgroup" if p <= MID_PMAX and m <= MID_MMAX else "tiled"


def expect_two_leaves(p, m, leaves=2, tiled_only=False):
    """stats()/counters of two_leaves_and_root(p, m).  With p + m <= 64 (or >= 2048) the relaxed amalgamation folds the last leaf into
    the root (no explicit zero is needed for that): one front of p + m pivots next to the remaining leaves of p pivots and m rows."""
    assert leaves * p + m > DENSE_N  # (smaller matrices are one dense front)
    if m == 0:
        e = {"nsuper": leaves, "max_front": p, "max_pivots": p}
    elif p + m <= SMALL_F or p + m >= RELAX_BIG:
        e = {"nsuper": leaves, "max_front": p + m, "max_pivots": p + m}
    else:
        e = {"nsuper": leaves + 1, "max_front": p + m, "max_pivots": max(p, m)}
    e["mid_fronts"] = 0 if tiled_only else leaves * (kind(p, m) == "one-workgroup") + (m > 0 and kind(m, 0) == "one-workgroup")
    return e


def expect_chain(p1, m1, p2, m2):
    assert kind(p2, m2) == "tiled" and p1 + p2 > 64  # (at most 64 columns: the middle front could absorb the leaf)
    return {"nsuper": 5, "max_front": max(p1 + m1, p2 + m2), "max_pivots": max(p1, p2, m2), "mid_fronts": int(kind(p1, m1) == "one-workgroup")}


# ---- one case, every solve path -------------------------------------------------------------------------------------------------------

def run_case(lib, case, expect, weak, env, log, name, columns=(9, 17)):
    """Factorise once WITHOUT refinement; solve, solve_many with 9 and 17 columns (the 8- and 16-column instances) and solve_transpose
    on the default schedule, then the same on a second handle whose solves are the level-set launches (HIPMF_FUSED_SOLVE=0, read at
    initialize).  Every solution against the longdouble reference, bounded by C times what unrefined LAPACK reaches; the determinant
    against slogdet.  `expect`: the figures of reached() the case is about."""
    from russell_amd.backend import Hipmf
    rng = np.random.default_rng(5)
    b = rng.standard_normal(case.n)
    B = {k: rng.standard_normal((k, case.n)) for k in columns}
    ref = Reference(case.A)
    ref_t = ref.transposed()
    for schedule, extra in (("default", {}), ("level-set", {"HIPMF_FUSED_SOLVE": "0"})):
        with environment(dict(env, **extra)):
            s = Hipmf(lib)
            try:
                if weak:  # (a maximum-product matching would put the +3 back on the diagonal: the interchanges are the point)
                    assert s.set_option("matching", 0) == 0
                assert s.initialize(case.n, case.rp, case.ci, ordering=ORDERING_NONE, refinement_nstep=0, general_symmetric=case.symmetric) == 0
                assert s.factorize(case.v, compute_determinant=True) == 0
                assert s.num_perturbed == 0 and s.counter("rematch") == 0
                got = reached(s)
                if schedule == "default":
                    log.append("%-40s n %d asked %s reached %s" % (name, case.n, expect, got))
                for k, val in expect.items():
                    assert got[k] == val, (name, k, got, expect)
                assert got["symmetric_ldlt"] == int(case.symmetric)
                check_determinant(case.A, s.det_coefficient, s.det_exponent)
                tag = "%s [%s]" % (name, schedule)
                ref.check(s.solve(b), b, tag + " solve", log)
                ref_t.check(s.solve_transpose(b), b, tag + " transpose", log)
                for k in columns:
                    X = s.solve_many(B[k])
                    for j in range(k):
                        ref.check(X[j], B[k][j], tag + " many%d col %d" % (k, j), log)
                assert s.stats()["refinement_steps"] == 0 and s.counter("krylov_iterations") == 0
            finally:
                s.close()


class ComplexReference(Reference):
    """the same for a complex matrix (numpy has no complex longdouble LAPACK either: clongdouble residuals, complex128 corrections)"""

    def __init__(self, Z):
        assert np.finfo(LD).eps < 2e-19
        self.A = Z
        self.Al = Z.astype(np.clongdouble)
        self._known = {}
        self._inv = np.linalg.inv(Z)
        self.cond = float(np.linalg.norm(Z, np.inf) * np.linalg.norm(self._inv, np.inf))

    def prepare(self, b):
        key = np.asarray(b).tobytes()
        if key not in self._known:
            x0 = np.linalg.solve(self.A, b)
            bl = np.asarray(b).astype(np.clongdouble)
            x = x0.astype(np.clongdouble)
            for _ in range(12):
                d = (self._inv @ (bl - self.Al @ x).astype(np.complex128)).astype(np.clongdouble)
                x = x + d
                if np.max(np.abs(d)) <= 1e-18 * np.max(np.abs(x)):
                    break
            else:
                raise AssertionError("the reference did not converge: cond_inf = %.3g" % self.cond)
            self._known[key] = (x, self._omega(x0, b), forward_error_c(x0, x))
        return self._known[key]

    def _omega(self, x, b):
        xl, bl = np.asarray(x).astype(np.clongdouble), np.asarray(b).astype(np.clongdouble)
        return float(np.max(np.abs(bl - self.Al @ xl) / (np.abs(self.Al) @ np.abs(xl) + np.abs(bl))))

    def figures(self, x, b):
        x_ref, om_l, fe_l = self.prepare(b)
        return self._omega(x, b), om_l, forward_error_c(x, x_ref), fe_l


def forward_error_c(x, x_ref):
    return float(np.max(np.abs(np.asarray(x).astype(np.clongdouble) - x_ref)) / np.max(np.abs(x_ref)))
