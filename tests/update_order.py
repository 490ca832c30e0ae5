"""Shared by tests/test_update_order_cpu.py and tests/test_update_order_gpu.py: the order of the workgroups of a trailing-update launch.

With HIPMF_UPD_LA_FIRST=1 (the default) the look-ahead pieces of a step's fronts are workgroups 0 .. nfollow - 1 of the k_update /
k_update32 launch and the tiles of all fronts follow; with 0 every look-ahead piece is the last workgroup of its front's range.  Both
orders run the same independent workgroups, so two handles that differ in the knob alone must agree bit for bit, and the default one
must stay inside tests/front_shapes.py's margin C of what unrefined LAPACK reaches.

The matrices: the natural order and a block pattern as `front_shapes.two_leaves_and_root`, but with leaves of DIFFERENT pivot counts on
one level, so that the number of fronts with a look-ahead piece shrinks from step to step and the fronts' tile counts differ.  The
leaves are listed with non-increasing pivots (the plan sorts them that way: slot order = the order given here)."""
import ctypes as C

import numpy as np

import front_shapes as F
from russell_amd._capi import load
from russell_amd.backend import Hipmf

NB = 32  # pivots per step of the tiled path


def leaves_and_root(ps, m, seed, weak=False, symmetric=False, group=32):
    """one leaf supernode of p columns for every p of `ps`, each coupled densely to the same m later rows / columns, then the dense
    m x m root.  Entries as front_shapes.two_leaves_and_root: N(0, 1) / sqrt(p + m) off the diagonal (the leaves' coupling blocks scaled
    by sqrt(2 / leaves), which keeps the root's Schur complement what two leaves make it), +3 on the diagonal, `weak`: pivot blocks
    whose every pivot search interchanges rows inside its 32-row diagonal tile."""
    assert not (weak and symmetric)
    rng = np.random.default_rng(seed)
    leaves = len(ps)
    coupling = min(1.0, float(np.sqrt(2.0 / leaves)))
    r0 = int(sum(ps))
    n = r0 + m
    A = np.zeros((n, n))
    a0 = 0
    for p in ps:
        s = 1.0 / np.sqrt(p + m)
        A[a0:a0 + p, a0:a0 + p] = F._pivot_block(rng, p, s, weak, symmetric, group)
        A[a0:a0 + p, r0:] = F._block(rng, p, m, s * coupling)
        A[r0:, a0:a0 + p] = A[a0:a0 + p, r0:].T if symmetric else F._block(rng, m, p, s * coupling)
        a0 += p
    s = 1.0 / np.sqrt(max(ps) + m)
    R = F._block(rng, m, m, s)
    A[r0:, r0:] = ((R + R.T) / np.sqrt(2.0) if symmetric else R) + np.eye(m) * F.STRONG
    return F.Case(A, symmetric)


def expect(ps, m):
    """stats() / counters of leaves_and_root(ps, m): every leaf a tiled front of its own, the root above them"""
    assert all(F.kind(p, m) == "tiled" for p in ps) and F.kind(m, 0) == "tiled"  # (p > 32 or m > 192: never a one-workgroup front)
    assert all(F.SMALL_F < p + m < F.RELAX_BIG for p in ps)                       # (no leaf is folded into the root)
    return {"nsuper": len(ps) + 1, "max_front": max(ps) + m, "max_pivots": max(max(ps), m), "mid_fronts": 0}


def nfollow_per_step(ps):
    """look-ahead pieces of the leaves' level, step by step"""
    return [sum(p > k0 + NB for p in ps) for k0 in range(0, max(ps), NB)]


# name -> (pivots of the leaves, m, symmetric, extra environment).  LU cases have weak pivot blocks: every look-ahead tile interchanges rows.
CASES = {
    # 32 x 32 tiles (largest front 166 rows); nfollow 3 -> 1 -> 0; at most four fronts: the prefix words are kernel arguments; p = 33: a one-pivot second step
    "a-three-leaves": ((96, 64, 33), 70, False, {}),
    # six fronts: prefix words from memory, one load and a ballot
    "b-six-leaves": ((96, 96, 64, 40, 33, 33), 70, False, {}),
    # seventy fronts: the binary search
    "c-seventy-leaves": (tuple([40] * 35 + [33] * 35), 70, False, {}),
    # 64 x 64 tiles (largest front 326 rows); the p = 20 leaf is tiled because m > 192 and never has a look-ahead piece
    "d-three-kinds": ((96, 64, 20), 230, False, {}),
    # nine and eight tiles per dimension in the full step k0 = 32: the XCD-aware order behind one look-ahead piece
    "e-xcd-order": ((96, 64), 420, False, {}),
    "f-symmetric-a": ((96, 64, 33), 70, True, {}),
    "f-symmetric-d": ((96, 64, 20), 230, True, {}),
}
# (emulator file only) an explicit HIPMF_UPD32_MAXF also applies to symmetric fronts: the L D L^T instance of k_update32
CASES_CPU_ONLY = {"f-symmetric-a-upd32": ((96, 64, 33), 70, True, {"HIPMF_UPD32_MAXF": "256"})}
COMPLEX = (40, 35)  # complex order p, m: real-equivalent leaves of 80 pivots and 70 rows, three steps, the PAIRED instance


def build(name):
    ps, m, symmetric, env = dict(CASES, **CASES_CPU_ONLY)[name]
    assert list(ps) == sorted(ps, reverse=True)
    seed = 1000 * len(ps) + m
    return leaves_and_root(ps, m, seed, weak=not symmetric, symmetric=symmetric), expect(ps, m), env


def _factor_words(s):
    """the row interchanges of the tiled and small fronts and the pivots, as they lie on the device"""
    parts = s.factor_buffers()
    lperm, diag = np.zeros(parts[1][1] // 4, np.int32), np.zeros(parts[3][1] // 8)
    s.d2h(lperm, parts[1][0])
    s.d2h(diag, parts[3][0])
    return lperm, diag


def run_real(lib, name, log):
    """two handles, HIPMF_UPD_LA_FIRST = 0 and 1, factorise and solve without refinement: bit for bit, then the default against the reference"""
    case, want, env = build(name)
    weak = not case.symmetric
    b = np.random.default_rng(5).standard_normal(case.n)
    out = {}
    for knob in ("0", "1"):
        with F.environment(dict(env, HIPMF_UPD_LA_FIRST=knob)):
            s = Hipmf(lib)
            try:
                if weak:  # (a maximum-product matching would put the +3 back on the diagonal: the interchanges are the point)
                    assert s.set_option("matching", 0) == 0
                assert s.initialize(case.n, case.rp, case.ci, ordering=F.ORDERING_NONE, refinement_nstep=0, general_symmetric=case.symmetric) == 0
                assert s.factorize(case.v, compute_determinant=True) == 0
                got = F.reached(s)
                for k, val in want.items():
                    assert got[k] == val, (name, k, got, want)
                assert got["symmetric_ldlt"] == int(case.symmetric) and s.counter("rematch") == 0
                x = s.solve(b)
                assert s.stats()["refinement_steps"] == 0 and s.counter("krylov_iterations") == 0
                lperm, diag = _factor_words(s)
                out[knob] = (x, float(s.det_coefficient), float(s.det_exponent), int(s.num_perturbed), s.permutation(), lperm, diag)
            finally:
                s.close()
    log.append("%-24s n %d reached %s look-ahead pieces per step %s" % (name, case.n, want, nfollow_per_step(dict(CASES, **CASES_CPU_ONLY)[name][0])))
    x0, c0, e0, np0, perm0, lperm0, diag0 = out["0"]
    x1, c1, e1, np1, perm1, lperm1, diag1 = out["1"]
    assert np.all(np.isfinite(x1))
    assert x0.tobytes() == x1.tobytes(), (name, "x", float(np.max(np.abs(x0 - x1))))
    assert np.float64(c0).tobytes() == np.float64(c1).tobytes() and np.float64(e0).tobytes() == np.float64(e1).tobytes(), (name, "determinant", c0, e0, c1, e1)
    assert np0 == np1 == 0, (name, "n_perturbed", np0, np1)
    assert np.array_equal(perm0, perm1), (name, "permutation")
    assert lperm0.tobytes() == lperm1.tobytes(), (name, "row interchanges")
    assert diag0.tobytes() == diag1.tobytes(), (name, "pivots")
    if weak:
        assert np.any(lperm1 != 0)  # (the look-ahead tiles did interchange rows)
    F.check_determinant(case.A, c1, e1)
    F.Reference(case.A).check(x1, b, name + " solve", log)


def run_complex(lib_path, log):
    """the complex twin (general storage, weak pivot blocks: paired pivot searches with interchanges) on two handles"""
    p, m = COMPLEX
    Z, rp, ci, zv = F.complex_two_leaves_and_root(p, m, 100 * p + m, weak=True, symmetric=False)
    n = Z.shape[0]
    lib = load(lib_path)
    rng = np.random.default_rng(5)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    bi = np.ascontiguousarray(np.stack([b.real, b.imag], axis=1).ravel())
    want = F.expect_two_leaves(2 * p, 2 * m)
    assert F.kind(2 * p, 2 * m) == "tiled" and want["mid_fronts"] == 0 and 2 * p > 2 * NB  # (three steps)
    out = {}
    for knob in ("0", "1"):
        h = lib.complex_solver_hipmf_new()
        assert h
        try:
            with F.environment({"HIPMF_MATCHING": "0", "HIPMF_UPD_LA_FIRST": knob}):
                assert lib.complex_solver_hipmf_initialize(h, F.ORDERING_NONE, 1, -1.0, 0, 0, 0, n, rp, ci, None) == 0
            npert, rc, dre, dim, dex = C.c_int32(), C.c_double(), C.c_double(), C.c_double(), C.c_double()
            assert lib.complex_solver_hipmf_factorize(h, None, None, C.byref(npert), C.byref(rc), C.byref(dre), C.byref(dim), C.byref(dex), 1, 0, zv) == 0
            ist, dst = np.zeros(16, np.int64), np.zeros(16)
            assert lib.complex_solver_hipmf_get_stats(h, ist, dst) == 0
            counter = lambda k: int(lib.complex_solver_hipmf_get_counter(h, Hipmf.COUNTERS[k]))
            got = {"nsuper": int(ist[2]), "max_front": int(ist[6]), "max_pivots": int(ist[7]), "mid_fronts": counter("mid_fronts")}
            assert got == want and counter("rematch") == 0, (got, want)
            x = np.zeros(2 * n)
            assert lib.complex_solver_hipmf_solve(h, x, bi, 0) == 0
            assert int(ist[10]) == 0 and counter("krylov_iterations") == 0
            out[knob] = (x, np.array([dre.value, dim.value, dex.value]), int(npert.value))
        finally:
            lib.complex_solver_hipmf_drop(h)
    (x0, d0, np0), (x1, d1, np1) = out["0"], out["1"]
    assert x0.tobytes() == x1.tobytes(), ("complex x", float(np.max(np.abs(x0 - x1))))
    assert d0.tobytes() == d1.tobytes(), ("complex determinant", d0, d1)
    assert np0 == np1 == 0
    sign, logabs = np.linalg.slogdet(Z)
    mant = complex(d1[0], d1[1])
    assert abs(np.log10(abs(mant)) + d1[2] - logabs / np.log(10.0)) < 1e-9 and abs(mant / abs(mant) - sign) < 1e-9
    F.ComplexReference(Z).check(x1[0::2] + 1j * x1[1::2], b, "complex p=%d m=%d solve" % (p, m), log)
