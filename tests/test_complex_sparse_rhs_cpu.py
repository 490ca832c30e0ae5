"""Sparse right-hand sides, selected rows and entries of the inverse for the complex handle (complex_solver_hipmf_solve_sparse with
trans = 0, 1, 2 for A, A^T, A^H; complex_solver_hipmf_inverse_entries) on the CPU emulator of the HIP kernels.
tests/test_complex_sparse_rhs_gpu.py repeats the run_* cases on the device (lib None = the product build).

The tolerance rule is that of tests/test_sparse_rhs_cpu.py (its FACTOR, FLOOR_ULPS and check_rule, |.| the complex modulus): the pruned
pass pair against numpy's dense solution with op(A), the yardstick being the handle's own unrefined solve of the expanded column --
complex_solver_hipmf_solve_many for trans = 0, complex_solver_hipmf_solve_transpose column by column for trans = 1, 2.
Measured ratios: profiles/r16_sparse_rhs_transpose.txt."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from russell_amd._capi import load
from test_complex_error_analysis_cpu import as_complex, interleave
from test_solve_updated_complex_cpu import (ERROR_HIPMF_INVALID_VALUE, ERROR_NEED_FACTORIZATION, ERROR_NEED_INITIALIZATION, ERROR_NULL_POINTER, ZH, full, matrix,
                                            perturbed_matrix, shifted_grid, structure)
from test_sparse_rhs_cpu import EPS, FACTOR, FLOOR_ULPS, _prune_always, check_rule

PRUNED_FWD_FRONTS, PRUNED_BWD_FRONTS, PRUNED_BLOCKS, PRUNED_TRANSPOSED_BLOCKS = 24, 25, 26, 38
OPS = {0: lambda A: A, 1: lambda A: A.T, 2: lambda A: A.conj().T}


def bits(z):
    return np.ascontiguousarray(z).view(np.uint64)


def counter(s, which):
    return int(s.lib.complex_solver_hipmf_get_counter(s.h, which))


def case(name):
    """name -> ((n, rp, ci, v0), keywords of ZH, dense A)"""
    if name == "grid":  # 30 x 28 complex shifted grid with an unsymmetric Laplacian: neither symmetric nor Hermitian
        n, rp, ci, vals = shifted_grid(30, 28, unsym=True)
        c, kw = (n, rp, ci, vals(1.0)), {}
    else:
        c, kw = matrix(name)
    return c, kw, full(*c, lower=kw.get("lower", False)).toarray()


def zcolumns(n, counts, seed):
    """compressed complex columns (ascending rows), and the same as dense rows"""
    rng = np.random.default_rng(seed)
    ptr, idx, val = [0], [], []
    for k in counts:
        r = np.sort(rng.choice(n, size=min(k, n), replace=False))
        idx += list(r)
        val += list(rng.uniform(0.5, 2.0, r.size) * np.exp(1j * rng.uniform(-np.pi, np.pi, r.size)))
        ptr.append(len(idx))
    ptr, idx, val = np.array(ptr, np.int32), np.array(idx, np.int32), np.array(val, complex)
    B = np.zeros((len(counts), n), complex)
    for c in range(len(counts)):
        B[c, idx[ptr[c]:ptr[c + 1]]] = val[ptr[c]:ptr[c + 1]]
    return ptr, idx, val, B


def zsparse(s, ptr, idx, val, trans, select=None, ldx=None, fill=0.0):
    """(nrhs, ldx) complex array: row c holds the selected entries of column c in its first nsel places"""
    nrhs = ptr.size - 1
    sel = None if select is None else np.ascontiguousarray(select, np.int32)
    nsel = s.n if sel is None else sel.size
    ldx = nsel if ldx is None else ldx
    x = np.full((nrhs, 2 * ldx), fill)
    code = s.lib.complex_solver_hipmf_solve_sparse(s.h, x, ldx, nrhs, ptr, idx, interleave(val), nsel, None if sel is None else sel.ctypes.data, trans, 0)
    if code != 0:
        raise s.error(code)
    return x.view(complex)


def yardstick(s, B, trans):
    """the handle's own unrefined solves of the dense columns"""
    nrhs, n = B.shape
    if trans == 0:
        x, b = np.zeros((nrhs, 2 * n)), np.ascontiguousarray(B).view(float)
        assert s.lib.complex_solver_hipmf_solve_many(s.h, x, b, nrhs, n, 0) == 0
        return x.view(complex)
    X = np.zeros((nrhs, n), complex)
    for c in range(nrhs):
        x = np.zeros(2 * n)
        assert s.lib.complex_solver_hipmf_solve_transpose(s.h, x, interleave(B[c]), int(trans == 2), 0) == 0
        X[c] = as_complex(x)
    return X


def run_accuracy(lib, name, counts=(1, 3, 0, 2, 9, 1, 40), env=None):
    c, kw, A = case(name)
    n = c[0]
    ptr, idx, val, B = zcolumns(n, counts, 2)
    Xd = {t: np.linalg.solve(OPS[t](A), B.T).T for t in OPS}
    live = [k for k, cnt in enumerate(counts) if cnt]
    symmetric = kw.get("lower", False)
    for a, b in ((0, 1), (0, 2), (1, 2)):  # the three systems must be told apart by the checks below
        if symmetric and (a, b) == (0, 1):
            continue
        assert all(np.abs(Xd[a][k] - Xd[b][k]).max() > 1e-3 * np.abs(Xd[a][k]).max() for k in live), (a, b)
    s = ZH(lib, *c, env=env, **kw)
    worst = {}
    try:
        assert s.num_perturbed == 0
        for t in OPS:
            X = zsparse(s, ptr, idx, val, t)
            assert counter(s, PRUNED_BLOCKS) == 1
            assert counter(s, PRUNED_TRANSPOSED_BLOCKS) == int(t == 2 or (t == 1 and not symmetric))
            worst[t] = check_rule(X, yardstick(s, B, t), Xd[t], "%s trans=%d" % (name, t))
        if symmetric:  # A^T = A: the same path, the same bits
            assert np.array_equal(bits(zsparse(s, ptr, idx, val, 1)), bits(zsparse(s, ptr, idx, val, 0)))
    finally:
        s.close()
    print("largest ratios on %s: %s" % (name, ", ".join("trans=%d %.2f" % kv for kv in sorted(worst.items()))))
    return worst


def run_selection(lib, name):
    c, kw, A = case(name)
    n = c[0]
    ptr, idx, val, _ = zcolumns(n, (1, 4, 0, 2, 1), 4)
    sel = np.random.default_rng(4).choice(n, size=min(6, n), replace=False).astype(np.int32)
    sel = np.concatenate([sel, sel[:2]])
    s = ZH(lib, *c, **kw)
    try:
        for t in OPS:
            X = zsparse(s, ptr, idx, val, t)
            Xs = zsparse(s, ptr, idx, val, t, select=sel)
            assert counter(s, PRUNED_BLOCKS) == 1 and counter(s, PRUNED_BWD_FRONTS) <= s.stats()[0][2]
            assert np.array_equal(bits(Xs), bits(X[:, sel])), t
            Xp = zsparse(s, ptr, idx, val, t, select=sel, ldx=sel.size + 3, fill=-7.0)  # ldx in complex elements; the padding is not written
            assert np.array_equal(bits(Xp[:, :sel.size]), bits(Xs)) and np.all(Xp[:, sel.size:].view(float) == -7.0)
            assert not X[2].any() and not Xs[2].any()  # (the empty column)
    finally:
        s.close()


def run_inverse_entries(lib, name):
    c, kw, A = case(name)
    n = c[0]
    rng = np.random.default_rng(12)
    cols = rng.choice(n, size=min(20, n), replace=False)
    rows = rng.integers(0, n, cols.size)
    rows, cols = np.concatenate([rows, rows[:5], rng.integers(0, n, 7)]), np.concatenate([cols, cols[:5], cols[:7]])
    pi = rng.permutation(rows.size)
    rows, cols = rows[pi].astype(np.int32), cols[pi].astype(np.int32)
    s = ZH(lib, *c, **kw)
    try:
        out = np.zeros(2 * rows.size)
        assert s.lib.complex_solver_hipmf_inverse_entries(s.h, rows.size, rows, cols, out, 0) == 0
        vals = as_complex(out)
        uc = np.unique(cols)
        assert uc.size > 16 and counter(s, PRUNED_BLOCKS) == (uc.size + 15) // 16 and counter(s, PRUNED_TRANSPOSED_BLOCKS) == 0
        Xm = yardstick(s, np.eye(n, dtype=complex)[uc], 0)
        Ainv = np.linalg.inv(A)
        for k, col in enumerate(uc):
            m = cols == col
            xd = Ainv[:, col]
            floor = FLOOR_ULPS * EPS * np.abs(xd).max()
            e_ref, e_p = np.abs(Xm[k] - xd).max(), np.abs(vals[m] - xd[rows[m]]).max()
            print("complex inverse_entries column %d: %.3e, yardstick %.3e" % (col, e_p, e_ref))
            assert e_p <= FACTOR * e_ref + floor, (col, e_p, e_ref)
        for e in range(rows.size):
            assert np.all(vals[(rows == rows[e]) & (cols == cols[e])] == vals[e])
    finally:
        s.close()


def run_perturbed(lib):
    """replaced pivots: every block goes to the ordinary / transposed solve of the expanded columns, whose bits come back"""
    A = perturbed_matrix()
    c = structure(A)
    n = c[0]
    s = ZH(lib, *c, env={"HIPMF_MATCHING": "0"}, pivot_epsilon=1e-13, ordering=2)
    try:
        assert s.num_perturbed > 0
        ptr, idx, val, B = zcolumns(n, (3, 1, 2), 8)
        sel = np.array([5, n - 1, 0], np.int32)
        for t in OPS:
            X = zsparse(s, ptr, idx, val, t)
            assert counter(s, PRUNED_BLOCKS) == 0 and counter(s, PRUNED_TRANSPOSED_BLOCKS) == 0
            assert np.array_equal(bits(X), bits(yardstick(s, B, t))), t
            assert np.array_equal(bits(zsparse(s, ptr, idx, val, t, select=sel)), bits(X[:, sel]))
    finally:
        s.close()


def run_unchanged_state(lib, name):
    """the bits of complex_solver_hipmf_solve, the determinant and the statistics around the new calls"""
    c, kw, A = case(name)
    n = c[0]
    b = np.random.default_rng(5).standard_normal(n) + 1j * np.random.default_rng(6).standard_normal(n)
    s = ZH(lib, *c, nstep=-1, **kw)
    try:
        def snapshot():
            x = s.solve(b)
            i, d = s.stats()
            keep = np.concatenate([i[:11], i[13:]])  # (without the launch counts and timers, which every solve moves)
            return bits(x).copy(), keep, d[:4].copy(), d[9], np.array(s.determinant())
        before = snapshot()
        ptr, idx, val, _ = zcolumns(n, (2, 5, 1), 3)
        for t in OPS:
            zsparse(s, ptr, idx, val, t, select=[0, n - 1])
        out = np.zeros(4)
        assert s.lib.complex_solver_hipmf_inverse_entries(s.h, 2, np.array([0, 1], np.int32), np.array([1, n - 1], np.int32), out, 0) == 0
        for a, c2 in zip(before, snapshot()):
            assert np.array_equal(a, c2)
    finally:
        s.close()


def run_status_codes(lib):
    """the order of solver_hipmf_solve_sparse: initialize, factorize, NULL pointers, invalid values; trans outside 0 .. 2"""
    c, _ = matrix("ref5")
    n = c[0]
    ptr, idx, val = np.array([0, 1, 2], np.int32), np.array([0, 3], np.int32), interleave(np.array([1.0 + 1j, 2.0]))
    x = np.zeros((2, 2 * n))
    s = ZH(lib, *c, factorize=False)
    fresh = load(lib).complex_solver_hipmf_new()
    try:
        call, inv = s.lib.complex_solver_hipmf_solve_sparse, s.lib.complex_solver_hipmf_inverse_entries
        r1, out1 = np.array([0], np.int32), np.zeros(2)
        assert call(fresh, x, n, 2, ptr, idx, val, 0, None, 0, 0) == ERROR_NEED_INITIALIZATION
        assert inv(fresh, 1, r1, r1, out1, 0) == ERROR_NEED_INITIALIZATION
        assert call(s.h, x, n, 2, ptr, idx, val, 0, None, 3, 0) == ERROR_NEED_FACTORIZATION  # (before the invalid values)
        assert inv(s.h, 1, r1, r1, out1, 0) == ERROR_NEED_FACTORIZATION
        assert s.lib.complex_solver_hipmf_factorize(s.h, None, None, None, None, None, None, None, 0, 0, interleave(c[3])) == 0
        bad = ERROR_HIPMF_INVALID_VALUE
        sel = np.array([1, 1, 4], np.int32)
        for t in OPS:
            assert call(s.h, x, n, 2, ptr, idx, val, 0, None, t, 0) == 0
            assert call(s.h, x, 3, 2, ptr, idx, val, 3, sel.ctypes.data, t, 0) == 0  # (duplicates in the selection are fine)
        assert call(s.h, x, n, 2, ptr, idx, val, 0, None, 3, 0) == bad and call(s.h, x, n, 2, ptr, idx, val, 0, None, -1, 0) == bad  # trans
        assert call(s.h, x, n, 0, ptr, idx, val, 0, None, 0, 0) == bad  # nrhs < 1
        assert call(s.h, x, n - 1, 2, ptr, idx, val, 0, None, 0, 0) == bad  # ldx < n with all rows
        assert call(s.h, x, 2, 2, ptr, idx, val, 3, sel.ctypes.data, 0, 0) == bad  # ldx < nsel
        assert call(s.h, x, 3, 2, ptr, idx, val, 0, sel.ctypes.data, 0, 0) == bad  # nsel < 1 with a selection
        assert call(s.h, x, n, 2, ptr, np.array([0, n], np.int32), val, 0, None, 0, 0) == bad  # row out of range
        assert call(s.h, x, n, 2, ptr, np.array([-1, 2], np.int32), val, 0, None, 2, 0) == bad
        p1 = np.array([0, 2], np.int32)
        assert call(s.h, x, n, 1, p1, np.array([3, 1], np.int32), val, 0, None, 0, 0) == bad  # unsorted rows in a column
        assert call(s.h, x, n, 1, p1, np.array([2, 2], np.int32), val, 0, None, 1, 0) == bad  # duplicate rows in a column
        assert call(s.h, x, n, 2, np.array([0, 2, 1], np.int32), idx, val, 0, None, 0, 0) == bad  # decreasing column pointers
        assert call(s.h, x, 3, 2, ptr, idx, val, 3, np.array([0, 5, 1], np.int32).ctypes.data, 0, 0) == bad  # selected row out of range
        assert inv(s.h, 0, r1, r1, out1, 0) == bad
        assert inv(s.h, 1, np.array([n], np.int32), r1, out1, 0) == bad
        assert inv(s.h, 1, r1, np.array([-1], np.int32), out1, 0) == bad
        raw = C.CDLL(s.lib._name)  # (untyped bindings: NULL pointers pass)
        raw.complex_solver_hipmf_solve_sparse.restype = raw.complex_solver_hipmf_inverse_entries.restype = C.c_int32
        h, xp, pp, ip, vp = C.c_void_p(s.h), x.ctypes.data_as(C.c_void_p), ptr.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p)
        for args in ((None, xp, pp, ip, vp), (h, None, pp, ip, vp), (h, xp, None, ip, vp), (h, xp, pp, None, vp), (h, xp, pp, ip, None)):
            assert raw.complex_solver_hipmf_solve_sparse(args[0], args[1], n, 2, args[2], args[3], args[4], 0, None, 0, 0) == ERROR_NULL_POINTER
        assert raw.complex_solver_hipmf_inverse_entries(h, 1, None, ip, vp, 0) == ERROR_NULL_POINTER
        assert raw.complex_solver_hipmf_inverse_entries(None, 1, ip, ip, vp, 0) == ERROR_NULL_POINTER
    finally:
        s.lib.complex_solver_hipmf_drop(fresh)
        s.close()


# ---- the tests on the emulator ----

def test_exports(emu_lib):
    raw = C.CDLL(emu_lib)
    for name in ("complex_solver_hipmf_solve_sparse", "complex_solver_hipmf_inverse_entries"):
        assert hasattr(raw, name), name
    c, kw = matrix("ref5")
    s = ZH(emu_lib, *c, **kw)
    try:
        assert [counter(s, k) for k in (PRUNED_FWD_FRONTS, PRUNED_BWD_FRONTS, PRUNED_BLOCKS, PRUNED_TRANSPOSED_BLOCKS)] == [0, 0, 0, 0]
    finally:
        s.close()


@pytest.mark.parametrize("name", ["ref5", "grid", "symlower"])
def test_accuracy_for_every_trans(emu_lib, monkeypatch, name):
    _prune_always(monkeypatch)
    run_accuracy(emu_lib, name)


@pytest.mark.parametrize("name", ["grid", "symlower"])
def test_selection_is_bitwise_the_rows_of_the_full_result(emu_lib, monkeypatch, name):
    _prune_always(monkeypatch)
    run_selection(emu_lib, name)


def test_inverse_entries(emu_lib, monkeypatch):
    _prune_always(monkeypatch)
    run_inverse_entries(emu_lib, "grid")


def test_plain_real_equivalent_factor(emu_lib, monkeypatch):
    """HIPMF_COMPLEX_PAIRS=0: the pruned paths do not lean on the pairing of the rows"""
    _prune_always(monkeypatch)
    run_accuracy(emu_lib, "grid", env={"HIPMF_COMPLEX_PAIRS": "0"})


def test_perturbed_factor_falls_back(emu_lib, monkeypatch):
    _prune_always(monkeypatch)
    run_perturbed(emu_lib)


def test_unchanged_state(emu_lib, monkeypatch):
    _prune_always(monkeypatch)
    run_unchanged_state(emu_lib, "grid")


def test_status_codes(emu_lib):
    run_status_codes(emu_lib)
