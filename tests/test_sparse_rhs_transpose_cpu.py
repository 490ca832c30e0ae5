"""Sparse right-hand sides, selected rows and entries of the inverse through A^T (solver_hipmf_solve_sparse_transpose / _device,
solver_hipmf_inverse_entries_by_rows, kernels_solve_pruned_transpose.hpp) on the CPU emulator of the HIP kernels.  The helpers, the
matrices and the tolerance rule are those of tests/test_sparse_rhs_cpu.py; tests/test_sparse_rhs_transpose_gpu.py repeats the run_* cases
on the device (lib None = the product build).

The tolerance rule here: the yardstick e_ref is the unrefined solver_hipmf_solve_transpose_many on the expanded block against the same
dense solution np.linalg.solve(A.T, B.T).  The pruned transposed pass pair launches the product kernels of that very solve on the marked
fronts, the two new forward kernels add the marked children in the same order, and a child left out adds exact zeros there -- ratios
near 1 are expected (a lone column's yardstick is the single-column transposed solve, whose sums are ordered differently).
Measured ratios, max over the columns of (e_pruned - floor)+ / e_ref (profiles/r16_sparse_rhs_transpose.txt): see that file.

mumps5, poisson (perturbed values), the convection-diffusion matrices are unsymmetric in value: a solve with A in place of A^T fails
them (test_the_matrices_tell_a_from_its_transpose); bfwb62 is a general LU handle whose values happen to be symmetric."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

from russell_amd import problems as P
from russell_amd.backend import Hipmf, HipmfError
from test_sparse_rhs_cpu import (EPS, ERROR_NEED_INITIALIZATION, FACTOR, FLOOR_ULPS, _new, _prune_always, check_rule, handle, matrices, sparse_columns)
from test_transpose_solve_cpu import ERROR_HIPMF_INVALID_VALUE, ERROR_NEED_FACTORIZATION, ERROR_NULL_POINTER, mumps_5x5
from test_transpose_solve_gpu import _pm1

UNSYMMETRIC = ["mumps5", "bfwb62", "poisson"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def big_fronts():
    n, rp, ci, v = P.convection_diffusion2d(44, 40, peclet=30)
    return sp.csr_matrix((v, ci, rp), shape=(n, n)).toarray(), (n, rp, ci), dict(values=v), v


def matched():
    """the rows of a convection-diffusion matrix in a fixed random order: the maximum-product matching has to move them back, so the entry
    permutation (rows) and the exit permutation (columns) differ"""
    n, rp, ci, v = P.convection_diffusion2d(20, peclet=30)
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))[np.random.default_rng(77).permutation(n)].tocsr()
    A.sort_indices()
    rp, ci, v = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(float)
    return A.toarray(), (n, rp, ci), dict(values=v), v


def run_accuracy(lib, A, init, kw, values, counts=(1, 3, 0, 2, 9, 1, 40), seed=2):
    n = A.shape[0]
    s = handle(lib, init, kw, values)
    try:
        assert s.num_perturbed == 0
        ptr, idx, val, B = sparse_columns(n, counts, seed)
        Xd = np.linalg.solve(A.T, B.T).T
        X = s.solve_sparse(ptr, idx, val, transpose=True)
        nb = (len(counts) + 15) // 16
        assert s.counter("pruned_blocks") == nb and s.counter("pruned_transposed_blocks") == nb
        assert s.counter("pruned_bwd_fronts") == s.stats()["nsuper"]
        Xm = s.solve_transpose_many(B)
        return check_rule(X, Xm, Xd, "solve_sparse_transpose")  # (asserts for every column)
    finally:
        s.close()


def run_selection(lib, A, init, kw, values, seed=4):
    """rows picked by sel_idx (duplicates, any order, padded ldx) are bit for bit the rows of the sel_idx = NULL result"""
    n = A.shape[0]
    s = handle(lib, init, kw, values)
    try:
        ptr, idx, val, B = sparse_columns(n, (1, 4, 0, 2, 1), seed)
        X = s.solve_sparse(ptr, idx, val, transpose=True)
        Xd = np.linalg.solve(A.T, B.T).T
        check_rule(X, s.solve_transpose_many(B), Xd, "selection, all rows")
        rng = np.random.default_rng(seed)
        sel = rng.choice(n, size=min(6, n), replace=False).astype(np.int32)
        sel = np.concatenate([sel, sel[:2]])
        Xs = s.solve_sparse(ptr, idx, val, select=sel, transpose=True)
        assert s.counter("pruned_blocks") == 1 and s.counter("pruned_transposed_blocks") == 1
        assert np.array_equal(bits(Xs), bits(X[:, sel]))
        Xp = s.solve_sparse(ptr, idx, val, select=sel, ldx=sel.size + 3, transpose=True)
        assert np.array_equal(bits(Xp[:, :sel.size]), bits(Xs)) and not Xp[:, sel.size:].any()
    finally:
        s.close()


def run_no_stale_data(lib, A, init, kw, values):
    """a dense solve_transpose_many of 18 columns, an ordinary solve_sparse and a transposed one with other columns before the call change
    nothing; an empty column gives zeros"""
    n = A.shape[0]
    ptr, idx, val, _ = sparse_columns(n, (2, 0, 5, 1), 9)
    sel = np.arange(0, n, max(1, n // 7), dtype=np.int32)
    fresh = handle(lib, init, kw, values)
    try:
        X0, S0 = fresh.solve_sparse(ptr, idx, val, transpose=True), fresh.solve_sparse(ptr, idx, val, select=sel, transpose=True)
    finally:
        fresh.close()
    s = handle(lib, init, kw, values)
    try:
        s.solve_transpose_many(np.random.default_rng(1).standard_normal((18, n)))
        s.solve_sparse(*sparse_columns(n, (7, 7, 7), 10)[:3])
        s.solve_sparse(*sparse_columns(n, (6, 8, 5), 11)[:3], transpose=True)
        X1, S1 = s.solve_sparse(ptr, idx, val, transpose=True), s.solve_sparse(ptr, idx, val, select=sel, transpose=True)
        assert np.array_equal(bits(X1), bits(X0)) and np.array_equal(bits(S1), bits(S0))
        assert not X1[1].any() and not S1[1].any()
    finally:
        s.close()


def run_other_solves_untouched(lib, A, init, kw, values):
    n = A.shape[0]
    s = handle(lib, init, kw, values, nstep=-1)
    try:
        b = np.random.default_rng(3).standard_normal(n)
        cols = sparse_columns(n, (3, 1), 5)[:3]
        x0, t0, p0 = s.solve(b), s.solve_transpose(b), s.solve_sparse(*cols, select=[0, n - 1])
        fb, i15 = s.counter("fused_fallbacks"), s.stats()["fused_fallbacks"]
        s.solve_sparse(*sparse_columns(n, (2, 4, 1), 6)[:3], select=[1, n - 2], transpose=True)
        assert s.counter("pruned_transposed_blocks") == 1
        assert np.array_equal(bits(s.solve(b)), bits(x0)) and np.array_equal(bits(s.solve_transpose(b)), bits(t0))
        assert np.array_equal(bits(s.solve_sparse(*cols, select=[0, n - 1])), bits(p0))
        assert s.counter("pruned_transposed_blocks") == 0
        assert s.counter("fused_fallbacks") == fb and s.stats()["fused_fallbacks"] == i15
    finally:
        s.close()


def run_counters(lib, A, init, kw, values):
    n = A.shape[0]
    s = handle(lib, init, kw, values)
    try:
        st = s.stats()
        one = (np.array([0, 1], np.int32), np.array([n // 3], np.int32), np.array([1.0]))
        x = s.solve_sparse(*one, select=[n // 2], transpose=True)
        assert s.counter("pruned_transposed_blocks") == 1 and s.counter("pruned_blocks") == 1
        assert 1 <= s.counter("pruned_fwd_fronts") <= st["nlevels"] and 1 <= s.counter("pruned_bwd_fronts") <= st["nlevels"]
        assert st["nlevels"] < st["nsuper"] and s.counter("pruned_bytes") > 0
        Ainv = np.linalg.inv(A)
        assert abs(x[0, 0] - Ainv[n // 3, n // 2]) <= 1e-12 * np.abs(Ainv).max()  # (A^{-T})(n/2, n/3)
        for ncols, nblocks in ((16, 1), (17, 2), (33, 3)):
            ptr, idx, val, _ = sparse_columns(n, [1 + c % 3 for c in range(ncols)], 30 + ncols)
            s.solve_sparse(ptr, idx, val, select=[0, 1], transpose=True)
            assert s.counter("pruned_blocks") == nblocks and s.counter("pruned_transposed_blocks") == nblocks
    finally:
        s.close()


def run_symmetric(lib, A, init, kw, values):
    """A^T = A: the ordinary pruned path, bit for bit"""
    n = A.shape[0]
    s = handle(lib, init, kw, values)
    try:
        ptr, idx, val, _ = sparse_columns(n, (1, 3, 0, 2, 9), 7)
        sel = np.array([n - 1, 2, 2, n // 2], np.int32)
        for select in (None, sel):
            X = s.solve_sparse(ptr, idx, val, select=select)
            Xt = s.solve_sparse(ptr, idx, val, select=select, transpose=True)
            assert s.counter("pruned_blocks") == 1 and s.counter("pruned_transposed_blocks") == 0
            assert np.array_equal(bits(X), bits(Xt))
        r, c = np.array([3, n - 1, 3], np.int32), np.array([5, 0, 5], np.int32)
        assert np.array_equal(bits(s.inverse_entries(r, c, by_rows=True)), bits(s.inverse_entries(c, r)))
        assert s.counter("pruned_transposed_blocks") == 0
    finally:
        s.close()


def run_fallback(lib, A, init, kw, values):
    """HIPMF_PRUNE_MAX_SHARE = 0: solve_transpose_many of the expanded block, then the selection, bit for bit"""
    n = A.shape[0]
    s = handle(lib, init, kw, values)
    try:
        ptr, idx, val, B = sparse_columns(n, (1, 3, 0, 2), 6)
        X = s.solve_sparse(ptr, idx, val, transpose=True)
        assert s.counter("pruned_blocks") == 0 and s.counter("pruned_transposed_blocks") == 0
        Xm = s.solve_transpose_many(B)
        assert np.array_equal(bits(X), bits(Xm))
        sel = np.array([n - 1, 0, n // 2], np.int32)
        assert np.array_equal(bits(s.solve_sparse(ptr, idx, val, select=sel, transpose=True)), bits(Xm[:, sel]))
    finally:
        s.close()


def run_perturbed(lib):
    """the +-1 matrix of test_sparse_rhs_cpu.run_perturbed (replaced pivots): the refined, rescued transposed solve runs"""
    A = _pm1(800, 4, np.random.default_rng(100))
    n, rp, ci, v = A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
    s = _new(lib)
    try:
        assert s.initialize(n, rp, ci, values=v) == 0 and s.factorize(v) == 0
        assert s.num_perturbed > 0
        ptr, idx, val, B = sparse_columns(n, (3, 1, 2), 8)
        X = s.solve_sparse(ptr, idx, val, transpose=True)
        assert s.counter("pruned_blocks") == 0 and s.counter("pruned_transposed_blocks") == 0
        assert np.array_equal(bits(X), bits(s.solve_transpose_many(B)))
        R = A.T @ X.T - B.T
        res = np.abs(R).max() / (np.abs(A).sum(axis=0).max() * np.abs(X).max())
        print("perturbed factor: scaled residual of A^T %.3e" % res)
        # refinement and the rescue stop at a componentwise backward error of a few eps; in this norm that is below n eps = 2e-13.  An
        # unrefined solve on a factor with pivots replaced at the sqrt(eps) scale leaves about 1e-8: 1e-10 separates the two
        assert res <= 1e-10
        sel = np.array([5, 700, 33], np.int32)
        assert np.array_equal(bits(s.solve_sparse(ptr, idx, val, select=sel, transpose=True)), bits(X[:, sel]))
    finally:
        s.close()


def run_inverse_entries_by_rows(lib, A, init, kw, values):
    """40 distinct rows (three blocks), arbitrary order, duplicates: against numpy's inverse with the transposed solve of the unit vectors as
    yardstick, and against inverse_entries on the same list"""
    n = A.shape[0]
    s = handle(lib, init, kw, values)
    try:
        rng = np.random.default_rng(12)
        rows = rng.choice(n, size=min(40, n), replace=False)
        cols = rng.integers(0, n, rows.size)
        rows, cols = np.concatenate([rows, rows[:5], rows[:7]]), np.concatenate([cols, cols[:5], rng.integers(0, n, 7)])
        pi = rng.permutation(rows.size)
        rows, cols = rows[pi].astype(np.int32), cols[pi].astype(np.int32)
        ur = np.unique(rows)
        assert ur.size > 16
        vals = s.inverse_entries(rows, cols, by_rows=True)
        nblocks = (ur.size + 15) // 16
        assert s.counter("pruned_blocks") == nblocks and s.counter("pruned_transposed_blocks") == nblocks
        vcol = s.inverse_entries(rows, cols)
        assert s.counter("pruned_transposed_blocks") == 0
        Xm = s.solve_transpose_many(np.eye(n)[ur])
        Ainv = np.linalg.inv(A)
        exact = Ainv[rows, cols]
        for k, r in enumerate(ur):
            m = rows == r
            xd = Ainv[r, :]  # column r of A^{-T}
            floor = FLOOR_ULPS * EPS * np.abs(xd).max()
            e_ref, e_p = np.abs(Xm[k] - xd).max(), np.abs(vals[m] - xd[cols[m]]).max()
            print("inverse_entries_by_rows row %d: %.3e, yardstick %.3e" % (r, e_p, e_ref))
            assert e_p <= FACTOR * e_ref + floor, (r, e_p, e_ref)
        for e in range(rows.size):  # the two layers agree: floor + FACTOR x the larger of the two errors against the dense inverse
            floor = FLOOR_ULPS * EPS * max(np.abs(Ainv[rows[e], :]).max(), np.abs(Ainv[:, cols[e]]).max())
            worse = max(abs(vals[e] - exact[e]), abs(vcol[e] - exact[e]))
            assert abs(vals[e] - vcol[e]) <= FACTOR * worse + floor, (e, vals[e], vcol[e], exact[e])
            same = (rows == rows[e]) & (cols == cols[e])
            assert np.all(vals[same] == vals[e])
    finally:
        s.close()


def run_device_entry(lib, A, init, kw, values):
    n = A.shape[0]
    s = handle(lib, init, kw, values)
    ptrs = []
    try:
        ptr, idx, val, _ = sparse_columns(n, (2, 0, 4, 1, 3) * 4, 14)  # 20 columns: two blocks
        sel = np.array([1, n - 2, n // 2, 1], np.int32)
        for select in (None, sel):
            Xh = s.solve_sparse(ptr, idx, val, select=select, transpose=True)
            nsel = n if select is None else select.size
            ld = nsel + 2
            out = np.full((ptr.size - 1, ld), -7.0)
            bufs = [ptr, idx, val, out] + ([] if select is None else [select])
            d = [s.dev_alloc(max(b.nbytes, 8)) for b in bufs]
            ptrs += d
            for dp, b in zip(d, bufs):
                if b.nbytes:
                    s.h2d(dp, b)
            s.solve_sparse_device(d[3], ld, ptr.size - 1, d[0], d[1], d[2], nsel, None if select is None else d[4], transpose=True)
            assert s.counter("pruned_transposed_blocks") == 2
            s.d2h(out, d[3])
            assert np.array_equal(bits(out[:, :nsel]), bits(Xh))
            assert np.all(out[:, nsel:] == -7.0)
    finally:
        for dp in ptrs:
            s.dev_free(dp)
        s.close()


# ---- the tests on the emulator ----

def test_exports(emu_lib):
    raw = C.CDLL(emu_lib)
    for name in ("solver_hipmf_solve_sparse_transpose", "solver_hipmf_solve_sparse_transpose_device", "solver_hipmf_inverse_entries_by_rows"):
        assert hasattr(raw, name), name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "russell_hipmf.h")).read()
    assert "#define HIPMF_COUNTER_PRUNED_TRANSPOSED_BLOCKS 38" in header and Hipmf.COUNTERS["pruned_transposed_blocks"] == 38
    (n, rp, ci, v), _ = mumps_5x5()
    s = handle(emu_lib, (n, rp, ci), dict(values=v), v)
    try:
        assert s.counter("pruned_transposed_blocks") == 0
    finally:
        s.close()


@pytest.mark.parametrize("name", ["mumps5", "poisson"])
def test_the_matrices_tell_a_from_its_transpose(name):
    """(bfwb62 is handed over as a general matrix -- so the transposed launches run on it -- but its values are symmetric: it checks
    the arithmetic, not the direction; mumps5, poisson, the big-front and the matched matrices check the direction)"""
    A = matrices()[name][0]
    n = A.shape[0]
    _, _, _, B = sparse_columns(n, (1, 3, 2, 9, 1, 40), 2)
    X, Xt = np.linalg.solve(A, B.T), np.linalg.solve(A.T, B.T)
    assert np.all(np.abs(X - Xt).max(axis=0) > 1e-3 * np.abs(Xt).max(axis=0))


@pytest.mark.parametrize("name", UNSYMMETRIC)
def test_accuracy_against_dense_solve(emu_lib, monkeypatch, name):
    _prune_always(monkeypatch)
    print("largest ratio on %s: %.2f" % (name, run_accuracy(emu_lib, *matrices()[name])))


@pytest.mark.parametrize("mid", ["1", "0"])
def test_big_fronts(emu_lib, monkeypatch, mid):
    """big fronts in both forms of E / E' (their skipped blocks), more than 32 pivots, 16-column tiles over f > 64"""
    _prune_always(monkeypatch)
    monkeypatch.setenv("HIPMF_MID_FRONT", mid)
    A, init, kw, v = big_fronts()
    s = handle(emu_lib, init, kw, v)
    st = s.stats()
    assert st["max_front"] > 64 and st["max_pivots"] > 32 and (s.counter("mid_fronts") > 0) == (mid == "1")
    s.close()
    print("largest ratio with HIPMF_MID_FRONT=%s: %.2f" % (mid, run_accuracy(emu_lib, A, init, kw, v)))
    run_selection(emu_lib, A, init, kw, v)


def test_matching_in_force(emu_lib, monkeypatch):
    _prune_always(monkeypatch)
    A, init, kw, v = matched()
    s = handle(emu_lib, init, kw, v)
    assert s.stats()["matched"] == 1
    s.close()
    print("largest ratio on the matched matrix: %.2f" % run_accuracy(emu_lib, A, init, kw, v))
    run_selection(emu_lib, A, init, kw, v)


@pytest.mark.parametrize("name", UNSYMMETRIC)
def test_selection_is_bitwise_the_rows_of_the_full_result(emu_lib, monkeypatch, name):
    _prune_always(monkeypatch)
    run_selection(emu_lib, *matrices()[name])


@pytest.mark.parametrize("name", ["poisson", "big"])
def test_no_stale_data(emu_lib, monkeypatch, name):
    _prune_always(monkeypatch)
    run_no_stale_data(emu_lib, *(big_fronts() if name == "big" else matrices()[name]))


def test_other_solves_untouched(emu_lib, monkeypatch):
    _prune_always(monkeypatch)
    run_other_solves_untouched(emu_lib, *matrices()["poisson"])


def test_counters_and_block_edges(emu_lib, monkeypatch):
    _prune_always(monkeypatch)
    run_counters(emu_lib, *matrices()["poisson"])


@pytest.mark.parametrize("name", ["poisson_lower", "saddle"])
def test_symmetric_handles_run_the_ordinary_path(emu_lib, monkeypatch, name):
    _prune_always(monkeypatch)
    run_symmetric(emu_lib, *matrices()[name])


@pytest.mark.parametrize("name", ["bfwb62", "poisson"])
def test_fallback_by_share(emu_lib, monkeypatch, name):
    monkeypatch.setenv("HIPMF_PRUNE_MAX_SHARE", "0")
    run_fallback(emu_lib, *matrices()[name])


def test_perturbed_factor_takes_the_transposed_solve(emu_lib, monkeypatch):
    _prune_always(monkeypatch)
    run_perturbed(emu_lib)


@pytest.mark.parametrize("name", ["bfwb62", "poisson", "matched"])
def test_inverse_entries_by_rows(emu_lib, monkeypatch, name):
    _prune_always(monkeypatch)
    run_inverse_entries_by_rows(emu_lib, *(matched() if name == "matched" else matrices()[name]))


def test_device_entry_point(emu_lib, monkeypatch):
    _prune_always(monkeypatch)
    run_device_entry(emu_lib, *matrices()["poisson"])


def test_status_codes(emu_lib):
    """the list of solver_hipmf_solve_sparse (tests/test_sparse_rhs_cpu.py::test_status_codes), in its order, for the new entry points"""
    (n, rp, ci, v), _ = mumps_5x5()
    s = _new(emu_lib)
    try:
        ptr, idx, val = np.array([0, 1, 2], np.int32), np.array([0, 3], np.int32), np.array([1.0, 2.0])
        x = np.zeros((2, n))
        call = s.lib.solver_hipmf_solve_sparse_transpose
        dev = s.lib.solver_hipmf_solve_sparse_transpose_device
        inv = s.lib.solver_hipmf_inverse_entries_by_rows
        r1, out1 = np.array([0], np.int32), np.zeros(1)
        p8 = C.c_void_p(8)
        assert call(s.h, x, n, 2, ptr, idx, val, 0, None, 0) == ERROR_NEED_INITIALIZATION
        assert dev(s.h, p8, n, 2, p8, p8, p8, 0, None, 0) == ERROR_NEED_INITIALIZATION
        assert inv(s.h, 1, r1, r1, out1, 0) == ERROR_NEED_INITIALIZATION
        assert s.initialize(n, rp, ci) == 0
        assert call(s.h, x, n, 2, ptr, idx, val, 0, None, 0) == ERROR_NEED_FACTORIZATION
        assert inv(s.h, 1, r1, r1, out1, 0) == ERROR_NEED_FACTORIZATION
        assert dev(s.h, p8, n, 2, p8, p8, p8, 0, None, 0) == ERROR_NEED_FACTORIZATION
        assert s.factorize(v) == 0
        assert call(s.h, x, n, 2, ptr, idx, val, 0, None, 0) == 0
        sel = np.array([1, 1, 4], np.int32)
        bad = ERROR_HIPMF_INVALID_VALUE
        assert call(s.h, x, n, 0, ptr, idx, val, 0, None, 0) == bad  # nrhs < 1
        assert dev(s.h, p8, n, 0, p8, p8, p8, 0, None, 0) == bad
        assert call(s.h, x, n - 1, 2, ptr, idx, val, 0, None, 0) == bad  # ldx < n with all rows
        assert dev(s.h, p8, n - 1, 2, p8, p8, p8, 0, None, 0) == bad
        assert call(s.h, x, 2, 2, ptr, idx, val, 3, sel.ctypes.data, 0) == bad  # ldx < nsel
        assert call(s.h, x, 3, 2, ptr, idx, val, 0, sel.ctypes.data, 0) == bad  # nsel < 1 with a selection
        assert dev(s.h, p8, 3, 2, p8, p8, p8, 0, p8, 0) == bad
        assert call(s.h, x, 3, 2, ptr, idx, val, 3, sel.ctypes.data, 0) == 0  # (duplicates in the selection are fine)
        assert call(s.h, x, n, 2, ptr, np.array([0, n], np.int32), val, 0, None, 0) == bad  # row out of range
        assert call(s.h, x, n, 2, ptr, np.array([-1, 2], np.int32), val, 0, None, 0) == bad
        p1 = np.array([0, 2], np.int32)
        assert call(s.h, x, n, 1, p1, np.array([3, 1], np.int32), val, 0, None, 0) == bad  # unsorted rows in a column
        assert call(s.h, x, n, 1, p1, np.array([2, 2], np.int32), val, 0, None, 0) == bad  # duplicate rows in a column
        assert call(s.h, x, n, 2, np.array([0, 2, 1], np.int32), idx, val, 0, None, 0) == bad  # decreasing column pointers
        assert call(s.h, x, 3, 2, ptr, idx, val, 3, np.array([0, 5, 1], np.int32).ctypes.data, 0) == bad  # selected row out of range
        assert inv(s.h, 0, r1, r1, out1, 0) == bad
        assert inv(s.h, 1, np.array([n], np.int32), r1, out1, 0) == bad
        assert inv(s.h, 1, r1, np.array([-1], np.int32), out1, 0) == bad
        with pytest.raises(HipmfError) as e:
            s.solve_sparse(ptr, idx, val, select=[7], transpose=True)
        assert e.value.code == bad
        raw = C.CDLL(s.lib._name)  # (untyped bindings: NULL pointers pass)
        raw.solver_hipmf_solve_sparse_transpose.restype = raw.solver_hipmf_inverse_entries_by_rows.restype = raw.solver_hipmf_solve_sparse_transpose_device.restype = C.c_int32
        h, xp, pp, ip, vp = C.c_void_p(s.h), x.ctypes.data_as(C.c_void_p), ptr.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p)
        for fn in (raw.solver_hipmf_solve_sparse_transpose, raw.solver_hipmf_solve_sparse_transpose_device):
            assert fn(h, None, n, 2, pp, ip, vp, 0, None, 0) == ERROR_NULL_POINTER
            assert fn(h, xp, n, 2, None, ip, vp, 0, None, 0) == ERROR_NULL_POINTER
            assert fn(None, xp, n, 2, pp, ip, vp, 0, None, 0) == ERROR_NULL_POINTER
        assert raw.solver_hipmf_solve_sparse_transpose(h, xp, n, 2, pp, None, vp, 0, None, 0) == ERROR_NULL_POINTER
        assert raw.solver_hipmf_inverse_entries_by_rows(h, 1, None, ip, vp, 0) == ERROR_NULL_POINTER
    finally:
        s.close()


def test_host_mirror(emu_lib, monkeypatch):
    """LinSolver.solve_sparse(transpose=True) / inverse_entries(by_rows=True) of russell_amd.sparse"""
    _prune_always(monkeypatch)
    from russell_amd import sparse as S

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    S._L().rh_set_hipmf_library(emu_lib.encode())
    try:
        n, rp, ci, v = P.convection_diffusion2d(20, 18, peclet=0.7, scale_decades=0.0)
        A = sp.csr_matrix((v, ci, rp), shape=(n, n))
        coo = A.tocoo()
        mat = S.CooMatrix.from_arrays(n, n, coo.row, coo.col, coo.data)
        solver = S.LinSolver(S.Genie.Hipmf)
        with pytest.raises(S.StrError, match="factorize must be called"):
            solver.solve_sparse([([0], [1.0])], transpose=True)
        solver.actual.factorize(mat)
        Ad = A.toarray()
        cols = [([3], [2.0]), ([], []), ([1, 7, 100], [1.0, -1.0, 0.5])]
        B = np.zeros((3, n))
        for c, (i, vals) in enumerate(cols):
            B[c, i] = vals
        Xd, Xn = np.linalg.solve(Ad.T, B.T).T, np.linalg.solve(Ad, B.T).T
        assert np.abs(Xd - Xn).max() > 1e-3 * np.abs(Xd).max()
        X = solver.solve_sparse(cols, transpose=True)
        assert X.shape == (3, n) and np.abs(X - Xd).max() <= 1e-13 * np.abs(Xd).max() and not X[1].any()
        sel = [5, 0, 5, n - 1]
        Xs = solver.solve_sparse(cols, select=sel, transpose=True)
        assert np.array_equal(bits(Xs), bits(X[:, sel]))
        rows, ccols = np.array([4, 9, 4, 200]), np.array([9, 4, 9, 17])
        Ainv = np.linalg.inv(Ad)
        assert np.abs(solver.inverse_entries(rows, ccols, by_rows=True) - Ainv[rows, ccols]).max() <= 1e-13 * np.abs(Ainv).max()
        with pytest.raises(S.StrError, match="outside range"):
            solver.solve_sparse([([n], [1.0])], transpose=True)
        with pytest.raises(S.StrError, match="outside range"):
            solver.inverse_entries([1], [n], by_rows=True)
    finally:
        S._L().rh_set_hipmf_library(os.path.join(root, "russell_amd", "lib", "librussell_hipmf.so").encode())
