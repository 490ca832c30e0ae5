"""Sparse right-hand sides, selected solution rows and entries of the inverse (solver_hipmf_solve_sparse / _device,
solver_hipmf_inverse_entries, kernels_solve_pruned.hpp) on the CPU emulator of the HIP kernels: accuracy against the dense solve with
the existing unrefined solve_many as the yardstick, the selection bit for bit, the counters of the pruning, independence from what an
earlier solve left behind, the fallbacks (share knob, replaced pivots), the blocks of inverse_entries, the status codes and the host
mirror.  tests/test_sparse_rhs_gpu.py repeats the run_* cases on the device (lib None = the product build).

The tolerance rule.  In exact arithmetic the pruned pass pair and the ordinary one give the same x: the fronts left out contribute
exact zeros.  In floating point only the order of the sums inside a front differs (the pruned kernels deal the contraction of a big
front to four wavefronts in 32-wide chunks, the dependency-driven ones sum it in slabs).  So with e_ref = max |solve_many - x_dense| on
a handle with refinement_nstep = 0 (the parent commit's code path, measured against the same dense solution):
    max |solve_sparse - x_dense| <= FACTOR * e_ref + FLOOR_ULPS * eps * max |x_dense|
The floor covers columns where the yardstick happens to hit the dense solution to the last bit (e_ref = 0)."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

from russell_amd import problems as P
from russell_amd.backend import Hipmf, HipmfError
from test_sym_indefinite_cpu import saddle_point
from test_transpose_solve_cpu import ERROR_HIPMF_INVALID_VALUE, ERROR_NEED_FACTORIZATION, ERROR_NULL_POINTER, mumps_5x5
from test_transpose_solve_gpu import _golden, _pm1

EPS = np.finfo(float).eps
ERROR_NEED_INITIALIZATION = 500000
# Measured ratios, max over the columns of (e_pruned - floor)+ / e_ref (profiles/r09_sparse_rhs.txt).  CPU emulator: 5x5 0.00, bfwb62 0.00,
# poisson 0.99, poisson-lower 0.82, saddle 0.67, big LU fronts 1.00, big L D L^T fronts 0.91, 17 columns 1.02, 33 columns 1.11.  MI355X
# (tests/test_sparse_rhs_gpu.py): the five matrices at most 1.00, the 300 x 200 grid 0.96 (LU) and 0.99 (L D L^T), 1M DOF 0.17.
# The largest is 1.11: the smallest power of two that covers it is 2; one doubling of headroom: 4.
FACTOR = 4.0
FLOOR_ULPS = 4.0  # "a few ulps" of max |x|: fixed beforehand, not measured


def _new(lib):
    return Hipmf(lib) if lib else Hipmf()


def _prune_always(monkeypatch):
    """the share knob at 1: a block is never sent to the ordinary solve because of its size (sel_idx = NULL alone reads more than the default share)"""
    monkeypatch.setenv("HIPMF_PRUNE_MAX_SHARE", "1")


def matrices():
    """name -> (dense A, initialize arguments, factorize values)"""
    out = {}
    (n, rp, ci, v), _ = mumps_5x5()
    out["mumps5"] = (sp.csr_matrix((v, ci, rp), shape=(n, n)).toarray(), (n, rp, ci), dict(values=v), v)
    A = _golden("bfwb62").tocsr()
    A.sort_indices()
    out["bfwb62"] = (A.toarray(), (A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32)), dict(values=A.data.astype(float)), A.data.astype(float))
    n, rp, ci, v = P.poisson2d(56, 54)
    v = v * (1.0 + 0.1 * np.random.default_rng(56).uniform(-1, 1, v.size))  # (general: not symmetric in value)
    out["poisson"] = (sp.csr_matrix((v, ci, rp), shape=(n, n)).toarray(), (n, rp, ci), dict(values=v), v)
    n, rp, ci, v = P.poisson2d(56, 54)
    lrp, lci, lv = P.lower_triangle(n, rp, ci, v)
    out["poisson_lower"] = (sp.csr_matrix((v, ci, rp), shape=(n, n)).toarray(), (n, lrp, lci), dict(general_symmetric=True), lv)
    A, L = saddle_point(24, 60)
    out["saddle"] = (A.toarray(), (A.shape[0], L.indptr.astype(np.int32), L.indices.astype(np.int32)),
                     dict(general_symmetric=True, values=L.data.astype(float)), L.data.astype(float))
    return out


def handle(lib, init, kw, values, nstep=0):
    s = _new(lib)
    assert s.initialize(*init, refinement_nstep=nstep, **kw) == 0
    assert s.factorize(values) == 0
    return s


def sparse_columns(n, counts, seed):
    """compressed columns with the given numbers of non-zeros (ascending rows), and the same as dense rows"""
    rng = np.random.default_rng(seed)
    ptr, idx, val = [0], [], []
    for k in counts:
        r = np.sort(rng.choice(n, size=min(k, n), replace=False))
        idx += list(r)
        val += list(rng.uniform(0.5, 2.0, r.size) * rng.choice([-1.0, 1.0], r.size))
        ptr.append(len(idx))
    ptr, idx, val = np.array(ptr, np.int32), np.array(idx, np.int32), np.array(val, float)
    B = np.zeros((len(counts), n))
    for c in range(len(counts)):
        B[c, idx[ptr[c]:ptr[c + 1]]] = val[ptr[c]:ptr[c + 1]]
    return ptr, idx, val, B


def check_rule(X, Xref_lib, Xd, what):
    """the tolerance rule, column by column; returns the largest measured ratio"""
    worst = 0.0
    for c in range(Xd.shape[0]):
        scale = np.abs(Xd[c]).max()
        e_p, e_ref = np.abs(X[c] - Xd[c]).max(), np.abs(Xref_lib[c] - Xd[c]).max()
        floor = FLOOR_ULPS * EPS * scale
        ratio = max(e_p - floor, 0.0) / e_ref if e_ref > 0 else (0.0 if e_p <= floor else np.inf)
        worst = max(worst, ratio)
        print("%s column %d: pruned %.3e, yardstick %.3e, scale %.3e, ratio %.4f" % (what, c, e_p, e_ref, scale, ratio))
        assert e_p <= FACTOR * e_ref + floor, (what, c, e_p, e_ref, scale)
    return worst


def run_accuracy(lib, A, init, kw, values, counts=(1, 3, 0, 2, 9, 1, 40), seed=2):
    n = A.shape[0]
    s = handle(lib, init, kw, values)
    try:
        assert s.num_perturbed == 0
        ptr, idx, val, B = sparse_columns(n, counts, seed)
        Xd = np.linalg.solve(A, B.T).T
        X = s.solve_sparse(ptr, idx, val)
        assert s.counter("pruned_blocks") == (len(counts) + 15) // 16
        assert s.counter("pruned_bwd_fronts") == s.stats()["nsuper"]
        Xm = s.solve_many(B)
        return check_rule(X, Xm, Xd, "solve_sparse")
    finally:
        s.close()


def run_selection(lib, A, init, kw, values, seed=4):
    """rows picked by sel_idx (duplicates, any order) are bit for bit the rows of the sel_idx = NULL result"""
    n = A.shape[0]
    s = handle(lib, init, kw, values)
    try:
        ptr, idx, val, _ = sparse_columns(n, (1, 4, 0, 2, 1), seed)
        X = s.solve_sparse(ptr, idx, val)
        rng = np.random.default_rng(seed)
        sel = rng.choice(n, size=min(6, n), replace=False).astype(np.int32)
        sel = np.concatenate([sel, sel[:2]])
        Xs = s.solve_sparse(ptr, idx, val, select=sel)
        assert s.counter("pruned_blocks") == 1
        assert np.array_equal(Xs.view(np.uint64), X[:, sel].view(np.uint64))
        Xp = s.solve_sparse(ptr, idx, val, select=sel, ldx=sel.size + 3)  # padded leading dimension: the padding is not written
        assert np.array_equal(Xp[:, :sel.size].view(np.uint64), Xs.view(np.uint64)) and not Xp[:, sel.size:].any()
    finally:
        s.close()


def run_counters(lib, A, init, kw, values):
    n = A.shape[0]
    s = handle(lib, init, kw, values)
    try:
        st = s.stats()
        one = (np.array([0, 1], np.int32), np.array([n // 3], np.int32), np.array([1.0]))
        x = s.solve_sparse(*one, select=[n // 2])
        assert s.counter("pruned_blocks") == 1
        assert 1 <= s.counter("pruned_fwd_fronts") <= st["nlevels"]  # a path has at most one front per level
        assert 1 <= s.counter("pruned_bwd_fronts") <= st["nlevels"]
        assert st["nlevels"] < st["nsuper"]
        assert abs(x[0, 0] - np.linalg.solve(A, np.eye(n)[n // 3])[n // 2]) <= 1e-12 * np.abs(np.linalg.inv(A)).max()
        s.solve_sparse(*one)
        assert s.counter("pruned_fwd_fronts") <= st["nlevels"] and s.counter("pruned_bwd_fronts") == st["nsuper"]
    finally:
        s.close()


def run_no_stale_data(lib, A, init, kw, values):
    """a dense solve_many before the sparse solve changes nothing; neither does an earlier sparse solve with other columns; an empty column is zero"""
    n = A.shape[0]
    ptr, idx, val, _ = sparse_columns(n, (2, 0, 5, 1), 9)
    sel = np.arange(0, n, max(1, n // 7), dtype=np.int32)
    fresh = handle(lib, init, kw, values)
    try:
        X0, S0 = fresh.solve_sparse(ptr, idx, val), fresh.solve_sparse(ptr, idx, val, select=sel)
    finally:
        fresh.close()
    s = handle(lib, init, kw, values)
    try:
        s.solve_many(np.random.default_rng(1).standard_normal((18, n)))
        other = sparse_columns(n, (7, 7, 7), 10)
        s.solve_sparse(*other[:3])
        X1, S1 = s.solve_sparse(ptr, idx, val), s.solve_sparse(ptr, idx, val, select=sel)
        assert np.array_equal(X1.view(np.uint64), X0.view(np.uint64)) and np.array_equal(S1.view(np.uint64), S0.view(np.uint64))
        assert not X1[1].any() and not S1[1].any()
    finally:
        s.close()


def run_ordinary_solve_untouched(lib, A, init, kw, values):
    """the pruned path leaves the workspace of the ordinary solves alone: solve() before and after a sparse solve gives the same bits"""
    n = A.shape[0]
    s = handle(lib, init, kw, values, nstep=-1)
    try:
        b = np.random.default_rng(3).standard_normal(n)
        x0 = s.solve(b)
        fb = s.stats()["fused_fallbacks"]
        s.solve_sparse(*sparse_columns(n, (3, 1), 5)[:3], select=[0, n - 1])
        assert s.counter("pruned_blocks") == 1
        assert np.array_equal(s.solve(b).view(np.uint64), x0.view(np.uint64))
        assert s.stats()["fused_fallbacks"] == fb
    finally:
        s.close()


def run_fallback(lib, A, init, kw, values):
    n = A.shape[0]
    s = handle(lib, init, kw, values)
    try:
        ptr, idx, val, B = sparse_columns(n, (1, 3, 0, 2), 6)
        Xd = np.linalg.solve(A, B.T).T
        X = s.solve_sparse(ptr, idx, val)
        assert s.counter("pruned_blocks") == 0
        Xm = s.solve_many(B)
        check_rule(X, Xm, Xd, "fallback")
        sel = np.array([n - 1, 0, n // 2], np.int32)
        assert np.array_equal(s.solve_sparse(ptr, idx, val, select=sel).view(np.uint64), X[:, sel].view(np.uint64))
    finally:
        s.close()


def run_perturbed(lib):
    """a member of the +-1 family of tests/test_matrix_zoo_gpu.py that replaces pivots: the ordinary refined, rescued solve runs"""
    rng = np.random.default_rng(100)
    A = _pm1(800, 4, rng)
    n, rp, ci, v = A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
    s = _new(lib)
    try:
        assert s.initialize(n, rp, ci, values=v) == 0 and s.factorize(v) == 0
        assert s.num_perturbed > 0
        ptr, idx, val, B = sparse_columns(n, (3,), 8)
        sel = np.array([5, 700, 33], np.int32)
        xs = s.solve_sparse(ptr, idx, val, select=sel)
        assert s.counter("pruned_blocks") == 0
        assert np.array_equal(xs[0].view(np.uint64), s.solve(B[0])[sel].view(np.uint64))
        ptr, idx, val, B = sparse_columns(n, (3, 1, 2), 8)
        X = s.solve_sparse(ptr, idx, val)
        assert s.counter("pruned_blocks") == 0
        assert np.array_equal(X.view(np.uint64), s.solve_many(B).view(np.uint64))
    finally:
        s.close()


def run_inverse_entries(lib, A, init, kw, values):
    """40 distinct columns (three blocks), arbitrary order, duplicates: against numpy's inverse by the tolerance rule, the yardstick being
    solve_many on the unit vectors"""
    n = A.shape[0]
    s = handle(lib, init, kw, values)
    try:
        rng = np.random.default_rng(12)
        cols = rng.choice(n, size=min(40, n), replace=False)
        rows = rng.integers(0, n, cols.size)
        rows, cols = np.concatenate([rows, rows[:5], rng.integers(0, n, 7)]), np.concatenate([cols, cols[:5], cols[:7]])
        pi = rng.permutation(rows.size)
        rows, cols = rows[pi].astype(np.int32), cols[pi].astype(np.int32)
        vals = s.inverse_entries(rows, cols)
        nblocks = (np.unique(cols).size + 15) // 16
        assert s.counter("pruned_blocks") == nblocks
        uc = np.unique(cols)
        Xm = s.solve_many(np.eye(n)[uc])
        Ainv = np.linalg.inv(A)
        for c in uc:
            m = cols == c
            xd, xm = Ainv[:, c], Xm[list(uc).index(c)]
            floor = FLOOR_ULPS * EPS * np.abs(xd).max()
            e_ref = np.abs(xm - xd).max()
            e_p = np.abs(vals[m] - xd[rows[m]]).max()
            print("inverse_entries column %d: %.3e, yardstick %.3e" % (c, e_p, e_ref))
            assert e_p <= FACTOR * e_ref + floor, (c, e_p, e_ref)
        # duplicates agree exactly
        for e in range(rows.size):
            same = (rows == rows[e]) & (cols == cols[e])
            assert np.all(vals[same] == vals[e])
    finally:
        s.close()


def run_device_entry(lib, A, init, kw, values):
    """the _device entry point with device-resident arrays gives the bits of the host entry point"""
    n = A.shape[0]
    s = handle(lib, init, kw, values)
    ptrs = []
    try:
        ptr, idx, val, _ = sparse_columns(n, (2, 0, 4, 1, 3) * 4, 14)  # 20 columns: two blocks
        sel = np.array([1, n - 2, n // 2, 1], np.int32)
        for select in (None, sel):
            Xh = s.solve_sparse(ptr, idx, val, select=select)
            nsel = n if select is None else select.size
            ld = nsel + 2
            out = np.full((ptr.size - 1, ld), -7.0)
            bufs = [ptr, idx, val, out] + ([] if select is None else [select])
            d = [s.dev_alloc(max(b.nbytes, 8)) for b in bufs]
            ptrs += d
            for dp, b in zip(d, bufs):
                if b.nbytes:
                    s.h2d(dp, b)
            s.solve_sparse_device(d[3], ld, ptr.size - 1, d[0], d[1], d[2], nsel, None if select is None else d[4])
            s.d2h(out, d[3])
            assert np.array_equal(out[:, :nsel].view(np.uint64), Xh.view(np.uint64))
            assert np.all(out[:, nsel:] == -7.0)
    finally:
        for dp in ptrs:
            s.dev_free(dp)
        s.close()


# ---- the tests on the emulator ----

def test_exports(emu_lib):
    """the three entry points and the three counters exist (they do not on the parent commit)"""
    raw = C.CDLL(emu_lib)
    for name in ("solver_hipmf_solve_sparse", "solver_hipmf_solve_sparse_device", "solver_hipmf_inverse_entries"):
        assert hasattr(raw, name), name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "russell_hipmf.h")).read()
    for name, num in (("PRUNED_FWD_FRONTS", 24), ("PRUNED_BWD_FRONTS", 25), ("PRUNED_BLOCKS", 26)):
        assert "#define HIPMF_COUNTER_%s %d" % (name, num) in header
        assert Hipmf.COUNTERS[name.lower()] == num
    (n, rp, ci, v), _ = mumps_5x5()
    s = handle(emu_lib, (n, rp, ci), dict(values=v), v)
    try:
        assert [s.counter(k) for k in ("pruned_fwd_fronts", "pruned_bwd_fronts", "pruned_blocks")] == [0, 0, 0]
    finally:
        s.close()


@pytest.mark.parametrize("name", ["mumps5", "bfwb62", "poisson", "poisson_lower", "saddle"])
def test_accuracy_against_dense_solve(emu_lib, monkeypatch, name):
    _prune_always(monkeypatch)
    A, init, kw, values = matrices()[name]
    s = handle(emu_lib, init, kw, values)
    if name == "poisson_lower":
        assert s.counter("symmetric_ldlt") == 1
    if name == "saddle":
        assert s.stats()["matched"] == 1 and s.counter("sym_expanded") == 1
    s.close()
    print("largest ratio on %s: %.2f" % (name, run_accuracy(emu_lib, A, init, kw, values)))


@pytest.mark.parametrize("mid", ["1", "0"])
def test_accuracy_on_big_fronts(emu_lib, monkeypatch, mid):
    """big fronts in both forms of E / E' (FD_DENSE_TOP and the tiled form with its skipped blocks), more than 32 pivots"""
    _prune_always(monkeypatch)
    monkeypatch.setenv("HIPMF_MID_FRONT", mid)
    n, rp, ci, v = P.convection_diffusion2d(44, 40, peclet=30)
    A = sp.csr_matrix((v, ci, rp), shape=(n, n)).toarray()
    s = handle(emu_lib, (n, rp, ci), dict(values=v), v)
    st = s.stats()
    assert st["max_front"] > 64 and st["max_pivots"] > 32 and (s.counter("mid_fronts") > 0) == (mid == "1")
    s.close()
    run_accuracy(emu_lib, A, (n, rp, ci), dict(values=v), v)
    run_selection(emu_lib, A, (n, rp, ci), dict(values=v), v)


def test_big_symmetric_fronts(emu_lib, monkeypatch):
    """L D L^T fronts with more than 32 pivots: the backward pass through D^{-1} and the transposed product"""
    _prune_always(monkeypatch)
    n, rp, ci, v = P.poisson2d(72, 70)
    lrp, lci, lv = P.lower_triangle(n, rp, ci, v)
    A = sp.csr_matrix((v, ci, rp), shape=(n, n)).toarray()
    s = handle(emu_lib, (n, lrp, lci), dict(general_symmetric=True), lv)
    st = s.stats()
    assert s.counter("symmetric_ldlt") == 1 and st["max_front"] > 64 and st["max_pivots"] > 32
    s.close()
    run_accuracy(emu_lib, A, (n, lrp, lci), dict(general_symmetric=True), lv)
    run_selection(emu_lib, A, (n, lrp, lci), dict(general_symmetric=True), lv)


@pytest.mark.parametrize("name", ["mumps5", "poisson", "poisson_lower", "saddle"])
def test_selection_is_bitwise_the_rows_of_the_full_result(emu_lib, monkeypatch, name):
    _prune_always(monkeypatch)
    run_selection(emu_lib, *matrices()[name])


@pytest.mark.parametrize("name", ["poisson", "poisson_lower"])
def test_pruning_happens(emu_lib, monkeypatch, name):
    _prune_always(monkeypatch)
    run_counters(emu_lib, *matrices()[name])


def test_default_rules_prune_a_selection_and_not_all_rows_or_a_lone_column(emu_lib, monkeypatch):
    """the default knobs: two columns with two rows run pruned; all rows read more than a quarter of a pass pair;
    one column alone on a factor this small goes to the single-column solve unless HIPMF_PRUNE_MIN_BYTES says otherwise"""
    monkeypatch.delenv("HIPMF_PRUNE_MAX_SHARE", raising=False)
    monkeypatch.delenv("HIPMF_PRUNE_MIN_BYTES", raising=False)
    A, init, kw, values = matrices()["poisson"]
    n = A.shape[0]
    s = handle(emu_lib, init, kw, values)
    try:
        ptr, idx, val, B = sparse_columns(n, (1, 2), 3)
        sel = np.array([3, 4], np.int32)
        xs = s.solve_sparse(ptr, idx, val, select=sel)
        assert s.counter("pruned_blocks") == 1 and 0 < s.counter("pruned_bytes") < 0.25 * 2 * 8 * (s.stats()["nnz_l"] + s.stats()["nnz_u"] + n)
        s.solve_sparse(ptr, idx, val)
        assert s.counter("pruned_blocks") == 0
        one = (ptr[:2], idx[:1], val[:1])
        x1 = s.solve_sparse(*one, select=sel)
        assert s.counter("pruned_blocks") == 0
        assert np.array_equal(x1[0].view(np.uint64), s.solve(B[0])[sel].view(np.uint64))
        monkeypatch.setenv("HIPMF_PRUNE_MIN_BYTES", "0")
        x1p = s.solve_sparse(*one, select=sel)
        assert s.counter("pruned_blocks") == 1
        assert np.array_equal(x1p[0].view(np.uint64), xs[0].view(np.uint64))
    finally:
        s.close()


@pytest.mark.parametrize("name", ["poisson", "poisson_lower", "saddle"])
def test_no_stale_data(emu_lib, monkeypatch, name):
    _prune_always(monkeypatch)
    run_no_stale_data(emu_lib, *matrices()[name])


def test_ordinary_solve_untouched(emu_lib, monkeypatch):
    _prune_always(monkeypatch)
    run_ordinary_solve_untouched(emu_lib, *matrices()["poisson"])


@pytest.mark.parametrize("name", ["bfwb62", "poisson", "poisson_lower"])
def test_fallback_by_share(emu_lib, monkeypatch, name):
    monkeypatch.setenv("HIPMF_PRUNE_MAX_SHARE", "0")
    run_fallback(emu_lib, *matrices()[name])


def test_perturbed_factor_takes_the_ordinary_solve(emu_lib, monkeypatch):
    _prune_always(monkeypatch)
    run_perturbed(emu_lib)


@pytest.mark.parametrize("name", ["bfwb62", "poisson", "saddle"])
def test_inverse_entries(emu_lib, monkeypatch, name):
    _prune_always(monkeypatch)
    run_inverse_entries(emu_lib, *matrices()[name])


def test_device_entry_point(emu_lib, monkeypatch):
    _prune_always(monkeypatch)
    run_device_entry(emu_lib, *matrices()["poisson"])


@pytest.mark.parametrize("ncols", [17, 33])
def test_block_edges(emu_lib, monkeypatch, ncols):
    """17 and 33 columns cross block boundaries: every column is what it is when solved alone, bit for bit"""
    _prune_always(monkeypatch)
    A, init, kw, values = matrices()["poisson"]
    n = A.shape[0]
    s = handle(emu_lib, init, kw, values)
    try:
        counts = [(c % 4) + (c % 3 == 0) for c in range(ncols)]
        ptr, idx, val, B = sparse_columns(n, counts, 20 + ncols)
        X = s.solve_sparse(ptr, idx, val)
        assert s.counter("pruned_blocks") == (ncols + 15) // 16
        Xd = np.linalg.solve(A, B.T).T
        check_rule(X, s.solve_many(B), Xd, "%d columns" % ncols)
        for c in (0, 15, 16, ncols - 1):
            one = s.solve_sparse(np.array([0, ptr[c + 1] - ptr[c]], np.int32), idx[ptr[c]:ptr[c + 1]], val[ptr[c]:ptr[c + 1]])
            assert np.array_equal(one[0].view(np.uint64), X[c].view(np.uint64)), c
    finally:
        s.close()


def test_status_codes(emu_lib):
    (n, rp, ci, v), _ = mumps_5x5()
    s = _new(emu_lib)
    try:
        ptr, idx, val = np.array([0, 1, 2], np.int32), np.array([0, 3], np.int32), np.array([1.0, 2.0])
        x = np.zeros((2, n))
        call = s.lib.solver_hipmf_solve_sparse
        inv = s.lib.solver_hipmf_inverse_entries
        r1, out1 = np.array([0], np.int32), np.zeros(1)
        assert call(s.h, x, n, 2, ptr, idx, val, 0, None, 0) == ERROR_NEED_INITIALIZATION
        assert inv(s.h, 1, r1, r1, out1, 0) == ERROR_NEED_INITIALIZATION
        assert s.initialize(n, rp, ci) == 0
        assert call(s.h, x, n, 2, ptr, idx, val, 0, None, 0) == ERROR_NEED_FACTORIZATION
        assert inv(s.h, 1, r1, r1, out1, 0) == ERROR_NEED_FACTORIZATION
        assert s.lib.solver_hipmf_solve_sparse_device(s.h, C.c_void_p(8), n, 2, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), 0, None, 0) == ERROR_NEED_FACTORIZATION
        assert s.factorize(v) == 0
        assert call(s.h, x, n, 2, ptr, idx, val, 0, None, 0) == 0
        sel = np.array([1, 1, 4], np.int32)
        bad = ERROR_HIPMF_INVALID_VALUE
        assert call(s.h, x, n, 0, ptr, idx, val, 0, None, 0) == bad  # nrhs < 1
        assert call(s.h, x, n - 1, 2, ptr, idx, val, 0, None, 0) == bad  # ldx < n with all rows
        assert call(s.h, x, 2, 2, ptr, idx, val, 3, sel.ctypes.data, 0) == bad  # ldx < nsel
        assert call(s.h, x, 3, 2, ptr, idx, val, 0, sel.ctypes.data, 0) == bad  # nsel < 1 with a selection
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
            s.solve_sparse(ptr, idx, val, select=[7])
        assert e.value.code == bad
        raw = C.CDLL(s.lib._name)  # (untyped bindings: NULL pointers pass)
        raw.solver_hipmf_solve_sparse.restype = raw.solver_hipmf_inverse_entries.restype = C.c_int32
        h, xp, pp, ip, vp = C.c_void_p(s.h), x.ctypes.data_as(C.c_void_p), ptr.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p)
        assert raw.solver_hipmf_solve_sparse(h, None, n, 2, pp, ip, vp, 0, None, 0) == ERROR_NULL_POINTER
        assert raw.solver_hipmf_solve_sparse(h, xp, n, 2, None, ip, vp, 0, None, 0) == ERROR_NULL_POINTER
        assert raw.solver_hipmf_solve_sparse(h, xp, n, 2, pp, None, vp, 0, None, 0) == ERROR_NULL_POINTER
        assert raw.solver_hipmf_solve_sparse(None, xp, n, 2, pp, ip, vp, 0, None, 0) == ERROR_NULL_POINTER
        assert raw.solver_hipmf_inverse_entries(h, 1, None, ip, vp, 0) == ERROR_NULL_POINTER
    finally:
        s.close()


def test_host_mirror(emu_lib, monkeypatch):
    """LinSolver.solve_sparse / inverse_entries of russell_amd.sparse: both argument forms, the selection, the error strings"""
    _prune_always(monkeypatch)
    from russell_amd import sparse as S

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    S._L().rh_set_hipmf_library(emu_lib.encode())
    try:
        n, rp, ci, v = P.poisson2d(20, 18)
        A = sp.csr_matrix((v, ci, rp), shape=(n, n))
        coo = A.tocoo()
        mat = S.CooMatrix.from_arrays(n, n, coo.row, coo.col, coo.data)
        solver = S.LinSolver(S.Genie.Hipmf)
        with pytest.raises(S.StrError, match="factorize must be called"):
            solver.solve_sparse([([0], [1.0])])
        solver.actual.factorize(mat)
        Ad = A.toarray()
        cols = [([3], [2.0]), ([], []), ([1, 7, 100], [1.0, -1.0, 0.5])]
        B = np.zeros((3, n))
        for c, (i, vals) in enumerate(cols):
            B[c, i] = vals
        Xd = np.linalg.solve(Ad, B.T).T
        X = solver.solve_sparse(cols)
        assert X.shape == (3, n) and np.abs(X - Xd).max() <= 1e-13 * np.abs(Xd).max() and not X[1].any()
        sel = [5, 0, 5, n - 1]
        ptr, idx, val = np.array([0, 1, 1, 4]), np.array([3, 1, 7, 100]), np.array([2.0, 1.0, -1.0, 0.5])
        Xs = solver.solve_sparse((ptr, idx, val), select=sel)
        assert np.array_equal(Xs.view(np.uint64), X[:, sel].view(np.uint64))
        rows, ccols = np.array([4, 9, 4, 200]), np.array([9, 4, 9, 17])
        assert np.abs(solver.inverse_entries(rows, ccols) - np.linalg.inv(Ad)[rows, ccols]).max() <= 1e-13 * np.abs(np.linalg.inv(Ad)).max()
        with pytest.raises(S.StrError, match="outside range"):
            solver.solve_sparse([([n], [1.0])])
        with pytest.raises(S.StrError, match="ascending and unique"):
            solver.solve_sparse([([4, 2], [1.0, 1.0])])
        with pytest.raises(S.StrError, match="same length"):
            solver.solve_sparse([([4, 2], [1.0])])
        with pytest.raises(S.StrError, match="selected row is outside range"):
            solver.solve_sparse(cols, select=[n])
        with pytest.raises(S.StrError, match="must not be empty"):
            solver.solve_sparse(cols, select=[])
        with pytest.raises(S.StrError, match="at least one column"):
            solver.solve_sparse([])
        with pytest.raises(S.StrError, match="same, positive length"):
            solver.inverse_entries([1, 2], [1])
        with pytest.raises(S.StrError, match="outside range"):
            solver.inverse_entries([1], [n])
    finally:
        S._L().rh_set_hipmf_library(os.path.join(root, "russell_amd", "lib", "librussell_hipmf.so").encode())
