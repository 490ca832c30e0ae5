"""Sparse right-hand sides, selected solution rows and entries of the inverse on the MI355X: the cases of tests/test_sparse_rhs_cpu.py
through the product build (its run_* functions with lib = None, its tolerance rule and constants), the 300 x 200 grid against the CPU
oracle test_gpu_parity.py uses at that size, and the 1M-DOF 2D matrix against solver_hipmf_solve_device on the expanded block."""
import numpy as np
import pytest
import scipy.sparse as sp

import oracle_lib as O
import test_sparse_rhs_cpu as T
from russell_amd import problems as P
from test_gpu_parity import oracle_solve

pytestmark = pytest.mark.gpu

SMALL = ["mumps5", "bfwb62", "poisson", "poisson_lower", "saddle"]


@pytest.fixture(scope="module")
def mats():
    return T.matrices()


@pytest.mark.parametrize("name", SMALL)
def test_accuracy_against_dense_solve(monkeypatch, mats, name):
    T._prune_always(monkeypatch)
    print("largest ratio on %s: %.2f" % (name, T.run_accuracy(None, *mats[name])))


@pytest.mark.parametrize("name", SMALL)
def test_selection_is_bitwise_the_rows_of_the_full_result(monkeypatch, mats, name):
    T._prune_always(monkeypatch)
    T.run_selection(None, *mats[name])


@pytest.mark.parametrize("name", ["poisson", "poisson_lower"])
def test_pruning_happens(monkeypatch, mats, name):
    T._prune_always(monkeypatch)
    T.run_counters(None, *mats[name])


@pytest.mark.parametrize("name", ["poisson", "poisson_lower", "saddle"])
def test_no_stale_data(monkeypatch, mats, name):
    T._prune_always(monkeypatch)
    T.run_no_stale_data(None, *mats[name])


@pytest.mark.parametrize("name", ["poisson", "poisson_lower"])
def test_ordinary_solve_untouched(monkeypatch, mats, name):
    """the tagged workspace of the single-column solve is not the pruned path's: same bits before and after, no fallback counted"""
    T._prune_always(monkeypatch)
    T.run_ordinary_solve_untouched(None, *mats[name])


@pytest.mark.parametrize("name", ["bfwb62", "poisson"])
def test_fallback_by_share(monkeypatch, mats, name):
    monkeypatch.setenv("HIPMF_PRUNE_MAX_SHARE", "0")
    T.run_fallback(None, *mats[name])


def test_perturbed_factor_takes_the_ordinary_solve(monkeypatch):
    T._prune_always(monkeypatch)
    T.run_perturbed(None)


@pytest.mark.parametrize("name", ["bfwb62", "poisson", "saddle"])
def test_inverse_entries(monkeypatch, mats, name):
    T._prune_always(monkeypatch)
    T.run_inverse_entries(None, *mats[name])


@pytest.mark.parametrize("name", ["poisson", "poisson_lower"])
def test_device_entry_point(monkeypatch, mats, name):
    T._prune_always(monkeypatch)
    T.run_device_entry(None, *mats[name])


@pytest.mark.parametrize("lower", [False, True])
def test_grid_300x200_against_the_oracle(monkeypatch, lower):
    """60 000 unknowns, tiled fronts of several hundred rows (LU and L D L^T): accuracy by the tolerance rule against the CPU oracle, the
    selection bit for bit, the counters"""
    T._prune_always(monkeypatch)
    n, rp, ci, v = P.poisson2d(300, 200)
    init, kw, values = (n, rp, ci), dict(values=v), v
    if lower:
        lrp, lci, lv = P.lower_triangle(n, rp, ci, v)
        init, kw, values = (n, lrp, lci), dict(general_symmetric=True), lv
    s = T.handle(None, init, kw, values)
    try:
        st = s.stats()
        assert st["max_front"] > 256 and s.counter("symmetric_ldlt") == int(lower)
        ptr, idx, val, B = T.sparse_columns(n, (1, 3, 0, 2, 9, 1, 40, 1, 1), 21)
        _, lu = oracle_solve(n, rp, ci, v, B[0], q=s.permutation())
        Xd = np.array([lu.solve(B[c]) for c in range(B.shape[0])])
        X = s.solve_sparse(ptr, idx, val)
        assert s.counter("pruned_blocks") == 1 and s.counter("pruned_bwd_fronts") == st["nsuper"]
        assert s.counter("pruned_fwd_fronts") < st["nsuper"]
        print("largest ratio: %.2f" % T.check_rule(X, s.solve_many(B), Xd, "300x200 lower=%s" % lower))
        sel = np.random.default_rng(2).choice(n, 50, replace=False).astype(np.int32)
        Xs = s.solve_sparse(ptr, idx, val, select=sel)
        assert np.array_equal(Xs.view(np.uint64), X[:, sel].view(np.uint64))
        assert s.counter("pruned_bwd_fronts") < st["nsuper"]
    finally:
        s.close()


def test_1m_dof_selected_rows_against_solve_device():
    """BASELINE config 2 (1000 x 1000 grid), refinement_nstep = 0: 16 unit columns in one corner region, 64 selected rows nearby.  The
    surrogate for the exact solution is a handle with the default refinement; the yardstick is solver_hipmf_solve_device on the expanded
    block of the unrefined handle, which also gives the scale."""
    n, rp, ci, v = P.poisson2d(1000)
    s = T.handle(None, (n, rp, ci), {}, v)
    ref = T.handle(None, (n, rp, ci), {}, v, nstep=-1)
    bufs = []
    try:
        st = s.stats()
        units = np.array([1000 * (3 + i // 4) + 5 + (i % 4) for i in range(16)], np.int32)
        sel = np.array([1000 * (2 + k // 8) + 3 + (k % 8) for k in range(64)], np.int32)
        ptr, val = np.arange(17, dtype=np.int32), np.ones(16)
        x0 = s.solve(np.ones(n))
        fb = s.stats()["fused_fallbacks"]
        Xs = s.solve_sparse(ptr, units, val, select=sel)
        assert s.counter("pruned_blocks") == 1  # (the default share: far below it)
        assert 0 < s.counter("pruned_fwd_fronts") < st["nsuper"] and 0 < s.counter("pruned_bwd_fronts") < st["nsuper"]
        print("fronts visited: forward %d, backward %d of %d" % (s.counter("pruned_fwd_fronts"), s.counter("pruned_bwd_fronts"), st["nsuper"]))
        assert s.stats()["fused_fallbacks"] == fb
        assert np.array_equal(s.solve(np.ones(n)).view(np.uint64), x0.view(np.uint64))
        B = np.zeros((16, n))
        B[np.arange(16), units] = 1.0
        d_b, d_x = s.dev_alloc(B.nbytes), s.dev_alloc(B.nbytes)
        bufs += [d_b, d_x]
        s.h2d(d_b, B)
        s.solve_device(d_x, d_b, nrhs=16)
        Xdev = np.zeros_like(B)
        s.d2h(Xdev, d_x)
        Xref = ref.solve_many(B)
        worst = 0.0
        for c in range(16):
            scale = np.abs(Xdev[c]).max()
            e_ref = np.abs(Xdev[c] - Xref[c]).max()
            e_p = np.abs(Xs[c] - Xref[c][sel]).max()
            floor = T.FLOOR_ULPS * T.EPS * scale
            worst = max(worst, max(e_p - floor, 0.0) / e_ref if e_ref > 0 else 0.0)
            print("column %d: pruned %.3e, solve_device %.3e, scale %.3e" % (c, e_p, e_ref, scale))
            assert e_p <= T.FACTOR * e_ref + floor, (c, e_p, e_ref, scale)
        print("largest ratio: %.2f" % worst)
    finally:
        for p in bufs:
            s.dev_free(p)
        s.close()
        ref.close()
