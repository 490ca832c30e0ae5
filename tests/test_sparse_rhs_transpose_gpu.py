"""Sparse right-hand sides, selected rows and entries of the inverse through A^T on the MI355X: the cases of
tests/test_sparse_rhs_transpose_cpu.py through the product build (its run_* functions with lib = None, the tolerance rule and constants
of tests/test_sparse_rhs_cpu.py), and the 300 x 200 grid with perturbed values against the CPU oracle of A^T."""
import numpy as np
import pytest
import scipy.sparse as sp

import test_sparse_rhs_cpu as T
import test_sparse_rhs_transpose_cpu as TT
from russell_amd import problems as P
from test_gpu_parity import oracle_solve

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mats():
    out = T.matrices()
    out["big"], out["matched"] = TT.big_fronts(), TT.matched()
    return out


@pytest.mark.parametrize("name", TT.UNSYMMETRIC + ["matched"])
def test_accuracy_against_dense_solve(monkeypatch, mats, name):
    T._prune_always(monkeypatch)
    print("largest ratio on %s: %.2f" % (name, TT.run_accuracy(None, *mats[name])))


@pytest.mark.parametrize("mid", ["1", "0"])
def test_big_fronts(monkeypatch, mats, mid):
    T._prune_always(monkeypatch)
    monkeypatch.setenv("HIPMF_MID_FRONT", mid)
    A, init, kw, v = mats["big"]
    s = T.handle(None, init, kw, v)
    st = s.stats()
    assert st["max_front"] > 64 and st["max_pivots"] > 32 and (s.counter("mid_fronts") > 0) == (mid == "1")
    s.close()
    print("largest ratio with HIPMF_MID_FRONT=%s: %.2f" % (mid, TT.run_accuracy(None, A, init, kw, v)))
    TT.run_selection(None, A, init, kw, v)


@pytest.mark.parametrize("name", TT.UNSYMMETRIC + ["matched"])
def test_selection_is_bitwise_the_rows_of_the_full_result(monkeypatch, mats, name):
    T._prune_always(monkeypatch)
    TT.run_selection(None, *mats[name])


@pytest.mark.parametrize("name", ["poisson", "big"])
def test_no_stale_data(monkeypatch, mats, name):
    T._prune_always(monkeypatch)
    TT.run_no_stale_data(None, *mats[name])


def test_other_solves_untouched(monkeypatch, mats):
    T._prune_always(monkeypatch)
    TT.run_other_solves_untouched(None, *mats["poisson"])


def test_counters_and_block_edges(monkeypatch, mats):
    T._prune_always(monkeypatch)
    TT.run_counters(None, *mats["poisson"])


@pytest.mark.parametrize("name", ["poisson_lower", "saddle"])
def test_symmetric_handles_run_the_ordinary_path(monkeypatch, mats, name):
    T._prune_always(monkeypatch)
    TT.run_symmetric(None, *mats[name])


@pytest.mark.parametrize("name", ["bfwb62", "poisson"])
def test_fallback_by_share(monkeypatch, mats, name):
    monkeypatch.setenv("HIPMF_PRUNE_MAX_SHARE", "0")
    TT.run_fallback(None, *mats[name])


def test_perturbed_factor_takes_the_transposed_solve(monkeypatch):
    T._prune_always(monkeypatch)
    TT.run_perturbed(None)


@pytest.mark.parametrize("name", ["bfwb62", "poisson", "matched"])
def test_inverse_entries_by_rows(monkeypatch, mats, name):
    T._prune_always(monkeypatch)
    TT.run_inverse_entries_by_rows(None, *mats[name])


def test_device_entry_point(monkeypatch, mats):
    T._prune_always(monkeypatch)
    TT.run_device_entry(None, *mats["poisson"])


def test_grid_300x200_against_the_oracle(monkeypatch):
    """60 000 unknowns, general LU with tiled fronts of several hundred rows, values perturbed so that A^T != A: accuracy by the tolerance
    rule against the CPU oracle's factorisation of A^T, the selection bit for bit, the counters"""
    T._prune_always(monkeypatch)
    n, rp, ci, v = P.poisson2d(300, 200)
    v = v * (1.0 + 0.1 * np.random.default_rng(300).uniform(-1, 1, v.size))
    At = sp.csr_matrix((v, ci, rp), shape=(n, n)).T.tocsr()
    At.sort_indices()
    s = T.handle(None, (n, rp, ci), dict(values=v), v)
    try:
        st = s.stats()
        assert st["max_front"] > 256 and s.counter("symmetric_ldlt") == 0
        ptr, idx, val, B = T.sparse_columns(n, (1, 3, 0, 2, 9, 1, 40, 1, 1), 21)
        _, lu = oracle_solve(n, At.indptr.astype(np.int32), At.indices.astype(np.int32), At.data, B[0])
        Xd = np.array([lu.solve(B[c]) for c in range(B.shape[0])])
        X = s.solve_sparse(ptr, idx, val, transpose=True)
        assert s.counter("pruned_blocks") == 1 and s.counter("pruned_transposed_blocks") == 1 and s.counter("pruned_bwd_fronts") == st["nsuper"]
        assert s.counter("pruned_fwd_fronts") < st["nsuper"]
        print("largest ratio: %.2f" % T.check_rule(X, s.solve_transpose_many(B), Xd, "300x200 transposed"))
        sel = np.random.default_rng(2).choice(n, 50, replace=False).astype(np.int32)
        Xs = s.solve_sparse(ptr, idx, val, select=sel, transpose=True)
        assert np.array_equal(Xs.view(np.uint64), X[:, sel].view(np.uint64))
        assert s.counter("pruned_bwd_fronts") < st["nsuper"]
    finally:
        s.close()
