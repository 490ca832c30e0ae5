"""The many-right-hand-side entry points at their edges, on the CPU emulator (tests/test_many_rhs_edges_gpu.py repeats it on the device):
padded columns (ld > n: ldx / cstr of Solver::solve_core, k_perm_in_cols, k_perm_out_cols without refinement; k_residual_cols and the
correcting launches with it; the host entry point stages its columns at stride n, so only the two device entry points carry cstr = ld), the column counts around
the 8- and 16-column instances (12 is the last count that takes 8-column blocks), a zero and a tiny column among ordinary ones (the
di > 0 guard of the blocked residual kernel), and the argument checks of all three entry points."""
import numpy as np
import pytest

import front_shapes as F
from russell_amd import problems as P
from russell_amd.backend import Hipmf, HipmfError

ERROR_HIPMF_INVALID_VALUE = 803
NRHS = [1, 2, 8, 9, 12, 13, 16, 17, 31, 32, 33, 64, 65]
SENTINEL = -7.25e77  # (any bit pattern no solve produces)


def _handle(lib, grid, symmetric, **kw):
    n, rp, ci, v = P.poisson2d(grid)
    rng = np.random.default_rng(grid)
    v = v * (1.0 + 0.2 * rng.uniform(-1, 1, v.size)) if not symmetric else v
    A = __import__("scipy.sparse", fromlist=["csr_matrix"]).csr_matrix((v, ci, rp), shape=(n, n)).toarray()
    if symmetric:
        rp, ci, v = P.lower_triangle(n, rp, ci, v)
    s = Hipmf(lib)
    assert s.initialize(n, rp, ci, general_symmetric=symmetric, **kw) == 0
    assert s.factorize(v) == 0
    assert s.counter("symmetric_ldlt") == int(symmetric)
    return s, n, A


def run_padded_columns(lib, symmetric, nrhs):
    """ld = n + 3 through solve_many (host), solve_device and solve_transpose_device: every column to the tolerance of
    tests/front_shapes.py (no refinement), the padding of x bit-identical to its sentinel, rhs unchanged"""
    case = F.chain(32, 100, 97, 31, seed=11, symmetric=symmetric)  # (the matrices the tolerance was measured on: tests/front_shapes.py)
    n, A = case.n, case.A
    s = Hipmf(lib)
    try:
        assert s.initialize(n, case.rp, case.ci, ordering=F.ORDERING_NONE, refinement_nstep=0, general_symmetric=symmetric) == 0
        assert s.factorize(case.v) == 0
        assert s.num_perturbed == 0 and s.counter("symmetric_ldlt") == int(symmetric)
        ld = n + 3
        rng = np.random.default_rng(nrhs)
        B = np.full((nrhs, ld), SENTINEL)
        B[:, :n] = rng.standard_normal((nrhs, n))
        B0 = B.copy()
        ref = F.Reference(A)
        ref_t = ref.transposed()
        X = s.solve_many(B, ld=ld)
        assert np.array_equal(B, B0) and np.array_equal(X[:, n:].view(np.uint64), B0[:, n:].view(np.uint64))
        for j in range(nrhs):
            ref.check(X[j, :n], B[j, :n], "solve_many ld=n+3 column %d" % j)
        d_b, d_x = s.dev_alloc(B.nbytes), s.dev_alloc(B.nbytes)
        try:
            for fn, r in ((s.solve_device, ref), (s.solve_transpose_device, ref_t)):
                s.h2d(d_b, B0)
                s.h2d(d_x, np.full((nrhs, ld), SENTINEL))
                fn(d_x, d_b, nrhs=nrhs, ld=ld)
                X, Bb = np.zeros((nrhs, ld)), np.zeros((nrhs, ld))
                s.d2h(X, d_x)
                s.d2h(Bb, d_b)
                assert np.array_equal(Bb.view(np.uint64), B0.view(np.uint64)), fn.__name__
                assert np.array_equal(X[:, n:].view(np.uint64), np.full((nrhs, 3), SENTINEL).view(np.uint64)), fn.__name__
                for j in range(nrhs):
                    r.check(X[j, :n], B0[j, :n], "%s ld=n+3 column %d" % (fn.__name__, j))
        finally:
            s.dev_free(d_b)
            s.dev_free(d_x)
    finally:
        s.close()


def run_padded_columns_refined(lib, symmetric, nrhs):
    """the same layout with DEFAULT refinement on a grid matrix, whose blocked first solve is far enough from eps for a step to run:
    k_residual_cols and the correcting k_perm_in_cols / k_perm_out_cols of the refinement loop with cstr = ld > n.  Each column
    against the single refined solve of that column (the bound of test_many_rhs_blocks_agree_with_single_solves)."""
    s, n, A = _handle(lib, 24, symmetric)
    try:
        ld = n + 3
        rng = np.random.default_rng(nrhs)
        B0 = np.full((nrhs, ld), SENTINEL)
        B0[:, :n] = rng.standard_normal((nrhs, n)) @ A.T
        pad = np.full((nrhs, 3), SENTINEL).view(np.uint64)
        d_b, d_x = s.dev_alloc(B0.nbytes), s.dev_alloc(B0.nbytes)
        try:
            for fn, single in ((s.solve_device, s.solve), (s.solve_transpose_device, s.solve_transpose)):
                s.h2d(d_b, B0)
                s.h2d(d_x, np.full((nrhs, ld), SENTINEL))
                fn(d_x, d_b, nrhs=nrhs, ld=ld)
                if fn == s.solve_device or symmetric:  # (general storage: the transposed columns are refined one by one, no step count in stats())
                    assert s.stats()["refinement_steps"] >= 1
                X, Bb = np.zeros((nrhs, ld)), np.zeros((nrhs, ld))
                s.d2h(X, d_x)
                s.d2h(Bb, d_b)
                assert np.array_equal(Bb.view(np.uint64), B0.view(np.uint64)), fn.__name__
                assert np.array_equal(X[:, n:].view(np.uint64), pad), fn.__name__
                for j in range(nrhs):
                    xj = single(B0[j, :n])
                    assert np.max(np.abs(X[j, :n] - xj)) <= 1e-12 * np.max(np.abs(xj)), (fn.__name__, j)
        finally:
            s.dev_free(d_b)
            s.dev_free(d_x)
    finally:
        s.close()


def run_column_counts(lib, symmetric, grid, counts):
    """each column of a block against the single solve of that column, at the bound of test_many_rhs_blocks_agree_with_single_solves"""
    s, n, A = _handle(lib, grid, symmetric)
    try:
        rng = np.random.default_rng(grid)
        XS = rng.standard_normal((max(counts), n))
        B = XS @ A.T
        singles = [s.solve(B[j]) for j in range(max(counts))]
        for nrhs in counts:
            X = s.solve_many(B[:nrhs])
            for j in range(nrhs):
                assert np.max(np.abs(X[j] - singles[j])) <= 1e-12 * np.max(np.abs(singles[j])), (nrhs, j)
            assert np.max(np.abs(X - XS[:nrhs])) / np.max(np.abs(XS)) < 1e-10
    finally:
        s.close()


def run_zero_and_tiny_columns(lib, symmetric):
    """default refinement: a zero column gives exactly zero, a column scaled by 1e-300 no NaN, the others what they give without them"""
    s, n, A = _handle(lib, 40, symmetric)
    try:
        rng = np.random.default_rng(3)
        B = rng.standard_normal((11, n))
        plain = s.solve_many(B)
        B2 = B.copy()
        B2[3] = 0.0
        B2[6] *= 1e-300
        X = s.solve_many(B2)
        assert np.all(np.isfinite(X))
        assert np.array_equal(X[3], np.zeros(n))
        for j in range(11):
            if j not in (3, 6):
                assert np.max(np.abs(X[j] - plain[j])) <= 1e-12 * np.max(np.abs(plain[j])), j
        assert np.max(np.abs(X[6] - plain[6] * 1e-300)) <= 1e-10 * np.max(np.abs(plain[6])) * 1e-300
    finally:
        s.close()


def run_argument_checks(lib):
    s, n, _ = _handle(lib, 12, False)
    try:
        b = np.zeros((2, n))
        d = s.dev_alloc(b.nbytes)
        try:
            assert s.lib.solver_hipmf_solve_many(s.h, b.copy(), b, 0, n, 0) == ERROR_HIPMF_INVALID_VALUE
            assert s.lib.solver_hipmf_solve_many(s.h, b.copy(), b, 2, n - 1, 0) == ERROR_HIPMF_INVALID_VALUE
            for fn in (s.solve_device, s.solve_transpose_device):
                for nrhs, ld in ((0, n), (2, n - 1)):
                    with pytest.raises(HipmfError) as e:
                        fn(d, d, nrhs=nrhs, ld=ld)
                    assert e.value.code == ERROR_HIPMF_INVALID_VALUE
            with pytest.raises(ValueError):
                s.solve_many(b, ld=n + 1)
        finally:
            s.dev_free(d)
    finally:
        s.close()


@pytest.mark.parametrize("symmetric", [False, True], ids=["lu", "ldlt"])
@pytest.mark.parametrize("nrhs", [1, 9, 17])
def test_padded_columns(emu_lib, symmetric, nrhs):
    run_padded_columns(emu_lib, symmetric, nrhs)


@pytest.mark.parametrize("symmetric", [False, True], ids=["lu", "ldlt"])
@pytest.mark.parametrize("nrhs", [9, 17])
def test_padded_columns_with_refinement(emu_lib, symmetric, nrhs):
    run_padded_columns_refined(emu_lib, symmetric, nrhs)


@pytest.mark.parametrize("symmetric", [False, True], ids=["lu", "ldlt"])
def test_column_counts_agree_with_single_solves(emu_lib, symmetric):
    run_column_counts(emu_lib, symmetric, 30, [1, 2, 8, 12, 13, 16, 33])


@pytest.mark.parametrize("symmetric", [False, True], ids=["lu", "ldlt"])
def test_zero_and_tiny_columns(emu_lib, symmetric):
    run_zero_and_tiny_columns(emu_lib, symmetric)


def test_argument_checks(emu_lib):
    run_argument_checks(emu_lib)
