"""Solve with new complex values on a kept factor on the MI355X: the cases of tests/test_solve_updated_complex_cpu.py through the product
build (its run_* functions with lib = None, its references and its accuracy rule), the 200 x 150 complex shifted grid -- tiled fronts: the
pass pair inside the iteration takes the dependency-driven schedule -- and the 500 x 500 grid through device pointers."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import test_solve_updated_complex_cpu as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("h1", [0.5, 2.0, 0.1])
def test_complex_arithmetic_is_used(h1):
    T.run_shift(None, h1)


def test_complex_arithmetic_is_used_unsymmetric():
    T.run_shift(None, 0.1, unsym=True)


@pytest.mark.parametrize("name", ["ref5", "weak300", "symlower"])
def test_unchanged_values_take_one_step(name):
    T.run_unchanged(None, name)


@pytest.mark.parametrize("name", ["ref5", "random200"])
def test_rank_three_change(name):
    T.run_rank_change(None, name)


@pytest.mark.parametrize("n", [512, 513, 2049])
def test_tile_edges(n):
    T.run_rank_change(None, "zchain%d" % n)


@pytest.mark.parametrize("restart", [T.ZPASSV, T.ZPASSV - 1])
def test_basis_count_edges(monkeypatch, restart):
    steps, zsteps, cycles = T.run_shift(None, 0.5, restart=restart, max_steps=200, monkeypatch=monkeypatch, real_too=False)
    assert zsteps >= T.ZPASSV + 2 and steps > restart and cycles >= 2


def test_restart_four_many_cycles(monkeypatch):
    steps, zsteps, cycles = T.run_shift(None, 10.0, restart=4, max_steps=400, monkeypatch=monkeypatch, real_too=False)
    assert steps > 8 and cycles > 2


def test_not_converged_zero_and_nan():
    T.run_not_converged(None)


@pytest.mark.parametrize("name", ["random200", "symlower"])
def test_mapped_values(name):
    T.run_mapped(None, name)


def test_status_codes():
    T.run_status_codes(None)


@pytest.mark.parametrize("name", ["random200", "weak300", "symlower"])
def test_no_side_effects(name):
    T.run_no_side_effects(None, name)


@pytest.mark.parametrize("name", ["random200", "symlower"])
def test_reproducible(name):
    T.run_reproducible(None, name)


def test_plain_real_equivalent_factor():
    T.run_reproducible(None, "random200", env={"HIPMF_COMPLEX_PAIRS": "0"})


def test_perturbed_factor():
    T.run_perturbed(None)


def test_device_entry_point():
    T.run_device_entry(None, "random200")


def test_host_mirror():
    T.run_host_mirror(None)


def cond2_shifted_grid(nx, ny, h):
    """cond_2 of K(h) = (alpha + i beta) / h I + L: L is symmetric with eigenvalues known in closed form, so K is normal, its singular
    values are the moduli of its eigenvalues c + lambda"""
    lx = 2.0 - 2.0 * np.cos(np.pi * np.arange(1, nx + 1) / (nx + 1))
    ly = 2.0 - 2.0 * np.cos(np.pi * np.arange(1, ny + 1) / (ny + 1))
    mod = np.abs(np.add.outer(lx, ly) + (T.ALPHA + 1j * T.BETA) / h)
    return float(mod.max() / mod.min())


def test_closed_form_condition_number():
    """the formula above against NumPy's cond on a small grid"""
    n, rp, ci, vals = T.shifted_grid(9, 7)
    cond = np.linalg.cond(T.full(n, rp, ci, vals(0.5)).toarray())
    assert abs(cond2_shifted_grid(9, 7, 0.5) - cond) <= 1e-10 * cond


def test_grid_200x150_tiled_fronts():
    """30 000 complex unknowns, a real-equivalent root separator of more than 256 rows: K(1) -> K(0.5)"""
    nx, ny = 200, 150
    n, rp, ci, vals = T.shifted_grid(nx, ny)
    v0, v1 = vals(1.0), vals(0.5)
    s = T.ZH(None, n, rp, ci, v0)
    try:
        istats, _ = s.stats()
        assert istats[6] > 256, istats[6]  # max_front
        b = T.rhs_for(n, 12)
        fb = s.counter("fused_fallbacks")
        x, steps, relres, status = s.solve_updated(b, v1, rel_tol=T.TOL)
        print("%d steps in %d cycle(s), relres %.3e, max_front %d" % (steps, s.counter("updated_cycles"), relres, istats[6]))
        assert status == 0 and s.counter("fused_fallbacks") == fb == 0 and s.counter("updated_complex_arithmetic") == 1
        A1 = T.full(n, rp, ci, v1)
        cond = cond2_shifted_grid(nx, ny, 0.5)
        xd = spla.spsolve(A1.tocsc(), b)  # (a direct sparse LU in double: its own error, cond eps, is far below the bound asserted)
        T.check_accuracy(A1, x, b, relres, cond, xd)
    finally:
        s.close()


def test_grid_500x500_through_device_pointers():
    """250 000 complex unknowns, K(1) -> K(0.5), default tolerance 1e-12; no dense reference exists at this size: the step count is
    printed, not bounded"""
    n, rp, ci, vals = T.shifted_grid(500, 500)
    v0, v1 = vals(1.0), vals(0.5)
    s = T.ZH(None, n, rp, ci, v0)
    ptrs = []
    try:
        b = T.rhs_for(n, 13)
        d_x, d_b, d_v = s.dev_alloc(16 * n), s.dev_alloc(16 * n), s.dev_alloc(16 * v1.size)
        ptrs += [d_x, d_b, d_v]
        s.h2d(d_b, T.interleave(b))
        s.h2d(d_v, T.interleave(v1))
        out = []
        for _ in range(2):
            steps, relres, status = s.solve_updated_device(d_x, d_b, d_v)
            x = np.zeros(2 * n)
            s.d2h(x, d_x)
            out.append((steps, relres, status, x))
        steps, relres, status, x = out[0]
        print("%d steps in %d cycle(s), relres %.3e" % (steps, s.counter("updated_cycles"), relres))
        assert status == 0 and relres <= 1e-12
        assert out[1][:3] == out[0][:3] and np.array_equal(out[1][3].view(np.uint64), x.view(np.uint64))
        assert s.counter("fused_fallbacks") == 0
        assert s.counter("updated_basis_bytes") == 61 * 2 * n * 8
        own, bound, bound_double = T.own_relres(T.full(n, rp, ci, v1), T.as_complex(x), b)
        print("own relres %.3e (rounding bounds %.3e own, %.3e double)" % (own, bound, bound_double))
        assert abs(relres - own) <= bound + bound_double
    finally:
        for p in ptrs:
            s.dev_free(p)
        s.close()
