#!/usr/bin/env python3
"""Blocked transposed solves against the column loop: device-resident random columns on one handle per matrix, median of 5 timings of
solve_transpose_device (one column at a time) and of solve_transpose_many_device (16 columns per pass pair over the factor), with
refinement off and with the default refinement; the largest componentwise backward error of three columns of the blocked result.
usage: transpose_many.py [c2] [3d] [quick]     (default: c2 with 64 and 256 columns, then 100^3 with 32; quick: c2 with 64 only;
                                               nstat: one blocked call of 64 columns on c2 and nothing else -- for a kernel trace)
       transpose_many.py --complex              the complex handle (profiles/r17_complex_transpose_many.txt): K = (alpha + i beta) I + L on the
                                               500 x 500 grid, 16 and 64 device-resident columns, A^H and A^T: median of 5 timings of
                                               complex_solver_hipmf_solve_transpose_many_device against the column loop (host pointers:
                                               complex_solver_hipmf_solve_transpose has no device form), ms per column"""
import os, sys, time
import numpy as np
import scipy.sparse as sp
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from russell_amd import problems as P
from russell_amd.backend import Hipmf

EPS = np.finfo(float).eps


def cd3d(k, peclet=20.0):
    h = 1.0 / (k + 1)
    T = sp.diags([-1.0 - 0.5 * peclet * h, 2.0, -1.0 + 0.5 * peclet * h], [-1, 0, 1], shape=(k, k))
    D = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(k, k))
    I = sp.identity(k)
    A = (sp.kron(sp.kron(I, I), T) + sp.kron(sp.kron(I, D), I) + sp.kron(sp.kron(D, I), I)).tocsr()
    A.sort_indices()
    return A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def omega_t(A, x, b):
    At = sp.csr_matrix(A.T)
    r = b - At @ x
    den = abs(At) @ np.abs(x) + np.abs(b)
    return float(np.max(np.abs(r) / np.where(den > 0, den, 1.0)))


def median5(fn):
    fn()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def run(name, problem, counts, trace_only=False):
    n, rp, ci, v = problem
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))
    for nstep, label in ((0, "refinement off"), (-1, "default refinement")):
        s = Hipmf()
        assert s.initialize(n, rp, ci, refinement_nstep=nstep) == 0
        assert s.factorize(v) == 0
        st = s.stats()
        for nrhs in counts:
            B = np.random.default_rng([8, nrhs]).standard_normal((nrhs, n))
            d_b, d_x = s.dev_alloc(B.nbytes), s.dev_alloc(B.nbytes)
            s.h2d(d_b, B)
            if trace_only:
                s.solve_transpose_many_device(d_x, d_b, nrhs)
                s.dev_free(d_b), s.dev_free(d_x), s.close()
                return
            t_blk = median5(lambda: s.solve_transpose_many_device(d_x, d_b, nrhs))
            blocks = s.counter("transposed_blocks")
            X = np.zeros_like(B)
            s.d2h(X, d_x)
            om = max(omega_t(A, X[j], B[j]) for j in (0, nrhs // 2, nrhs - 1))
            t_loop = median5(lambda: s.solve_transpose_device(d_x, d_b, nrhs=nrhs))
            print("%s n=%d max_front=%d factor %.2f GB, %d columns, %s: blocked %.2f ms (%.3f ms/column, %d blocks), column loop %.2f ms "
                  "(%.3f ms/column), ratio %.2f; omega of the blocked result (3 columns) <= %.1f eps" %
                  (name, n, st["max_front"], s.counter("persistent_bytes") / 1e9, nrhs, label, t_blk, t_blk / nrhs, blocks, t_loop, t_loop / nrhs,
                   t_loop / t_blk, om / EPS), flush=True)
            s.dev_free(d_b), s.dev_free(d_x)
        s.close()


def run_complex(out_path):
    import ctypes as C
    from russell_amd._capi import load
    lib = load()
    nx = ny = 500
    lap = lambda m: sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    L = sp.csr_matrix(sp.kron(sp.identity(ny), lap(nx)) + sp.kron(lap(ny), sp.identity(nx)))
    L.sort_indices()
    n, rp, ci = L.shape[0], L.indptr.astype(np.int32), L.indices.astype(np.int32)
    v = L.data + (2.6811 + 3.0504j) * (np.repeat(np.arange(n), np.diff(rp)) == ci)
    zv = np.ascontiguousarray(np.stack([v.real, v.imag], axis=1).ravel())
    h = lib.complex_solver_hipmf_new()
    assert h and lib.complex_solver_hipmf_initialize(h, 0, 1, -1.0, -1, 0, 0, n, rp, ci, zv.ctypes.data) == 0
    assert lib.complex_solver_hipmf_factorize(h, None, None, None, None, None, None, None, 0, 0, zv) == 0
    lines = ["complex_solver_hipmf_solve_transpose_many_device against complex_solver_hipmf_solve_transpose column by column, complex shifted grid %d x %d "
             "(n = %d complex), default refinement, one MI355X, median of 5" % (nx, ny, n)]
    for nrhs in (16, 64):
        B = np.ascontiguousarray(np.random.default_rng([8, nrhs]).standard_normal((nrhs, 2 * n)))
        X = np.zeros_like(B)
        d_b, d_x = lib.hipmf_device_malloc(B.nbytes), lib.hipmf_device_malloc(B.nbytes)
        assert d_b and d_x and lib.hipmf_memcpy_h2d(d_b, B.ctypes.data_as(C.c_void_p), B.nbytes) == 0
        for conjugate in (1, 0):
            def blocked():
                assert lib.complex_solver_hipmf_solve_transpose_many_device(h, d_x, d_b, nrhs, n, conjugate) == 0
                assert lib.hipmf_device_synchronize() == 0

            def loop():
                for c in range(nrhs):
                    assert lib.complex_solver_hipmf_solve_transpose(h, X[c], B[c], conjugate, 0) == 0
            t_blk, blocks = median5(blocked), int(lib.complex_solver_hipmf_get_counter(h, 23))
            t_loop = median5(loop)
            lines.append("  %s, %d columns: blocked %.2f ms (%.3f ms/column, %d blocks), column loop %.2f ms (%.3f ms/column), ratio %.2f" %
                         ("A^H" if conjugate else "A^T", nrhs, t_blk, t_blk / nrhs, blocks, t_loop, t_loop / nrhs, t_loop / t_blk))
            print(lines[-1], flush=True)
        lib.hipmf_device_free(d_b), lib.hipmf_device_free(d_x)
    lib.complex_solver_hipmf_drop(h)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--complex" in args:
        run_complex(os.path.join(ROOT, "profiles", "r17_complex_transpose_many.txt"))
        sys.exit(0)
    if "nstat" in args:
        run("c2", P.convection_diffusion2d(1000), [64], trace_only=True)
        sys.exit(0)
    if not args or "c2" in args or "quick" in args:
        run("c2", P.convection_diffusion2d(1000), [64] if "quick" in args else [64, 256])
    if not args or "3d" in args:
        run("3d-100", cd3d(100), [32])
