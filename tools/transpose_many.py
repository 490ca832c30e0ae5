#!/usr/bin/env python3
"""Blocked transposed solves against the column loop: device-resident random columns on one handle per matrix, median of 5 timings of
solve_transpose_device (one column at a time) and of solve_transpose_many_device (16 columns per pass pair over the factor), with
refinement off and with the default refinement; the largest componentwise backward error of three columns of the blocked result.
usage: transpose_many.py [c2] [3d] [quick]     (default: c2 with 64 and 256 columns, then 100^3 with 32; quick: c2 with 64 only;
                                               nstat: one blocked call of 64 columns on c2 and nothing else -- for a kernel trace)"""
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


if __name__ == "__main__":
    args = sys.argv[1:]
    if "nstat" in args:
        run("c2", P.convection_diffusion2d(1000), [64], trace_only=True)
        sys.exit(0)
    if not args or "c2" in args or "quick" in args:
        run("c2", P.convection_diffusion2d(1000), [64] if "quick" in args else [64, 256])
    if not args or "3d" in args:
        run("3d-100", cd3d(100), [32])
