#!/usr/bin/env python3
"""solver_hipmf_solve_updated_device against the caller's alternative (factorize_device + solve_device on the new values): the table of
profiles/r10_solve_updated.txt.  Needs an MI355X.

    python tools/solve_updated.py [--matrix 2d|3d|both] [--reps 9] [--warmup 2] [--tol 1e-10] [--out FILE]

Per matrix (the 1M-DOF 2D 5-point Poisson matrix + I, the 100^3 7-point one + I, general storage: LU) and per change of the values
    shift s1/s0 = 1.1, 2, 10     the diagonal shift of gamma M - J after a step-size change (s0 = 1)
    rank 16                      all entries of 16 rows rescaled by factors in [0.5, 1.5]
the line gives the steps of the call, the median wall time of a call (host clock around the blocking call, device-resident x, rhs and
values), the time per step, its split into pass pair / SpMV / Arnoldi kernels (HIP events inside the driver, HIPMF_UPDATED_TIMING=1, taken
in calls of their own: the events are not part of the timed calls), and the median wall time of solver_hipmf_factorize_device +
solver_hipmf_solve_device with the same new values on a second handle (default refinement).  Those two entry points are not touched by
the solve_updated change, so the second column is what the parent commit does.  break-even = alternative / time per step.

    python tools/solve_updated.py --nrhs N [--matrix ...] [--out profiles/r11_solve_updated_many.txt]

The block form (profiles/r11_solve_updated_many.txt): per matrix and change of the values three median wall times from the same run, on N
random device-resident columns:
    (a) ONE solver_hipmf_solve_updated_many_device call,
    (b) N solver_hipmf_solve_updated_device calls on the same columns (that code is not touched by the block form: what the parent offers),
    (c) solver_hipmf_factorize_device + solver_hipmf_solve_device(nrhs = N) on a second handle,
with the per-column step counts, UPDATED_STEPS (blocked pass pairs), UPDATED_COLUMN_STEPS and the split of (a) into pass pair / SpMV /
Arnoldi kernels (HIP events, calls of their own).  The figure of merit is (a)/N against (b)/N.

    python tools/solve_updated.py --complex [--out profiles/r12_solve_updated_complex.txt]

The complex form (profiles/r12_solve_updated_complex.txt): K(h) = (alpha + i beta) / h I + L on the 500 x 500 unit-spacing grid, Radau5's
alpha = 2.6811, beta = 3.0504, factorised at h0 = 1; per step-size change h0 -> h0/2 and h0 -> h0/10 the steps of
complex_solver_hipmf_solve_updated_device, the median wall time of a call (device-resident x, rhs and values), the time per step and its
split into pass pair / SpMV / Arnoldi kernels (HIP events, calls of their own), and the median wall time of
complex_solver_hipmf_factorize_mapped + complex_solver_hipmf_solve with the same new values on a second handle (host pointers: the complex
C-ABI has no device entry points for them) -- the parent commit's only way.  All medians come from the same run.

    python tools/solve_updated.py --complex --nrhs N [--out profiles/r13_solve_updated_complex_many.txt]

The complex block form (profiles/r13_solve_updated_complex_many.txt): the same grid and factor, h0 -> h0/2, N random device-resident
complex columns, three median wall times from the same run:
    (a) ONE complex_solver_hipmf_solve_updated_many_device call,
    (b) N complex_solver_hipmf_solve_updated_device calls on the same columns (that code is not touched by the block form),
    (c) complex_solver_hipmf_factorize_mapped + complex_solver_hipmf_solve_many(nrhs = N) on a second handle (host pointers),
with the per-column step counts, UPDATED_STEPS (blocked pass pairs), UPDATED_COLUMN_STEPS and the split of (a) into pass pair / SpMV /
Arnoldi kernels (HIP events, calls of their own).  The figures of merit are (a)/N, (b)/N and (c)/N.

    python tools/solve_updated.py --transpose [--complex] [--nrhs N] [--conjugate 0|1]

The transposed forms (profiles/r17_solve_updated_transpose.txt, appended to when --out is not given): the same matrices, changes and
measurements as the four modes above with A_new^T as the system -- solver_hipmf_solve_updated_transpose_device / _many_device,
complex_solver_hipmf_solve_updated_transpose_device / _many_device (--conjugate 1: A_new^H, the default; 0: A_new^T) -- the caller's
alternative being factorize + solve_transpose (block form: solve_transpose_many) on the new values, and, in the same run, the median
wall time of the non-transposed call on the same inputs ("plain").  The pass pair / SpMV / Arnoldi split is that of the transposed call."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from russell_amd import problems as P  # noqa: E402
from russell_amd.backend import Hipmf  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def run(name, n, rp, ci, v, args, out):
    diag = np.repeat(np.arange(n), np.diff(rp)) == ci
    v0 = v + 1.0 * diag
    rng = np.random.default_rng(5)
    rows = rng.choice(n, 16, replace=False)
    vr = v0.copy()
    for i in rows:
        vr[rp[i]:rp[i + 1]] *= rng.uniform(0.5, 1.5, rp[i + 1] - rp[i])
    cases = [("shift 1.1", v + 1.1 * diag), ("shift 2", v + 2.0 * diag), ("shift 10", v + 10.0 * diag), ("rank 16", vr)]
    s, alt = Hipmf(), Hipmf()
    for h in (s, alt):
        assert h.initialize(n, rp, ci) == 0
    assert s.factorize(v0) == 0 and alt.factorize(v0) == 0
    b = rng.standard_normal(n)
    d_x, d_b, d_v = s.dev_alloc(8 * n), s.dev_alloc(8 * n), s.dev_alloc(8 * v0.size)
    s.h2d(d_b, b)
    st = s.stats()
    out("%s: n = %d, nnz = %d, factor %.0f MB; tolerance %.0e, restart 30" % (name, n, v.size, 8e-6 * (st["nnz_l"] + st["nnz_u"]), args.tol))
    out("  %-10s %5s %9s %9s | %8s %8s %8s | %12s %10s" % ("change", "steps", "ms/call", "ms/step", "passpair", "spmv", "arnoldi", "refactor+solve", "break-even"))
    for label, v1 in cases:
        s.h2d(d_v, v1)
        res = {}

        def call():
            res["r"] = s.solve_updated_device(d_x, d_b, d_v, rel_tol=args.tol, transpose=args.transpose)
        os.environ.pop("HIPMF_UPDATED_TIMING", None)
        med, lo, hi = timed(call, args.reps, args.warmup)
        steps, relres, status = res["r"]
        plain = timed(lambda: s.solve_updated_device(d_x, d_b, d_v, rel_tol=args.tol), args.reps, args.warmup)[0] if args.transpose else None
        os.environ["HIPMF_UPDATED_TIMING"] = "1"
        parts = []
        for _ in range(3):
            call()
            parts.append([s.counter(k) / 1e3 / max(steps, 1) for k in ("updated_precond_us", "updated_spmv_us", "updated_arnoldi_us")])
        os.environ.pop("HIPMF_UPDATED_TIMING", None)
        parts = np.median(np.array(parts), axis=0)

        def alternative():
            alt.factorize_device(d_v)
            if args.transpose:
                alt.solve_transpose_device(d_x, d_b)
            else:
                alt.solve_device(d_x, d_b)
        amed, alo, ahi = timed(alternative, args.reps, args.warmup)
        per_step = med / max(steps, 1)
        out("  %-10s %5d %9.3f %9.3f | %8.3f %8.3f %8.3f | %12.3f %10.1f   (status %d, relres %.1e; call %.3f-%.3f, alternative %.3f-%.3f ms%s)" %
            (label, steps, med, per_step, parts[0], parts[1], parts[2], amed, amed / per_step, status, relres, lo, hi, alo, ahi,
             "; plain form %.3f ms/call" % plain if args.transpose else ""))
    for p in (d_x, d_b, d_v):
        s.dev_free(p)
    s.close()
    alt.close()


def run_many(name, n, rp, ci, v, args, out):
    nrhs = args.nrhs
    diag = np.repeat(np.arange(n), np.diff(rp)) == ci
    v0 = v + 1.0 * diag
    rng = np.random.default_rng(5)
    rows = rng.choice(n, 16, replace=False)
    vr = v0.copy()
    for i in rows:
        vr[rp[i]:rp[i + 1]] *= rng.uniform(0.5, 1.5, rp[i + 1] - rp[i])
    cases = [("shift 1.1", v + 1.1 * diag), ("shift 2", v + 2.0 * diag), ("shift 10", v + 10.0 * diag), ("rank 16", vr)]
    s, alt = Hipmf(), Hipmf()
    for h in (s, alt):
        assert h.initialize(n, rp, ci) == 0
    assert s.factorize(v0) == 0 and alt.factorize(v0) == 0
    B = rng.standard_normal((nrhs, n))
    d_x, d_b, d_v = s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * v0.size)
    s.h2d(d_b, B)
    st = s.stats()
    out("%s: n = %d, nnz = %d, factor %.0f MB; %d columns, tolerance %.0e, restart 30" % (name, n, v.size, 8e-6 * (st["nnz_l"] + st["nnz_u"]), nrhs, args.tol))
    out("  %-10s | %9s %9s | %9s %9s | %7s | %12s | %6s %8s | %8s %8s %8s" % ("change", "(a) ms", "(a)/N", "(b) ms", "(b)/N", "(a)/(b)", "(c) refac+slv", "pairs", "colsteps",
                                                                             "passpair", "spmv", "arnoldi"))
    for label, v1 in cases:
        s.h2d(d_v, v1)
        res = {}

        def blocked():
            res["a"] = s.solve_updated_many_device(d_x, d_b, nrhs, d_v, rel_tol=args.tol, transpose=args.transpose)

        def looped():
            res["b"] = [s.solve_updated_device(d_x + 8 * n * c, d_b + 8 * n * c, d_v, rel_tol=args.tol, transpose=args.transpose) for c in range(nrhs)]
        os.environ.pop("HIPMF_UPDATED_TIMING", None)
        a_med, a_lo, a_hi = timed(blocked, args.reps, args.warmup)
        steps, relres, status = res["a"]
        pairs, colsteps, blocks = s.counter("updated_steps"), s.counter("updated_column_steps"), s.counter("updated_blocks")
        b_med, b_lo, b_hi = timed(looped, args.reps, args.warmup)
        b_steps = [r[0] for r in res["b"]]
        os.environ["HIPMF_UPDATED_TIMING"] = "1"
        parts = []
        for _ in range(3):
            blocked()
            parts.append([s.counter(k) / 1e3 for k in ("updated_precond_us", "updated_spmv_us", "updated_arnoldi_us")])
        os.environ.pop("HIPMF_UPDATED_TIMING", None)
        parts = np.median(np.array(parts), axis=0)

        def alternative():
            alt.factorize_device(d_v)
            if args.transpose:
                alt.solve_transpose_many_device(d_x, d_b, nrhs)
            else:
                alt.solve_device(d_x, d_b, nrhs=nrhs)
        c_med, c_lo, c_hi = timed(alternative, args.reps, args.warmup)
        plain = timed(lambda: s.solve_updated_many_device(d_x, d_b, nrhs, d_v, rel_tol=args.tol), args.reps, args.warmup)[0] if args.transpose else None
        out("  %-10s | %9.3f %9.3f | %9.3f %9.3f | %7.3f | %12.3f | %6d %8d | %8.3f %8.3f %8.3f" %
            (label, a_med, a_med / nrhs, b_med, b_med / nrhs, a_med / b_med, c_med, pairs, colsteps, parts[0], parts[1], parts[2]))
        out("      status %d / %s, max relres %.1e / %.1e; %d block(s); (a) %.3f-%.3f, (b) %.3f-%.3f, (c) %.3f-%.3f ms" %
            (status, sorted(set(r[2] for r in res["b"])), float(np.max(relres)), max(r[1] for r in res["b"]), blocks, a_lo, a_hi, b_lo, b_hi, c_lo, c_hi))
        out("      steps per column (a): %s" % " ".join(str(int(k)) for k in steps))
        out("      steps per column (b): %s" % " ".join(str(int(k)) for k in b_steps))
        if plain is not None:
            out("      plain form (solve_updated_many_device) on the same inputs: %.3f ms, %.3f per column" % (plain, plain / nrhs))
    for p in (d_x, d_b, d_v):
        s.dev_free(p)
    s.close()
    alt.close()


def complex_grid(nx, ny):
    """(library, n, values(h) interleaved, two handles factorised at h = 1, L) for K(h) = (alpha + i beta) / h I + L on the nx x ny grid"""
    import scipy.sparse as sp

    from russell_amd._capi import load

    lib = load()
    alpha, beta = 2.6811, 3.0504
    T = lambda m: sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    L = sp.csr_matrix(sp.kron(sp.identity(ny), T(nx)) + sp.kron(T(ny), sp.identity(nx)))
    L.sort_indices()
    n, rp, ci = L.shape[0], L.indptr.astype(np.int32), L.indices.astype(np.int32)
    diag = np.repeat(np.arange(n), np.diff(rp)) == ci

    def values(h):  # interleaved (re, im)
        v = L.data + (alpha + 1j * beta) / h * diag
        return np.ascontiguousarray(np.stack([v.real, v.imag], axis=1).ravel())
    v0 = values(1.0)
    handles = []
    for _ in range(2):
        h = lib.complex_solver_hipmf_new()
        assert h
        assert lib.complex_solver_hipmf_initialize(h, 0, 1, -1.0, -1, 0, 0, n, rp, ci, v0.ctypes.data) == 0
        assert lib.complex_solver_hipmf_factorize(h, None, None, None, None, None, None, None, 0, 0, v0) == 0
        handles.append(h)
    return lib, n, values, handles, L


def run_complex(args, out):
    import ctypes as C

    nx = ny = 500
    lib, n, values, handles, L = complex_grid(nx, ny)
    v0 = values(1.0)
    s, alt = handles
    counter = lambda which: int(lib.complex_solver_hipmf_get_counter(s, which))
    rng = np.random.default_rng(5)
    b = np.ascontiguousarray(rng.standard_normal(2 * n))
    d_x, d_b, d_v = (lib.hipmf_device_malloc(16 * n), lib.hipmf_device_malloc(16 * n), lib.hipmf_device_malloc(8 * v0.size))
    assert d_x and d_b and d_v
    assert lib.hipmf_memcpy_h2d(d_b, b.ctypes.data_as(C.c_void_p), b.nbytes) == 0
    istats, dstats = np.zeros(16, np.int64), np.zeros(16)
    assert lib.complex_solver_hipmf_get_stats(s, istats, dstats) == 0
    out("complex shifted grid %d x %d: n = %d complex, nnz = %d complex, real-equivalent factor %.0f MB, max_front %d; tolerance %.0e, restart 30" %
        (nx, ny, n, L.nnz, 8e-6 * (istats[4] + istats[5]), istats[6], args.tol))
    out("  %-10s %5s %9s %9s | %8s %8s %8s | %14s %10s" % ("change", "steps", "ms/call", "ms/step", "passpair", "spmv", "arnoldi", "refactor+solve", "break-even"))
    xh = np.zeros(2 * n)
    for label, h1 in (("h0 -> h0/2", 0.5), ("h0 -> h0/10", 0.1)):
        v1 = values(h1)
        assert lib.hipmf_memcpy_h2d(d_v, v1.ctypes.data_as(C.c_void_p), v1.nbytes) == 0
        res = {}

        def call():
            steps, relres = C.c_int32(0), C.c_double(0.0)
            if args.transpose:
                code = lib.complex_solver_hipmf_solve_updated_transpose_device(s, d_x, d_b, d_v, 0, args.tol, 0, C.byref(steps), C.byref(relres), args.conjugate)
            else:
                code = lib.complex_solver_hipmf_solve_updated_device(s, d_x, d_b, d_v, 0, args.tol, 0, C.byref(steps), C.byref(relres))
            res["r"] = (steps.value, relres.value, code)

        def plain_call():
            steps, relres = C.c_int32(0), C.c_double(0.0)
            lib.complex_solver_hipmf_solve_updated_device(s, d_x, d_b, d_v, 0, args.tol, 0, C.byref(steps), C.byref(relres))
        os.environ.pop("HIPMF_UPDATED_TIMING", None)
        med, lo, hi = timed(call, args.reps, args.warmup)
        steps, relres, status = res["r"]
        plain = timed(plain_call, args.reps, args.warmup)[0] if args.transpose else None
        os.environ["HIPMF_UPDATED_TIMING"] = "1"
        parts = []
        for _ in range(3):
            call()
            parts.append([counter(k) / 1e3 / max(steps, 1) for k in (31, 32, 33)])  # HIPMF_COUNTER_UPDATED_PRECOND_US / _SPMV_US / _ARNOLDI_US
        os.environ.pop("HIPMF_UPDATED_TIMING", None)
        parts = np.median(np.array(parts), axis=0)

        def alternative():
            assert lib.complex_solver_hipmf_factorize_mapped(alt, None, None, None, None, 0, v1) == 0
            if args.transpose:
                assert lib.complex_solver_hipmf_solve_transpose(alt, xh, b, args.conjugate, 0) == 0
            else:
                assert lib.complex_solver_hipmf_solve(alt, xh, b, 0) == 0
        amed, alo, ahi = timed(alternative, args.reps, args.warmup)
        per_step = med / max(steps, 1)
        out("  %-10s %5d %9.3f %9.3f | %8.3f %8.3f %8.3f | %14.3f %10.1f   (status %d, relres %.1e, complex arithmetic %d; call %.3f-%.3f, alternative %.3f-%.3f ms%s)" %
            (label, steps, med, per_step, parts[0], parts[1], parts[2], amed, amed / per_step, status, relres, counter(37), lo, hi, alo, ahi,
             "; plain form %.3f ms/call" % plain if args.transpose else ""))
    for p_ in (d_x, d_b, d_v):
        lib.hipmf_device_free(p_)
    for h in handles:
        lib.complex_solver_hipmf_drop(h)


def run_complex_many(args, out):
    import ctypes as C

    nx = ny = 500
    nrhs = args.nrhs
    lib, n, values, handles, L = complex_grid(nx, ny)
    v0, v1 = values(1.0), values(0.5)
    s, alt = handles
    counter = lambda which: int(lib.complex_solver_hipmf_get_counter(s, which))
    rng = np.random.default_rng(5)
    B = np.ascontiguousarray(rng.standard_normal((nrhs, 2 * n)))  # rows: the columns, n interleaved complex numbers each
    col = 16 * n  # bytes of a column
    d_x, d_b, d_v = (lib.hipmf_device_malloc(col * nrhs), lib.hipmf_device_malloc(col * nrhs), lib.hipmf_device_malloc(8 * v0.size))
    assert d_x and d_b and d_v
    assert lib.hipmf_memcpy_h2d(d_b, B.ctypes.data_as(C.c_void_p), B.nbytes) == 0
    assert lib.hipmf_memcpy_h2d(d_v, v1.ctypes.data_as(C.c_void_p), v1.nbytes) == 0
    istats, dstats = np.zeros(16, np.int64), np.zeros(16)
    assert lib.complex_solver_hipmf_get_stats(s, istats, dstats) == 0
    out("complex shifted grid %d x %d, h0 -> h0/2: n = %d complex, nnz = %d complex, real-equivalent factor %.0f MB, max_front %d; %d columns, tolerance %.0e, restart 30" %
        (nx, ny, n, L.nnz, 8e-6 * (istats[4] + istats[5]), istats[6], nrhs, args.tol))
    res = {}
    steps, relres = np.zeros(nrhs, np.int32), np.zeros(nrhs)

    def blocked():
        if args.transpose:
            res["a"] = lib.complex_solver_hipmf_solve_updated_transpose_many_device(s, d_x, d_b, nrhs, n, d_v, 0, args.tol, 0, steps.ctypes.data, relres.ctypes.data,
                                                                                    args.conjugate)
        else:
            res["a"] = lib.complex_solver_hipmf_solve_updated_many_device(s, d_x, d_b, nrhs, n, d_v, 0, args.tol, 0, steps.ctypes.data, relres.ctypes.data)

    def looped():
        r = []
        for c in range(nrhs):
            st, rel = C.c_int32(0), C.c_double(0.0)
            if args.transpose:
                code = lib.complex_solver_hipmf_solve_updated_transpose_device(s, d_x + col * c, d_b + col * c, d_v, 0, args.tol, 0, C.byref(st), C.byref(rel),
                                                                               args.conjugate)
            else:
                code = lib.complex_solver_hipmf_solve_updated_device(s, d_x + col * c, d_b + col * c, d_v, 0, args.tol, 0, C.byref(st), C.byref(rel))
            r.append((st.value, rel.value, code))
        res["b"] = r
    os.environ.pop("HIPMF_UPDATED_TIMING", None)
    a_med, a_lo, a_hi = timed(blocked, args.reps, args.warmup)
    pairs, colsteps, blocks, basis = counter(28), counter(35), counter(34), counter(36)  # UPDATED_STEPS, _COLUMN_STEPS, _BLOCKS, _BLOCK_BASIS_BYTES
    a_steps, a_rel = steps.copy(), relres.copy()
    b_med, b_lo, b_hi = timed(looped, args.reps, args.warmup)
    os.environ["HIPMF_UPDATED_TIMING"] = "1"
    parts = []
    for _ in range(3):
        blocked()
        parts.append([counter(k) / 1e3 for k in (31, 32, 33)])  # HIPMF_COUNTER_UPDATED_PRECOND_US / _SPMV_US / _ARNOLDI_US
    os.environ.pop("HIPMF_UPDATED_TIMING", None)
    parts = np.median(np.array(parts), axis=0)
    X = np.zeros_like(B)

    def alternative():
        assert lib.complex_solver_hipmf_factorize_mapped(alt, None, None, None, None, 0, v1) == 0
        if args.transpose:
            assert lib.complex_solver_hipmf_solve_transpose_many(alt, X.reshape(-1), B.reshape(-1), nrhs, n, args.conjugate, 0) == 0
        else:
            assert lib.complex_solver_hipmf_solve_many(alt, X.reshape(-1), B.reshape(-1), nrhs, n, 0) == 0
    c_med, c_lo, c_hi = timed(alternative, args.reps, args.warmup)
    plain = None
    if args.transpose:
        plain = timed(lambda: lib.complex_solver_hipmf_solve_updated_many_device(s, d_x, d_b, nrhs, n, d_v, 0, args.tol, 0, None, None), args.reps, args.warmup)[0]
    out("  %9s %9s | %9s %9s | %9s %9s | %7s | %6s %8s | %8s %8s %8s" % ("(a) ms", "(a)/N", "(b) ms", "(b)/N", "(c) ms", "(c)/N", "(a)/(b)", "pairs", "colsteps", "passpair",
                                                                        "spmv", "arnoldi"))
    out("  %9.3f %9.3f | %9.3f %9.3f | %9.3f %9.3f | %7.3f | %6d %8d | %8.3f %8.3f %8.3f" %
        (a_med, a_med / nrhs, b_med, b_med / nrhs, c_med, c_med / nrhs, a_med / b_med, pairs, colsteps, parts[0], parts[1], parts[2]))
    out("      status %d / %s, max relres %.1e / %.1e, complex arithmetic %d; %d block(s), block bases %.0f MB; (a) %.3f-%.3f, (b) %.3f-%.3f, (c) %.3f-%.3f ms" %
        (res["a"], sorted(set(r[2] for r in res["b"])), float(np.max(a_rel)), max(r[1] for r in res["b"]), counter(37), blocks, 1e-6 * basis, a_lo, a_hi, b_lo, b_hi,
         c_lo, c_hi))
    out("      steps per column (a): %s" % " ".join(str(int(k)) for k in a_steps))
    out("      steps per column (b): %s" % " ".join(str(r[0]) for r in res["b"]))
    if plain is not None:
        out("      plain form (complex_solver_hipmf_solve_updated_many_device) on the same inputs: %.3f ms, %.3f per column" % (plain, plain / nrhs))
    for p_ in (d_x, d_b, d_v):
        lib.hipmf_device_free(p_)
    for h in handles:
        lib.complex_solver_hipmf_drop(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--complex", action="store_true", help="the complex form on the 500 x 500 complex shifted grid (see the module docstring)")
    ap.add_argument("--nrhs", type=int, default=0, help="N > 0: the block form on N columns against N single calls (see the module docstring)")
    ap.add_argument("--transpose", action="store_true", help="the transposed forms (A_new^T; complex: see --conjugate) against factorize + solve_transpose(_many)")
    ap.add_argument("--conjugate", type=int, default=1, choices=[0, 1], help="with --complex --transpose: 1 = A_new^H (default), 0 = A_new^T")
    ap.add_argument("--matrix", default="both", choices=["2d", "3d", "both"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    args = ap.parse_args()
    if args.transpose and args.out is None:
        args.out, args.append = os.path.join(ROOT, "profiles", "r17_solve_updated_transpose.txt"), True
    lines = []

    def out(line):
        print(line, flush=True)
        lines.append(line)
    if args.transpose:
        out("TRANSPOSED forms%s: the calls named below are their _transpose twins, the alternative ends in solve_transpose%s" %
            ((" (conjugate = %d)" % args.conjugate) if args.complex else "", "_many" if args.nrhs > 0 else ""))
    if args.complex and args.nrhs > 0:
        out("(a) one complex_solver_hipmf_solve_updated_many_device call, (b) %d complex_solver_hipmf_solve_updated_device calls, (c) complex_solver_hipmf_factorize_mapped + "
            "complex_solver_hipmf_solve_many(nrhs = %d), one MI355X; median of %d after %d warm-up" % (args.nrhs, args.nrhs, args.reps, args.warmup))
        run_complex_many(args, out)
    elif args.complex:
        out("complex_solver_hipmf_solve_updated_device against complex_solver_hipmf_factorize_mapped + complex_solver_hipmf_solve, one MI355X; "
            "median of %d calls after %d warm-up calls" % (args.reps, args.warmup))
        run_complex(args, out)
    elif args.nrhs > 0:
        out("(a) one solve_updated_many_device call, (b) %d solve_updated_device calls, (c) factorize_device + solve_device(nrhs = %d), one MI355X; "
            "median of %d after %d warm-up" % (args.nrhs, args.nrhs, args.reps, args.warmup))
    else:
        out("solve_updated_device against factorize_device + solve_device, one MI355X; median of %d calls after %d warm-up calls" % (args.reps, args.warmup))
    go = run_many if args.nrhs > 0 else run
    if not args.complex and args.matrix in ("2d", "both"):
        go("poisson2d 1000 x 1000 + I", *P.poisson2d(1000), args, out)
    if not args.complex and args.matrix in ("3d", "both"):
        go("poisson3d 100^3 + I", *P.poisson3d(100), args, out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
