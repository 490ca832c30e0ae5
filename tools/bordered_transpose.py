#!/usr/bin/env python3
"""solver_hipmf_solve_bordered_transpose_device on the 1M-DOF Poisson matrix: the table of profiles/r22_bordered_transpose.txt.
Needs an MI355X.

    python tools/bordered_transpose.py [--n 1000] [--ks 1,16,64] [--nrhs 1,16] [--reps 7] [--warmup 2] [--out FILE]
    python tools/bordered_transpose.py --kernels [--n 1000] [--ks 16,64]          (under a kernel-tracing profiler)

The 5-point Poisson matrix on an n x n grid in general storage (LU; the transposed pass pair and k_border_residual_nt) and as its lower
triangle (L D L^T; A^T = A: the plain pass pair and k_border_residual_n), border entries uniform in (-1, 1), B != C.  Per handle, k and
nrhs, on device-resident operands:
    ms of the FIRST solve_bordered_transpose_device after a set_border_device (it builds V = A^{-T} C: k refined transposed solves),
    ms per later call, per column and per block step (the start counts as one),
    ms per solve_bordered_device of the same columns beside it,
-- medians of host-clock times around the blocking calls, the calls ALTERNATING in one process.
For k = 1, nrhs = 1 also the loop a caller runs by hand: two solve_transpose calls on host vectors, two host inner products, one
combination -- against solve_bordered_transpose on the same host vectors.

--kernels: a few calls of both forms, 16 columns, on the general-storage handle and nothing else.  The matrix is symmetric in VALUE, so
k_border_residual_nt (columns tiled by four, rows of A^T) and k_border_residual_n (column by column, rows of A) then do the same
arithmetic on the same shape: their average durations in the profiler's kernel statistics are the comparison of the tiling."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from russell_amd import problems as P  # noqa: E402
from russell_amd.backend import Hipmf  # noqa: E402


def median_ms(calls, reps, warmup):
    """{label: median ms, min, max} of the calls, alternating"""
    times = {k: [] for k in calls}
    for rep in range(warmup + reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            if rep >= warmup:
                times[k].append(1e3 * (time.perf_counter() - t0))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in times.items()}


def device_border(s, rng, n, k):
    B, Cm, D = rng.uniform(-1, 1, (k, n)), rng.uniform(-1, 1, (k, n)), rng.uniform(-1, 1, (k, k))  # (rows = the columns of the border)
    d_B, d_C, d_D = s.dev_alloc(8 * n * k), s.dev_alloc(8 * n * k), s.dev_alloc(8 * k * k)
    s.h2d(d_B, B), s.h2d(d_C, Cm), s.h2d(d_D, np.ascontiguousarray(D.T))
    return (B, Cm, D), (d_B, d_C, d_D)


def run_handle(label, n, init, kw, values, args, out):
    s = Hipmf()
    codes = (s.initialize(*init, **kw), s.factorize(values))
    assert codes == (0, 0), "%s: initialize / factorize returned %r" % (label, codes)
    st = s.stats()
    out("%s: n = %d, factor %.0f MB, %d replaced pivots, symmetric_ldlt %d" % (label, n, 8e-6 * (st["nnz_l"] + st["nnz_u"]), st["n_perturbed"], s.counter("symmetric_ldlt")))
    rng = np.random.default_rng(22)
    for k in args.ks:
        (B, Cm, D), dev = device_border(s, rng, n, k)
        for nrhs in args.nrhs:
            F, G = rng.standard_normal((nrhs, n)), rng.standard_normal((nrhs, k))
            d_x, d_f, d_z, d_g = s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * k * nrhs), s.dev_alloc(8 * k * nrhs)
            s.h2d(d_f, F), s.h2d(d_g, G)
            first = []
            for _ in range(3):  # (every set_border drops V: the next transposed call builds it again)
                assert s.set_border_device(k, *dev)[1] == 0
                t0 = time.perf_counter()
                s.solve_bordered_transpose_device(d_x, d_z, d_f, d_g, nrhs, ldz=k)
                first.append(1e3 * (time.perf_counter() - t0))
            res = {}
            t = median_ms({"transposed": lambda: res.__setitem__("t", s.solve_bordered_transpose_device(d_x, d_z, d_f, d_g, nrhs, ldz=k)),
                           "plain": lambda: res.__setitem__("p", s.solve_bordered_device(d_x, d_z, d_f, d_g, nrhs, ldz=k))}, args.reps, args.warmup)
            info, steps, blocks = res["t"], s.counter("bordered_transposed_steps"), s.counter("bordered_transposed_blocks")
            out("  k = %2d, nrhs = %2d: first transposed call %9.3f ms (median of 3, %.3f - %.3f; %.1f MB held for V and D^T); later calls %9.3f ms/call (%.3f - %.3f), "
                "%.3f per column, %.3f per block step (%d step(s) + the start in %d block(s)); solve_bordered_device %9.3f ms/call (%.3f - %.3f, %d step(s)); "
                "steps per column %s, states %s, omega <= %.2e" %
                (k, nrhs, float(np.median(first)), min(first), max(first), 1e-6 * s.counter("border_transposed_bytes"), t["transposed"][0], t["transposed"][1],
                 t["transposed"][2], t["transposed"][0] / nrhs, t["transposed"][0] / (steps + blocks), steps, blocks, t["plain"][0], t["plain"][1], t["plain"][2],
                 s.counter("bordered_steps"), sorted(set(int(q) for q in info[:, 0])), sorted(set(int(q) for q in info[:, 3])), float(np.max(info[:, 1]))))
            if k == 1 and nrhs == 1:
                host_loop(s, B[0], Cm[0], float(D[0, 0]), F[0], float(G[0, 0]), args, out)
            for p in (d_x, d_f, d_z, d_g):
                s.dev_free(p)
        s.set_border(None, None, None)
        for p in dev:
            s.dev_free(p)
    s.close()


def host_loop(s, b, c, d, p, q, args, out):
    """the caller's own transposed bordering (two solves with A^T, two inner products, a combination) against the call, on host vectors"""
    res = {}

    def by_hand():
        y0, v = s.solve_transpose(p), s.solve_transpose(c)
        w = (q - float(b @ y0)) / (d - float(b @ v))
        res["hand"] = (y0 - w * v, w)

    pa, qa = np.ascontiguousarray(p), np.array([q])
    t = median_ms({"hand": by_hand, "call": lambda: res.__setitem__("lib", s.solve_bordered_transpose(pa, qa))}, args.reps, args.warmup)
    yh, wh = res["hand"]
    yl, wl, info = res["lib"]
    diff = max(float(np.max(np.abs(yh - yl)) / np.max(np.abs(yl))), abs(wh - wl[0]) / abs(wl[0]))
    out("    k = 1, host vectors: two solve_transpose calls + two inner products + combination %9.3f ms (%.3f - %.3f); solve_bordered_transpose %9.3f ms "
        "(%.3f - %.3f), %d step(s); the two answers differ by %.2e relative" % (t["hand"][0], t["hand"][1], t["hand"][2], t["call"][0], t["call"][1], t["call"][2],
                                                                               int(info[0]), diff))


def run_kernels(n, init, kw, values, args, out):
    s = Hipmf()
    assert (s.initialize(*init, **kw), s.factorize(values)) == (0, 0)
    rng = np.random.default_rng(22)
    nrhs = 16
    for k in args.ks:
        _, dev = device_border(s, rng, n, k)
        assert s.set_border_device(k, *dev)[1] == 0
        F, G = rng.standard_normal((nrhs, n)), rng.standard_normal((nrhs, k))
        d_x, d_f, d_z, d_g = s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * k * nrhs), s.dev_alloc(8 * k * nrhs)
        s.h2d(d_f, F), s.h2d(d_g, G)
        for _ in range(3):
            s.solve_bordered_transpose_device(d_x, d_z, d_f, d_g, nrhs, ldz=k)
            s.solve_bordered_device(d_x, d_z, d_f, d_g, nrhs, ldz=k)
        out("--kernels: k = %d, 16 columns: 3 calls of each form, %d + %d block steps and starts per call" %
            (k, s.counter("bordered_transposed_steps") + 1, s.counter("bordered_steps") + 1))
        s.set_border(None, None, None)
        for p in dev + (d_x, d_f, d_z, d_g):
            s.dev_free(p)
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000, help="edge of the Poisson grid (1000: 1M unknowns)")
    ap.add_argument("--ks", default=None)
    ap.add_argument("--nrhs", default="1,16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernels", action="store_true", help="only the calls whose residual kernels a profiler is to time")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_bordered_transpose.txt"))
    args = ap.parse_args()
    args.ks = [int(q) for q in (args.ks or ("16,64" if args.kernels else "1,16,64")).split(",") if q]
    args.nrhs = [int(q) for q in args.nrhs.split(",") if q]
    lines = []

    def out(line):
        print(line, flush=True)
        lines.append(line)

    out("tools/bordered_transpose.py --n %d --ks %s --nrhs %s --reps %d --warmup %d%s" %
        (args.n, ",".join(map(str, args.ks)), ",".join(map(str, args.nrhs)), args.reps, args.warmup, " --kernels" if args.kernels else ""))
    n, rp, ci, v = P.poisson2d(args.n, args.n)
    if args.kernels:
        run_kernels(n, (n, rp, ci), dict(values=v), v, args, out)
    else:
        run_handle("poisson %d x %d, general storage (LU)" % (args.n, args.n), n, (n, rp, ci), dict(values=v), v, args, out)
        lrp, lci, lv = P.lower_triangle(n, rp, ci, v)
        run_handle("poisson %d x %d, lower triangle (L D L^T)" % (args.n, args.n), n, (n, lrp, lci), dict(general_symmetric=True), lv, args, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
