#!/usr/bin/env python3
"""solver_hipmf_values_outer_device / solver_hipmf_solve_adjoint_device on the 1M-DOF Poisson matrix: the table of
profiles/r21_sensitivity.txt.  Needs an MI355X.

    python tools/sensitivity.py [--n 1000] [--nrhs 1,16] [--reps 9] [--warmup 2] [--out FILE]

The 5-point Poisson matrix on an n x n grid in general storage, device-resident operands.  Per column count:
    the outer kernel alone (HIPMF_COUNTER_SENS_OUTER_US: HIP events around it), beta = 0 and beta = 1, and its share of the HBM rate for
        the algorithmic bytes of DESIGN.md section 16 -- per stored entry 4 (column index) + 8 (result) + 8 with beta != 0, plus 8 per
        entry and column for the gathers of w -- and for the compulsory ones, where u and w are read from HBM once (16 n per column);
        both against the measured device-to-device copy rate (hipmf_device_copy_bandwidth) and the 8 TB/s of the data sheet;
    the same call through a value map (one triplet per entry, in a random order): outer + scatter, the scatter by difference;
    the symmetric-lower handle's outer kernel (two products per off-diagonal entry);
    solve_adjoint_device (lambda and the gradient) against solve_transpose_many_device alone, host clock around the blocking calls,
        medians of calls ALTERNATING in one process;
    the caller's way today: lambda and x to the host, the gather over the pattern in NumPy, the gradient back to the device."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from russell_amd import problems as P  # noqa: E402
from russell_amd.backend import Hipmf  # noqa: E402


def median_of(fn, reps, warmup, read=None):
    """median, min, max of read() (None: the host clock, in ms) over reps calls of fn"""
    v = []
    for rep in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        t = 1e3 * (time.perf_counter() - t0) if read is None else read()
        if rep >= warmup:
            v.append(t)
    return float(np.median(v)), float(np.min(v)), float(np.max(v))


def alternating(calls, reps, warmup):
    times = {k: [] for k in calls}
    for rep in range(warmup + reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            if rep >= warmup:
                times[k].append(1e3 * (time.perf_counter() - t0))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000, help="edge of the Poisson grid (1000: 1M unknowns)")
    ap.add_argument("--nrhs", default="1,16")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_sensitivity.txt"))
    args = ap.parse_args()
    counts = [int(q) for q in args.nrhs.split(",") if q]
    lines = []

    def out(line):
        print(line, flush=True)
        lines.append(line)

    out("tools/sensitivity.py --n %d --nrhs %s --reps %d --warmup %d" % (args.n, ",".join(map(str, counts)), args.reps, args.warmup))
    n, rp, ci, v = P.poisson2d(args.n, args.n)
    nnz = int(rp[n])
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    s = Hipmf()
    assert (s.initialize(n, rp, ci, values=v), s.factorize(v)) == (0, 0)
    bw = C.c_double(0.0)
    assert s.lib.hipmf_device_copy_bandwidth(1 << 30, 5, C.byref(bw)) == 0
    copy_rate = 1e9 * bw.value
    out("poisson %d x %d, general storage: n = %d, nnz = %d; measured device-to-device copy rate %.2f TB/s (read + written bytes)" % (args.n, args.n, n, nnz, 1e-12 * copy_rate))
    rng = np.random.default_rng(21)
    perm = rng.permutation(nnz).astype(np.int32)  # CSR entry k reads the triplet perm[k]
    assert s.set_value_map(np.arange(nnz + 1, dtype=np.int32), perm) == 0
    us = lambda: 1e-3 * s.counter("sens_outer_us")  # ms
    for nrhs in counts:
        X, G = rng.standard_normal((nrhs, n)), rng.standard_normal((nrhs, n))
        d_x, d_g, d_lam, d_grad = s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * nnz)
        s.h2d(d_x, X), s.h2d(d_g, G), s.h2d(d_grad, np.zeros(nnz))
        s.solve_transpose_many_device(d_lam, d_g, nrhs)
        for beta in (0.0, 1.0):
            t = median_of(lambda: s.values_outer_device(d_grad, d_lam, d_x, nrhs, alpha=-1.0, beta=beta), args.reps, args.warmup, us)
            stream = nnz * (4 + 8 + (8 if beta else 0))
            algorithmic, compulsory = stream + 8 * nnz * nrhs, stream + 16 * n * nrhs
            out("  nrhs = %2d, beta = %d: outer kernel %8.4f ms (%.4f - %.4f); algorithmic bytes %.1f MB: %.2f TB/s = %.0f %% of the copy rate, %.0f %% of 8 TB/s; "
                "compulsory bytes %.1f MB: %.2f TB/s = %.0f %% of the copy rate (the row array adds %.1f MB to either)" %
                (nrhs, int(beta), t[0], t[1], t[2], 1e-6 * algorithmic, 1e-9 * algorithmic / t[0], 100 * 1e3 * algorithmic / t[0] / copy_rate, 100 * 1e3 * algorithmic / t[0] / 8e12,
                 1e-6 * compulsory, 1e-9 * compulsory / t[0], 100 * 1e3 * compulsory / t[0] / copy_rate, 4e-6 * nnz))
            if beta == 0.0:
                plain = t[0]
        t = median_of(lambda: s.values_outer_device(d_grad, d_lam, d_x, nrhs, alpha=-1.0, mapped=True), args.reps, args.warmup, us)
        out("  nrhs = %2d, through a value map of %d triplets: outer + scatter %8.4f ms (%.4f - %.4f): the scatter %.4f ms (reads 8 + 4 + 4, writes 8 bytes per triplet: %.2f TB/s)" %
            (nrhs, nnz, t[0], t[1], t[2], t[0] - plain, 1e-9 * 24 * nnz / max(t[0] - plain, 1e-9)))
        t = alternating({"adjoint": lambda: s.solve_adjoint_device(d_lam, d_grad, d_x, d_g, nrhs),
                         "transpose": lambda: s.solve_transpose_many_device(d_lam, d_g, nrhs),
                         "outer": lambda: s.values_outer_device(d_grad, d_lam, d_x, nrhs, alpha=-1.0)}, args.reps, args.warmup)
        out("  nrhs = %2d: solve_adjoint_device %8.3f ms/call (%.3f - %.3f); solve_transpose_many_device alone %8.3f ms/call (%.3f - %.3f); values_outer_device as a call of its own %.3f ms "
            "(host clock, blocking calls)" % (nrhs, t["adjoint"][0], t["adjoint"][1], t["adjoint"][2], t["transpose"][0], t["transpose"][1], t["transpose"][2], t["outer"][0]))
        # the caller's way today: two vectors to the host, the gather in NumPy, the gradient back
        lam_h, x_h, grad_h = np.zeros((nrhs, n)), np.zeros((nrhs, n)), np.zeros(nnz)
        parts = {"d2h": [], "gather": [], "h2d": []}
        for rep in range(args.warmup + max(3, args.reps // 3)):
            t0 = time.perf_counter()
            s.d2h(lam_h, d_lam), s.d2h(x_h, d_x)
            t1 = time.perf_counter()
            grad_h[:] = 0.0
            for c in range(nrhs):
                grad_h -= lam_h[c][rows] * x_h[c][ci]
            t2 = time.perf_counter()
            s.h2d(d_grad, grad_h)
            t3 = time.perf_counter()
            if rep >= args.warmup:
                parts["d2h"].append(1e3 * (t1 - t0)), parts["gather"].append(1e3 * (t2 - t1)), parts["h2d"].append(1e3 * (t3 - t2))
        m = {k: float(np.median(q)) for k, q in parts.items()}
        lib_grad = np.zeros(nnz)
        s.values_outer_device(d_grad, d_lam, d_x, nrhs, alpha=-1.0)
        s.d2h(lib_grad, d_grad)
        out("  nrhs = %2d, by hand: lambda and x to the host %.3f ms, NumPy gather over %d entries %.3f ms, gradient to the device %.3f ms: %.3f ms in all; "
            "largest difference to the library's gradient %.2e relative" % (nrhs, m["d2h"], nnz, m["gather"], m["h2d"], sum(m.values()),
                                                                           float(np.max(np.abs(lib_grad - grad_h)) / np.max(np.abs(grad_h)))))
        for p in (d_x, d_g, d_lam, d_grad):
            s.dev_free(p)
    s.close()
    lrp, lci, lv = P.lower_triangle(n, rp, ci, v)
    s = Hipmf()
    assert s.initialize(n, lrp, lci, general_symmetric=True) == 0
    us = lambda: 1e-3 * s.counter("sens_outer_us")
    nl = int(lrp[n])
    for nrhs in counts:
        d_u, d_w, d_grad = s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * nl)
        s.h2d(d_u, rng.standard_normal((nrhs, n))), s.h2d(d_w, rng.standard_normal((nrhs, n)))
        t = median_of(lambda: s.values_outer_device(d_grad, d_u, d_w, nrhs), args.reps, args.warmup, us)
        out("poisson %d x %d, lower triangle (%d stored entries), nrhs = %2d, beta = 0: outer kernel %8.4f ms (%.4f - %.4f)" % (args.n, args.n, nl, nrhs, t[0], t[1], t[2]))
        for p in (d_u, d_w, d_grad):
            s.dev_free(p)
    s.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
