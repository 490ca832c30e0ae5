#!/usr/bin/env python3
"""solver_hipmf_eigs_near_shift / _device on the 1M-DOF Poisson matrix: the table of profiles/r25_eigs.txt.  Needs an MI355X.

    python tools/eigs.py [--n 1000] [--nev 1,6,16] [--sigmas 0,0.01] [--reps 5] [--warmup 1] [--tol 1e-10] [--out FILE]

The 5-point Poisson matrix K on an n x n grid, M = I and a lumped M (a diagonal uniform in (0.5, 2)); per shift the handle is
initialised from the lower triangle of A = K - sigma M and factorised (sigma = 0: L D L^T of a positive definite matrix; the interior
shift: indefinite).  Per handle, M and nev:
    ms per call on device vectors and per call on host vectors, steps, restarts, converged pairs, the largest backward error;
    the split of the device call from the HIPMF_COUNTER_EIGS_*_US counters, per step;
    the achieved TB/s of k_eig_rotate ((m + k) 8 n bytes per rotation) and of the CGS2 kernels ((4 (j + 1) + 6) 8 n bytes per step with
    j + 1 basis vectors, the SpMVs not counted) -- to hold against the 3 TB/s the solve kernels reach;
    the host-driven loop a caller writes today: scipy.sparse.linalg.eigsh(K, nev, M, sigma, OPinv = the handle's host-pointer solve), same
    tolerance, on the same handle in the same process;
    factorize and the inertia for scale.
Medians of host-clock times around the blocking calls, the calls ALTERNATING in one process.  The square grid has double eigenvalues
(lambda_ij = lambda_ji): a single-vector Lanczos returns one vector of each such pair, which changes nothing in what a step costs."""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

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


def basis_bytes(n, nev, m, steps):
    """bytes the CGS2 kernels move over the steps of a call (the restart rule of Solver::eigs_near_shift), and the rotations' bytes"""
    k = min(nev + (m - nev) // 2, m - 1)
    cgs, rot, j, restarts = 0, 0, 0, 0
    for _ in range(steps):
        cgs += (4 * (j + 1) + 6) * 8 * n
        j += 1
        if j == m:
            rot += (m + k) * 8 * n
            j, restarts = k, restarts + 1
    return cgs, rot + (max(j, nev) + nev) * 8 * n, restarts


def run_shift(n, rp, ci, kv, sigma, args, out):
    N = rp.size - 1
    rows = np.repeat(np.arange(N), np.diff(rp))
    diag = (rows == ci).astype(float)
    lumped = np.random.default_rng(25).uniform(0.5, 2.0, N)
    K = sp.csr_matrix((kv, ci, rp), shape=(N, N))
    for mname, mv in (("M = I", None), ("lumped M", diag * lumped[rows])):
        av = kv - sigma * (diag if mv is None else mv)
        lrp, lci, lav = P.lower_triangle(N, rp, ci, av)
        mlow = None if mv is None else P.lower_triangle(N, rp, ci, mv)[2]
        Mfull = None if mv is None else sp.csr_matrix((mv, ci, rp), shape=(N, N))
        s = Hipmf()
        assert s.initialize(N, lrp, lci, general_symmetric=True) == 0
        tf = median_ms({"factorize": lambda: s.factorize(lav)}, args.reps, args.warmup)["factorize"]
        st = s.stats()
        try:
            inertia = "inertia (%d, %d, %d) status %d" % s.inertia()
        except Exception as e:  # (no L D L^T plan)
            inertia = "inertia not available (%s)" % e
        ti = median_ms({"inertia": lambda: s.inertia()}, args.reps, args.warmup)["inertia"] if "status" in inertia else (0.0, 0.0, 0.0)
        out("sigma = %g, %s: factorize %.3f ms (%.3f - %.3f), %d replaced pivots, symmetric_ldlt %d, %s, %.3f ms per inertia call" %
            (sigma, mname, tf[0], tf[1], tf[2], st["n_perturbed"], s.counter("symmetric_ldlt"), inertia, ti[0]))
        d_m = None
        if mlow is not None:
            d_m = s.dev_alloc(8 * mlow.size)
            s.h2d(d_m, mlow)
        for nev in args.nev:
            d_X = s.dev_alloc(8 * N * nev)
            res = {}
            t = median_ms({"device": lambda: res.__setitem__("d", s.eigs_near_shift_device(nev, sigma, d_X, d_m, tol=args.tol)),
                           "host": lambda: res.__setitem__("h", s.eigs_near_shift(nev, sigma, mlow, tol=args.tol))}, args.reps, args.warmup)
            s.eigs_near_shift_device(nev, sigma, d_X, d_m, tol=args.tol)  # (the counters of a device call)
            lam, be, nconv, steps, status = res["d"]
            us = [s.counter(c) for c in ("eigs_solve_us", "eigs_spmv_us", "eigs_orth_us", "eigs_rotate_us")]
            m = min(N, max(2 * nev + 8, 24))
            cgs, rot, _ = basis_bytes(N, nev, m, steps)
            out("  nev = %2d (ncv %d): device vectors %9.3f ms (%.3f - %.3f), host vectors %9.3f ms (%.3f - %.3f); status %d, %d converged, %d steps, %d restarts, "
                "backward error <= %.2e, basis %.1f MB" % (nev, m, t["device"][0], t["device"][1], t["device"][2], t["host"][0], t["host"][1], t["host"][2], status, nconv,
                                                          steps, s.counter("eigs_restarts"), float(np.max(be)), 1e-6 * s.counter("eigs_basis_bytes")))
            out("      per step: solve %.3f ms, SpMV %.3f ms, CGS2 + norms %.3f ms (%.2f TB/s of the basis traffic); rotations %.3f ms in all (%.2f TB/s)" %
                (1e-3 * us[0] / steps, 1e-3 * us[1] / steps, 1e-3 * us[2] / steps, cgs / max(us[2], 1) * 1e-6, 1e-3 * us[3], rot / max(us[3], 1) * 1e-6))
            # the loop a caller writes today, on the same handle
            nsolve = [0]

            def opinv(b):
                nsolve[0] += 1
                return s.solve(b)

            def by_hand():
                nsolve[0] = 0
                res["e"] = spla.eigsh(K, k=nev, M=Mfull, sigma=sigma, which="LM", tol=args.tol, OPinv=spla.LinearOperator((N, N), matvec=opinv, dtype=float))

            th = median_ms({"eigsh": by_hand}, max(1, args.reps // 2), min(1, args.warmup))["eigsh"]
            w = np.sort(res["e"][0])
            out("      scipy eigsh with OPinv = solver_hipmf_solve: %9.3f ms (%.3f - %.3f), %d solves; eigenvalues differ by %.2e" %
                (th[0], th[1], th[2], nsolve[0], float(np.max(np.abs(w - np.sort(lam))))))
            s.dev_free(d_X)
        if d_m is not None:
            s.dev_free(d_m)
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000, help="edge of the Poisson grid (1000: 1M unknowns)")
    ap.add_argument("--nev", default="1,6,16")
    ap.add_argument("--sigmas", default="0,0.01", help="the shifts: 0 (positive definite) and one interior shift")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_eigs.txt"))
    args = ap.parse_args()
    args.nev = [int(q) for q in args.nev.split(",") if q]
    lines = []

    def out(line):
        print(line, flush=True)
        lines.append(line)

    out("tools/eigs.py --n %d --nev %s --sigmas %s --reps %d --warmup %d --tol %g" % (args.n, ",".join(map(str, args.nev)), args.sigmas, args.reps, args.warmup, args.tol))
    n, rp, ci, v = P.poisson2d(args.n, args.n)
    for sigma in (float(q) for q in args.sigmas.split(",") if q):
        run_shift(args.n, np.asarray(rp), np.asarray(ci), np.asarray(v, dtype=float), sigma, args, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
