#!/usr/bin/env python3
"""solver_hipmf_set_border_device / solver_hipmf_solve_bordered_device on the 1M-DOF Poisson matrix: the table of
profiles/r19_bordered.txt.  Needs an MI355X.

    python tools/bordered.py [--n 1000] [--ks 1,16,64] [--nrhs 1,16] [--reps 7] [--warmup 2] [--assembled-ks 1] [--out FILE]

The 5-point Poisson matrix on an n x n grid in general storage (LU) and as its lower triangle (L D L^T; there C = B and D symmetric), border
entries uniform in (-1, 1).  Per handle, k and nrhs, on device-resident operands:
    ms per set_border_device (k refined solves in blocks of 16, the Gram product, the LU of S),
    ms per solve_bordered_device: per call, per column, and per block step (the start counts as one),
    ms per solve_device of the same columns at default refinement (the plain solve the bordered one is built on),
-- medians of host-clock times around the blocking calls, the calls ALTERNATING in one process.
For k = 1, nrhs = 1 also the loop a caller runs by hand (the bordering branch of russell_nonlin's arc-length solver): two solve calls on
host vectors, two host inner products, one combination -- against solve_bordered on the same host vectors.
For the k of --assembled-ks: initialize + factorize + solve of the assembled (n + k) matrix in general storage, once each."""
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


def run_handle(label, n, init, kw, values, symmetric, args, out):
    s = Hipmf()
    codes = (s.initialize(*init, **kw), s.factorize(values))
    assert codes == (0, 0), "%s: initialize / factorize returned %r" % (label, codes)
    st = s.stats()
    out("%s: n = %d, factor %.0f MB, %d replaced pivots, symmetric_ldlt %d" % (label, n, 8e-6 * (st["nnz_l"] + st["nnz_u"]), st["n_perturbed"], s.counter("symmetric_ldlt")))
    rng = np.random.default_rng(19)
    for k in args.ks:
        B = rng.uniform(-1, 1, (k, n))  # (rows = the columns of the border: column-major n x k)
        Cm = B if symmetric else rng.uniform(-1, 1, (k, n))
        D = rng.uniform(-1, 1, (k, k))
        D = 0.5 * (D + D.T) if symmetric else D
        d_B, d_D = s.dev_alloc(8 * n * k), s.dev_alloc(8 * k * k)
        d_C = d_B if symmetric else s.dev_alloc(8 * n * k)
        s.h2d(d_B, B), s.h2d(d_D, np.ascontiguousarray(D.T))
        if not symmetric:
            s.h2d(d_C, Cm)
        binfo = {}
        t = median_ms({"set": lambda: binfo.__setitem__("v", s.set_border_device(k, d_B, d_C, d_D))}, max(3, args.reps // 2), 1)["set"]
        info, status = binfo["v"]
        assert status == 0
        out("  k = %2d: set_border_device %9.3f ms (%.3f - %.3f; %.3f ms per border column), min / max |u_ii| of S %.3e, %.0f MB held" %
            (k, t[0], t[1], t[2], t[0] / k, info[0], 1e-6 * info[3]))
        for nrhs in args.nrhs:
            F, G = rng.standard_normal((nrhs, n)), rng.standard_normal((nrhs, k))
            d_x, d_f, d_z, d_g = s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * k * nrhs), s.dev_alloc(8 * k * nrhs)
            s.h2d(d_f, F), s.h2d(d_g, G)
            res = {}
            t = median_ms({"bordered": lambda: res.__setitem__("v", s.solve_bordered_device(d_x, d_z, d_f, d_g, nrhs, ldz=k)),
                           "plain": lambda: s.solve_device(d_x, d_f, nrhs)}, args.reps, args.warmup)
            info = res["v"]
            steps, blocks = s.counter("bordered_steps"), s.counter("bordered_blocks")
            out("    nrhs = %2d: solve_bordered_device %9.3f ms/call (%.3f - %.3f), %.3f per column, %.3f per block step (%d step(s) + the start in %d block(s)); "
                "solve_device %9.3f ms/call (%d refinement step(s)); steps per column %s, states %s, omega <= %.2e" %
                (nrhs, t["bordered"][0], t["bordered"][1], t["bordered"][2], t["bordered"][0] / nrhs, t["bordered"][0] / (steps + blocks), steps, blocks,
                 t["plain"][0], s.stats()["refinement_steps"], sorted(set(int(q) for q in info[:, 0])), sorted(set(int(q) for q in info[:, 3])), float(np.max(info[:, 1]))))
            if k == 1 and nrhs == 1:
                host_loop(s, n, B[0], Cm[0], float(D[0, 0]), F[0], float(G[0, 0]), args, out)
            for p in (d_x, d_f, d_z, d_g):
                s.dev_free(p)
        s.set_border(None, None, None)
        for p in {d_B, d_C, d_D}:
            s.dev_free(p)
    s.close()


def host_loop(s, n, b, c, d, f, g, args, out):
    """the caller's own bordering (two solves with A, two inner products, a combination) against solve_bordered, both on host vectors"""
    res = {}

    def by_hand():
        y, w = s.solve(f), s.solve(b)
        den = d - float(c @ w)
        z = (g - float(c @ y)) / den
        res["hand"] = (y - z * w, z)

    fa, ga = np.ascontiguousarray(f), np.array([g])
    t = median_ms({"hand": by_hand, "bordered": lambda: res.__setitem__("lib", s.solve_bordered(fa, ga))}, args.reps, args.warmup)
    xh, zh = res["hand"]
    xl, zl, info = res["lib"]
    diff = max(float(np.max(np.abs(xh - xl)) / np.max(np.abs(xl))), abs(zh - zl[0]) / abs(zl[0]))
    out("    k = 1, host vectors: two solve calls + two inner products + combination %9.3f ms (%.3f - %.3f); solve_bordered %9.3f ms (%.3f - %.3f), %d step(s); "
        "the two answers differ by %.2e relative" % (t["hand"][0], t["hand"][1], t["hand"][2], t["bordered"][0], t["bordered"][1], t["bordered"][2], int(info[0]), diff))


def assembled(n, rp, ci, v, k, out):
    import scipy.sparse as sp

    rng = np.random.default_rng(19)
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))
    B, Cm, D = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (k, k))
    M = sp.csr_matrix(sp.bmat([[A, sp.csr_matrix(B)], [sp.csr_matrix(Cm.T), sp.csr_matrix(D)]]))
    M.sort_indices()
    m, mrp, mci, mv = M.shape[0], M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64)
    rhs = rng.standard_normal(m)
    s = Hipmf()
    t0 = time.perf_counter()
    c0 = s.initialize(m, mrp, mci, values=mv)
    t1 = time.perf_counter()
    c1 = s.factorize(mv)
    t2 = time.perf_counter()
    assert (c0, c1) == (0, 0), (c0, c1)
    s.solve(rhs)
    ts = []
    for _ in range(5):
        t3 = time.perf_counter()
        s.solve(rhs)
        ts.append(1e3 * (time.perf_counter() - t3))
    st = s.stats()
    out("  assembled (n + %d) matrix, general storage: initialize %.1f ms, factorize %.1f ms (first), solve %.3f ms (host vectors, median of 5), factor %.0f MB, "
        "%d replaced pivots" % (k, 1e3 * (t1 - t0), 1e3 * (t2 - t1), float(np.median(ts)), 8e-6 * (st["nnz_l"] + st["nnz_u"]), st["n_perturbed"]))
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000, help="edge of the Poisson grid (1000: 1M unknowns)")
    ap.add_argument("--ks", default="1,16,64")
    ap.add_argument("--nrhs", default="1,16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--assembled-ks", default="1", help="border widths for which the assembled matrix is analysed, factorised and solved (empty: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_bordered.txt"))
    args = ap.parse_args()
    args.ks = [int(q) for q in args.ks.split(",") if q]
    args.nrhs = [int(q) for q in args.nrhs.split(",") if q]
    lines = []

    def out(line):
        print(line, flush=True)
        lines.append(line)

    out("tools/bordered.py --n %d --ks %s --nrhs %s --reps %d --warmup %d --assembled-ks %s" %
        (args.n, ",".join(map(str, args.ks)), ",".join(map(str, args.nrhs)), args.reps, args.warmup, args.assembled_ks))
    n, rp, ci, v = P.poisson2d(args.n, args.n)
    run_handle("poisson %d x %d, general storage (LU)" % (args.n, args.n), n, (n, rp, ci), dict(values=v), v, False, args, out)
    lrp, lci, lv = P.lower_triangle(n, rp, ci, v)
    run_handle("poisson %d x %d, lower triangle (L D L^T)" % (args.n, args.n), n, (n, lrp, lci), dict(general_symmetric=True), lv, True, args, out)
    for k in [int(q) for q in args.assembled_ks.split(",") if q]:
        assembled(n, rp, ci, v, k, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
