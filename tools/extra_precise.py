#!/usr/bin/env python3
"""solver_hipmf_solve_extra_precise_device against solver_hipmf_solve_device at default refinement on the same handle: the table of
profiles/r18_extra_precise.txt.  Needs an MI355X.

    python tools/extra_precise.py [--n 1000] [--nrhs 1] [--shift-grid 301] [--reps 9] [--warmup 2] [--out FILE]

Two matrices, general storage (LU): the 5-point Poisson matrix on an n x n grid (1M unknowns by default, well conditioned) and the
unit-spacing 5-point Laplacian on a g x (g - 2) grid minus (lambda + 1e-10) I, lambda the eigenvalue at 200 / 483 of the
spectrum (closed form): the shift1e-10 matrix of tests/extra_precise.py at a larger grid, cond_2 about 4e10.  Per matrix, on device-resident vectors (nrhs random columns):
    ms per call of solve_device (default refinement: the parent commit's solve) and of solve_extra_precise_device, without and with a tail
    -- medians of host-clock times around the blocking calls, the calls ALTERNATING in one process --,
    ms per step of the extra-precise call and its split into the doubled residual, the correction pass pair and the update launch (HIP
    events inside the driver, HIPMF_EXTRA_TIMING=1, in calls of their own),
    the step counts, states and bounds of the columns.
Then the errors of x + tail of the tailed cases of tests/extra_precise.py (exact residual in rational arithmetic) on this device."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from russell_amd import problems as P  # noqa: E402
from russell_amd.backend import Hipmf  # noqa: E402


def shifted_laplacian(nx, ny, delta):
    import scipy.sparse as sp

    T = lambda m: sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    lx = 2.0 - 2.0 * np.cos(np.pi * np.arange(1, nx + 1) / (nx + 1))
    ly = 2.0 - 2.0 * np.cos(np.pi * np.arange(1, ny + 1) / (ny + 1))
    lam = np.sort(np.add.outer(lx, ly).ravel())
    k = (200 * lam.size) // 483  # (the place of lambda_200 in the spectrum of the 23 x 21 grid of the tests; the median, 4, would cancel the diagonal)
    shift = lam[k] + delta
    gap = float(np.min(np.abs(lam - shift)))
    A = sp.csr_matrix(sp.kron(sp.identity(ny), T(nx)) + sp.kron(T(ny), sp.identity(nx)) - shift * sp.identity(nx * ny))
    A.sort_indices()
    return A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64), float(np.max(np.abs(lam - shift))) / gap


def run(name, n, rp, ci, v, note, args, out):
    nrhs = args.nrhs
    s = Hipmf()
    codes = (s.initialize(n, rp, ci, values=v), s.factorize(v))
    assert codes == (0, 0), "%s: initialize / factorize returned %r" % (name, codes)
    rng = np.random.default_rng(18)
    B = rng.standard_normal((nrhs, n))
    d_x, d_t, d_b = s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * n * nrhs), s.dev_alloc(8 * n * nrhs)
    s.h2d(d_b, B)
    st = s.stats()
    out("%s: n = %d, nnz = %d, factor %.0f MB, %d replaced pivots, %d column(s)%s" % (name, n, v.size, 8e-6 * (st["nnz_l"] + st["nnz_u"]), st["n_perturbed"], nrhs, note))
    res = {}
    calls = {
        "solve_device (default refinement)": lambda: s.solve_device(d_x, d_b, nrhs),
        "extra_precise_device": lambda: res.__setitem__("plain", s.solve_extra_precise_device(d_x, None, d_b, nrhs)),
        "extra_precise_device + tail": lambda: res.__setitem__("tail", s.solve_extra_precise_device(d_x, d_t, d_b, nrhs, dx_tol=1e-24)),
    }
    os.environ.pop("HIPMF_EXTRA_TIMING", None)
    times = {k: [] for k in calls}
    for rep in range(args.warmup + args.reps):
        for k, fn in calls.items():  # (alternating: every round runs each call once)
            t0 = time.perf_counter()
            fn()
            if rep >= args.warmup:
                times[k].append(1e3 * (time.perf_counter() - t0))
    for k in calls:
        out("  %-36s %9.3f ms/call (median of %d; %.3f - %.3f)" % (k, np.median(times[k]), args.reps, np.min(times[k]), np.max(times[k])))
    os.environ["HIPMF_EXTRA_TIMING"] = "1"
    for label, key, tail in (("extra_precise_device", "plain", None), ("extra_precise_device + tail", "tail", d_t)):
        parts = []
        for _ in range(3):
            s.solve_extra_precise_device(d_x, tail, d_b, nrhs, dx_tol=1e-24 if tail else 0.0)
            steps = max(s.counter("extra_precise_steps"), 1)
            parts.append([s.counter(c) / 1e3 / steps for c in ("extra_precise_residual_us", "extra_precise_precond_us", "extra_precise_update_us")])
        parts = np.median(np.array(parts), axis=0)
        info, status = res[key]
        out("  %-36s %d block step(s) in %d block(s), status %d; per block step: residual %.3f, pass pair %.3f, update %.3f ms (sum %.3f; call / steps %.3f)" %
            (label, s.counter("extra_precise_steps"), s.counter("extra_precise_blocks"), status, parts[0], parts[1], parts[2], parts.sum(),
             np.median(times[label]) / steps))
        out("    steps per column %s, states %s" % (sorted(set(int(q) for q in info[:, 0])), sorted(set(int(q) for q in info[:, 6]))))
        out("    dn %.3e, normwise bound %.3e, dc %.3e, componentwise bound %.3e, rho_max %.3e (column 0)" % tuple(info[0][[1, 2, 3, 4, 5]]))
    os.environ.pop("HIPMF_EXTRA_TIMING", None)
    out("    refinement steps of solve_device: %d, omega-based; counters after: fused_fallbacks %d" % (s.stats()["refinement_steps"], s.counter("fused_fallbacks")))
    for p in (d_x, d_t, d_b):
        s.dev_free(p)
    s.close()


def tail_errors(out):
    import extra_precise as X

    out("errors of x + tail (dx_tol 1e-24), exact residual in rational arithmetic, the cases of tests/extra_precise.py on this device:")
    for name in X.TAILED:
        out("  %-16s normwise %.3e" % (name, X.run_tail(None, name)))
    out("  %-16s normwise %.3e (moduli of the complex components)" % ("complex", X.run_complex(None)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000, help="edge of the Poisson grid (1000: 1M unknowns)")
    ap.add_argument("--nrhs", type=int, default=1)
    ap.add_argument("--shift-grid", type=int, default=301, help="g: the shifted Laplacian lives on a g x (g - 2) grid")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_extra_precise.txt"))
    args = ap.parse_args()
    lines = []

    def out(line):
        print(line, flush=True)
        lines.append(line)

    out("tools/extra_precise.py --n %d --nrhs %d --shift-grid %d --reps %d --warmup %d" % (args.n, args.nrhs, args.shift_grid, args.reps, args.warmup))
    n, rp, ci, v = P.poisson2d(args.n, args.n)
    run("poisson %d x %d" % (args.n, args.n), n, rp, ci, v, "", args, out)
    g = args.shift_grid
    n, rp, ci, v, cond2 = shifted_laplacian(g, g - 2, 1e-10)
    run("shift1e-10 on %d x %d" % (g, g - 2), n, rp, ci, v, ", cond_2 %.2e (closed form)" % cond2, args, out)
    tail_errors(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
