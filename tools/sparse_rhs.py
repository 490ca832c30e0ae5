#!/usr/bin/env python3
"""Pruned solves (solver_hipmf_solve_sparse_device / solver_hipmf_inverse_entries) against solver_hipmf_solve_device on the expanded
block: the table of profiles/r09_sparse_rhs.txt.  Needs an MI355X.

    python tools/sparse_rhs.py [--matrix 2d|3d|both] [--reps 15] [--warmup 3]

Handles are initialised with refinement_nstep = 0, so both sides run one pass pair per column.  Per matrix (the 1M-DOF 2D 5-point Poisson
matrix, the 100^3 7-point one) and case
    a  one unit column, one selected row
    b  16 unit columns in one leaf region, 16 selected rows nearby
    c  16 unit columns spread uniformly, all rows
    d  inverse_entries for 256 diagonal entries (16 blocks; spread uniformly)
the line gives the fronts the forward / backward pass visited, the share of a full pass pair's factor entries they hold and the bytes
that is, the median HIP-event time of the pruned call (dstats[8]: uploads, launches and copies of the call; HIPMF_PRUNE_MAX_SHARE=1 so
that the pruned path runs whatever its share) and of solver_hipmf_solve_device on the expanded block on the same handle, each over
--reps calls after --warmup.  Case d has no expanded twin of the same shape: its reference is 256 / 16 times the 16-column solve.

    python tools/sparse_rhs.py --transpose [...]

the table of profiles/r16_sparse_rhs_transpose.txt: cases a, b and d through A^T (solver_hipmf_solve_sparse_transpose_device,
solver_hipmf_inverse_entries_by_rows) against solver_hipmf_solve_transpose_many_device on the expanded block.  The matrices are handed
over in general form, so the transposed launches run.  The transposed dense solve keeps no HIP-event time of its own: BOTH sides of this
table are host wall-clock medians around the call (the calls return synchronised); the pruned call's own event time is printed beside it."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from russell_amd import problems as P  # noqa: E402
from russell_amd.backend import Hipmf  # noqa: E402


def median_ms(fn, s, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        fn()
        t.append(s.stats()["solve_total_ms"])
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def median_wall_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def dev(s, arr, keep):
    a = np.ascontiguousarray(arr)
    p = s.dev_alloc(max(a.nbytes, 8))
    keep.append(p)
    if a.nbytes:
        s.h2d(p, a)
    return p


def run_matrix_transposed(name, n, rp, ci, v, coords, reps, warmup, out):
    """cases a, b, d through A^T; wall-clock medians on both sides"""
    s = Hipmf()
    keep = []
    try:
        t0 = time.perf_counter()
        assert s.initialize(n, rp, ci, refinement_nstep=0) == 0
        assert s.factorize(v) == 0
        st = s.stats()
        assert s.counter("symmetric_ldlt") == 0
        out("%s, A^T: n = %d, nsuper = %d, levels = %d, max front = %d, factor (L + U entries) %.1f MB, set-up %.1f s"
            % (name, n, st["nsuper"], st["nlevels"], st["max_front"], 8.0 * (st["nnz_l"] + st["nnz_u"]) / 1e6, time.perf_counter() - t0))
        out("  case  cols  rows        fwd fronts  bwd fronts  MB visited  transposed blocks  pruned wall ms (min .. max)  [event ms]   solve_transpose_many_device wall ms (min .. max)   ratio")
        d_x, d_b = s.dev_alloc(8 * n * 16), s.dev_alloc(8 * n * 16)
        keep += [d_x, d_b]
        dense_ms = {}
        for tag, cols, sel in [("a", coords(1, "leaf"), coords(1, "leaf")), ("b", coords(16, "leaf"), coords(16, "leaf") + 1)]:
            k, nsel = cols.size, sel.size
            d_ptr, d_idx, d_val = dev(s, np.arange(k + 1, dtype=np.int32), keep), dev(s, cols.astype(np.int32), keep), dev(s, np.ones(k), keep)
            d_sel, d_out = dev(s, sel.astype(np.int32), keep), dev(s, np.zeros(nsel * k), keep)
            B = np.zeros((k, n))
            B[np.arange(k), cols] = 1.0
            s.h2d(d_b, B)
            pm = median_wall_ms(lambda: s.solve_sparse_device(d_out, nsel, k, d_ptr, d_idx, d_val, nsel, d_sel, transpose=True), reps, warmup)
            ev = s.stats()["solve_total_ms"]
            ff, bf, tb = s.counter("pruned_fwd_fronts"), s.counter("pruned_bwd_fronts"), s.counter("pruned_transposed_blocks")
            dm = median_wall_ms(lambda: s.solve_transpose_many_device(d_x, d_b, k), reps, warmup)
            dense_ms[k] = dm[0]
            X, Xs = np.zeros((k, n)), np.zeros((k, nsel))
            s.d2h(X, d_x)
            s.d2h(Xs, d_out)
            agree = np.abs(Xs - X[:, sel]).max() / np.abs(X).max()
            out("  %-4s  %4d  %-10s  %10d  %10d  %10.1f  %17d  %8.3f (%.3f .. %.3f)  [%.3f]   %8.3f (%.3f .. %.3f)   %6.2f   max |pruned - dense| / |x| = %.1e"
                % (tag, k, str(nsel), ff, bf, s.counter("pruned_bytes") / 1e6, tb, pm[0], pm[1], pm[2], ev, dm[0], dm[1], dm[2], pm[0] / dm[0], agree))
        diag = coords(min(256, n // 2), "spread").astype(np.int32)
        pm = median_wall_ms(lambda: s.inverse_entries(diag, diag, by_rows=True), max(3, reps // 3), 1)
        out("  %-4s  %4d  %-10s  %10d  %10d  %10.1f  %17d  %8.3f (%.3f .. %.3f)  [%.3f]   %8.3f (16 x the 16-column solve)   %6.2f   (fronts and MB: the last block)"
            % ("d", diag.size, "diagonal", s.counter("pruned_fwd_fronts"), s.counter("pruned_bwd_fronts"), s.counter("pruned_bytes") / 1e6, s.counter("pruned_transposed_blocks"),
               pm[0], pm[1], pm[2], s.stats()["solve_total_ms"], 16 * dense_ms[16], pm[0] / (16 * dense_ms[16])))
    finally:
        for p in keep:
            s.dev_free(p)
        s.close()


def run_matrix(name, n, rp, ci, v, coords, reps, warmup, out):
    """coords(k, region): k distinct unknowns, region 'leaf' = neighbours in one corner, 'spread' = uniformly over the grid"""
    s = Hipmf()
    keep = []
    try:
        t0 = time.perf_counter()
        assert s.initialize(n, rp, ci, refinement_nstep=0) == 0
        assert s.factorize(v) == 0
        st = s.stats()
        pf_bytes = 8.0 * (st["nnz_l"] + st["nnz_u"])
        out("%s: n = %d, nsuper = %d, levels = %d, max front = %d, factor (L + U entries) %.1f MB, set-up %.1f s"
            % (name, n, st["nsuper"], st["nlevels"], st["max_front"], pf_bytes / 1e6, time.perf_counter() - t0))
        out("  case  cols  rows        fwd fronts  bwd fronts  MB visited  pruned blocks  pruned ms (min .. max)       solve_device ms (min .. max)   ratio")
        cases = [("a", coords(1, "leaf"), coords(1, "leaf")), ("b", coords(16, "leaf"), coords(16, "leaf") + 1), ("c", coords(16, "spread"), None)]
        d_x = s.dev_alloc(8 * n * 16)
        d_b = s.dev_alloc(8 * n * 16)
        keep += [d_x, d_b]
        dense_ms = {}
        for tag, cols, sel in cases:
            k = cols.size
            ptr, val = np.arange(k + 1, dtype=np.int32), np.ones(k)
            d_ptr, d_idx, d_val = dev(s, ptr, keep), dev(s, cols.astype(np.int32), keep), dev(s, val, keep)
            nsel = n if sel is None else sel.size
            d_sel = None if sel is None else dev(s, sel.astype(np.int32), keep)
            d_out = dev(s, np.zeros(nsel * k), keep)
            B = np.zeros((k, n))
            B[np.arange(k), cols] = 1.0
            s.h2d(d_b, B)
            pm = median_ms(lambda: s.solve_sparse_device(d_out, nsel, k, d_ptr, d_idx, d_val, nsel, d_sel), s, reps, warmup)
            ff, bf, pb = s.counter("pruned_fwd_fronts"), s.counter("pruned_bwd_fronts"), s.counter("pruned_blocks")
            dm = median_ms(lambda: s.solve_device(d_x, d_b, nrhs=k), s, reps, warmup)
            dense_ms[k] = dm[0]
            X, Xs = np.zeros((k, n)), np.zeros((k, nsel))
            s.d2h(X, d_x)
            s.d2h(Xs, d_out)
            ref = X if sel is None else X[:, sel]
            agree = np.abs(Xs - ref).max() / np.abs(X).max()
            out("  %-4s  %4d  %-10s  %10d  %10d  %10.1f  %13d  %8.3f (%.3f .. %.3f)   %8.3f (%.3f .. %.3f)   %6.2f   max |pruned - dense| / |x| = %.1e"
                % (tag, k, "all" if sel is None else str(nsel), ff, bf, s.counter("pruned_bytes") / 1e6, pb, pm[0], pm[1], pm[2], dm[0], dm[1], dm[2], pm[0] / dm[0], agree))
        diag = coords(min(256, n // 2), "spread").astype(np.int32)
        pm = median_ms(lambda: s.inverse_entries(diag, diag), s, max(3, reps // 3), 1)
        out("  %-4s  %4d  %-10s  %10d  %10d  %10.1f  %13d  %8.3f (%.3f .. %.3f)   %8.3f (16 x the 16-column solve)            %6.2f   (fronts and MB: the last block)"
            % ("d", diag.size, "diagonal", s.counter("pruned_fwd_fronts"), s.counter("pruned_bwd_fronts"), s.counter("pruned_bytes") / 1e6, s.counter("pruned_blocks"), pm[0], pm[1], pm[2],
               16 * dense_ms[16], pm[0] / (16 * dense_ms[16])))
        assert s.stats()["fused_fallbacks"] == 0
    finally:
        for p in keep:
            s.dev_free(p)
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", default="both", choices=["2d", "3d", "both"])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nx2d", type=int, default=1000, help="grid edge of the 2D matrix (smaller: a rehearsal)")
    ap.add_argument("--nx3d", type=int, default=100, help="grid edge of the 3D matrix")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--transpose", action="store_true", help="cases a, b, d through A^T against solver_hipmf_solve_transpose_many_device")
    a = ap.parse_args()
    run = run_matrix_transposed if a.transpose else run_matrix
    os.environ["HIPMF_PRUNE_MAX_SHARE"] = "1"

    def out(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.matrix in ("2d", "both"):
        nx = a.nx2d
        n, rp, ci, v = P.poisson2d(nx)

        def c2(k, region):
            if region == "leaf":
                return np.array([nx * (3 + i // 4) + 5 + (i % 4) for i in range(k)])
            return np.linspace(0, n - 1, k + 2)[1:-1].astype(np.int64)

        run("2D 5-point Poisson %d x %d" % (nx, nx), n, rp, ci, v, c2, a.reps, a.warmup, out)
    if a.matrix in ("3d", "both"):
        nx = a.nx3d
        n, rp, ci, v = P.poisson3d(nx)

        def c3(k, region):
            if region == "leaf":
                return np.array([nx * nx * (3 + i // 8) + nx * (4 + (i // 4) % 2) + 5 + (i % 4) for i in range(k)])
            return np.linspace(0, n - 1, k + 2)[1:-1].astype(np.int64)

        run("3D 7-point Poisson %d^3" % nx, n, rp, ci, v, c3, a.reps, a.warmup, out)


if __name__ == "__main__":
    main()
