#!/usr/bin/env python3
"""complex_solver_hipmf_set_border_device / _solve_bordered_device / _solve_bordered_transpose_device on the 500 x 500 complex shifted
grid of tools/solve_updated.py --complex: the table of profiles/r24_bordered_complex.txt.  Needs an MI355X.

    python tools/bordered_complex.py [--n 500] [--ks 1,16,32] [--nrhs 1,16] [--reps 7] [--warmup 2] [--out FILE]

K = (alpha + i beta) I + L on an n x n unit-spacing grid (Radau5's complex system at h = 1), border entries uniform in (-1, 1) in real and
imaginary part, right-hand sides complex standard normal.  Per k, on device-resident operands:
    ms per set_border_device (k refined complex solves in blocks of 16, the Gram product, the complex LU of S),
    ms of the FIRST solve_bordered_transpose_device after a set_border (it builds V = A^{-H} conj(C) and the LU of D^H - B^H V),
and per nrhs, the calls ALTERNATING in one process, medians of 7 after 2 warm-ups of host-clock times around the blocking calls:
    solve_bordered_device, solve_bordered_transpose_device with conjugate = 1 (M^H) and 0 (M^T),
    complex_solver_hipmf_solve_device of the same columns at default refinement (the plain solve the bordered ones are built on).
For k = 1, nrhs = 1 also the loop a caller runs by hand -- two complex_solver_hipmf_solve calls on host vectors, two host inner products,
one combination -- against complex_solver_hipmf_solve_bordered on the same host vectors."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from russell_amd.backend import ComplexHipmf  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bordered import median_ms  # noqa: E402


def shifted_grid(nx, ny):
    """K = (alpha + i beta) I + L as tools/solve_updated.py's complex_grid builds it at h = 1"""
    import scipy.sparse as sp

    alpha, beta = 2.6811, 3.0504
    T = lambda m: sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    K = sp.csr_matrix(sp.kron(sp.identity(ny), T(nx)) + sp.kron(T(ny), sp.identity(nx)) + (alpha + 1j * beta) * sp.identity(nx * ny)).astype(np.complex128)
    K.sort_indices()
    return K


def host_loop(s, b, c, d, f, g, args, out):
    """the caller's own bordering against solve_bordered, both on host vectors"""
    res = {}

    def by_hand():
        y, w = s.solve(f), s.solve(b)
        z = (g - c @ y) / (d - c @ w)  # (C^T: the plain transpose)
        res["hand"] = (y - z * w, z)

    ga = np.array([g])
    t = median_ms({"hand": by_hand, "bordered": lambda: res.__setitem__("lib", s.solve_bordered(f, ga))}, args.reps, args.warmup)
    xh, zh = res["hand"]
    xl, zl, info = res["lib"]
    diff = max(float(np.max(np.abs(xh - xl)) / np.max(np.abs(xl))), abs(zh - zl[0]) / abs(zl[0]))
    out("    k = 1, host vectors: two solve calls + two inner products + combination %9.3f ms (%.3f - %.3f); solve_bordered %9.3f ms (%.3f - %.3f), %d step(s); "
        "the two answers differ by %.2e relative" % (t["hand"][0], t["hand"][1], t["hand"][2], t["bordered"][0], t["bordered"][1], t["bordered"][2], int(info[0]), diff))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500, help="edge of the grid (500: 250k complex unknowns)")
    ap.add_argument("--ks", default="1,16,32")
    ap.add_argument("--nrhs", default="1,16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_bordered_complex.txt"))
    args = ap.parse_args()
    args.ks = [int(q) for q in args.ks.split(",") if q]
    args.nrhs = [int(q) for q in args.nrhs.split(",") if q]
    lines = []

    def out(line):
        print(line, flush=True)
        lines.append(line)

    out("tools/bordered_complex.py --n %d --ks %s --nrhs %s --reps %d --warmup %d" % (args.n, ",".join(map(str, args.ks)), ",".join(map(str, args.nrhs)), args.reps, args.warmup))
    K = shifted_grid(args.n, args.n)
    n = K.shape[0]
    s = ComplexHipmf()
    codes = (s.initialize(n, K.indptr.astype(np.int32), K.indices.astype(np.int32), values=K.data), s.factorize(K.data))
    assert codes == (0, 0), "initialize / factorize returned %r" % (codes,)
    out("complex shifted grid %d x %d: n = %d complex, nnz = %d complex" % (args.n, args.n, n, K.nnz))
    rng = np.random.default_rng(24)
    draw = lambda *shape: rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)
    for k in args.ks:
        B, Cm, D = draw(k, n), draw(k, n), draw(k, k)  # (rows = the columns of the border: column-major n x k)
        d_B, d_C, d_D = s.dev_alloc(16 * n * k), s.dev_alloc(16 * n * k), s.dev_alloc(16 * k * k)
        s.h2d(d_B, B), s.h2d(d_C, Cm), s.h2d(d_D, np.ascontiguousarray(D.T))
        binfo, first = {}, []
        d_y, d_p = s.dev_alloc(16 * n), s.dev_alloc(16 * n)
        s.h2d(d_p, rng.standard_normal(n) + 1j * rng.standard_normal(n))

        def set_then_first():
            binfo["v"] = s.set_border_device(k, d_B, d_C, d_D)
            t0 = time.perf_counter()
            s.solve_bordered_transpose_device(d_y, None, d_p, None, 1)
            first.append(1e3 * (time.perf_counter() - t0))

        t = median_ms({"set": lambda: binfo.__setitem__("v", s.set_border_device(k, d_B, d_C, d_D))}, max(3, args.reps // 2), 1)["set"]
        for _ in range(3):
            set_then_first()
        later = median_ms({"t": lambda: s.solve_bordered_transpose_device(d_y, None, d_p, None, 1)}, 3, 0)["t"][0]
        info, status = binfo["v"]
        assert status == 0
        out("  k = %2d: set_border_device %9.3f ms (%.3f - %.3f; %.3f ms per border column), min / max |u_ii| of S %.3e, %.1f MB held; first transposed call after it "
            "%9.3f ms (a later one %.3f), %.1f MB more" % (k, t[0], t[1], t[2], t[0] / k, info[0], 1e-6 * info[4], float(np.median(first)), later,
                                                         1e-6 * s.counter("complex_border_transposed_bytes")))
        for nrhs in args.nrhs:
            F, G = rng.standard_normal((nrhs, n)) + 1j * rng.standard_normal((nrhs, n)), rng.standard_normal((nrhs, k)) + 1j * rng.standard_normal((nrhs, k))
            d_x, d_f, d_z, d_g = s.dev_alloc(16 * n * nrhs), s.dev_alloc(16 * n * nrhs), s.dev_alloc(16 * k * nrhs), s.dev_alloc(16 * k * nrhs)
            s.h2d(d_f, F), s.h2d(d_g, G)
            res = {}
            calls = {"plain": lambda: res.__setitem__("plain", s.solve_bordered_device(d_x, d_z, d_f, d_g, nrhs, ldz=k)),
                     "M^H": lambda: res.__setitem__("M^H", s.solve_bordered_transpose_device(d_x, d_z, d_f, d_g, nrhs, conjugate=True, ldz=k)),
                     "M^T": lambda: res.__setitem__("M^T", s.solve_bordered_transpose_device(d_x, d_z, d_f, d_g, nrhs, conjugate=False, ldz=k)),
                     "solve": lambda: s.lib.complex_solver_hipmf_solve_device(s.h, d_x, d_f, nrhs, n)}
            t = median_ms(calls, args.reps, args.warmup)
            out("    nrhs = %2d: solve_bordered_device %9.3f ms/call (%.3f - %.3f), M^H %9.3f (%.3f - %.3f), M^T %9.3f (%.3f - %.3f); complex_solver_hipmf_solve_device "
                "%9.3f ms/call; steps per column %s / %s / %s, states %s, omega <= %.2e" %
                (nrhs, t["plain"][0], t["plain"][1], t["plain"][2], t["M^H"][0], t["M^H"][1], t["M^H"][2], t["M^T"][0], t["M^T"][1], t["M^T"][2], t["solve"][0],
                 sorted(set(int(q) for q in res["plain"][:, 0])), sorted(set(int(q) for q in res["M^H"][:, 0])), sorted(set(int(q) for q in res["M^T"][:, 0])),
                 sorted(set(int(q) for v in res.values() for q in v[:, 3])), max(float(np.max(v[:, 1])) for v in res.values())))
            if k == 1 and nrhs == 1:
                host_loop(s, np.ascontiguousarray(B[0]), np.ascontiguousarray(Cm[0]), D[0, 0], np.ascontiguousarray(F[0]), G[0, 0], args, out)
            for p in (d_x, d_f, d_z, d_g):
                s.dev_free(p)
        s.set_border(None, None, None)
        for p in (d_B, d_C, d_D, d_y, d_p):
            s.dev_free(p)
    s.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
