"""Cost of complex_solver_hipmf_solve_with_error_analysis (options 2 and 1) against the plain complex solve on the 250 000-unknown complex
shifted 2D system (gamma + i omega) I - A of tests/test_complex_error_analysis_gpu.py (A: convection-diffusion, 500 x 500 grid, Peclet 30).
Wall-clock per call from the host (host vectors in and out, as the C-ABI takes them), median of `--reps` calls after warm-up.
Usage: python tools/complex_error_analysis.py [--reps 20] [--out profiles/complex_error_analysis_250k.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _median_ms(fn, reps):
    for _ in range(3):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "complex_error_analysis_250k.txt"))
    a = ap.parse_args()
    from test_complex_error_analysis_cpu import COUNTER_ANALYSIS_SOLVES, ZHandle, shifted_convection_diffusion

    A = shifted_convection_diffusion(500)
    n = A.shape[0]
    rng = np.random.default_rng(5)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    s = ZHandle(None, A)
    ist, _ = s.stats()
    out = {"n_complex": n, "max_front": int(ist[6])}
    out["solve_ms"] = _median_ms(lambda: s.solve(b), a.reps)
    bi, xh = np.ascontiguousarray(np.stack([b.real, b.imag], axis=1).ravel()), np.zeros(2 * n)
    out["solve_transpose_h_ms"] = _median_ms(lambda: s.lib.complex_solver_hipmf_solve_transpose(s.h, xh, bi, 1, 0), a.reps)  # (refined A^H solve)
    for opt in (2, 1):
        out["analysis_opt%d_ms" % opt] = _median_ms(lambda: s.solve_ea(b, opt), max(3, a.reps // 2))
    out["analysis_opt1_pass_pairs"] = s.counter(COUNTER_ANALYSIS_SOLVES)
    _, ea = s.solve_ea(b, 1)
    out["mumps_stats"] = [float("%.6e" % v) for v in ea]
    s.close()
    line = repr(out)
    print(line)
    with open(a.out, "w") as fh:
        fh.write("# tools/complex_error_analysis.py: medians of %d (solve) / %d (analysis) calls, ms per call\n" % (a.reps, max(3, a.reps // 2)))
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
