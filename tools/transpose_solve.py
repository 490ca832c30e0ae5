"""Transposed pass pair (solver_hipmf_solve_transpose_device, unrefined) beside the ordinary default pass pair and the level-set pass pair
(HIPMF_FUSED_SOLVE=0) of the same matrix, and the cost of solver_hipmf_solve_with_error_analysis (options 1 and 2) against a plain solve.
Wall-clock per call on the device (each call ends with a stream synchronisation), median of `--reps` calls after warm-up.
Usage: python tools/transpose_solve.py [--reps 20] [--out profiles/r07_transpose_solve.txt]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _cases():
    from russell_amd import problems as P
    return {"c2_convection_diffusion_1000": lambda: P.convection_diffusion2d(1000), "c2_poisson_1000": lambda: P.poisson2d(1000, 1000),
            "poisson3d_100": lambda: P.poisson3d(100)}


def _median_ms(fn, reps):
    for _ in range(3):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def run_case(name, reps):
    """one process per (case, path): HIPMF_FUSED_SOLVE is read at initialize"""
    from russell_amd.backend import Hipmf
    n, rp, ci, v = _cases()[name]()
    s = Hipmf()
    assert s.initialize(n, rp, ci, values=v, refinement_nstep=0) == 0
    assert s.factorize(v) == 0
    b = np.random.default_rng(1).standard_normal(n)
    d_b, d_x = s.dev_alloc(8 * n), s.dev_alloc(8 * n)
    s.h2d(d_b, b)
    out = {"n": n, "max_front": s.stats()["max_front"]}
    out["ordinary_ms"] = _median_ms(lambda: s.solve_device(d_x, d_b), reps)
    out["transposed_ms"] = _median_ms(lambda: s.solve_transpose_device(d_x, d_b), reps)
    if os.environ.get("HIPMF_FUSED_SOLVE") != "0":
        s2 = Hipmf()
        assert s2.initialize(n, rp, ci, values=v) == 0  # (default refinement: the analysed solve is the user's solve)
        assert s2.factorize(v) == 0
        out["solve_host_ms"] = _median_ms(lambda: s2.solve(b), reps)
        for opt in (2, 1):
            out["analysis_opt%d_ms" % opt] = _median_ms(lambda: s2.solve_with_error_analysis(b, opt), max(3, reps // 4))
        out["analysis_opt1_pass_pairs"] = s2.counter("analysis_solves")
        s2.close()
    s.dev_free(d_b), s.dev_free(d_x)
    s.close()
    print(repr(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_transpose_solve.txt"))
    ap.add_argument("--case")
    a = ap.parse_args()
    if a.case:
        return run_case(a.case, a.reps)
    lines = ["# tools/transpose_solve.py: medians of %d calls, ms per call (unrefined device solves: perm in + pass pair + perm out)" % a.reps]

    def write(complete):
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines + ([] if complete else ["# INCOMPLETE: the run stopped at the first failed step (nothing started after it)"])) + "\n")

    # Each (case, path) is a process of its own; the first one that fails -- nonzero status, a signal, a time-out -- ends the tool:
    # nothing more is started on the GPU after it.
    for name in _cases():
        for env in ({}, {"HIPMF_FUSED_SOLVE": "0"}):
            e = dict(os.environ, **env)
            tag = "level-set" if env else "default"
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps)], env=e, capture_output=True,
                                   text=True, timeout=900)
            except subprocess.TimeoutExpired:
                lines.append("%s [%s path] timed out after 900 s" % (name, tag))
                print(lines[-1], flush=True)
                write(False)
                sys.exit(1)
            lines.append("%s [%s path] rc=%d %s" % (name, tag, r.returncode, r.stdout.strip().splitlines()[-1] if r.stdout.strip() else r.stderr[-400:]))
            print(lines[-1], flush=True)
            if r.returncode != 0:
                write(False)
                sys.exit(1)
    write(True)

if __name__ == "__main__":
    main()
