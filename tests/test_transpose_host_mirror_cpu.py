"""The host mirror's pieces of the transposed solves and the error analysis, on the CPU emulator: the benchmark harness
(solve_matrix_market) prints the MUMPS-style mumps_stats block when asked for error estimates / condition numbers and keeps its
output unchanged otherwise; the complex actual solver of russell_amd.sparse solves with A^T and A^H."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "russell_amd", "lib", "solve_matrix_market")
MTX = os.path.join(ROOT, "tests", "golden", "mtx")


def _run(emu_lib, *args):
    env = dict(os.environ, RUSSELL_HIPMF_LIB=emu_lib)
    p = subprocess.run([HARNESS] + list(args), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p.stdout


def _json(out):
    return json.loads(out[out.index("{"):])


def test_harness_error_analysis_flags(emu_lib):
    f = os.path.join(MTX, "bfwb62.mtx")
    plain = _json(_run(emu_lib, f))["mumps_stats"]
    assert all(v == 0.0 for v in plain.values())
    est = _json(_run(emu_lib, "-x", f))["mumps_stats"]
    assert est["inf_norm_a"] > 0.0 and est["inf_norm_x"] > 0.0 and est["condition_number1"] == 0.0
    full = _json(_run(emu_lib, "-x", "-y", f))["mumps_stats"]
    assert full["inf_norm_a"] == est["inf_norm_a"] and full["condition_number1"] >= 1.0
    assert full["normalized_delta_x"] == pytest.approx(full["backward_error_omega1"] * full["condition_number1"]
                                                       + full["backward_error_omega2"] * full["condition_number2"], rel=1e-14, abs=1e-300)


@pytest.fixture
def emu_backend(emu_lib):
    """the host mirror of russell_amd.sparse bound to the emulator library for one test"""
    from russell_amd import sparse as S
    S._L().rh_set_hipmf_library(emu_lib.encode())
    yield S
    S._L().rh_set_hipmf_library(os.path.join(ROOT, "russell_amd", "lib", "librussell_hipmf.so").encode())


def test_complex_actual_solver_transpose(emu_backend):
    S = emu_backend
    rng = np.random.default_rng(7)
    n = 40
    D = np.diag(4.0 + rng.random(n) + 1j * rng.random(n)) + (np.eye(n, k=1) * (0.5 - 1j)) + (np.eye(n, k=-3) * (0.2 + 0.7j))
    coo = S.ComplexCooMatrix(n, n, int(np.count_nonzero(D)), S.Sym.No)
    for i, j in zip(*np.nonzero(D)):
        coo.put(int(i), int(j), complex(D[i, j]))
    solver = S.ComplexLinSolver(S.Genie.Hipmf)
    solver.actual.factorize(coo)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    assert np.abs(solver.actual.solve_transpose(b) - np.linalg.solve(D.T, b)).max() < 1e-12
    assert np.abs(solver.actual.solve_transpose(b, conjugate=True) - np.linalg.solve(D.conj().T, b)).max() < 1e-12
