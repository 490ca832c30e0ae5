"""The environment knobs (russell_amd/csrc/tunables.hpp): read once per initialize() call into `requested`, kept for the life of that
analysis -- a re-analysis by a re-matching factorize included -- and started over by the next initialize(); the table's parsing rules
through the debug hook hipmf_debug_knobs.  CPU emulator."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from front_shapes import environment
from russell_amd.backend import Hipmf
from test_gpu_parity import _random_unsymmetric

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 400


@pytest.fixture(scope="module")
def system():
    # diagonal 1000 x weaker than the off-diagonals: a handle that got no values at initialize re-matches at its first factorize
    M, rng = _random_unsymmetric(N, 1e-3, 3)
    return M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.copy(), M @ rng.standard_normal(N)


def _run(lib, system, env_init, env_rest, values_at_init, refused_first=None):
    """initialize under env_init, factorize + solve under env_rest (HIPMF_PLAN_DIGEST set throughout); refused_first: an environment
    under which a first initialize of the same handle is refused.  -> (digest, solution, rematch count)"""
    rp, ci, v, b = system
    s = Hipmf(lib)
    try:
        with environment({"HIPMF_PLAN_DIGEST": "1"}):
            if refused_first is not None:
                with environment(refused_first):
                    assert s.initialize(N, rp, ci, values=v) != 0
            with environment(env_init):
                assert s.initialize(N, rp, ci, values=v if values_at_init else None) == 0
            with environment(env_rest):
                assert s.factorize(v) == 0
                x = s.solve(b)
                return s.counter("plan_digest"), x, s.counter("rematch")
    finally:
        s.close()


@pytest.fixture(scope="module")
def clean(emu_lib, system):
    for k in list(os.environ):
        assert not k.startswith("HIPMF_"), k  # (the comparisons below need a clean environment)
    return _run(emu_lib, system, {}, {}, True)


@pytest.mark.parametrize("env", [{"HIPMF_ND_LEAF": "0"}, {"HIPMF_RELAX": "1,1,1,0,0,0"}], ids=["nd_leaf", "relax"])
def test_reanalysis_keeps_the_knobs_of_initialize(emu_lib, system, clean, env):
    d_out, x_out, r_out = _run(emu_lib, system, env, {}, False)   # initialized inside, factorized (= re-analysed) outside
    d_in, x_in, r_in = _run(emu_lib, system, env, env, False)     # both inside
    d_new, x_new, r_new = _run(emu_lib, system, env, env, True)   # a fresh handle given the values at initialize
    assert (r_out, r_in, r_new) == (1, 1, 0)
    assert d_out == d_in == d_new
    assert np.array_equal(x_out, x_in) and np.array_equal(x_out, x_new)
    assert d_out != clean[0] and d_out != 0  # (else the knob would not show in the plan and the test proved nothing)


@pytest.mark.parametrize("knob", ["HIPMF_MID_FRONT", "HIPMF_TREE_SOLVE"])
def test_retried_initialize_starts_from_defaults(emu_lib, system, clean, knob):
    d_knob, x_knob, _ = _run(emu_lib, system, {knob: "0"}, {}, True)
    d, x, r = _run(emu_lib, system, {}, {}, True, refused_first={knob: "0", "HIPMF_POOL_LIMIT_GB": "0.000001"})
    assert r == 0
    if knob == "HIPMF_MID_FRONT":
        assert d == clean[0] and d_knob != clean[0]
    else:
        assert not np.array_equal(x_knob, clean[1])
    assert np.array_equal(x, clean[1])


def test_unchanged_environment_rematch_equals_fresh_handle(emu_lib, system, clean):
    d, x, r = _run(emu_lib, system, {}, {}, False)
    assert r == 1 and d == clean[0] and np.array_equal(x, clean[1])


# ---- parsing ----

def _knobs(lib):
    f = C.CDLL(lib).hipmf_debug_knobs
    f.restype, f.argtypes = C.c_int64, [C.c_char_p, C.c_int64]
    need = f(None, 0)
    buf = C.create_string_buffer(need)
    assert f(buf, need) == need
    rows = [re.fullmatch(r"(\w+)=(\S*) (initialize|per-call|per-process) (default-path|test-aid|profiling-aid|rejected)( profiles/\S+)?", line)
            for line in buf.value.decode().splitlines()]
    assert all(rows)
    names = [m.group(1) for m in rows]
    assert len(set(names)) == len(names)  # every name exactly once
    for m in rows:
        if m.group(5):
            assert os.path.exists(os.path.join(ROOT, m.group(5).strip())), m.group(0)
    return {m.group(1): m.group(2) for m in rows}, {m.group(1): m.group(3) for m in rows}


DEFAULTS = {
    "SYM_LDLT": "1", "ND_LEAF": "16", "SPLIT_PIVOTS": "4096", "DENSE_ROWS": "10", "ND_THREADS": "0", "PAR_MIN": "200000", "PAR_CHUNK": "4096",
    "RELAX": "4,16,64,0.8,0.1,0.05", "RELAX_BIG": "2048", "ARENA_REUSE": "1", "ALIGN_PANELS": "1", "MATCHING": "1", "POOL_LIMIT_GB": "0",
    "PLAN_DIGEST": "0", "PLAN_THREAD": "1", "EVENT_FENCE": "0", "FACTOR_GRAPH": "0", "BLOCK_INV": "0", "UPD_SPLIT": "0", "OVERLAP_SMALL": "1",
    "SMALL_PAIR": "0", "FACTOR_CHAIN": "0", "CHAIN_FINE": "0", "CHAIN_MAX_STEPS": "8", "CHAIN_MAX_WGS": "16384", "CHAIN_MIN_WGS": "0",
    "UPD32_MAXF": "256", "MID_FRONT": "1", "MID_MMAX": "0", "MID_LU": "1", "MID_LU_MMAX": "192", "MID_LU_SPLIT": "0", "DIAG0_MIN": "512",
    "UPD_G4": "2048", "UPD_G8": "4096", "UPD_G16": str(1 << 30), "SMALL_WIDE": "7000", "SMALL_SPLIT": "28", "UPD_LA_FIRST": "1", "UPD_XCD": "1",
    "EA_LDS": "1", "EA_LU": "1", "FUSED_SOLVE": "1", "TREE_SOLVE": "1", "WT_FRONTS": "24", "WT_KB": "64", "UP_STAGE": "32", "UP_STAGE_BWD": "48",
    "UP_STAGE_MID": "8", "UP_TOP_FRONTS": "40", "UP_PAIR_XCD": "1", "UP_MAX_GROUPS": "32", "UP_REPLICAS": "1", "TAG_SOLVE": "1", "WAVE_FRONTS": "1",
    "WAVE_FRONTS_BWD": "1", "MID_BWD_LEN4": "256", "MID_BWD_LEN5": "64", "HOST_DIRECT": "1", "SF_BIG_ROWS": "6", "SF_BIG_FRONT": "2048",
    "SF_ASM_FRONT": "2048", "SOLVE_SLAB64": "0", "SF_FWD_LEVELS": "0", "SF_TRACE": "", "BLOCKED_SLABS": "0", "LEAF_KERNELS": "1",
    "SPLIT_TASKS": "512", "SPLIT_MINLEN": "2048", "REARM_TAGS": "0", "PLAIN_BAND": "1", "BLOCK_GROUPS": "0", "BLOCK_GROUPS_BYTES": "1e+18",
    "KRYLOV": "1", "KRYLOV_RESTART": "40", "KRYLOV_TOL": "1e-13", "KRYLOV_OMEGA": "1e-13", "BLOCK_COLS": "0", "UPDATED_RESTART": "30",
    "UPDATED_TIMING": "0", "EXTRA_TIMING": "0", "TRANSPOSE_BLOCKED": "1", "PRUNE_MAX_SHARE": "0.25", "PRUNE_MIN_BYTES": "2000000000",
    "SYM_EXPAND": "1", "BCAST_SLICES": "1", "BCAST_SLICE_MIN": str(64 << 20), "COMPLEX_PAIRS": "1", "PROCESS_GATE": "1",
}
PER_CALL = {"BLOCK_COLS", "UPDATED_RESTART", "UPDATED_TIMING", "EXTRA_TIMING", "TRANSPOSE_BLOCKED", "PRUNE_MAX_SHARE", "PRUNE_MIN_BYTES", "SYM_EXPAND",
            "BCAST_SLICES", "BCAST_SLICE_MIN", "COMPLEX_PAIRS"}


@pytest.fixture
def clean_env(monkeypatch):
    for k in list(os.environ):
        if k.startswith("HIPMF_"):
            monkeypatch.delenv(k)
    return monkeypatch


def test_clean_environment_prints_every_default(emu_lib, clean_env):
    values, when = _knobs(emu_lib)
    assert values == {"HIPMF_" + k: v for k, v in DEFAULTS.items()}
    assert {k for k, w in when.items() if w == "per-call"} == {"HIPMF_" + k for k in PER_CALL}
    assert [k for k, w in when.items() if w == "per-process"] == ["HIPMF_PROCESS_GATE"]


# name -> (value given, value read): one below, inside and above each range
CLAMPS = {
    "MID_MMAX": [(-1, 0), (80, 80), (193, 192)],
    "UP_MAX_GROUPS": [(1, 2), (16, 16), (33, 32)],
    "SF_BIG_ROWS": [(-1, 0), (3, 3), (8, 7)],
    "SF_BIG_FRONT": [(64, 65), (100, 100), (1 << 20, 1 << 20)],
    "SPLIT_MINLEN": [(63, 64), (100, 100), (1 << 20, 1 << 20)],
    "KRYLOV_RESTART": [(3, 4), (10, 10), (1000, 1000)],
    "UP_STAGE": [(-8, 0), (7, 0), (23, 16), (64, 64), (72, 64)],
    "UP_STAGE_BWD": [(0, 8), (7, 8), (23, 16), (64, 64), (72, 64)],
    "UP_STAGE_MID": [(-8, 0), (7, 0), (23, 16), (32, 32), (40, 32)],
    "UPD_G4": [(64, 65), (65, 65), (300, 300)],
    "ND_LEAF": [(0, 64), (1, 1), (64, 64), (65, 64)],
}


@pytest.mark.parametrize("name", sorted(CLAMPS))
def test_clamps_of_the_custom_rows(emu_lib, clean_env, name):
    for given, read in CLAMPS[name]:
        clean_env.setenv("HIPMF_" + name, str(given))
        values, _ = _knobs(emu_lib)
        assert values["HIPMF_" + name] == str(read), (name, given)
        assert {k: v for k, v in values.items() if v != DEFAULTS[k[6:]]}.keys() <= {"HIPMF_" + name}  # (no other row moves)


def test_update_group_thresholds_are_ordered(emu_lib, clean_env):
    clean_env.setenv("HIPMF_UPD_G4", "300")
    clean_env.setenv("HIPMF_UPD_G8", "100")
    values, _ = _knobs(emu_lib)
    assert (values["HIPMF_UPD_G4"], values["HIPMF_UPD_G8"], values["HIPMF_UPD_G16"]) == ("300", "300", str(1 << 30))
    clean_env.setenv("HIPMF_UPD_G16", "64")
    assert _knobs(emu_lib)[0]["HIPMF_UPD_G16"] == "300"
    clean_env.setenv("HIPMF_UPD_G8", "500")
    values, _ = _knobs(emu_lib)
    assert (values["HIPMF_UPD_G8"], values["HIPMF_UPD_G16"]) == ("500", "500")


def test_relax_is_six_values_or_ignored(emu_lib, clean_env):
    for bad in ("1,1,1", "1,1,1,0,0", "a,b,c,d,e,f", ""):
        clean_env.setenv("HIPMF_RELAX", bad)
        assert _knobs(emu_lib)[0]["HIPMF_RELAX"] == DEFAULTS["RELAX"], bad
    clean_env.setenv("HIPMF_RELAX", "1,2,3,0.5,0.25,0")
    assert _knobs(emu_lib)[0]["HIPMF_RELAX"] == "1,2,3,0.5,0.25,0"


def test_only_the_table_reads_the_environment():
    csrc = os.path.join(ROOT, "russell_amd", "csrc")
    hits = []
    for folder, _, files in os.walk(csrc):
        for f in files:
            with open(os.path.join(folder, f), errors="replace") as fh:
                if re.search(r"\bgetenv\b", fh.read()):
                    hits.append(os.path.relpath(os.path.join(folder, f), csrc))
    assert hits == ["tunables.hpp"]
