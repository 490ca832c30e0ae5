"""tests/test_front_shapes_gpu.py on the CPU emulator: the explicit lists of front shapes (the device file imports them), the runners, and
the subset of the lists that keeps the CPU suite short.  The emulator runs the same kernel sources, so a tile that drops its last row, a
partial 32-pivot step that skips a pivot or a slab whose dot product stops early fails here first, with the shape in the test id
(profiles/r08_front_shapes.txt lists the mutations this subset was shown to catch)."""
import ctypes as C
import os

import numpy as np
import pytest

import front_shapes as F
from russell_amd._capi import load
from russell_amd.backend import Hipmf

TILED_ONLY = {"HIPMF_MID_FRONT": "0"}
MODES = ["lu", "weak", "ldlt"]  # LU, LU with an interchange in every pivot search, L D L^T on the lower triangle

# p + m <= 64 (k_small_factor: eight pivots per block, the whole front in LDS)
SMALL = [(p, m) for p in (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64) for m in sorted({0, 1, 64 - p - 1, 64 - p}) if m >= 0 and p + m <= 64]
# k_front_lu takes p <= 32 and m <= 192: both sides of both limits
ONE_WORKGROUP = [(p, m) for p in (1, 31, 32, 33) for m in (191, 192, 193)]
# thinned cross product of p in 33 ... 257 and m in 0 ... 257: every p and every m at least three times, all nine classes (p mod 32, m mod 32)
TILED = [(33, 33), (33, 127), (33, 256), (63, 33), (63, 128), (63, 256), (64, 63), (64, 128), (64, 256), (65, 1), (65, 63), (65, 128), (65, 257),
         (95, 1), (95, 63), (95, 129), (95, 257), (96, 0), (96, 1), (96, 64), (96, 129), (96, 257), (97, 0), (97, 31), (97, 64), (97, 129), (127, 0),
         (127, 31), (127, 64), (127, 193), (128, 31), (128, 65), (128, 193), (129, 32), (129, 65), (129, 193), (255, 32), (255, 65), (255, 255),
         (256, 32), (256, 127), (256, 255), (257, 33), (257, 127), (257, 255)]
# (leaf: small, one-workgroup, tiled) x (tiled middle front at three edge sizes)
CHAINS = ([(8, 40), (32, 100), (65, 64)], [(64, 65), (97, 31), (129, 128)])
# complex order p, m: real-equivalent pivot blocks of 32, 34, 64, 66, 128, 130
COMPLEX = [(16, 16), (17, 15), (16, 80), (17, 96), (32, 32), (33, 31), (32, 96), (33, 64), (64, 64), (65, 63), (64, 1), (65, 0)]

# 48 leaves on one level (more than the 40 tiled fronts a TOP level may hold): below the top levels the solves give fronts of at most
# 128 rows and 32 pivots to one wavefront each (sf_fwd_wave / sf_bwd_wave); both sides of the row limit, the pivot limit, a small root
WAVE_LEAVES = 48
WAVE = [(1, 127), (1, 128), (8, 60), (16, 100), (32, 96), (32, 97), (33, 64)]
WAVE_CASES = [(p, m, mode) for p, m in WAVE for mode in MODES if not (mode == "weak" and p == 1)]
CPU_WAVE = [(1, 128, "lu"), (16, 100, "ldlt"), (32, 96, "weak")]

CPU_SMALL = [(1, 0, "lu"), (1, 63, "lu"), (7, 57, "weak"), (8, 56, "ldlt"), (9, 0, "weak"), (9, 55, "lu"), (17, 46, "weak"), (33, 31, "ldlt"), (63, 1, "weak"),
             (64, 0, "lu")]
ONE_WORKGROUP_CASES = [(p, m, mode) for p, m in ONE_WORKGROUP for mode in ("lu", "weak") if not (mode == "weak" and p == 1)]
CPU_ONE_WORKGROUP = [(1, 192, "lu"), (31, 191, "weak"), (32, 192, "weak"), (32, 193, "lu"), (33, 191, "weak")]
CPU_TILED = [(33, 33, "weak"), (63, 33, "ldlt"), (64, 63, "lu"), (65, 1, "weak"), (65, 63, "ldlt"), (95, 1, "lu"), (96, 0, "weak"), (96, 64, "ldlt"),
             (97, 31, "lu"), (97, 129, "weak"), (127, 64, "lu"), (128, 31, "ldlt"), (129, 65, "weak"), (129, 32, "lu")]
CPU_CHAINS = [((8, 40), (64, 65), "lu"), ((32, 100), (97, 31), "weak"), ((65, 64), (129, 128), "ldlt"), ((65, 64), (64, 65), "weak")]
CPU_COMPLEX = [(17, 15, False), (33, 31, True), (33, 64, False), (64, 1, True)]


@pytest.fixture
def record_figures():
    """the lines a case logs (shape asked for and reached, omega, omega_lapack, fe, fe_lapack): printed, and appended to the file
    HIPMF_FRONT_SHAPES_LOG names -- that is how profiles/r08_front_shapes.txt was written"""
    log = []
    yield log
    print("\n".join(log))
    if os.environ.get("HIPMF_FRONT_SHAPES_LOG"):
        with open(os.environ["HIPMF_FRONT_SHAPES_LOG"], "a") as fh:
            fh.write("\n".join(log) + "\n")


def _seed(p, m):
    return 100 * p + m


def run_small(lib, p, m, mode, log):
    if mode == "weak" and p == 1:
        mode = "lu"  # (one pivot: nothing to interchange)
    leaves = max(2, -(-(F.DENSE_N + 1 - m) // p))  # enough leaves for an order above 32: smaller matrices are ONE dense front
    case = F.two_leaves_and_root(p, m, _seed(p, m), weak=mode == "weak", symmetric=mode == "ldlt", leaves=leaves)
    expect = F.expect_two_leaves(p, m, leaves)
    assert expect["max_front"] <= F.SMALL_F and expect["mid_fronts"] == 0
    F.run_case(lib, case, expect, mode == "weak", {}, log, "small p=%d m=%d %s" % (p, m, mode))


def run_one_workgroup(lib, p, m, mode, log):
    assert not (mode == "weak" and p == 1)  # (one pivot: nothing to interchange; the lists carry no such case)
    case = F.two_leaves_and_root(p, m, _seed(p, m), weak=mode == "weak")
    expect = F.expect_two_leaves(p, m)
    assert expect["mid_fronts"] == (2 if p <= 32 and m <= 192 else 0)  # p = 33 or m = 193: the tiled launches, by default
    F.run_case(lib, case, expect, mode == "weak", {}, log, "one-workgroup p=%d m=%d %s" % (p, m, mode))


def run_tiled(lib, p, m, mode, log, columns=(9, 17)):
    assert F.kind(p, m) != "small"
    case = F.two_leaves_and_root(p, m, _seed(p, m), weak=mode == "weak", symmetric=mode == "ldlt")
    F.run_case(lib, case, F.expect_two_leaves(p, m, tiled_only=True), mode == "weak", TILED_ONLY, log, "tiled p=%d m=%d %s" % (p, m, mode), columns)


def run_wave(lib, p, m, mode, log):
    case = F.two_leaves_and_root(p, m, _seed(p, m) + 7, weak=mode == "weak", symmetric=mode == "ldlt", leaves=WAVE_LEAVES,
                                 coupling=np.sqrt(2.0 / WAVE_LEAVES))
    expect = F.expect_two_leaves(p, m, WAVE_LEAVES)
    if mode == "ldlt":
        expect["mid_fronts"] = 0  # (the one-workgroup kernel is an LU kernel)
    expect["wave_fronts"] = WAVE_LEAVES if F.SMALL_F < p + m <= 128 and p <= 32 else 0
    F.run_case(lib, case, expect, mode == "weak", {}, log, "wave p=%d m=%d x%d %s" % (p, m, WAVE_LEAVES, mode))


BEYOND_LDS = 7968  # rows of ONE dense front: more than the 7 936 doubles the level-set solve kernels stage in LDS


def run_beyond_lds_staging(lib, mode, log):
    """one dense front of 7 968 rows (no leaves beside it, no root above it); above 4 096 pivots the analysis splits it into a chain of
    two links of 4 000 and 3 968 pivots, the first with all 7 968 rows.  The level-set handle then has no LDS-staged path: the
    dependency-driven kernels, one launch per level."""
    case = F.two_leaves_and_root(BEYOND_LDS, 0, _seed(BEYOND_LDS, 0), weak=mode == "weak", symmetric=mode == "ldlt", leaves=1)
    expect = {"nsuper": 2, "max_front": BEYOND_LDS, "max_pivots": 4000, "mid_fronts": 0}
    assert expect["max_front"] > 7936
    columns = (9, 17) if mode == "lu" else (9,)  # (the longdouble reference of a 7 968 x 7 968 matrix costs 4 s per right-hand side)
    F.run_case(lib, case, expect, mode == "weak", TILED_ONLY, log, "beyond LDS staging p=%d m=0 %s" % (BEYOND_LDS, mode), columns)


def run_chain(lib, leaf, middle, mode, log):
    case = F.chain(leaf[0], leaf[1], middle[0], middle[1], _seed(*leaf) + middle[0], weak=mode == "weak", symmetric=mode == "ldlt")
    expect = F.expect_chain(leaf[0], leaf[1], middle[0], middle[1])
    if mode == "ldlt":
        expect["mid_fronts"] = 0  # (the one-workgroup kernel is an LU kernel)
    F.run_case(lib, case, expect, mode == "weak", {}, log, "chain %s -> %s %s" % (leaf, middle, mode))


def run_complex(lib_path, p, m, symmetric, log):
    """complex_solver_hipmf_*: solve and (unconjugated) transposed solve without refinement against the complex longdouble reference,
    the determinant against slogdet; weak pivot blocks in general storage (paired pivot searches with interchanges)"""
    Z, rp, ci, zv = F.complex_two_leaves_and_root(p, m, _seed(p, m), weak=not symmetric, symmetric=symmetric)
    n = Z.shape[0]
    name = "complex p=%d m=%d %s" % (p, m, "symmetric-lower" if symmetric else "general")
    lib = load(lib_path)
    rng = np.random.default_rng(5)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    ref, ref_t = F.ComplexReference(Z), F.ComplexReference(Z.T.copy())
    inter = lambda z: np.ascontiguousarray(np.stack([z.real, z.imag], axis=1).ravel())
    want = F.expect_two_leaves(2 * p, 2 * m)  # the real-equivalent fronts: twice the complex pivots and rows
    sign, logabs = np.linalg.slogdet(Z)
    for schedule, extra in (("default", {}), ("level-set", {"HIPMF_FUSED_SOLVE": "0"})):
        h = lib.complex_solver_hipmf_new()
        assert h
        try:
            with F.environment(dict({"HIPMF_MATCHING": "0"}, **extra)):  # (matching: see front_shapes.run_case)
                assert lib.complex_solver_hipmf_initialize(h, F.ORDERING_NONE, 1, -1.0, 0, 0, int(symmetric), n, rp, ci, None) == 0
            npert, rc, dre, dim, dex = C.c_int32(), C.c_double(), C.c_double(), C.c_double(), C.c_double()
            assert lib.complex_solver_hipmf_factorize(h, None, None, C.byref(npert), C.byref(rc), C.byref(dre), C.byref(dim), C.byref(dex), 1, 0, zv) == 0
            assert npert.value == 0
            ist, dst = np.zeros(16, np.int64), np.zeros(16)
            assert lib.complex_solver_hipmf_get_stats(h, ist, dst) == 0
            counter = lambda k: int(lib.complex_solver_hipmf_get_counter(h, Hipmf.COUNTERS[k]))
            got = {"nsuper": int(ist[2]), "max_front": int(ist[6]), "max_pivots": int(ist[7]), "mid_fronts": counter("mid_fronts")}
            if schedule == "default":
                log.append("%-44s n %d asked %s reached %s" % (name, n, want, got))
            # (symmetric-lower complex storage is mirrored to general storage: the paired pivot searches are LU searches)
            assert got == want and counter("rematch") == 0 and counter("symmetric_ldlt") == 0, (name, got, want)
            mant = complex(dre.value, dim.value)
            assert abs(np.log10(abs(mant)) + dex.value - logabs / np.log(10.0)) < 1e-9 and abs(mant / abs(mant) - sign) < 1e-9
            x = np.zeros(2 * n)
            tag = "%s [%s]" % (name, schedule)
            assert lib.complex_solver_hipmf_solve(h, x, inter(b), 0) == 0
            ref.check(x[0::2] + 1j * x[1::2], b, tag + " solve", log)
            assert lib.complex_solver_hipmf_solve_transpose(h, x, inter(b), 0, 0) == 0
            ref_t.check(x[0::2] + 1j * x[1::2], b, tag + " transpose", log)
            assert int(ist[10]) == 0 and counter("krylov_iterations") == 0
        finally:
            lib.complex_solver_hipmf_drop(h)


@pytest.mark.parametrize("p,m,mode", CPU_SMALL)
def test_small_fronts(emu_lib, p, m, mode, record_figures):
    run_small(emu_lib, p, m, mode, record_figures)


@pytest.mark.parametrize("p,m,mode", CPU_ONE_WORKGROUP)
def test_one_workgroup_fronts_and_their_limits(emu_lib, p, m, mode, record_figures):
    run_one_workgroup(emu_lib, p, m, mode, record_figures)


@pytest.mark.parametrize("p,m,mode", CPU_TILED)
def test_tiled_fronts(emu_lib, p, m, mode, record_figures):
    run_tiled(emu_lib, p, m, mode, record_figures)


@pytest.mark.parametrize("p,m,mode", CPU_WAVE)
def test_wave_fronts_and_their_limits(emu_lib, p, m, mode, record_figures):
    run_wave(emu_lib, p, m, mode, record_figures)


@pytest.mark.parametrize("leaf,middle,mode", CPU_CHAINS)
def test_chains_into_a_tiled_front(emu_lib, leaf, middle, mode, record_figures):
    run_chain(emu_lib, leaf, middle, mode, record_figures)


@pytest.mark.parametrize("p,m,symmetric", CPU_COMPLEX)
def test_complex_twin(emu_lib, p, m, symmetric, record_figures):
    run_complex(emu_lib, p, m, symmetric, record_figures)


def test_the_lists_cover_what_they_claim():
    from collections import Counter
    assert min(Counter(p for p, _ in TILED).values()) >= 3 and min(Counter(m for _, m in TILED).values()) >= 3
    assert {p for p, _ in TILED} == {33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 255, 256, 257}
    assert {m for _, m in TILED} == {0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193, 255, 256, 257}
    assert {(p % 32, m % 32) for p, m in TILED} >= {(a, b) for a in (31, 0, 1) for b in (31, 0, 1)}
    assert all(F.kind(p, m) != "small" for p, m in TILED)
    assert {(p, m, mode) for p, m, mode in CPU_TILED} <= {(p, m, mode) for p, m in TILED for mode in MODES}
    assert {(p, m) for p, m, _ in CPU_SMALL} <= set(SMALL) and {(p, m) for p, m, _ in CPU_ONE_WORKGROUP} <= set(ONE_WORKGROUP)
    assert set(CPU_WAVE) <= set(WAVE_CASES)
    assert {(p, m) for p, m, _ in CPU_COMPLEX} <= set(COMPLEX) and {2 * p for p, _ in COMPLEX} == {32, 34, 64, 66, 128, 130}
    assert F.C in (1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0)
