"""The factorisation and substitution kernels WITHOUT refinement, at fronts placed by hand on the edges of their tiles, on the device.

Every other accuracy assertion of the suite is made after `solve` has repaired itself (two steps of refinement, a Krylov rescue), on
whatever fronts nested dissection makes of a grid.  Here tests/front_shapes.py builds fronts of prescribed (p pivots, m off-diagonal
rows): eight pivots per block and 64 rows of the small fronts, 32 pivots / 192 rows of the one-workgroup fronts, 32-pivot steps, 128-row
strips, 32 x 32 and 64 x 64 trailing tiles, rank 64 ... 256 passes and 32 x 64 extend-add tiles of the tiled path (LU, LU with
interchanges in every diagonal tile, L D L^T), chains in which a tiled front with off-diagonal rows of its own receives a contribution
block, and the complex twin on the same edges.  Each case runs solve, solve_many (9 and 17 columns), solve_transpose on the default
schedule and on the level-set launches with refinement_nstep = 0, asserts the front kind that formed, and bounds the componentwise
backward error and the forward error, both evaluated in longdouble, by front_shapes.C times what unrefined LAPACK reaches on the same
system.  The figures of one run are in profiles/r08_front_shapes.txt; the emulator subset is tests/test_front_shapes_cpu.py."""
import pytest

from test_front_shapes_cpu import (CHAINS, COMPLEX, MODES, ONE_WORKGROUP_CASES, SMALL, TILED, WAVE_CASES, record_figures, run_beyond_lds_staging, run_chain,  # noqa: F401 (the fixture)
                                   run_complex, run_one_workgroup, run_small, run_tiled, run_wave)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["lu", "weak", "ldlt"])
@pytest.mark.parametrize("p,m", SMALL)
def test_small_fronts(p, m, mode, record_figures):
    run_small(None, p, m, mode, record_figures)


@pytest.mark.parametrize("p,m,mode", ONE_WORKGROUP_CASES)
def test_one_workgroup_fronts_and_their_limits(p, m, mode, record_figures):
    run_one_workgroup(None, p, m, mode, record_figures)


@pytest.mark.parametrize("p,m,mode", WAVE_CASES)
def test_wave_fronts_and_their_limits(p, m, mode, record_figures):
    run_wave(None, p, m, mode, record_figures)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("p,m", TILED)
def test_tiled_fronts(p, m, mode, record_figures):
    run_tiled(None, p, m, mode, record_figures)


@pytest.mark.parametrize("mode", MODES)
def test_front_of_2048_rows(mode, record_figures):
    # 1024 pivots and 1024 off-diagonal rows: the forward pass assembles the front's vector once (sf_asm_front) and takes 64-row slabs
    # (sf_big_front), the factorisation runs rank-256 passes over sixteen 128-row strips
    run_tiled(None, 1024, 1024, mode, record_figures)


@pytest.mark.parametrize("mode", MODES)
def test_front_beyond_the_lds_staging_of_the_level_set_solves(mode, record_figures):
    run_beyond_lds_staging(None, mode, record_figures)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("leaf,middle", [(c, mid) for c in CHAINS[0] for mid in CHAINS[1]])
def test_chains_into_a_tiled_front(leaf, middle, mode, record_figures):
    run_chain(None, leaf, middle, mode, record_figures)


@pytest.mark.parametrize("symmetric", [False, True], ids=["general", "symmetric-lower"])
@pytest.mark.parametrize("p,m", COMPLEX)
def test_complex_twin(p, m, symmetric, record_figures):
    run_complex(None, p, m, symmetric, record_figures)
