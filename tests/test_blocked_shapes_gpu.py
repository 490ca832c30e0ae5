"""The substitution kernels that carry sixteen right-hand sides through a front, WITHOUT refinement, at fronts placed by hand on the edges of
their tiles, on the device.

tests/test_front_shapes_gpu.py does this for solve, solve_transpose and solve_many.  Here the blocked transposed solves
(solve_transpose_many, host and device form), the pruned pass pairs for sparse right-hand sides (solve_sparse with A and A^T, a row selection,
inverse_entries by columns and by rows), a stale workspace, and the complex handle's solve_many, solve_transpose_many and solve_sparse run on
every entry of the lists of tests/test_blocked_shapes_cpu.py: 64-row chunks dealt to four wavefronts at f = 63 ... 513, contractions that
start at a non-zero row, 32-wide chunks at p = 31 ... 257, tiles of sixteen that straddle the pivots, FD_DENSE_TOP leaves, one-wavefront
fronts, chains with marked and unmarked children.  tests/blocked_shapes.py runs a case: every column against the longdouble reference,
bounded by front_shapes.C times what unrefined LAPACK reaches, the counters that show the path ran.  The figures of one run are in
profiles/r23_blocked_shapes.txt."""
import pytest

import blocked_shapes as B
from test_blocked_shapes_cpu import CASES, CHAIN_CASES, COMPLEX, record_figures, run_chain, run_two_leaves  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("p,m,mode", CASES)
def test_blocked_and_pruned_solves(p, m, mode, record_figures):
    run_two_leaves(None, p, m, mode, record_figures)


@pytest.mark.parametrize("leaf,middle,mode", CHAIN_CASES)
def test_chains_with_marked_and_unmarked_children(leaf, middle, mode, record_figures):
    run_chain(None, leaf, middle, mode, record_figures)


@pytest.mark.parametrize("symmetric", [False, True], ids=["general", "symmetric-lower"])
@pytest.mark.parametrize("p,m", COMPLEX)
def test_complex_twin(p, m, symmetric, record_figures):
    B.run_complex(None, p, m, symmetric, record_figures)
