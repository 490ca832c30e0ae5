"""tests/test_blocked_shapes_gpu.py on the CPU emulator: the explicit lists of front shapes (the device file imports them), the runners, and
the subset of the lists that keeps the CPU suite short.  (p, m) are the pivots and off-diagonal rows of the THREE leaves of
front_shapes.two_leaves_and_root, f = p + m; every value sits on an edge read from kernels_solve_transpose_blocked.hpp,
kernels_solve_pruned.hpp and kernels_solve_pruned_transpose.hpp.  The emulator runs the same kernel sources: a contraction that stops after
its first round, a tile that drops its last column or a parent that reads an unmarked child's slot fails here first, with the shape in the
test id (profiles/r23_blocked_shapes.txt lists the mutations this subset was shown to catch)."""
import pytest

import blocked_shapes as B
import front_shapes as F
from test_front_shapes_cpu import record_figures  # noqa: F401 (the fixture)

LEAVES = 3  # leaf 0 carries the sparse non-zeros, leaf 1 the selected rows, leaf 2 is left out by both pruned passes
MODES = ["lu", "weak", "ldlt"]

# k_tr_gemm_blk deals 64-row chunks of its contraction to four wavefronts (stride 256); backward it runs over rows [32 (c0 / 32), f)
CHUNK_64 = [(16, 47), (16, 48), (16, 49), (16, 239), (16, 240), (16, 241), (16, 496), (16, 497)]
# ... from a non-zero i0: the tile at c0 = 64 contracts 64 and 65 rows, the tile at c0 = 96 161 rows
NONZERO_I0 = [(65, 63), (65, 64), (97, 160)]
# forward contractions of length p (the update columns of E'; k_sp_gemm<true>: chunks of 32, stride 128)
FORWARD_P = [(31, 40), (32, 40), (33, 40), (63, 33), (64, 33), (65, 33), (127, 33), (128, 33), (129, 33), (255, 17), (256, 17), (257, 17)]
# backward pruned contraction [32 (r0 / 32), f) of k_sp_gemm<false> at 127, 128, 129
BACKWARD_PRUNED = [(16, 111), (16, 112), (16, 113)]
# a tile that straddles p, partial last tiles: p mod 16 and m mod 16 in {15, 0, 1} (the pruned row tiles restart at p)
STRADDLE = [(33, 33), (47, 50), (49, 31), (65, 15), (65, 16), (65, 17)]
# FD_DENSE_TOP: the leaves are one-workgroup fronts on the default schedule (every other big shape runs with HIPMF_MID_FRONT=0)
DENSE_TOP = [(31, 191), (32, 192)]
# one wavefront, the panel in LDS (f <= 64)
SMALL = [(1, 63), (8, 56), (9, 55), (17, 46), (33, 31), (63, 1), (64, 0)]
BULLETS = {"chunk of 64": CHUNK_64, "non-zero i0": NONZERO_I0, "forward p": FORWARD_P, "backward pruned": BACKWARD_PRUNED, "straddle": STRADDLE,
           "dense top": DENSE_TOP, "small": SMALL}
SHAPES = [s for group in BULLETS.values() for s in group]

# the fixed thirds: every bullet at least once in each; L D L^T at f = 257 and f = 513 (k_sp_gather_sym, then k_tr_gemm_blk<false>)
WEAK = [(16, 49), (16, 240), (16, 496), (65, 63), (31, 40), (64, 33), (129, 33), (255, 17), (16, 111), (33, 33), (65, 17), (31, 191), (8, 56), (17, 46), (63, 1)]
LDLT = [(16, 48), (16, 241), (16, 497), (97, 160), (33, 40), (63, 33), (128, 33), (257, 17), (16, 113), (47, 50), (65, 15), (32, 192), (9, 55), (33, 31)]
CASES = [(p, m, "lu") for p, m in SHAPES] + [(p, m, "weak") for p, m in WEAK] + [(p, m, "ldlt") for p, m in LDLT]

# a parent with marked and unmarked children: (leaf) -> (tiled middle front) -> root, the sparse non-zeros once in the big leaf and once in
# the one-pivot leaf under the root
CHAINS = ([(32, 100), (65, 64)], [(97, 31), (129, 128)])
CHAIN_CASES = [(leaf, mid, "lu") for leaf in CHAINS[0] for mid in CHAINS[1]] + [((32, 100), (97, 31), "weak"), ((65, 64), (129, 128), "ldlt")]
# complex order p, m of the three leaves, in general (weak pivot blocks) and symmetric-lower storage
COMPLEX = [(17, 15), (16, 80), (33, 31), (33, 64), (64, 1)]

CPU_CASES = [(16, 241, "lu"), (16, 241, "ldlt"), (257, 17, "lu"), (16, 113, "ldlt"), (129, 33, "weak"), (65, 17, "lu"), (31, 191, "weak"), (8, 56, "lu")]
CPU_CHAINS = [((32, 100), (97, 31), "lu")]
CPU_COMPLEX = [(17, 15, False), (33, 31, True)]


def _seed(p, m):
    return 100 * p + m


def run_two_leaves(lib, p, m, mode, log):
    weak, sym = mode == "weak", mode == "ldlt"
    if F.kind(p, m) == "small":
        # run_small's leaf count (an order above 32: smaller matrices are ONE dense front), and never fewer than three leaves
        leaves = max(LEAVES, -(-(F.DENSE_N + 1 - m) // p))
        env, tiled_only = {}, False
    else:
        leaves = LEAVES
        env, tiled_only = ({}, False) if (p, m) in DENSE_TOP else (B.TILED_ONLY, True)
    case = F.two_leaves_and_root(p, m, _seed(p, m), weak=weak, symmetric=sym, leaves=leaves)
    expect = F.expect_two_leaves(p, m, leaves, tiled_only=tiled_only)
    if F.kind(p, m) == "small":
        assert expect["max_front"] <= F.SMALL_F and expect["mid_fronts"] == 0
    if (p, m) in DENSE_TOP:
        # (the one-workgroup kernel is an LU kernel: L D L^T leaves of this shape take the tiled launches)
        expect["mid_fronts"] = 0 if sym else leaves
        assert F.kind(p, m) == "one-workgroup" and F.kind(m, 0) == "tiled"
    B.run_case(lib, case, expect, weak, env, log, "blocked p=%d m=%d %s" % (p, m, mode), [B.two_leaves_layout(p, m, leaves)])


def run_chain(lib, leaf, middle, mode, log):
    case = F.chain(leaf[0], leaf[1], middle[0], middle[1], _seed(*leaf) + middle[0], weak=mode == "weak", symmetric=mode == "ldlt")
    expect = F.expect_chain(leaf[0], leaf[1], middle[0], middle[1])
    if mode == "ldlt":
        expect["mid_fronts"] = 0  # (the one-workgroup kernel is an LU kernel)
    B.run_case(lib, case, expect, mode == "weak", {}, log, "blocked chain %s -> %s %s" % (leaf, middle, mode), B.chain_layouts(leaf[0], middle[0], middle[1]))


@pytest.mark.parametrize("p,m,mode", CPU_CASES)
def test_blocked_and_pruned_solves(emu_lib, p, m, mode, record_figures):
    run_two_leaves(emu_lib, p, m, mode, record_figures)


@pytest.mark.parametrize("leaf,middle,mode", CPU_CHAINS)
def test_chains_with_marked_and_unmarked_children(emu_lib, leaf, middle, mode, record_figures):
    run_chain(emu_lib, leaf, middle, mode, record_figures)


@pytest.mark.parametrize("p,m,symmetric", CPU_COMPLEX)
def test_complex_twin(emu_lib, p, m, symmetric, record_figures):
    B.run_complex(emu_lib, p, m, symmetric, record_figures)


def test_the_lists_cover_what_they_claim():
    f = lambda shapes: {p + m for p, m in shapes}
    assert {63, 64, 65, 255, 256, 257, 512, 513} <= f(CHUNK_64) and all(p == 16 for p, _ in CHUNK_64)
    assert {(p // 32 * 32, p + m - p // 32 * 32) for p, m in NONZERO_I0} == {(64, 64), (64, 65), (96, 161)}  # (i0 of the last tile, rows it contracts)
    assert {p for p, _ in FORWARD_P} == {31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257} and all(F.kind(p, m) != "small" for p, m in FORWARD_P)
    assert f(BACKWARD_PRUNED) == {127, 128, 129}
    assert {p % 16 for p, _ in STRADDLE} == {15, 1} and {m % 16 for _, m in STRADDLE} >= {15, 0, 1}  # (p mod 16 = 0: every p of CHUNK_64)
    assert {(p % 16, m % 16) for p, m in STRADDLE + CHUNK_64} >= {(15, 2), (1, 15), (1, 0), (1, 1), (0, 15), (0, 0), (0, 1)}
    assert all(F.kind(p, m) == "one-workgroup" for p, m in DENSE_TOP) and all(F.kind(p, m) == "small" for p, m in SMALL)
    assert all((F.kind(p, m) == "small") == ((p, m) in SMALL + CHUNK_64[:2]) for p, m in SHAPES)  # (f = 63, 64 of CHUNK_64: one wavefront too)
    assert len(set(SHAPES)) == len(SHAPES) == 41
    # the thirds: fixed, inside the list, a third of it each, every bullet in each; weak needs a pivot to interchange with
    for third in (WEAK, LDLT):
        assert set(third) <= set(SHAPES) and len(set(third)) == len(third) and 3 * len(third) >= len(SHAPES)
        assert all(set(third) & set(group) for group in BULLETS.values())
    assert all(p > 1 for p, _ in WEAK)
    assert {257, 513} <= f(LDLT)  # k_sp_gather_sym followed by k_tr_gemm_blk<false> beyond one and two rounds of the four wavefronts
    assert set(CPU_CASES) <= set(CASES) and set(CPU_CHAINS) <= set(CHAIN_CASES)
    assert {mode for _, _, mode in CHAIN_CASES} == set(MODES) and {mode for _, _, mode in CPU_CASES} == set(MODES)
    assert {(p, m) for p, m, _ in CPU_COMPLEX} <= set(COMPLEX) and {s for _, _, s in CPU_COMPLEX} == {False, True}
    assert max(LEAVES * p + m for p, m in SHAPES) <= 800  # (a GPU case: a few seconds with its longdouble reference)
    assert B.NRHS == 17 and B.counts(16) == (1, 3, 0, 2, 9, 1, 16) and B.counts(1) == (1, 3, 0, 2, 1, 1, 1)
    assert F.C == 16.0
