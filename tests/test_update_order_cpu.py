"""The order of the workgroups of a trailing-update launch (HIPMF_UPD_LA_FIRST) on the CPU emulator: the cases of tests/update_order.py
on two handles that differ in the knob alone, bit for bit, and the default order against the longdouble reference.  The emulator runs
the same kernel sources and the same host plan, so a look-ahead piece mapped to the wrong slot, a tile that lost its place behind the
look-ahead pieces or a prefix search that is off by nfollow fails here first.  tests/test_update_order_gpu.py repeats them on the device."""
import numpy as np
import pytest

import front_shapes as F
import update_order as U


@pytest.fixture
def record_figures():
    log = []
    yield log
    print("\n".join(log))


def test_the_cases_are_what_they_claim():
    look = {name: U.nfollow_per_step(c[0]) for name, c in U.CASES.items()}
    assert look["a-three-leaves"] == [3, 1, 0] and look["b-six-leaves"] == [6, 2, 0] and look["c-seventy-leaves"] == [70, 0]
    assert look["d-three-kinds"] == [2, 1, 0] and look["e-xcd-order"] == [2, 1, 0]
    largest = {name: max(c[0]) + c[1] for name, c in U.CASES.items()}
    assert largest["a-three-leaves"] <= 256 and largest["b-six-leaves"] <= 256 and largest["c-seventy-leaves"] <= 256  # 32 x 32 tiles
    assert largest["d-three-kinds"] > 256 and largest["e-xcd-order"] > 256                                              # 64 x 64 tiles
    assert len(U.CASES["a-three-leaves"][0]) <= 4 < len(U.CASES["b-six-leaves"][0]) <= 64 < len(U.CASES["c-seventy-leaves"][0])
    assert 2550 <= U.build("c-seventy-leaves")[0].n <= 2650
    # e: tiles per dimension of the full step k0 = 32 (base = 64: [64, f) in tiles of 64, plus one for the 64 rows of E')
    assert [-(-(p + 420 - 64) // 64) + 1 for p in U.CASES["e-xcd-order"][0]] == [9, 8]


@pytest.mark.parametrize("name", sorted(U.CASES) + sorted(U.CASES_CPU_ONLY))
def test_the_reference_itself_is_inside_the_margin(name):
    # numpy alone: the unrefined LAPACK solve against the longdouble solution, on the scale every assertion below is made on
    case, _, _ = U.build(name)
    b = np.random.default_rng(5).standard_normal(case.n)
    ref = F.Reference(case.A)
    x_ref, om_l, fe_l = ref.prepare(b)
    assert om_l <= F.C * F.EPS and fe_l <= F.C * F.EPS * ref.cond, (name, om_l, fe_l, ref.cond)
    ref.check(np.linalg.solve(case.A, b), b, name + " numpy")


def test_the_complex_reference_itself_is_inside_the_margin():
    p, m = U.COMPLEX
    Z, _, _, _ = F.complex_two_leaves_and_root(p, m, 100 * p + m, weak=True, symmetric=False)
    rng = np.random.default_rng(5)
    b = rng.standard_normal(Z.shape[0]) + 1j * rng.standard_normal(Z.shape[0])
    ref = F.ComplexReference(Z)
    _, om_l, fe_l = ref.prepare(b)
    assert om_l <= F.C * F.EPS and fe_l <= F.C * F.EPS * ref.cond, (om_l, fe_l, ref.cond)


@pytest.mark.parametrize("name", sorted(U.CASES) + sorted(U.CASES_CPU_ONLY))
def test_both_orders_agree_bit_for_bit(emu_lib, name, record_figures):
    U.run_real(emu_lib, name, record_figures)


def test_both_orders_agree_bit_for_bit_complex(emu_lib, record_figures):
    U.run_complex(emu_lib, record_figures)
