"""The transposed bordered solve on the kept factor (solver_hipmf_solve_bordered_transpose and its _device form; kernels_border.hpp) on
the CPU emulator of the HIP kernels.  The cases, the NumPy restatement and the bounds are in tests/bordered_transpose.py;
tests/test_bordered_transpose_gpu.py repeats them on the device (the emulator takes 5 columns of the large matrix where the device
takes 17: two tiles of the residual kernel, the second ragged, in a block of their own)."""
import numpy as np
import pytest

import bordered_transpose as T
from russell_amd.backend import Hipmf
from test_device_ownership_cpu import _baseline, _live


def test_exports(emu_lib):
    """the two entry points, the three counters and their names (none of them exists on the parent commit)"""
    T.check_exports(emu_lib)


@pytest.mark.parametrize("k", T.K_SHAPES)
def test_border_widths(emu_lib, k):
    T.run_shape(emu_lib, "ulap4087", k, 1)


@pytest.mark.parametrize("nrhs", T.NRHS_SHAPES)
def test_right_hand_side_counts(emu_lib, nrhs):
    T.run_shape(emu_lib, "ulap483", 3, nrhs, variants=nrhs in (1, 17))


def test_many_columns_of_the_large_matrix(emu_lib):
    T.run_shape(emu_lib, "ulap4087", 3, 5)


def test_unsymmetric_pattern(emu_lib):
    T.run_shape(emu_lib, "upat483", 17, 5, variants=True)


@pytest.mark.parametrize("name", ["ufold1e-6", "ufold1e-10"])
@pytest.mark.parametrize("k", [1, 3, 17])
def test_near_a_fold(emu_lib, name, k):
    T.run_fold(emu_lib, name, k)


@pytest.mark.parametrize("k", [1, 17])
def test_symmetric_handle_keeps_its_factor(emu_lib, k):
    T.run_symmetric(emu_lib, k)


@pytest.mark.parametrize("name,k", [("ulap483", 3), ("upat483", 17), ("biharm300_lower", 3)])
def test_adjoint_identity_with_the_plain_form(emu_lib, name, k):
    T.run_adjoint_identity(emu_lib, name, k)


@pytest.mark.parametrize("name", ["ulap483", "biharm300_lower"])
def test_interleaving_the_two_forms_changes_no_bit(emu_lib, name):
    T.run_interleaved(emu_lib, name, 3, 5)


def test_composes_with_values_outer(emu_lib):
    T.run_sensitivity(emu_lib)


def test_life_cycle_and_status_codes(emu_lib):
    T.run_status_codes(emu_lib)


@pytest.mark.parametrize("name", ["ulap483", "biharm300_lower"])
def test_reproducible_and_without_side_effects(emu_lib, name):
    T.run_side_effects(emu_lib, name)


@pytest.mark.parametrize("name", ["ulap483", "biharm300_lower"])
def test_handle_that_used_the_transposed_form_gives_back_everything(emu_lib, name):
    """the allocation count rule of tests/test_device_ownership_cpu.py; set_border(k = 0) gives back what the border held, both sides"""
    live = _live(emu_lib)
    init, kw, values, _ = T.matrix(name)
    Pm, Qm = T.rhs_of(name, 3, 18)
    base = _baseline(live)
    s = Hipmf(emu_lib)
    assert s.initialize(*init, **kw) == 0 and s.factorize(values) == 0
    s.solve_transpose(Pm[0]), s.solve_many(Pm)
    before = live()
    assert s.set_border(*T.border_of(name, 3))[1] == 0
    y2, _, _ = s.solve_bordered_transpose(Pm[:2], Qm[:2])
    y18, _, _ = s.solve_bordered_transpose(Pm, Qm)  # (wider blocks than the 2-column call's: the block buffers are allocated again)
    assert np.allclose(y2, y18[:2], rtol=1e-12, atol=0.0) and s.counter("border_transposed_bytes") > 0
    with_border = live()
    assert with_border[0] > before[0]
    assert s.set_border(None, None, None)[1] == 0 and s.counter("border_transposed_bytes") == 0
    after = live()
    if name == "biharm300_lower":
        assert after == before  # (A^T = A: no transposed plan was built on the way)
    else:
        assert after[0] < with_border[0]  # (what stays is the transposed plan of the handle, as after solve_transpose_many)
    s.close()
    assert live() == base
