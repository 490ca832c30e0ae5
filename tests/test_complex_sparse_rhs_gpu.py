"""Sparse right-hand sides, selected rows and entries of the inverse for the complex handle on the MI355X: the cases of
tests/test_complex_sparse_rhs_cpu.py through the product build (its run_* functions with lib = None)."""
import pytest

import test_complex_sparse_rhs_cpu as Z
from test_sparse_rhs_cpu import _prune_always

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["ref5", "grid", "symlower"])
def test_accuracy_for_every_trans(monkeypatch, name):
    _prune_always(monkeypatch)
    Z.run_accuracy(None, name)


@pytest.mark.parametrize("name", ["grid", "symlower"])
def test_selection_is_bitwise_the_rows_of_the_full_result(monkeypatch, name):
    _prune_always(monkeypatch)
    Z.run_selection(None, name)


def test_inverse_entries(monkeypatch):
    _prune_always(monkeypatch)
    Z.run_inverse_entries(None, "grid")


def test_plain_real_equivalent_factor(monkeypatch):
    _prune_always(monkeypatch)
    Z.run_accuracy(None, "grid", env={"HIPMF_COMPLEX_PAIRS": "0"})


def test_perturbed_factor_falls_back(monkeypatch):
    _prune_always(monkeypatch)
    Z.run_perturbed(None)


def test_unchanged_state(monkeypatch):
    _prune_always(monkeypatch)
    Z.run_unchanged_state(None, "grid")


def test_status_codes():
    Z.run_status_codes(None)
