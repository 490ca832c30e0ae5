"""Blocked transposed solves on the complex handle on the MI355X: the cases of tests/test_complex_transpose_many_cpu.py through the product
build (its run_* functions with lib = None and its bounds)."""
import pytest

import test_complex_transpose_many_cpu as U

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["ref5", "zchain257", "grid"])
def test_against_single_and_numpy(name):
    U.run_against_single_and_numpy(None, name)


def test_column_loop(monkeypatch):
    U.run_column_loop(None, monkeypatch)


def test_status_codes():
    U.run_status_codes(None)


def test_host_mirror():
    U.run_host_mirror(None)
