"""tests/test_update_order_cpu.py on the device: the look-ahead pieces at the head of every trailing-update launch (HIPMF_UPD_LA_FIRST=1,
the default) against the old order on a second handle, bit for bit, and against the longdouble reference of tests/front_shapes.py."""
import pytest

import update_order as U
from test_update_order_cpu import record_figures  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_both_orders_agree_bit_for_bit(name, record_figures):
    U.run_real(None, name, record_figures)


def test_both_orders_agree_bit_for_bit_complex(record_figures):
    U.run_complex(None, record_figures)
