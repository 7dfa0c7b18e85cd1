"""The body of tests/test_launch_order.py on the device: the launch order of a step call against numpy's stable sort and the work figure
of its keys against the estimate's formula in float64, at batch sizes that select every instantiation of the sort kernel (1, 1, 2, 4 and
8 keys per thread of its 1 024)."""
import pytest

import test_launch_order as body
from sides import VecSide

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", body.GPU_B)
def test_launch_order_is_pinned(B):
    body.launch_order_is_pinned(VecSide, B)
