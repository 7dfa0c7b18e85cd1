"""The body of tests/test_obs_map_sizes.py on the device: observations at map sizes that are no multiple of 4 (the column-by-column
store arm of maps 2-4 and its guard), float32 and bf16, against the oracle."""
import pytest

import test_obs_map_sizes as body
from sides import VecSide

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("obs_dtype", body.DTYPES)
@pytest.mark.parametrize("G", body.MAP_SIZES)
def test_unaligned_map_rows_match_oracle(G, obs_dtype):
    body.unaligned_map_rows_match_oracle(VecSide, G, obs_dtype)
