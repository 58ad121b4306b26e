"""trajectories.sample_batch on a 2 GiB tensor: two trajectories of 2^27 complex64 elements with the batch bit at memory bit 4.
Here artn_born_plan(2^27).block_bits = 11: a trajectory of at least 2^27 elements is the only way to a block above 2^10, where a
thread owns two segments of a block.  Row b equals born.sample on a dense clone of slice b bit for bit."""
import pytest

import artensor_amd as A

from test_sample_batch_gpu import assert_device_case_equals_unbatched, device_case

pytestmark = pytest.mark.gpu


def test_blocks_of_2048_elements_on_2_gib():
    t, u = device_case(27, 64, 27)
    info = A.sample_batch_info(t.shape, t.stride(), [1], 64)
    assert (info["block_bits"], info["blocks_per_trajectory"], info["form"], info["fields"]) == (11, 1 << 16, "TILED", [(4, 1, 0)])
    assert_device_case_equals_unbatched(t, u)
