"""vrt_volume_smooth at resolutions 0, 1 and 2 (N = 2, 3, 5: one brick, one tile of a pass, a work box that is the whole grid), in
both formats, with and without the empty-space tables, over the field with NaN and +-0 samples that the other volume calls meet in
tests/test_volume_ops_extremes_gpu.py.  The same cases go through the host pass in tests/test_volume_smooth.py.  The kernels launch one
lane or one tile per sample without a capped grid-stride loop, so there is no path that only a 257^3 grid reaches.  Tolerance 0."""
import pytest

import extreme_cases as X
import smooth_cases as K
import volume_ref as R
from test_volume_fill_gpu import EDITED, assert_same_buffers, buffers
from test_volume_smooth_gpu import _fresh_slots  # noqa: F401 -- the autouse fixture: both slots start unused and are freed after
from test_volume_smooth_gpu import smooth_and_check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt", X.FORMATS)
@pytest.mark.parametrize("N", K.SMALL)
def test_smooth_on_the_smallest_grids(renderer, N, fmt):
    stored, material = X.small_field(N, fmt)
    written = 0
    for what, rec in K.small_cases(N):
        for table in (True, False):
            want = K.reference(stored, material, fmt, rec, ("small", N))
            written += smooth_and_check(renderer, what, stored, material, fmt, rec, want, table)["written"]  # the reference's result, a full upload
            vol = K.volume(N, table)
            assert_same_buffers(buffers(renderer, EDITED), R.device_bytes(want[0], want[1], fmt, vol.density_scale, vol.step_max),
                                f"{what} ({N}^3, format {fmt}, tables {table}) against the reference of the upload")
    assert written > 0
