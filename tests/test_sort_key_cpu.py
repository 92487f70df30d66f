"""drm_sam_sort_key, the key of a SAM line under DRM_SAM_SORT=coordinate, and drm_sort_order's empty case, which touches
no device: the key is strictly increasing in (tid, pos, reverse) taken lexicographically, range ends included; tid -1
(RNAME "*") gives 2^64 - 1, above every other key; anything outside 0 <= tid < 2^29, 0 <= pos < 2^33 is refused."""
import itertools

import numpy as np
import pytest

from deepreadmapper_amd import DrmError, sam_sort_key, sort_order, sort_order_workspace, sort_scan_tiles, sort_tile
from deepreadmapper_amd._native import DRM_ERR_ARG, DRM_ERR_UNSUPPORTED

TIDS = [0, 1, 2, 24, 25, 2 ** 28, 2 ** 29 - 2, 2 ** 29 - 1]
POSITIONS = [0, 1, 2, 255, 256, 49_999_999, 2 ** 31, 2 ** 32, 2 ** 33 - 2, 2 ** 33 - 1]


def test_the_key_is_strictly_increasing_in_tid_pos_reverse():
    grid = list(itertools.product(TIDS, POSITIONS, (0, 1)))
    assert grid == sorted(grid)
    keys = [sam_sort_key(*g) for g in grid]
    assert all(a < b for a, b in zip(keys, keys[1:]))
    for (tid, pos, rev), k in zip(grid, keys):
        assert k == (((tid << 33) | pos) << 1) | rev
    assert sam_sort_key(0, 1, 0) == 2 and sam_sort_key(0, 1, 1) == 3
    assert sam_sort_key(2, 100, 1) == ((2 * 2 ** 33 + 100) << 1) + 1
    assert sam_sort_key(0, 1, 16) == 3  # flag & 16 as it is


def test_the_unmapped_key_is_above_every_other():
    top = sam_sort_key(-1, 0, 0)
    assert top == 2 ** 64 - 1 == sam_sort_key(-1, 12345, 1)
    assert sam_sort_key(2 ** 29 - 1, 2 ** 33 - 1, 1) == 2 ** 63 - 1 < top


@pytest.mark.parametrize("tid,pos", [(2 ** 29, 0), (0, 2 ** 33), (0, -1), (-2, 0), (5, 2 ** 40), (2 ** 40, 5)])
def test_out_of_range_is_refused(tid, pos):
    with pytest.raises(DrmError) as e:
        sam_sort_key(tid, pos, 0)
    assert e.value.code == DRM_ERR_ARG


def test_an_empty_sort_needs_no_device():
    out = sort_order(np.zeros(0, dtype=np.uint64))
    assert out.dtype == np.uint32 and out.shape == (0,)
    assert sort_order_workspace(0) == 0
    with pytest.raises(DrmError) as e:
        sort_order_workspace(2 ** 31)
    assert e.value.code == DRM_ERR_UNSUPPORTED
    # about 20 bytes per key and 1 KiB per tile
    n = 10 * sort_tile() + 1
    assert 20 * n <= sort_order_workspace(n) <= 20 * n + 1024 * 11 + 16 * 1024
    assert sort_tile() % 64 == 0 and sort_scan_tiles() >= 1
