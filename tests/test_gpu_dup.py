"""GPU tests of the first-seen duplicate set (drm_dupset, csrc/dup_set.hip): every first[] equals the plain restatement
(tests/dup_ref.py) exactly -- on small tables filled to capacity whose seeds tests/test_dup_ref_cpu.py proves to chain
and to wrap, with every item sharing one key, with half the keys repeated and the run cut three ways, for swapped mates,
single ends and keyless items, and around the calls the set refuses."""
import ctypes as C

import numpy as np
import pytest

import dup_ref as D

pytestmark = pytest.mark.gpu

N = 4096


@pytest.fixture(scope="module")
def half():
    """4,096 items, about half repeating an earlier key, and the reference's answers; shared and left unchanged."""
    ends = D.half_repeated(17, N)
    want = D.FirstSeen(N).mark(ends)
    dup = (want >= 0) & (want != np.arange(N))
    assert 0.35 * N < dup.sum() < 0.65 * N
    ends.setflags(write=False)
    want.setflags(write=False)
    return ends, want


@pytest.mark.parametrize("max_items", sorted(D.SMALL_SEEDS))
def test_small_tables_filled_to_capacity(max_items):
    from deepreadmapper_amd import DupSet
    ends = D.distinct_ends(D.SMALL_SEEDS[max_items], max_items)
    s = DupSet(max_items)
    assert s.info() == dict(max_items=max_items, slots=D.slots_for(max_items), next_item=0)
    assert np.array_equal(s.mark(ends), np.arange(max_items))
    assert s.info()["next_item"] == max_items
    s.free()
    # the same keys once more behind themselves, in two calls: everybody's first is the first copy
    s = DupSet(2 * max_items)
    assert np.array_equal(s.mark(ends), np.arange(max_items))
    assert np.array_equal(s.mark(ends[::-1, ::-1]), np.arange(max_items)[::-1])
    s.free()


def test_all_items_share_one_key():
    from deepreadmapper_amd import DupSet
    ends = np.tile(np.array([[D.end_word(1000, 0), D.end_word(1250, 1)]], dtype=np.uint64), (N, 1))
    ends[1::2] = ends[1::2, ::-1]  # every other pair with its mates swapped
    s = DupSet(N)
    assert np.array_equal(s.mark(ends), np.zeros(N, np.int64))
    s.free()


def test_half_repeated_one_call_seven_calls_and_device(half):
    from deepreadmapper_amd import DupSet
    from deepreadmapper_amd.device import DeviceBuffer, synchronize
    ends, want = half
    s = DupSet(N)
    one = s.mark(ends)
    s.free()
    s, parts, lo = DupSet(N), [], 0
    for hi in (1, 2, 65, 66, 1000, 3333, N):  # 7 uneven calls
        parts.append(s.mark(ends[lo:hi]))
        assert s.info()["next_item"] == hi
        lo = hi
    s.free()
    s, dev, lo = DupSet(N), [], 0
    d_ends = DeviceBuffer.from_host(ends)
    for hi in (1500, N):
        d_first = s.mark_device(d_ends.ptr + 16 * lo, hi - lo, first_item=lo)
        synchronize()
        dev.append(d_first.download())
        lo = hi
    s.free()
    assert np.array_equal(one, want)
    assert np.array_equal(np.concatenate(parts), want)
    assert np.array_equal(np.concatenate(dev), want)


def test_swapped_mates_single_ends_and_keyless_items():
    from deepreadmapper_amd import DupSet
    a, b, c = D.end_word(500, 0), D.end_word(780, 1), D.end_word(500, 1)
    ends = np.array([(a, b), (b, a), (a, 0), (0, a), (0, 0), (0, 0), (b, 0), (a, b), (c, b), (a, a), (a, 0)],
                    dtype=np.uint64)
    want = D.FirstSeen(16).mark(ends)
    assert list(want) == [0, 0, 2, 2, -1, -1, 6, 0, 8, 9, 2]
    s = DupSet(16)
    assert np.array_equal(s.mark(ends), want)
    # (0, 0) left the set unchanged: a call of keyless items only, then every key again
    assert list(s.mark(np.zeros((2, 2), np.uint64))) == [-1, -1]
    assert s.info()["next_item"] == 13
    assert np.array_equal(s.mark(ends[:3]), want[:3])
    s.free()


def test_refused_calls_leave_the_set_as_it_was(half):
    from deepreadmapper_amd import DrmError, DupSet
    from deepreadmapper_amd._native import DRM_ERR_ARG, lib
    ends, want = half
    ref, s = D.FirstSeen(300), DupSet(300)
    assert np.array_equal(s.mark(ends[:100]), ref.mark(ends[:100]))
    for first_item, n in ((99, 10), (0, 1), (100, 201), (299, 2), (300, 1)):  # below next_item; past max_items
        with pytest.raises(DrmError) as e:
            s.mark(ends[100:100 + n], first_item=first_item)
        assert e.value.code == DRM_ERR_ARG
        assert s.info()["next_item"] == 100
    first = np.zeros(4, np.int64)
    assert lib().drm_dupset_mark(s.handle, None, 4, 100, first.ctypes.data) == DRM_ERR_ARG
    assert lib().drm_dupset_mark(s.handle, ends[:4].ctypes.data, -1, 100, first.ctypes.data) == DRM_ERR_ARG
    assert lib().drm_dupset_mark(None, ends[:4].ctypes.data, 4, 100, first.ctypes.data) == DRM_ERR_ARG
    assert lib().drm_dupset_mark_device(s.handle, None, 4, 100, None, None) == DRM_ERR_ARG
    assert len(s.mark(ends[:0], first_item=5)) == 0 and s.info()["next_item"] == 100  # n == 0 touches nothing
    # a gap in the item numbers is accepted, and the answers are the reference's
    assert np.array_equal(s.mark(ends[100:200], first_item=150), ref.mark(ends[100:200], first_item=150))
    assert np.array_equal(s.mark(ends[200:250]), ref.mark(ends[200:250]))
    assert s.info() == dict(max_items=300, slots=1024, next_item=300)
    s.free()
    for bad in (0, -1, (1 << 31) + 1):
        h = C.c_void_p()
        assert lib().drm_dupset_create(bad, 0, C.byref(h)) == DRM_ERR_ARG
    assert lib().drm_dupset_create(8, 0, None) == DRM_ERR_ARG and lib().drm_dupset_free(None) == 0
