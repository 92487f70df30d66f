"""GPU tests of drm_sort_order / drm_sort_order_device (csrc/sort_order.hip): the order equals np.argsort(keys,
kind="stable") exactly, at sizes around a wave, around a tile, over several tiles and over more tiles than one step of
the scan covers, for keys that skip every pass (all equal), that keep exactly one pass (one byte varies, each of the
eight), that keep all eight (random 64-bit), where stability decides nearly everything (16 values), that come sorted or
reversed, for real SAM keys with all-ones keys scattered through, and for keys whose upper bytes only tell the all-ones
keys from the rest (all but one of those passes dropped) or nearly do (none dropped). Both entry points agree, the keys
are left unchanged, two runs give the same order, and a workspace that is too small is refused before anything is
launched."""
import ctypes as C

import numpy as np
import pytest

from deepreadmapper_amd import (DrmError, sam_sort_key, sort_order, sort_order_device, sort_order_workspace,
                                sort_scan_tiles, sort_tile)
from deepreadmapper_amd._native import DRM_ERR_ARG, lib
from deepreadmapper_amd.device import DeviceBuffer, Stream, synchronize

pytestmark = pytest.mark.gpu

T = sort_tile()
LONG = (sort_scan_tiles() + 1) * T + 5  # the scan of a pass takes two steps, the second over one tile and a bit
SIZES = [1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17, LONG]
KINDS = (["equal", "random", "sixteen", "sorted", "reversed", "sam"] + [f"byte{p}" for p in range(8)] +
         ["ones_rest", "ones_trap", "ones_only"])
LONG_KINDS = ("equal", "random", "sixteen", "sam", "byte0", "byte3", "byte7", "ones_rest", "ones_trap")
ONES = np.uint64(2 ** 64 - 1)


def _sam_keys(rng, n):
    """Keys as a paired run over 25 contigs gives them, 2 % of them the all-ones key of a line without RNAME."""
    tid = rng.integers(0, 25, n).astype(np.uint64)
    pos = rng.integers(1, 50_000_000, n).astype(np.uint64)
    rev = rng.integers(0, 2, n).astype(np.uint64)
    keys = (((tid << np.uint64(33)) | pos) << np.uint64(1)) | rev
    for i in range(min(n, 3)):
        assert int(keys[i]) == sam_sort_key(int(tid[i]), int(pos[i]), int(rev[i]))
    keys[rng.random(n) < 0.02] = ONES
    if n > 5:
        keys[n // 2] = ONES
        keys[n // 3] = keys[0]  # an equal pair of real keys
    return keys


def _keys(kind, n):
    rng = np.random.default_rng(1000 * KINDS.index(kind) + n % 997)
    if kind == "equal":
        return np.full(n, 0x0123456789ABCDEF, dtype=np.uint64)
    if kind == "random":
        return rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    if kind == "sixteen":
        return rng.integers(0, 16, n, dtype=np.uint64) * np.uint64(0x0101010101010101)  # every byte varies, 16 values
    if kind == "sorted":
        return np.sort(rng.integers(0, 2 ** 64, n, dtype=np.uint64))
    if kind == "reversed":
        return np.sort(rng.integers(0, 2 ** 64, n, dtype=np.uint64))[::-1].copy()
    if kind == "sam":
        return _sam_keys(rng, n)
    if kind in ("ones_rest", "ones_trap", "ones_only"):
        # bytes 2 .. 7 are 0x11 in every key that is not all-ones, so each of them only tells the all-ones keys from the
        # rest and one of those passes is enough; in the trap some keys hold 0xFF there without being all-ones, so those
        # bytes tell more than that and every pass must stay; ones_only has nothing but the two kinds of key
        low = rng.integers(0, 1 << 16, n, dtype=np.uint64) if kind != "ones_only" else np.full(n, 0x2222, dtype=np.uint64)
        keys = np.uint64(0x1111111111110000) | low
        pick = rng.random(n)
        if kind == "ones_trap":
            keys[pick < 0.1] |= np.uint64(0xFFFFFFFFFFFF0000)
        keys[pick < 0.05] = ONES
        if n > 3:
            keys[1] = ONES
        return keys
    p = int(kind[4:])
    keep = np.uint64(0x5A5A5A5A5A5A5A5A) & ~(np.uint64(255) << np.uint64(8 * p))
    return keep | (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(8 * p))


_cache = {}


def _case(kind, n):
    """(keys, expected order), made once and never changed."""
    if (kind, n) not in _cache:
        keys = _keys(kind, n)
        want = np.argsort(keys, kind="stable").astype(np.uint32)
        keys.setflags(write=False)
        want.setflags(write=False)
        _cache[(kind, n)] = (keys, want)
    return _cache[(kind, n)]


CASES = [(k, n) for n in SIZES for k in KINDS if n != LONG or k in LONG_KINDS]


@pytest.mark.parametrize("kind,n", CASES, ids=[f"{k}-{n}" for k, n in CASES])
def test_the_order_is_numpys_stable_argsort(kind, n):
    keys, want = _case(kind, n)
    got = sort_order(keys)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    if kind == "equal":
        assert np.array_equal(got, np.arange(n, dtype=np.uint32))  # every pass skipped: the identity


def test_the_one_byte_sets_keep_one_pass_each():
    for p in range(8):
        keys, _ = _case(f"byte{p}", 3 * T + 17)
        varying = [q for q in range(8) if len(np.unique((keys >> np.uint64(8 * q)) & np.uint64(255))) > 1]
        assert varying == [p]


@pytest.mark.parametrize("kind,n", [("sam", 3 * T + 17), ("sixteen", T + 1), ("random", LONG), ("equal", 65),
                                    ("byte5", T - 1)])
def test_the_device_entry_point_agrees_leaves_the_keys_and_repeats_itself(kind, n):
    keys, want = _case(kind, n)
    d_keys = DeviceBuffer.from_host(keys)
    before = d_keys.checksum()
    s = Stream()
    first = sort_order_device(d_keys, n, stream=s)
    second = sort_order_device(d_keys, n, stream=s)  # the same stream: the workspace is used in turn
    s.synchronize()
    a, b = first.download(), second.download()
    assert np.array_equal(a, want) and np.array_equal(a, b)
    assert d_keys.checksum() == before and np.array_equal(d_keys.download(), keys)
    assert np.array_equal(sort_order(keys), a)
    for buf in (d_keys, first, second):
        buf.free()


def test_a_small_workspace_is_refused_without_a_launch():
    n = 3 * T + 17
    keys, _ = _case("random", n)
    need = sort_order_workspace(n)
    d_keys = DeviceBuffer.from_host(keys)
    d_order = DeviceBuffer.from_host(np.full(n, 0xDEADBEEF, dtype=np.uint32))
    work = DeviceBuffer((need - 1,), np.uint8)
    work.zero()
    synchronize()
    marks = (d_order.checksum(), work.checksum())
    with pytest.raises(DrmError) as e:
        sort_order_device(d_keys, n, d_order=d_order, work=work)
    assert e.value.code == DRM_ERR_ARG and "workspace" in str(e.value)
    for args in ((None, n, d_order.ptr, work.ptr, need), (d_keys.ptr, n, None, work.ptr, need),
                 (d_keys.ptr, n, d_order.ptr, None, need), (d_keys.ptr, -1, d_order.ptr, work.ptr, need)):
        assert lib().drm_sort_order_device(*[C.c_void_p(a) if i in (0, 2, 3) else a for i, a in enumerate(args)],
                                           None) == DRM_ERR_ARG
    synchronize()
    assert (d_order.checksum(), work.checksum()) == marks  # nothing ran
    assert lib().drm_sort_order_device(None, 0, None, None, 0, None) == 0  # n == 0: nothing to do
    for buf in (d_keys, d_order, work):
        buf.free()
