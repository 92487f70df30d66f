"""Duplicate marking: the unclipped 5' end of an alignment record (drm_sam_end5), the end word of a mapped mate
(drm_dup_end_word), and the first-seen set of the templates' end pairs that lives on a device across the blocks of a
run (drm_dupset, the HIP kernels of csrc/dup_set.hip). The definitions are in include/drm_hip.h."""
import ctypes as C

import numpy as np

from ._native import check, lib, ptr
from .rerank import SW_ALIGNMENT_DTYPE


def sam_end5(record, tag_prefix, region_start, region_len, reverse):
    """drm_sam_end5: the 0-based forward-strand coordinate under the read's first sequenced base, were its leading clip
    aligned without gaps; the record is relative to genome[region_start ..+ region_len), reverse-complemented when
    `reverse`. For a window record the region is (window_id // 2, ref_len, window_id & 1)."""
    r = np.zeros(1, dtype=SW_ALIGNMENT_DTYPE)
    r[0] = tuple(int(record[f]) for f in SW_ALIGNMENT_DTYPE.names)
    e = C.c_int64(0)
    check(lib().drm_sam_end5(ptr(r), int(tag_prefix), int(region_start), int(region_len), int(bool(reverse)),
                             C.byref(e)))
    return e.value


def dup_end_word(end5, reverse):
    """drm_dup_end_word: (((end5 + 2^20) << 1) | reverse) + 1 for -2^20 <= end5 < 2^61; 0 is the unmapped mate."""
    w = C.c_uint64(0)
    check(lib().drm_dup_end_word(int(end5), int(bool(reverse)), C.byref(w)))
    return w.value


def dup_slot(lo, hi, slots):
    """drm_dup_slot: the home slot of the key (lo, hi) in a table of `slots` slots (a power of two)."""
    s = C.c_int64(0)
    check(lib().drm_dup_slot(int(lo), int(hi), int(slots), C.byref(s)))
    return s.value


class DupSet:
    """A first-seen set of end-word pairs on a device (drm_dupset) for up to max_items items numbered over the run."""

    def __init__(self, max_items, device=0):
        self.device = int(device)
        self.handle = C.c_void_p()
        check(lib().drm_dupset_create(int(max_items), self.device, C.byref(self.handle)))

    def info(self):
        """drm_dupset_get_info: dict(max_items, slots, next_item)."""
        m, s, n = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().drm_dupset_get_info(self.handle, C.byref(m), C.byref(s), C.byref(n)))
        return {"max_items": m.value, "slots": s.value, "next_item": n.value}

    def mark(self, ends, first_item=None):
        """drm_dupset_mark on a host array ends [n, 2] u64 of end words: items first_item .. first_item + n (default:
        from the set's next item). Returns first [n] i64: the smallest item index so far with the item's key, -1 for an
        item without one; item i is a duplicate iff 0 <= first[i] != first_item + i."""
        e = np.ascontiguousarray(ends, dtype=np.uint64)
        if e.ndim != 2 or e.shape[1] != 2:
            raise ValueError("ends must be [n, 2]")
        if first_item is None:
            first_item = self.info()["next_item"]
        first = np.zeros(len(e), dtype=np.int64)
        check(lib().drm_dupset_mark(self.handle, ptr(e) if len(e) else None, len(e), int(first_item),
                                    ptr(first) if len(e) else None))
        return first

    def mark_device(self, d_ends, n, first_item=None, d_first=None, stream=None):
        """drm_dupset_mark_device: the same on device memory, enqueued on `stream`. d_ends is a DeviceBuffer or a raw
        device address of [n, 2] u64; d_first the output buffer (a new one when None). Returns d_first; synchronise the
        stream before downloading."""
        from .device import DeviceBuffer

        def addr(b):
            return None if b is None else C.c_void_p(b.ptr if hasattr(b, "ptr") else int(b))
        if first_item is None:
            first_item = self.info()["next_item"]
        if d_first is None:
            d_first = DeviceBuffer((int(n),), np.int64)
        check(lib().drm_dupset_mark_device(self.handle, addr(d_ends), int(n), int(first_item), addr(d_first),
                                           stream.handle if stream is not None else None))
        return d_first

    def free(self):
        if self.handle:
            check(lib().drm_dupset_free(self.handle))
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
