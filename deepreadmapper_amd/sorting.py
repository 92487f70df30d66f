"""Coordinate order of the SAM lines: the key of a line (drm_sam_sort_key) and the stable sort of the keys on a device
(drm_sort_order, the HIP kernels of csrc/sort_order.hip). The definitions are in include/drm_hip.h."""
import ctypes as C

import numpy as np

from ._native import check, lib, ptr


def sam_sort_key(tid, pos, reverse):
    """drm_sam_sort_key: (((tid << 33) | pos) << 1) | reverse for 0 <= tid < 2^29, 0 <= pos < 2^33; 2^64 - 1 for
    tid == -1 (RNAME "*")."""
    k = C.c_uint64(0)
    check(lib().drm_sam_sort_key(int(tid), int(pos), int(bool(reverse)), C.byref(k)))
    return k.value


def sort_tile():
    """drm_sort_tile: the keys one block of the scatter kernel places."""
    return int(lib().drm_sort_tile())


def sort_scan_tiles():
    """drm_sort_scan_tiles: the tiles one step of the scan kernel covers."""
    return int(lib().drm_sort_scan_tiles())


def sort_order_workspace(n):
    """drm_sort_order_workspace: the bytes of scratch memory drm_sort_order_device needs for n keys."""
    b = C.c_size_t(0)
    check(lib().drm_sort_order_workspace(int(n), C.byref(b)))
    return b.value


def sort_order(keys, device=0):
    """drm_sort_order on a host array of u64 keys: order [n] u32, order[i] the input index of the key that comes i-th,
    equal keys in input order (np.argsort(keys, kind="stable")). An empty array touches no device."""
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    if k.ndim != 1:
        raise ValueError("keys must be one-dimensional")
    order = np.zeros(len(k), dtype=np.uint32)
    check(lib().drm_sort_order(ptr(k) if len(k) else None, len(k), int(device), ptr(order) if len(k) else None))
    return order


_work = None  # the workspace of sort_order_device, kept between calls and grown on demand


def sort_order_device(d_keys, n, d_order=None, stream=None, work=None):
    """drm_sort_order_device: the same on device memory of the current device, enqueued on `stream`. d_keys is a
    DeviceBuffer or a raw device address of [n] u64, left unchanged; d_order the output buffer (a new one when None).
    The workspace is the module's own, kept until a larger one is needed (synchronised before it is replaced), unless
    `work` names a DeviceBuffer to use. Returns d_order; synchronise the stream before downloading."""
    from .device import DeviceBuffer, synchronize
    global _work

    def addr(b):
        return None if b is None else C.c_void_p(b.ptr if hasattr(b, "ptr") else int(b))
    if d_order is None:
        d_order = DeviceBuffer((int(n),), np.uint32)
    if work is None and n > 0:
        need = sort_order_workspace(n)
        if _work is None or _work.nbytes < need:
            if _work is not None:
                synchronize()  # an earlier sort may still use it
                _work.free()
            _work = DeviceBuffer((need,), np.uint8)
        work = _work
    check(lib().drm_sort_order_device(addr(d_keys), int(n), addr(d_order), addr(work),
                                      work.nbytes if work is not None else 0,
                                      stream.handle if stream is not None else None))
    return d_order
