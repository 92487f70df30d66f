"""BAM output: BGZF compression on a device (drm_bgzf_compress, the HIP kernels of csrc/bgzf.hip), the fixed numbers of
BGZF, and the host-side encoders of the BAM header and of one alignment record (csrc/bam.cpp). The definitions are in
include/drm_hip.h."""
import ctypes as C

import numpy as np

from ._native import check, lib, ptr


def bgzf_block():
    """drm_bgzf_block: the input bytes of one BGZF block, 65,280."""
    return int(lib().drm_bgzf_block())


def bgzf_bound(n):
    """drm_bgzf_bound: the most bytes the members of n input bytes can take, n + 31 per block."""
    b = C.c_size_t(0)
    check(lib().drm_bgzf_bound(int(n), C.byref(b)))
    return b.value


def bgzf_eof():
    """drm_bgzf_eof: the 28-byte empty member that ends a BGZF file."""
    out = (C.c_uint8 * 28)()
    check(lib().drm_bgzf_eof(out))
    return bytes(out)


def bgzf_workspace(n):
    """drm_bgzf_workspace: the bytes of scratch memory bgzf_compress_device needs for n input bytes."""
    b = C.c_size_t(0)
    check(lib().drm_bgzf_workspace(int(n), C.byref(b)))
    return b.value


def bgzf_compress(data, device=0):
    """drm_bgzf_compress on host bytes: the gzip members of the 65,280-byte blocks of `data`, back to back (no EOF
    member). Empty input touches no device and gives b""."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.empty(bgzf_bound(len(a)), dtype=np.uint8)
    got = C.c_size_t(0)
    check(lib().drm_bgzf_compress(ptr(a) if len(a) else None, len(a), int(device), ptr(out) if len(a) else None,
                                  out.nbytes, C.byref(got)))
    return out[:got.value].tobytes()


def bgzf_compress_device(d_data, n, d_out=None, d_sizes=None, stream=None, work=None):
    """drm_bgzf_compress_device: the same on device memory of the current device, enqueued on `stream`. d_data is a
    DeviceBuffer or a raw device address of [n] bytes, left unchanged. Returns (d_out, d_sizes): the packed stream in a
    buffer of bgzf_bound(n) bytes and every member's length [ceil(n / 65280)] u32 (new buffers when None);
    synchronise the stream before downloading. `work` names the scratch DeviceBuffer to use; without one a buffer is
    allocated for the call and freed after a synchronisation of the device."""
    from .device import DeviceBuffer, synchronize

    def addr(b):
        return None if b is None else C.c_void_p(b.ptr if hasattr(b, "ptr") else int(b))
    n = int(n)
    blocks = -(-n // bgzf_block())
    if d_out is None:
        d_out = DeviceBuffer((bgzf_bound(n),), np.uint8)
    if d_sizes is None:
        d_sizes = DeviceBuffer((blocks,), np.uint32)
    own = work is None and n > 0
    if own:
        work = DeviceBuffer((bgzf_workspace(n),), np.uint8)
    try:
        check(lib().drm_bgzf_compress_device(addr(d_data), n, addr(d_out), addr(d_sizes), addr(work),
                                             work.nbytes if work is not None else 0,
                                             stream.handle if stream is not None else None))
    finally:
        if own:
            synchronize()
            work.free()
    return d_out, d_sizes


def _take(call):
    """Runs call(out, cap, bytes) with a buffer that is grown once to the size the call reports."""
    cap = 1 << 12
    for _ in range(2):
        out = (C.c_uint8 * cap)()
        got = C.c_size_t(0)
        rc = call(out, cap, C.byref(got))
        if rc == 0 or got.value <= cap:
            check(rc)
            return bytes(out[:got.value])
        cap = got.value
    raise AssertionError("unreachable")


def bam_header(text):
    """drm_bam_header: the uncompressed BAM header of a SAM header text (str or bytes)."""
    t = text.encode() if isinstance(text, str) else bytes(text)
    return _take(lambda out, cap, got: lib().drm_bam_header(t, len(t), out, cap, got))


def bam_record(line, ref_names):
    """drm_bam_record: the BAM alignment record (block_size first) of one SAM text line; ref_names are the @SQ names in
    order."""
    t = line.encode() if isinstance(line, str) else bytes(line)
    names = [n.encode() if isinstance(n, str) else bytes(n) for n in ref_names]
    arr = (C.c_char_p * max(len(names), 1))(*names)
    return _take(lambda out, cap, got: lib().drm_bam_record(t, len(t), arr, len(names), out, cap, got))
