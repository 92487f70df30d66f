"""Paired-end reads: which hit of mate 1 and which hit of mate 2 belong to one fragment (drm_pair_hits, the HIP kernel
of csrc/pair_hits.hip), and the SAM fields that relate a pair's two lines (drm_sam_pair_fields). The definitions are
in include/drm_hip.h."""
import ctypes as C

import numpy as np

from ._native import check, lib, ptr

# drm_pair_result (include/drm_hip.h)
PAIR_RESULT_DTYPE = np.dtype([(f, np.int32) for f in ("j1", "j2", "score", "tlen", "n_proper", "status")])
# drm_sam_mate / drm_sam_mate_fields
SAM_MATE_DTYPE = np.dtype([("mapped", np.int32), ("reverse", np.int32), ("pos1", np.int64), ("ref_span", np.int32)],
                          align=True)
SAM_MATE_FIELDS_DTYPE = np.dtype([("flag", np.int32), ("has_rname", np.int32), ("pos", np.int64), ("pnext", np.int64),
                                  ("tlen", np.int64)], align=True)


def pair_params(ref_len, min_tlen=0, max_tlen=1000, unpaired_penalty=17):
    """drm_pair_params as the int32 array the C ABI reads."""
    return np.array([int(ref_len), int(min_tlen), int(max_tlen), int(unpaired_penalty)], dtype=np.int32)


def _rows(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a.reshape(-1, a.shape[-1]) if a.ndim > 2 else a


def pair_hits(ids1, scores1, cnt1, ids2, scores2, cnt2, ref_len, min_tlen=0, max_tlen=1000, unpaired_penalty=17,
              row_step=1):
    """drm_pair_hits on host arrays: ids_m [rows, k] u64 window ids, scores_m [rows, k] i32 and cnt_m [rows] i32 of
    the two mates' rerank outputs; pair p reads row p * row_step of each. row_step = 2 with ids2 = ids1[1:],
    scores2 = scores1[1:], cnt2 = cnt1[1:] takes one interleaved batch (read 2p is mate 1, read 2p + 1 mate 2).
    Returns a structured array (PAIR_RESULT_DTYPE), one record per pair."""
    i1, i2 = _rows(ids1, np.uint64), _rows(ids2, np.uint64)
    s1, s2 = _rows(scores1, np.int32), _rows(scores2, np.int32)
    c1, c2 = np.ascontiguousarray(cnt1, dtype=np.int32), np.ascontiguousarray(cnt2, dtype=np.int32)
    k, row_step = int(i1.shape[1]), int(row_step)
    if row_step < 1:
        raise ValueError("row_step must be >= 1")
    if not (i1.ndim == 2 and i1.shape == s1.shape and i2.shape == s2.shape and i2.shape[1] == k and
            len(c1) == len(i1) and len(c2) == len(i2)):
        raise ValueError("ids, scores [rows, k] and counts [rows] of a mate must agree, and k of the two mates")
    npairs = (len(c1) + row_step - 1) // row_step
    if npairs and (npairs - 1) * row_step + 1 > len(c2):
        raise ValueError("mate 2 has fewer rows than the pairs of mate 1 need")
    out = np.zeros(npairs, dtype=PAIR_RESULT_DTYPE)
    prm = pair_params(ref_len, min_tlen, max_tlen, unpaired_penalty)
    check(lib().drm_pair_hits(ptr(prm), ptr(i1) if i1.size else None, ptr(s1) if s1.size else None, ptr(c1),
                              ptr(i2) if i2.size else None, ptr(s2) if s2.size else None, ptr(c2), npairs, k, row_step,
                              ptr(out)))
    return out


def pair_hits_device(d_ids1, d_scores1, d_cnt1, d_ids2, d_scores2, d_cnt2, npairs, k, ref_len, min_tlen=0,
                     max_tlen=1000, unpaired_penalty=17, row_step=1, d_out=None, stream=None):
    """drm_pair_hits_device: the same on device memory, enqueued on `stream`. Each d_* argument is a DeviceBuffer or a
    raw device address (an int, e.g. buffer.ptr + an offset for the interleaved layout). Returns the DeviceBuffer of
    npairs records (d_out, or a new one); synchronise the stream before downloading it."""
    from .device import DeviceBuffer

    def addr(b):
        return C.c_void_p(b.ptr if hasattr(b, "ptr") else int(b))
    if d_out is None:
        d_out = DeviceBuffer((int(npairs),), PAIR_RESULT_DTYPE)
    prm = pair_params(ref_len, min_tlen, max_tlen, unpaired_penalty)
    check(lib().drm_pair_hits_device(ptr(prm), addr(d_ids1), addr(d_scores1), addr(d_cnt1), addr(d_ids2),
                                     addr(d_scores2), addr(d_cnt2), int(npairs), int(k), int(row_step), addr(d_out),
                                     stream.handle if stream is not None else None))
    return d_out


def sam_pair_fields(mate1, mate2, proper):
    """drm_sam_pair_fields: mate_m = (mapped, reverse, pos1, ref_span), with ref_span = ref_end - ref_begin of the
    mate's alignment record (an unmapped mate may be None). Returns the two lines' fields as a pair of dicts with
    flag, has_rname, pos, pnext and tlen."""
    m = np.zeros(2, dtype=SAM_MATE_DTYPE)
    for i, x in enumerate((mate1, mate2)):
        if x is not None:
            m[i] = tuple(int(v) for v in x)
    out = np.zeros(2, dtype=SAM_MATE_FIELDS_DTYPE)
    check(lib().drm_sam_pair_fields(ptr(m), int(bool(proper)), ptr(out)))
    return tuple({f: int(out[f][i]) for f in SAM_MATE_FIELDS_DTYPE.names} for i in range(2))
