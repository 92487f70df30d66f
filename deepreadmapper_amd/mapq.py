"""Mapping quality: the locus scan of a read's reranked hit list (drm_hit_mapq, the HIP kernel hit_mapq_kernel of
csrc/mapq.hip), the same for a read pair with the best proper combination outside the chosen loci (drm_pair_mapq,
pair_mapq_kernel), the formula that turns best / competitor / count into a MAPQ (drm_mapq_value) and the rule for a
rescued mate (drm_pair_mapq_rescued). The definitions are in include/drm_hip.h."""
import ctypes as C

import numpy as np

from ._native import check, lib, ptr
from .pairing import PAIR_RESULT_DTYPE, _rows, pair_params

# drm_mapq_result / drm_pair_mapq_result (include/drm_hip.h)
MAPQ_RESULT_DTYPE = np.dtype([(f, np.int32) for f in ("best", "best_score", "locus_rows", "sub_row", "sub_score",
                                                      "n_sub", "mapq", "status")])
PAIR_MAPQ_RESULT_DTYPE = np.dtype([(f, np.int32) for f in ("mapq1", "mapq2", "q_se1", "q_se2", "q_pe", "sub_pair")])
MAPQ_MIN_DEFAULT = 39  # the largest chance score measured for 150-base reads
MAPQ_SUB_BAND = 2      # one substitution under the rerank's scoring {1, 1, 0, 1}


def mapq_params(ref_len, locus_span=None, min_score=MAPQ_MIN_DEFAULT, sub_band=MAPQ_SUB_BAND):
    """drm_mapq_params as the int32 array the C ABI reads; locus_span defaults to ref_len."""
    return np.array([int(ref_len), int(ref_len if locus_span is None else locus_span), int(min_score), int(sub_band)],
                    dtype=np.int32)


def _addr(b):
    return None if b is None else C.c_void_p(b.ptr if hasattr(b, "ptr") else int(b))


def hit_mapq(ids, scores, cnt, full, ref_len, head=None, locus_span=None, min_score=MAPQ_MIN_DEFAULT,
             sub_band=MAPQ_SUB_BAND):
    """drm_hit_mapq on host arrays: ids [reads, k] u64 window ids, scores [reads, k] i32 and cnt [reads] i32 of the
    rerank output, full [reads] i32 the reads' self scores (their lengths without tags), head [reads] i32 the head
    rows (None or -1: the top hit). Returns a structured array (MAPQ_RESULT_DTYPE), one record per read."""
    i, s = _rows(ids, np.uint64), _rows(scores, np.int32)
    c, f = np.ascontiguousarray(cnt, dtype=np.int32), np.ascontiguousarray(full, dtype=np.int32)
    h = None if head is None else np.ascontiguousarray(head, dtype=np.int32)
    if not (i.ndim == 2 and i.shape == s.shape and len(c) == len(i) and f.shape == c.shape and
            (h is None or h.shape == c.shape)):
        raise ValueError("ids, scores [reads, k] and cnt, full, head [reads] must agree")
    out = np.zeros(len(c), dtype=MAPQ_RESULT_DTYPE)
    prm = mapq_params(ref_len, locus_span, min_score, sub_band)
    check(lib().drm_hit_mapq(ptr(prm), ptr(i) if i.size else None, ptr(s) if s.size else None, ptr(c),
                             None if h is None else ptr(h), ptr(f), len(c), int(i.shape[1]), ptr(out)))
    return out


def hit_mapq_device(d_ids, d_scores, d_cnt, d_full, nreads, k, ref_len, d_head=None, locus_span=None,
                    min_score=MAPQ_MIN_DEFAULT, sub_band=MAPQ_SUB_BAND, d_out=None, stream=None):
    """drm_hit_mapq_device: the same on device memory, enqueued on `stream`. Each d_* argument is a DeviceBuffer or a
    raw device address. Returns the DeviceBuffer of nreads records (d_out, or a new one); synchronise the stream before
    downloading it."""
    from .device import DeviceBuffer
    if d_out is None:
        d_out = DeviceBuffer((int(nreads),), MAPQ_RESULT_DTYPE)
    prm = mapq_params(ref_len, locus_span, min_score, sub_band)
    check(lib().drm_hit_mapq_device(ptr(prm), _addr(d_ids), _addr(d_scores), _addr(d_cnt), _addr(d_head),
                                    _addr(d_full), int(nreads), int(k), _addr(d_out),
                                    stream.handle if stream is not None else None))
    return d_out


def _pair_records(pairs):
    p = np.zeros(len(pairs), dtype=PAIR_RESULT_DTYPE)
    for f in PAIR_RESULT_DTYPE.names:
        p[f] = pairs[f]
    return p


def pair_mapq(ids1, scores1, cnt1, ids2, scores2, cnt2, full1, full2, pairs, ref_len, min_tlen=0, max_tlen=1000,
              unpaired_penalty=17, row_step=1, locus_span=None, min_score=MAPQ_MIN_DEFAULT, sub_band=MAPQ_SUB_BAND):
    """drm_pair_mapq on host arrays: the lists as pair_hits takes them (row_step included), full_m indexed like cnt_m,
    pairs the records pair_hits returned for them. Returns a structured array (PAIR_MAPQ_RESULT_DTYPE), one record per
    pair."""
    i1, i2 = _rows(ids1, np.uint64), _rows(ids2, np.uint64)
    s1, s2 = _rows(scores1, np.int32), _rows(scores2, np.int32)
    c1, c2 = np.ascontiguousarray(cnt1, dtype=np.int32), np.ascontiguousarray(cnt2, dtype=np.int32)
    f1, f2 = np.ascontiguousarray(full1, dtype=np.int32), np.ascontiguousarray(full2, dtype=np.int32)
    k, row_step = int(i1.shape[1]), int(row_step)
    if row_step < 1:
        raise ValueError("row_step must be >= 1")
    if not (i1.ndim == 2 and i1.shape == s1.shape and i2.shape == s2.shape and i2.shape[1] == k and
            len(c1) == len(i1) and len(c2) == len(i2) and f1.shape == c1.shape and f2.shape == c2.shape):
        raise ValueError("ids, scores [rows, k] and counts, full [rows] of a mate must agree, and k of the two mates")
    npairs = (len(c1) + row_step - 1) // row_step
    if npairs and (npairs - 1) * row_step + 1 > len(c2):
        raise ValueError("mate 2 has fewer rows than the pairs of mate 1 need")
    p = _pair_records(pairs)
    if len(p) != npairs:
        raise ValueError("one pair record per pair")
    out = np.zeros(npairs, dtype=PAIR_MAPQ_RESULT_DTYPE)
    pp = pair_params(ref_len, min_tlen, max_tlen, unpaired_penalty)
    mp = mapq_params(ref_len, locus_span, min_score, sub_band)
    check(lib().drm_pair_mapq(ptr(pp), ptr(mp), ptr(i1) if i1.size else None, ptr(s1) if s1.size else None, ptr(c1),
                              ptr(i2) if i2.size else None, ptr(s2) if s2.size else None, ptr(c2), ptr(f1), ptr(f2),
                              ptr(p), npairs, k, row_step, ptr(out)))
    return out


def pair_mapq_device(d_ids1, d_scores1, d_cnt1, d_ids2, d_scores2, d_cnt2, d_full1, d_full2, d_pairs, npairs, k,
                     ref_len, min_tlen=0, max_tlen=1000, unpaired_penalty=17, row_step=1, locus_span=None,
                     min_score=MAPQ_MIN_DEFAULT, sub_band=MAPQ_SUB_BAND, d_out=None, stream=None):
    """drm_pair_mapq_device: the same on device memory, enqueued on `stream`; d_pairs is pair_hits_device's output.
    Returns the DeviceBuffer of npairs records (d_out, or a new one); synchronise the stream before downloading it."""
    from .device import DeviceBuffer
    if d_out is None:
        d_out = DeviceBuffer((int(npairs),), PAIR_MAPQ_RESULT_DTYPE)
    pp = pair_params(ref_len, min_tlen, max_tlen, unpaired_penalty)
    mp = mapq_params(ref_len, locus_span, min_score, sub_band)
    check(lib().drm_pair_mapq_device(ptr(pp), ptr(mp), _addr(d_ids1), _addr(d_scores1), _addr(d_cnt1), _addr(d_ids2),
                                     _addr(d_scores2), _addr(d_cnt2), _addr(d_full1), _addr(d_full2), _addr(d_pairs),
                                     int(npairs), int(k), int(row_step), _addr(d_out),
                                     stream.handle if stream is not None else None))
    return d_out


def mapq_value(s1, sub, n_sub, full, min_score=MAPQ_MIN_DEFAULT):
    """drm_mapq_value: the MAPQ of a best score s1 against the best competing score `sub`, n_sub competing loci, the
    read's self score `full` and the chance level min_score. Host only."""
    q = C.c_int32(0)
    check(lib().drm_mapq_value(int(s1), int(sub), int(n_sub), int(full), int(min_score), C.byref(q)))
    return q.value


def pair_mapq_rescued(pairs, mapq, rescue_score, full1, full2, ref_len, row_step=1, locus_span=None,
                      min_score=MAPQ_MIN_DEFAULT, sub_band=MAPQ_SUB_BAND):
    """drm_pair_mapq_rescued: pairs are the records after pair_rescue_choose (statuses 0 to 6), mapq the pair_mapq
    records of the pre-rescue pairs, rescue_score[p] the rescued mate's own score, full_m indexed as in pair_mapq.
    Returns a copy of mapq in which a rescued mate's MAPQ is the smaller of its anchor's and its own. Host only."""
    p = _pair_records(pairs)
    out = np.zeros(len(p), dtype=PAIR_MAPQ_RESULT_DTYPE)
    for f in PAIR_MAPQ_RESULT_DTYPE.names:
        out[f] = mapq[f]
    rs = np.ascontiguousarray(rescue_score, dtype=np.int32)
    f1, f2 = np.ascontiguousarray(full1, dtype=np.int32), np.ascontiguousarray(full2, dtype=np.int32)
    need = (len(p) - 1) * int(row_step) + 1 if len(p) else 0
    if len(rs) != len(p) or int(row_step) < 1 or len(f1) < need or len(f2) < need:
        raise ValueError("one rescue score per pair, and full_m for row p * row_step of every pair")
    mp = mapq_params(ref_len, locus_span, min_score, sub_band)
    check(lib().drm_pair_mapq_rescued(ptr(mp), ptr(p), ptr(rs), ptr(f1), ptr(f2), len(p), int(row_step), ptr(out)))
    return out
