"""Paired-end reads: which hit of mate 1 and which hit of mate 2 belong to one fragment (drm_pair_hits, the HIP kernel
of csrc/pair_hits.hip), the SAM fields that relate a pair's two lines (drm_sam_pair_fields), and the rescue of a mate
the search lost: its score-only alignment over the insert window of its mate's hit (drm_mate_rescue, the HIP kernel
of csrc/mate_rescue.hip) and the decision that follows (drm_pair_rescue_choose); and the template-length window the
three of them take, estimated from the reads: the histogram of the confident pairs' template lengths (drm_tlen_scan,
the HIP kernel of csrc/tlen_scan.hip) and the window read off it (drm_tlen_estimate). The definitions are in
include/drm_hip.h."""
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


# ------------------------------------------------------------------------------------------- mate rescue
# drm_rescue_result (include/drm_hip.h)
RESCUE_RESULT_DTYPE = np.dtype([("region_start", np.int64)] +
                               [(f, np.int32) for f in ("region_len", "reverse", "score", "ref_end", "q_end", "status")])
RESCUE_SCORING = (1, 1, 0, 1)  # the rerank's scoring: what makes a rescued score comparable with a reranked one


def _scoring(scoring):
    s = np.array([int(x) for x in scoring], dtype=np.int32)
    if s.shape != (4,):
        raise ValueError("scoring is (match, mismatch, gap_open, gap_extend)")
    return s


def mate_rescue(table, anchor_ids, task_query, query_seqs, min_tlen=0, max_tlen=1000, scoring=RESCUE_SCORING,
                ref_len=None):
    """drm_mate_rescue on host arrays: task t aligns, score only, query task_query[t] of query_seqs (a list, or
    pack_queries' (buffer, lengths)) against the insert window of the hit anchor_ids[t] on a GenomeTable. ref_len
    defaults to the table's. Returns a structured array (RESCUE_RESULT_DTYPE), one record per task."""
    from .rerank import pack_queries
    wid = np.ascontiguousarray(anchor_ids, dtype=np.uint64)
    tq = np.ascontiguousarray(task_query, dtype=np.int64)
    if wid.shape != tq.shape or wid.ndim != 1:
        raise ValueError("anchor_ids and task_query must be 1-d arrays of one length")
    qbuf, qlen = query_seqs if isinstance(query_seqs, tuple) else pack_queries(query_seqs)
    out = np.zeros(len(wid), dtype=RESCUE_RESULT_DTYPE)
    prm = pair_params(table.ref_len if ref_len is None else ref_len, min_tlen, max_tlen, 0)
    check(lib().drm_mate_rescue(table.handle, ptr(_scoring(scoring)), ptr(prm), ptr(wid), ptr(tq), len(wid),
                                ptr(qbuf), ptr(qlen), qbuf.shape[1], len(qlen), ptr(out)))
    return out


def mate_rescue_device(table, d_anchor_ids, d_task_query, ntasks, d_queries, d_q_len, q_stride, nq, min_tlen=0,
                       max_tlen=1000, scoring=RESCUE_SCORING, d_out=None, stream=None):
    """drm_mate_rescue_device: the same on device memory, enqueued on `stream`. Each d_* argument is a DeviceBuffer or
    a raw device address. Returns the DeviceBuffer of ntasks records (d_out, or a new one); synchronise the stream
    before downloading it."""
    from .device import DeviceBuffer

    def addr(b):
        return C.c_void_p(b.ptr if hasattr(b, "ptr") else int(b))
    if d_out is None:
        d_out = DeviceBuffer((int(ntasks),), RESCUE_RESULT_DTYPE)
    prm = pair_params(table.ref_len, min_tlen, max_tlen, 0)
    check(lib().drm_mate_rescue_device(table.handle, ptr(_scoring(scoring)), ptr(prm), addr(d_anchor_ids),
                                       addr(d_task_query), int(ntasks), addr(d_queries), addr(d_q_len), int(q_stride),
                                       int(nq), addr(d_out), stream.handle if stream is not None else None))
    return d_out


def mate_rescue_region(glen, ref_len, anchor_id, min_tlen=0, max_tlen=1000):
    """(start, length, reverse) of an anchor's rescue region on a genome of glen bases (drm_mate_rescue_region): the
    bytes genome[start : start + length], reverse-complemented when reverse; length 0 for an empty region."""
    start, n, rev = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    prm = pair_params(ref_len, min_tlen, max_tlen, 0)
    check(lib().drm_mate_rescue_region(ptr(prm), int(glen), int(anchor_id), C.byref(start), C.byref(n), C.byref(rev)))
    return start.value, n.value, rev.value


def _rescue_record(r):
    rec = np.zeros(1, dtype=RESCUE_RESULT_DTYPE)
    rec[0] = tuple(int(r[f]) for f in RESCUE_RESULT_DTYPE.names)
    return rec


def mate_rescue_window(record, ref_len, glen):
    """drm_mate_rescue_window: the window id under which the aligners find a rescued hit (a status-0 record)."""
    w = C.c_uint64(0)
    check(lib().drm_mate_rescue_window(ptr(_rescue_record(record)), int(ref_len), int(glen), C.byref(w)))
    return int(w.value)


def pair_rescue_choose(pair, s1, s2, anchor1, anchor2, rA, rB, ref_len, glen, unpaired_penalty=17, min_score=0):
    """drm_pair_rescue_choose: `pair` is one record of pair_hits, s1 / s2 and anchor1 / anchor2 the scores and window
    ids of its chosen rows (0 where j = -1), rA / rB the rescue records anchored on mate 1's / mate 2's hit (None = no
    task). Returns (record, rescued_id): the pair's record, with status 5 or 6 and the rescued mate's window id when a
    rescue replaces the choice, unchanged (and 0) otherwise."""
    p = np.zeros(1, dtype=PAIR_RESULT_DTYPE)
    p[0] = tuple(int(pair[f]) for f in PAIR_RESULT_DTYPE.names)
    a = None if rA is None else _rescue_record(rA)
    b = None if rB is None else _rescue_record(rB)
    out = np.zeros(1, dtype=PAIR_RESULT_DTYPE)
    w = C.c_uint64(0)
    check(lib().drm_pair_rescue_choose(ptr(p), int(s1), int(s2), int(anchor1), int(anchor2), ptr(a), ptr(b),
                                       int(ref_len), int(glen), int(unpaired_penalty), int(min_score), ptr(out),
                                       C.byref(w)))
    return out[0], int(w.value)


# ------------------------------------------------------------------------------------------- template-length window
# drm_tlen_sample / drm_tlen_estimate_t (include/drm_hip.h)
TLEN_SAMPLE_DTYPE = np.dtype([(f, np.int32) for f in ("cls", "tlen", "mapq1", "mapq2")])
TLEN_ESTIMATE_DTYPE = np.dtype([("n", np.int64), ("n_trim", np.int64)] +
                               [(f, np.int32) for f in ("p25", "p50", "p75", "trim_lo", "trim_hi", "mean", "sd", "low",
                                                        "high", "status")])
TLEN_ESTIMATE_FIELDS = TLEN_ESTIMATE_DTYPE.names
TLEN_MAX_SCAN = 10000    # bin/pipeline's: max(ref_len, 10000)
TLEN_MIN_MAPQ = 20       # DRM_PAIR_TLEN_MAPQ's default
TLEN_MIN_SAMPLES = 10    # bwa-mem's


def _tlen_params(ref_len, min_mapq, max_scan, locus_span, min_score, sub_band):
    from .mapq import MAPQ_MIN_DEFAULT, MAPQ_SUB_BAND, mapq_params
    max_scan = max(int(ref_len), TLEN_MAX_SCAN) if max_scan is None else int(max_scan)
    mp = mapq_params(ref_len, locus_span, MAPQ_MIN_DEFAULT if min_score is None else min_score,
                     MAPQ_SUB_BAND if sub_band is None else sub_band)
    return mp, np.array([int(min_mapq), max_scan], dtype=np.int32), max_scan


def tlen_scan(ids1, scores1, cnt1, ids2, scores2, cnt2, full1, full2, ref_len, min_mapq=TLEN_MIN_MAPQ, max_scan=None,
              row_step=1, locus_span=None, min_score=None, sub_band=None, samples=True):
    """drm_tlen_scan on host arrays: the lists and full_m as pair_mapq takes them (row_step included); the MAPQ
    parameters default to mapq_params', max_scan to max(ref_len, 10000). Returns (samples, hist): a structured array
    (TLEN_SAMPLE_DTYPE), one record per pair (None with samples=False), and the histogram [3, max_scan + 1] u32 of the
    FR, RF and same-strand template lengths."""
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
    mp, tp, max_scan = _tlen_params(ref_len, min_mapq, max_scan, locus_span, min_score, sub_band)
    out = np.zeros(npairs, dtype=TLEN_SAMPLE_DTYPE) if samples else None
    hist = np.zeros((3, max(max_scan, 0) + 1), dtype=np.uint32)
    check(lib().drm_tlen_scan(ptr(mp), ptr(tp), ptr(i1) if i1.size else None, ptr(s1) if s1.size else None, ptr(c1),
                              ptr(i2) if i2.size else None, ptr(s2) if s2.size else None, ptr(c2), ptr(f1), ptr(f2),
                              npairs, k, row_step, ptr(out), ptr(hist)))
    return out, hist


def tlen_scan_device(d_ids1, d_scores1, d_cnt1, d_ids2, d_scores2, d_cnt2, d_full1, d_full2, npairs, k, ref_len, d_hist,
                     min_mapq=TLEN_MIN_MAPQ, max_scan=None, row_step=1, locus_span=None, min_score=None, sub_band=None,
                     d_samples=None, stream=None):
    """drm_tlen_scan_device: the same on device memory, enqueued on `stream`. Each d_* argument is a DeviceBuffer or a
    raw device address. ADDS into d_hist ([3, max_scan + 1] u32, zeroed by the caller); d_samples (npairs records of
    TLEN_SAMPLE_DTYPE) may be None. Returns d_hist; synchronise the stream before downloading it."""
    def addr(b):
        return None if b is None else C.c_void_p(b.ptr if hasattr(b, "ptr") else int(b))
    mp, tp, _ = _tlen_params(ref_len, min_mapq, max_scan, locus_span, min_score, sub_band)
    check(lib().drm_tlen_scan_device(ptr(mp), ptr(tp), addr(d_ids1), addr(d_scores1), addr(d_cnt1), addr(d_ids2),
                                     addr(d_scores2), addr(d_cnt2), addr(d_full1), addr(d_full2), int(npairs), int(k),
                                     int(row_step), addr(d_samples), addr(d_hist),
                                     stream.handle if stream is not None else None))
    return d_hist


def tlen_estimate(hist_row, min_samples=TLEN_MIN_SAMPLES):
    """drm_tlen_estimate: the template-length window of one histogram row (bin T = the number of samples of template
    length T), as a dict over TLEN_ESTIMATE_FIELDS; status 1 (every other field 0) below min_samples samples. `low` and
    `high` are the window to map with. Host only."""
    h = np.ascontiguousarray(hist_row, dtype=np.uint32)
    if h.ndim != 1:
        raise ValueError("one histogram row")
    out = np.zeros(1, dtype=TLEN_ESTIMATE_DTYPE)
    check(lib().drm_tlen_estimate(ptr(h) if h.size else None, len(h), int(min_samples), ptr(out)))
    return {f: int(out[f][0]) for f in TLEN_ESTIMATE_FIELDS}
