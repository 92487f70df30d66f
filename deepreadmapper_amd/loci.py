"""The locus list of a read's reranked hit list (drm_hit_loci, the HIP kernel hit_loci_kernel of csrc/hit_loci.hip):
the distinct placements a SAM writer prints as the primary line and its secondary lines or XA entries, together with
the MAPQ record drm_hit_mapq gives for the same list. The definition is in include/drm_hip.h."""
import numpy as np

from ._native import check, lib, ptr
from .mapq import MAPQ_MIN_DEFAULT, MAPQ_RESULT_DTYPE, MAPQ_SUB_BAND, _addr, mapq_params
from .pairing import _rows

LOCI_DROP_DEFAULT = 80  # bwa-mem's XA drop ratio: an alternative scores at least 80 % of the primary


def loci_params(max_loci, drop_pct=LOCI_DROP_DEFAULT):
    """drm_loci_params as the int32 array the C ABI reads."""
    return np.array([int(max_loci), int(drop_pct)], dtype=np.int32)


def hit_loci(ids, scores, cnt, full, ref_len, max_loci, drop_pct=LOCI_DROP_DEFAULT, head=None, locus_span=None,
             min_score=MAPQ_MIN_DEFAULT, sub_band=MAPQ_SUB_BAND):
    """drm_hit_loci on host arrays; the lists, counts, self scores and heads as hit_mapq takes them. Returns
    (records, n_loci, n_pass, loci_ids, loci_scores, loci_rows, loci_size): the MAPQ records (MAPQ_RESULT_DTYPE), the
    slots recorded and the loci that pass per read [reads] i32, and the slots [reads, max_loci] (ids u64, the others
    i32); a slot at or beyond n_loci holds id 2^64 - 1, score 0, row -1, size 0."""
    i, s = _rows(ids, np.uint64), _rows(scores, np.int32)
    c, f = np.ascontiguousarray(cnt, dtype=np.int32), np.ascontiguousarray(full, dtype=np.int32)
    h = None if head is None else np.ascontiguousarray(head, dtype=np.int32)
    if not (i.ndim == 2 and i.shape == s.shape and len(c) == len(i) and f.shape == c.shape and
            (h is None or h.shape == c.shape)):
        raise ValueError("ids, scores [reads, k] and cnt, full, head [reads] must agree")
    n, width = len(c), max(int(max_loci), 0)
    out = np.zeros(n, dtype=MAPQ_RESULT_DTYPE)
    n_loci, n_pass = np.zeros(n, np.int32), np.zeros(n, np.int32)
    l_ids = np.zeros((n, width), np.uint64)
    l_sc, l_rows, l_size = (np.zeros((n, width), np.int32) for _ in range(3))
    mp, lp = mapq_params(ref_len, locus_span, min_score, sub_band), loci_params(max_loci, drop_pct)
    check(lib().drm_hit_loci(ptr(mp), ptr(lp), ptr(i) if i.size else None, ptr(s) if s.size else None, ptr(c),
                             None if h is None else ptr(h), ptr(f), n, int(i.shape[1]), ptr(out), ptr(n_loci),
                             ptr(n_pass), ptr(l_ids), ptr(l_sc), ptr(l_rows), ptr(l_size)))
    return out, n_loci, n_pass, l_ids, l_sc, l_rows, l_size


def hit_loci_device(d_ids, d_scores, d_cnt, d_full, nreads, k, ref_len, max_loci, drop_pct=LOCI_DROP_DEFAULT,
                    d_head=None, locus_span=None, min_score=MAPQ_MIN_DEFAULT, sub_band=MAPQ_SUB_BAND, d_out=None,
                    d_n_loci=None, d_n_pass=None, d_loci_ids=None, d_loci_scores=None, d_loci_rows=None,
                    d_loci_size=None, stream=None):
    """drm_hit_loci_device: the same on device memory, enqueued on `stream`. Each d_* argument is a DeviceBuffer or a
    raw device address; an output left None is allocated. Returns the seven output DeviceBuffers in hit_loci's order;
    synchronise the stream before downloading them."""
    from .device import DeviceBuffer
    n, width = int(nreads), max(int(max_loci), 1)
    d_out = DeviceBuffer((n,), MAPQ_RESULT_DTYPE) if d_out is None else d_out
    d_n_loci = DeviceBuffer((n,), np.int32) if d_n_loci is None else d_n_loci
    d_n_pass = DeviceBuffer((n,), np.int32) if d_n_pass is None else d_n_pass
    d_loci_ids = DeviceBuffer((n, width), np.uint64) if d_loci_ids is None else d_loci_ids
    d_loci_scores = DeviceBuffer((n, width), np.int32) if d_loci_scores is None else d_loci_scores
    d_loci_rows = DeviceBuffer((n, width), np.int32) if d_loci_rows is None else d_loci_rows
    d_loci_size = DeviceBuffer((n, width), np.int32) if d_loci_size is None else d_loci_size
    mp, lp = mapq_params(ref_len, locus_span, min_score, sub_band), loci_params(max_loci, drop_pct)
    check(lib().drm_hit_loci_device(ptr(mp), ptr(lp), _addr(d_ids), _addr(d_scores), _addr(d_cnt), _addr(d_head),
                                    _addr(d_full), n, int(k), _addr(d_out), _addr(d_n_loci), _addr(d_n_pass),
                                    _addr(d_loci_ids), _addr(d_loci_scores), _addr(d_loci_rows), _addr(d_loci_size),
                                    stream.handle if stream is not None else None))
    return d_out, d_n_loci, d_n_pass, d_loci_ids, d_loci_scores, d_loci_rows, d_loci_size
