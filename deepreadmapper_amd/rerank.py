"""Smith-Waterman rerank: drop-ins for calc_sw_score (src/utils/metrics.cpp:10-45), sw_reranker
(src/utils/reranker.cpp:3-51) and post_process_sw_static (src/utils/post_processor.cpp:454-549).
All scoring runs in the HIP kernels of libdrm_hip.so."""
import ctypes as C

import numpy as np

from ._native import DrmError, DRM_ERR_CANDS, check, lib, ptr


def _as_bytes(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def calc_sw_scores(seqs1, seqs2):
    """Batched calc_sw_score(seqs1[p], seqs2[p])."""
    a = [_as_bytes(s) for s in seqs1]
    b = [_as_bytes(s) for s in seqs2]
    if len(a) != len(b):
        raise ValueError("length mismatch")
    n = len(a)
    if n == 0:
        return np.zeros(0, dtype=np.int32)
    buf1 = np.frombuffer(b"".join(a) or b"\0", dtype=np.uint8).copy()
    buf2 = np.frombuffer(b"".join(b) or b"\0", dtype=np.uint8).copy()
    l1 = np.array([len(s) for s in a], dtype=np.int32)
    l2 = np.array([len(s) for s in b], dtype=np.int32)
    o1 = np.concatenate([[0], np.cumsum(l1[:-1], dtype=np.int64)]).astype(np.int64)
    o2 = np.concatenate([[0], np.cumsum(l2[:-1], dtype=np.int64)]).astype(np.int64)
    out = np.empty(n, dtype=np.int32)
    check(lib().drm_sw_scores(ptr(buf1), ptr(o1), ptr(l1), ptr(buf2), ptr(o2), ptr(l2), n, ptr(out)))
    return out


def calc_sw_score(seq1, seq2):
    return int(calc_sw_scores([seq1], [seq2])[0])


class _SwBand:
    """The opt-in banded SW of a window / genome handle (drm_refs_set_sw_band): 0 = the reference's full DP
    (default, bit-exact); 8, 16 or 32 = only the cells |i - j| <= band (non-parity, see include/drm_hip.h)."""

    @property
    def sw_band(self):
        b = C.c_int32(0)
        check(lib().drm_refs_get_sw_band(self._h, C.byref(b)))
        return b.value

    @sw_band.setter
    def sw_band(self, band):
        check(lib().drm_refs_set_sw_band(self._h, int(band)))

    @property
    def sw_chunk(self):
        """Queries per chunk of one SW rerank call (drm_refs_set_sw_chunk): -1 = the library's plan, 0 = one launch
        sequence on the caller's stream; the results are the same bytes in every mode."""
        n = C.c_int64(0)
        check(lib().drm_refs_get_sw_chunk(self._h, C.byref(n)))
        return n.value

    @sw_chunk.setter
    def sw_chunk(self, chunk):
        check(lib().drm_refs_set_sw_chunk(self._h, int(chunk)))


class WindowTable(_SwBand):
    """Device-resident `ref_seqs` (static lookup table of equal-length windows)."""

    def __init__(self, windows, device=0):
        if isinstance(windows, np.ndarray):
            arr = np.ascontiguousarray(windows, dtype=np.uint8)
        else:
            ws = [_as_bytes(w) for w in windows]
            L = len(ws[0]) if ws else 0
            if any(len(w) != L for w in ws):
                raise ValueError("static window table needs equal-length windows")
            arr = np.frombuffer(b"".join(ws), dtype=np.uint8).reshape(len(ws), L) if ws else np.zeros((0, 0), np.uint8)
        self.n_ref, self.ref_len = arr.shape
        h = C.c_void_p()
        check(lib().drm_refs_create(ptr(arr) if arr.size else None, self.n_ref, self.ref_len, self.ref_len,
                                    int(device), C.byref(h)))
        self._h = h.value

    @property
    def handle(self):
        return self._h

    def free(self):
        if self._h:
            check(lib().drm_refs_free(self._h))
            self._h = None

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().drm_refs_free(self._h)
        except Exception:
            pass


class GenomeTable(_SwBand):
    """Device-resident genome string for the dynamic lookup (use_dynamic): window id w is
    genome[w // 2 : w // 2 + ref_len], reverse-complemented when w is odd (find_sequence,
    src/utils/post_processor.cpp:47-64)."""

    def __init__(self, genome, ref_len, device=0):
        g = np.frombuffer(genome, dtype=np.uint8) if isinstance(genome, (bytes, bytearray)) else \
            np.ascontiguousarray(genome, dtype=np.uint8)
        self.glen, self.ref_len = int(g.size), int(ref_len)
        h = C.c_void_p()
        check(lib().drm_refs_create_genome(ptr(g) if g.size else None, g.size, int(ref_len), int(device), C.byref(h)))
        self._h = h.value

    @property
    def handle(self):
        return self._h

    def free(self):
        if self._h:
            check(lib().drm_refs_free(self._h))
            self._h = None

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self.free()
        except Exception:
            pass


def extract_fasta_sequence(path):
    """extract_FASTA_sequence (src/utils/parse_inputs.cpp:174-220) -> bytes."""
    n = C.c_int64(0)
    check(lib().drm_extract_fasta_sequence(str(path).encode(), None, C.byref(n)))
    out = np.empty(max(n.value, 1), dtype=np.uint8)
    n2 = C.c_int64(n.value)
    check(lib().drm_extract_fasta_sequence(str(path).encode(), ptr(out), C.byref(n2)))
    return bytes(out[:n.value])


def rerank_dynamic_arrays(genome_table, neighbors, query_seqs, stride, k, k_clusters):
    """Array form of post_process_sw_dynamic on a GenomeTable: (scores, ids, counts) like rerank_arrays."""
    nb = np.ascontiguousarray(neighbors, dtype=np.int64)
    nq, kk = nb.shape
    qbuf, qlen = query_seqs if isinstance(query_seqs, tuple) else pack_queries(query_seqs)
    scores = np.empty((nq, k), dtype=np.int32)
    ids = np.empty((nq, k), dtype=np.uint64)
    counts = np.empty(nq, dtype=np.int32)
    bad = C.c_int64(-1)
    check(lib().drm_post_process_sw_dynamic(genome_table.handle, ptr(nb), nq, kk, ptr(qbuf), ptr(qlen), qbuf.shape[1],
                                            int(stride), int(k), int(k_clusters), ptr(scores), ptr(ids), ptr(counts),
                                            C.byref(bad)))
    return scores, ids, counts


def post_process_sw_dynamic(neighbors, distances, ref_genome, query_seqs, ref_len, stride, k, k_clusters):
    """post_process_sw_dynamic (src/utils/post_processor.cpp:357-452): flattened (final_seqs,
    final_scores, final_ids); ref_genome is the genome string (bytes / str) or a GenomeTable."""
    g = ref_genome.encode() if isinstance(ref_genome, str) else ref_genome
    table = g if isinstance(g, GenomeTable) else GenomeTable(g, ref_len)
    nb = np.asarray([list(r) for r in neighbors], dtype=np.int64) if not isinstance(neighbors, np.ndarray) else neighbors
    try:
        scores, ids, counts = rerank_dynamic_arrays(table, nb, query_seqs, stride, k, k_clusters)
    except DrmError as e:
        raise RuntimeError(str(e)) from e
    seqs, sc, fid = [], [], []
    for i in range(len(counts)):
        for j in range(int(counts[i])):
            wid = int(ids[i, j])
            sc.append(int(scores[i, j]))
            fid.append(wid)
            if not isinstance(g, GenomeTable):
                pos = wid // 2
                w = g[pos:pos + ref_len] if pos + ref_len <= len(g) else b""
                if wid % 2 == 1 and w:
                    w = bytes(_COMP_TABLE[np.frombuffer(w, dtype=np.uint8)[::-1]])
                seqs.append(bytes(w))
    return seqs, sc, fid


_COMP_TABLE = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ATCGN", b"TAGCN"):
    _COMP_TABLE[_a] = _b


def pack_queries(query_seqs):
    qs = [_as_bytes(q) for q in query_seqs]
    stride = max([len(q) for q in qs] + [1])
    buf = np.zeros((len(qs), stride), dtype=np.uint8)
    for i, q in enumerate(qs):
        buf[i, :len(q)] = np.frombuffer(q, dtype=np.uint8)
    return buf, np.array([len(q) for q in qs], dtype=np.int32)


def rerank_arrays(table, neighbors, query_seqs, stride, k, k_clusters):
    """Array form of post_process_sw_static: returns (scores [nq,k] i32, ids [nq,k] u64, counts [nq])."""
    nb = np.ascontiguousarray(neighbors, dtype=np.int64)
    nq, kk = nb.shape
    qbuf, qlen = query_seqs if isinstance(query_seqs, tuple) else pack_queries(query_seqs)
    scores = np.empty((nq, k), dtype=np.int32)
    ids = np.empty((nq, k), dtype=np.uint64)
    counts = np.empty(nq, dtype=np.int32)
    bad = C.c_int64(-1)
    rc = lib().drm_post_process_sw_static(table.handle, ptr(nb), nq, kk, ptr(qbuf), ptr(qlen), qbuf.shape[1],
                                          int(stride), int(k), int(k_clusters), ptr(scores), ptr(ids), ptr(counts),
                                          C.byref(bad))
    check(rc)
    return scores, ids, counts


def post_process_sw_static(neighbors, distances, ref_seqs, query_seqs, ref_len, stride, k, k_clusters):
    """Reference-shaped result: flattened (final_seqs, final_scores, final_ids) over all queries
    (post_processor.cpp:533-548). Raises RuntimeError like the reference on k / candidate errors."""
    table = ref_seqs if isinstance(ref_seqs, WindowTable) else WindowTable(ref_seqs)
    nb = np.asarray([list(r) for r in neighbors], dtype=np.int64) if not isinstance(neighbors, np.ndarray) else neighbors
    try:
        scores, ids, counts = rerank_arrays(table, nb, query_seqs, stride, k, k_clusters)
    except DrmError as e:
        raise RuntimeError(str(e)) from e
    seqs, sc, fid = [], [], []
    for i in range(len(counts)):
        for j in range(int(counts[i])):
            wid = int(ids[i, j])
            sc.append(int(scores[i, j]))
            fid.append(wid)
            if not isinstance(ref_seqs, WindowTable):
                seqs.append(ref_seqs[wid])
    return seqs, sc, fid


def sw_reranker(cand_seqs, cand_ids, query_seq, k):
    """sw_reranker(cand_seqs, cand_ids, query_seq, k) -> (top_seqs, top_scores, top_ids)."""
    n = len(cand_seqs)
    if n == 0 or k == 0:
        return [], [], []
    scores = calc_sw_scores(cand_seqs, [query_seq] * n)
    if n < k:
        raise RuntimeError(f"Not enough candidates ({n} < {k})")
    order = partial_sort_order(scores, k)
    return [cand_seqs[i] for i in order], [int(scores[i]) for i in order], [cand_ids[i] for i in order]


def partial_sort_order(scores, k):
    """std::partial_sort order of reranker.cpp:38-40 computed on the device: the rerank kernel sorts
    candidate windows of a one-query table whose scores are the given ones."""
    scores = np.asarray(scores, dtype=np.int32)
    n = len(scores)
    # A window table whose window c scores exactly scores[c] against a query of 'A'*m:
    # window c = 'A'*scores[c] + 'C'*(L - scores[c]) with L = max score (calc_sw_score = run of A's).
    L = max(int(scores.max()) if n else 0, 1)
    if scores.min(initial=0) < 0:
        raise ValueError("scores must be >= 0")
    win = np.full((n, L), ord("C"), dtype=np.uint8)
    for c, s in enumerate(scores):
        win[c, :s] = ord("A")
    table = WindowTable(win)
    q = b"A" * L
    nb = np.arange(n, dtype=np.int64)[None, :]
    _, ids, _ = rerank_arrays(table, nb, [q], 1, k, n)
    table.free()
    return [int(i) for i in ids[0]]


# ------------------------------------------------------------------------------------------- SW alignment
# drm_sw_alignment (include/drm_hip.h)
SW_ALIGNMENT_DTYPE = np.dtype([(f, np.int32) for f in ("score", "ref_begin", "ref_end", "q_begin", "q_end", "nm",
                                                       "n_ops", "status")])


def _sw_align_call(table, wid, pq, qbuf, qlen, ops_stride):
    rec = np.zeros(len(wid), dtype=SW_ALIGNMENT_DTYPE)
    ops = np.zeros((len(wid), ops_stride), dtype=np.uint32)
    check(lib().drm_sw_align(table.handle, ptr(wid), ptr(pq), len(wid), ptr(qbuf), ptr(qlen), qbuf.shape[1],
                             len(qlen), ptr(rec), ptr(ops) if ops.size else None, int(ops_stride)))
    return rec, ops


def sw_scoring(scoring):
    """drm_sw_scoring (match, mismatch, gap_open, gap_extend) as the int32 array the C ABI reads."""
    s = np.array([int(x) for x in scoring], dtype=np.int32)
    if s.shape != (4,):
        raise ValueError("scoring is (match, mismatch, gap_open, gap_extend)")
    return s


def _sw_align_affine_call(table, scoring, flank, wid, pq, qbuf, qlen, ops_stride):
    rec = np.zeros(len(wid), dtype=SW_ALIGNMENT_DTYPE)
    ops = np.zeros((len(wid), ops_stride), dtype=np.uint32)
    check(lib().drm_sw_align_affine(table.handle, ptr(scoring), int(flank), ptr(wid), ptr(pq), len(wid), ptr(qbuf),
                                    ptr(qlen), qbuf.shape[1], len(qlen), ptr(rec), ptr(ops) if ops.size else None,
                                    int(ops_stride)))
    return rec, ops


def sw_align_arrays(table, window_ids, pair_query, query_seqs, ops_stride=16):
    """The alignment behind the rerank score (drm_sw_align): pair p aligns window window_ids[p] of a WindowTable
    or GenomeTable with query pair_query[p] of query_seqs (a list, or pack_queries' (buffer, lengths)). Returns
    (records, ops): a structured array (SW_ALIGNMENT_DTYPE) and, per pair, its BAM operation words
    (len << 4 | op, M = 0, I = 1, D = 2) in forward order. Pairs with more than ops_stride runs (status 2) are
    aligned again as a sub-list with a stride that cannot overflow, so every returned status is 0 or 1."""
    wid = np.ascontiguousarray(window_ids, dtype=np.uint64)
    pq = np.ascontiguousarray(pair_query, dtype=np.int64)
    if wid.shape != pq.shape or wid.ndim != 1:
        raise ValueError("window_ids and pair_query must be 1-d arrays of one length")
    qbuf, qlen = query_seqs if isinstance(query_seqs, tuple) else pack_queries(query_seqs)
    def call(w, q, stride):
        return _sw_align_call(table, w, q, qbuf, qlen, stride)
    rec, ops = call(wid, pq, ops_stride)
    return _retry_truncated(call, wid, pq, rec, ops, ops_stride, int(qbuf.shape[1]) + int(table.ref_len))


def _retry_truncated(call, wid, pq, rec, ops, ops_stride, full):
    """Per-pair operation lists of one alignment call; the pairs with more than ops_stride runs (status 2) are
    aligned again as a sub-list with the stride `full`, which cannot overflow."""
    out = [ops[p, :min(int(rec["n_ops"][p]), ops_stride)].copy() for p in range(len(wid))]
    again = np.flatnonzero(rec["status"] == 2)
    if len(again):
        rec2, ops2 = call(np.ascontiguousarray(wid[again]), np.ascontiguousarray(pq[again]), full)
        for x, p in enumerate(again):
            rec[p] = rec2[x]
            out[p] = ops2[x, :int(rec2["n_ops"][x])].copy()
    return rec, out


def sw_align_affine_arrays(table, window_ids, pair_query, query_seqs, scoring, flank=0, ops_stride=16):
    """The affine-gap alignment over a flanked region (drm_sw_align_affine): sw_align_arrays with a scoring
    (match, mismatch, gap_open, gap_extend), the last three penalties, and on a GenomeTable `flank` genome bases on
    either side of the window as the target (sw_align_region gives a pair's region; ref_begin / ref_end are relative
    to it). Pairs with more than ops_stride runs are aligned again, so every returned status is 0 or 1."""
    wid = np.ascontiguousarray(window_ids, dtype=np.uint64)
    pq = np.ascontiguousarray(pair_query, dtype=np.int64)
    if wid.shape != pq.shape or wid.ndim != 1:
        raise ValueError("window_ids and pair_query must be 1-d arrays of one length")
    qbuf, qlen = query_seqs if isinstance(query_seqs, tuple) else pack_queries(query_seqs)
    sc = sw_scoring(scoring)

    def call(w, q, stride):
        return _sw_align_affine_call(table, sc, flank, w, q, qbuf, qlen, stride)
    rec, ops = call(wid, pq, ops_stride)
    return _retry_truncated(call, wid, pq, rec, ops, ops_stride, int(qbuf.shape[1]) + int(table.ref_len) + 2 * int(flank))


def sw_clip(penalty, tags=(1, 1)):
    """drm_sw_clip (penalty, tag_prefix, tag_postfix) as the int32 array the C ABI reads."""
    c = np.array([int(penalty), int(tags[0]), int(tags[1])], dtype=np.int32)
    if c.shape != (3,):
        raise ValueError("tags is (tag_prefix, tag_postfix)")
    return c


def sw_align_affine_clip_arrays(table, window_ids, pair_query, query_seqs, scoring, clip, tags=(1, 1), flank=0,
                                ops_stride=16):
    """The end-aware affine-gap alignment (drm_sw_align_affine_clip): sw_align_affine_arrays with the clipping
    penalty `clip` (0..63) that an alignment pays for stopping short of either end of the read, the read being the
    query without its `tags` = (tag_prefix, tag_postfix) bytes. Records and words are of the same form; `score` is the
    plain affine score of the printed walk. Pairs with more than ops_stride runs are aligned again, so every returned
    status is 0 or 1."""
    wid = np.ascontiguousarray(window_ids, dtype=np.uint64)
    pq = np.ascontiguousarray(pair_query, dtype=np.int64)
    if wid.shape != pq.shape or wid.ndim != 1:
        raise ValueError("window_ids and pair_query must be 1-d arrays of one length")
    qbuf, qlen = query_seqs if isinstance(query_seqs, tuple) else pack_queries(query_seqs)
    sc, cl = sw_scoring(scoring), sw_clip(clip, tags)

    def call(w, q, stride):
        rec = np.zeros(len(w), dtype=SW_ALIGNMENT_DTYPE)
        ops = np.zeros((len(w), stride), dtype=np.uint32)
        check(lib().drm_sw_align_affine_clip(table.handle, ptr(sc), ptr(cl), int(flank), ptr(w), ptr(q), len(w),
                                             ptr(qbuf), ptr(qlen), qbuf.shape[1], len(qlen), ptr(rec),
                                             ptr(ops) if ops.size else None, int(stride)))
        return rec, ops
    rec, ops = call(wid, pq, ops_stride)
    return _retry_truncated(call, wid, pq, rec, ops, ops_stride, int(qbuf.shape[1]) + int(table.ref_len) + 2 * int(flank))


def sw_align_region(table, window_id, flank):
    """(start, length, reverse) of a window id's target region on a GenomeTable (drm_sw_align_region): the bytes
    genome[start : start + length], reverse-complemented when reverse; length 0 for a window past the genome end."""
    start, n, rev = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    check(lib().drm_sw_align_region(table.handle, int(window_id), int(flank), C.byref(start), C.byref(n), C.byref(rev)))
    return start.value, n.value, rev.value


def _sam_cigar_call(fn, record, ops, *args):
    r = np.zeros(1, dtype=SW_ALIGNMENT_DTYPE)
    r[0] = tuple(int(record[f]) for f in SW_ALIGNMENT_DTYPE.names)
    o = np.ascontiguousarray(ops, dtype=np.uint32)
    cap = 16 * (len(o) + 2) + 1
    buf = C.create_string_buffer(cap)
    pos = C.c_int64(0)
    check(fn(ptr(r), ptr(o) if o.size else None, *args, C.byref(pos), buf, cap))
    return pos.value, buf.value.decode()


def sam_cigar_region(record, ops, q_len, region_start, region_len, reverse, tags=(1, 1)):
    """(pos1, cigar) of one record relative to the region genome[region_start ..+ region_len)
    (drm_sam_cigar_region): sam_cigar's rules, pos1 = region_start + (region_len - ref_end if reverse else
    ref_begin) + 1, the CIGAR reversed when reverse."""
    return _sam_cigar_call(lib().drm_sam_cigar_region, record, ops, int(q_len), int(tags[0]), int(tags[1]),
                           int(region_start), int(region_len), int(bool(reverse)))


def sam_cigar(record, ops, q_len, ref_len, window_id, tags=(1, 1)):
    """(pos1, cigar) of one alignment record (drm_sam_cigar): 1-based leftmost position on the forward strand and
    the CIGAR with soft clips; both are flipped for an odd window id. `tags` are the bytes to drop from the query's
    ends (format_fastq's "<" and ">")."""
    return _sam_cigar_call(lib().drm_sam_cigar, record, ops, int(q_len), int(tags[0]), int(tags[1]), int(ref_len),
                           int(window_id))


# ------------------------------------------------------------------------------------------- MD words
# drm_sw_md (include/drm_hip.h)
SW_MD_DTYPE = np.dtype([(f, np.int32) for f in ("n_words", "n_match", "n_mismatch", "n_ins", "n_del", "status")])


def sw_align_md_arrays(table, window_ids, pair_query, query_seqs, records, ops, flank=0, md_stride=16):
    """The MD words of aligned pairs (drm_sw_align_md): pair p is window window_ids[p] against query pair_query[p] as
    in sw_align_arrays / sw_align_affine_arrays, `records` and `ops` what one of them returned for the same pairs
    (a SW_ALIGNMENT_DTYPE array and one operation list per pair) and `flank` the flank it aligned with. Returns
    (md_records, words): a structured array (SW_MD_DTYPE) and, per pair, its MD words ((value << 4) | kind: 0 a run of
    matches, 1 a mismatch, 2 a deleted base, the value of the last two being the reference byte). Pairs with more than
    md_stride words (status 2) are computed again with a stride that cannot overflow, so every returned status is 0,
    1 or 3."""
    wid = np.ascontiguousarray(window_ids, dtype=np.uint64)
    pq = np.ascontiguousarray(pair_query, dtype=np.int64)
    if wid.shape != pq.shape or wid.ndim != 1:
        raise ValueError("window_ids and pair_query must be 1-d arrays of one length")
    rec = np.ascontiguousarray(records, dtype=SW_ALIGNMENT_DTYPE)
    if rec.shape != wid.shape or len(ops) != len(wid):
        raise ValueError("one record and one operation list per pair")
    qbuf, qlen = query_seqs if isinstance(query_seqs, tuple) else pack_queries(query_seqs)
    lists = [np.ascontiguousarray(o, dtype=np.uint32).ravel() for o in ops]
    off = np.zeros(len(wid), dtype=np.int64)
    if len(lists) > 1:
        off[1:] = np.cumsum([len(o) for o in lists[:-1]])
    flat = np.concatenate(lists + [np.zeros(1, dtype=np.uint32)])

    def call(sel, stride):
        h = np.zeros(len(sel), dtype=SW_MD_DTYPE)
        words = np.zeros((len(sel), stride), dtype=np.uint32)
        w, q, r, o = (np.ascontiguousarray(x[sel]) for x in (wid, pq, rec, off))
        check(lib().drm_sw_align_md(table.handle, int(flank), ptr(w), ptr(q), len(sel), ptr(qbuf), ptr(qlen),
                                    qbuf.shape[1], len(qlen), ptr(r), ptr(flat), ptr(o), ptr(h),
                                    ptr(words) if words.size else None, int(stride)))
        return h, words
    every = np.arange(len(wid))
    h, words = call(every, int(md_stride))
    out = [words[p, :min(int(h["n_words"][p]), int(md_stride))].copy() for p in every]
    again = np.flatnonzero(h["status"] == 2)
    if len(again):
        h2, words2 = call(again, 2 * (int(table.ref_len) + 2 * int(flank)) + 1)
        for x, p in enumerate(again):
            h[p] = h2[x]
            out[p] = words2[x, :int(h2["n_words"][x])].copy()
    return h, out


def sam_md(md_record, words, reverse):
    """The MD:Z string of one pair's MD record and words (drm_sam_md), on the forward strand when `reverse` says the
    pair's region was a reverse complement."""
    h = np.zeros(1, dtype=SW_MD_DTYPE)
    h[0] = tuple(int(md_record[f]) for f in SW_MD_DTYPE.names)
    w = np.ascontiguousarray(words, dtype=np.uint32)
    cap = 12 * (len(w) + 1) + 1
    buf = C.create_string_buffer(cap)
    check(lib().drm_sam_md(ptr(h), ptr(w) if w.size else None, int(bool(reverse)), buf, cap))
    return buf.value.decode()


# ------------------------------------------------------------------------------------------- L2 rerank
def embed_windows(table, encoder, stream=None):
    """Fill the table's device embedding of every window with the read encoder (drm_refs_embed): the rows the
    reference's post_process_l2_static re-embeds per run (src/utils/post_processor.cpp:1075-1080)."""
    check(lib().drm_refs_embed(table.handle, encoder.handle, stream.handle if stream is not None else None))


def window_embeddings_ptr(table):
    """(device pointer, width) of the table's window embeddings (0, 0 before embed_windows)."""
    p, d = C.c_void_p(), C.c_int32(0)
    check(lib().drm_refs_embeddings(table.handle, C.byref(p), C.byref(d)))
    return p.value or 0, d.value


def l2_rerank_arrays(table, neighbors, query_embeddings, stride, k_clusters):
    """Array form of post_process_l2_static on an embedded WindowTable: (dists [nq,k_clusters] f32,
    ids [nq,k_clusters] u64, counts [nq])."""
    nb = np.ascontiguousarray(neighbors, dtype=np.int64)
    nq, kk = nb.shape
    qe = np.ascontiguousarray(query_embeddings, dtype=np.float32)
    if qe.shape[0] != nq:
        raise ValueError("one query embedding per neighbor row")
    dists = np.empty((nq, k_clusters), dtype=np.float32)
    ids = np.empty((nq, k_clusters), dtype=np.uint64)
    counts = np.empty(nq, dtype=np.int32)
    bad = C.c_int64(-1)
    check(lib().drm_post_process_l2_static(table.handle, ptr(nb), nq, kk, ptr(qe), qe.shape[1], int(stride),
                                           int(k_clusters), ptr(dists), ptr(ids), ptr(counts), C.byref(bad)))
    return dists, ids, counts


def post_process_l2_static(neighbors, distances, ref_seqs, query_seqs, ref_len, stride, k, query_embeddings,
                           vectorizer, k_clusters):
    """post_process_l2_static (src/utils/post_processor.cpp:1023-1162), the reference's live rerank
    (src/main.cpp:330): flattened (final_seqs, final_dists, final_ids), k_clusters rows per query
    (batch_reranker is called with k = k_clusters; `k` and `query_seqs` are unused there too). ref_seqs is a
    WindowTable or a list of windows; vectorizer an Encoder (embeds the table once on the device)."""
    table = ref_seqs if isinstance(ref_seqs, WindowTable) else WindowTable(ref_seqs)
    if window_embeddings_ptr(table)[0] == 0:
        embed_windows(table, getattr(vectorizer, "encoder", vectorizer))
    nb = np.asarray([list(r) for r in neighbors], dtype=np.int64) if not isinstance(neighbors, np.ndarray) else neighbors
    try:
        dists, ids, counts = l2_rerank_arrays(table, nb, query_embeddings, stride, k_clusters)
    except DrmError as e:
        raise RuntimeError(str(e)) from e
    seqs, dd, fid = [], [], []
    for i in range(len(counts)):
        for j in range(int(counts[i])):
            wid = int(ids[i, j])
            dd.append(float(dists[i, j]))
            fid.append(wid)
            if not isinstance(ref_seqs, WindowTable):
                seqs.append(ref_seqs[wid])
    return seqs, dd, fid


def l2_rerank_dynamic_arrays(genome_table, neighbors, query_embeddings, stride, k, k_clusters):
    """post_process_l2_dynamic's rerank (stride > 1) on an embedded GenomeTable: (dists [nq,k] f32,
    ids [nq,k] u64, counts [nq])."""
    nb = np.ascontiguousarray(neighbors, dtype=np.int64)
    nq, kk = nb.shape
    qe = np.ascontiguousarray(query_embeddings, dtype=np.float32)
    if qe.shape[0] != nq:
        raise ValueError("one query embedding per neighbor row")
    dists = np.empty((nq, k), dtype=np.float32)
    ids = np.empty((nq, k), dtype=np.uint64)
    counts = np.empty(nq, dtype=np.int32)
    bad = C.c_int64(-1)
    check(lib().drm_post_process_l2_dynamic(genome_table.handle, ptr(nb), nq, kk, ptr(qe), qe.shape[1], int(stride),
                                            int(k), int(k_clusters), ptr(dists), ptr(ids), ptr(counts), C.byref(bad)))
    return dists, ids, counts


def post_process_l2_dynamic(neighbors, distances, ref_genome, query_seqs, ref_len, stride, k, query_embeddings,
                            vectorizer, k_clusters):
    """post_process_l2_dynamic (src/utils/post_processor.cpp:553-750): flattened (final_seqs, final_dists,
    final_ids). At stride 1 the reference reranks nothing: each query's first min(k, kk) search neighbours with
    their search distances (:633-660). At stride > 1 the L2 rerank of l2_rerank_dynamic_arrays, k rows per query.
    ref_genome is the genome string (bytes / str) or a GenomeTable; vectorizer an Encoder or Vectorizer."""
    g = ref_genome.encode() if isinstance(ref_genome, str) else ref_genome
    table = g if isinstance(g, GenomeTable) else GenomeTable(g, ref_len)
    nb = np.asarray([list(r) for r in neighbors], dtype=np.int64) if not isinstance(neighbors, np.ndarray) else neighbors

    def window(wid):
        if isinstance(g, GenomeTable):
            return None
        pos = wid // 2
        w = g[pos:pos + ref_len] if pos + ref_len <= len(g) else b""
        if wid % 2 == 1 and w:
            w = bytes(_COMP_TABLE[np.frombuffer(w, dtype=np.uint8)[::-1]])
        return bytes(w)

    seqs, dd, fid = [], [], []
    if stride == 1:
        for i in range(nb.shape[0]):
            for j in range(min(k, nb.shape[1])):
                wid = int(nb[i, j]) & (2**64 - 1)
                fid.append(wid)
                dd.append(float(distances[i][j]))
                seqs.append(window(wid))
        return seqs, dd, fid
    if window_embeddings_ptr(table)[0] == 0:
        embed_windows(table, getattr(vectorizer, "encoder", vectorizer))
    try:
        dists, ids, counts = l2_rerank_dynamic_arrays(table, nb, query_embeddings, stride, k, k_clusters)
    except DrmError as e:
        raise RuntimeError(str(e)) from e
    for i in range(len(counts)):
        for j in range(int(counts[i])):
            wid = int(ids[i, j])
            dd.append(float(dists[i, j]))
            fid.append(wid)
            seqs.append(window(wid))
    return seqs, dd, fid
