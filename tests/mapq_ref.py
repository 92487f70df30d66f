"""The mapping-quality definition of include/drm_hip.h (drm_hit_mapq, drm_mapq_value, drm_pair_mapq,
drm_pair_mapq_rescued) restated in plain Python: loops over Python integers with explicit "removed" sets, no packed keys
and no code shared with the kernel. The pair table's "proper" is pair_ref's."""
import numpy as np

import pair_ref as P

FIELDS = ("best", "best_score", "locus_rows", "sub_row", "sub_score", "n_sub", "mapq", "status")
PAIR_FIELDS = ("mapq1", "mapq2", "q_se1", "q_se2", "q_pe", "sub_pair")
NOTHING = dict(best=-1, best_score=0, locus_rows=0, sub_row=-1, sub_score=0, n_sub=0, mapq=0, status=1)


def mapq_value(s1, sub, n_sub, full, min_score):
    s1, sub, n_sub, full, min_score = int(s1), int(sub), int(n_sub), int(full), int(min_score)
    if s1 <= 0 or full <= 0:
        return 0
    c, s2 = min(s1, full), max(sub, min_score)
    if c <= s2:
        return 0
    q = (60 * (c - s2) * c) // ((c - min_score) * full)
    q -= 3 * ((n_sub + 1).bit_length() - 1)  # floor(log2(n_sub + 1))
    return min(max(q, 0), 60)


def same_locus(wa, wb, span):
    wa, wb = int(wa), int(wb)
    return (wa & 1) == (wb & 1) and abs((wa >> 1) - (wb >> 1)) < span


def _top(rows, scores):
    """The row of `rows` (ascending) with the largest score, the smallest row among equals; None for no rows."""
    top = None
    for j in rows:
        if top is None or scores[j] > scores[top]:
            top = j
    return top


def locus_scan(ids, scores, cnt, head, span, band):
    """(record without mapq as a dict, the set of locus 0's rows) of one list."""
    k = len(ids)
    c = min(max(int(cnt), 0), k)
    w = [int(x) for x in ids[:c]]
    s = [int(x) for x in scores[:c]]
    live = [j for j in range(c) if s[j] > 0]
    head = int(head)
    if head == -1:
        head = _top(live, s)
        if head is None:
            return dict(NOTHING), set()
    elif head not in live:
        return dict(NOTHING), set()
    locus0 = {j for j in live if same_locus(w[j], w[head], span)}
    removed = set(locus0)
    rec = dict(best=head, best_score=s[head], locus_rows=len(locus0), sub_row=-1, sub_score=0, n_sub=0, mapq=0,
               status=0)
    remain = [j for j in live if j not in removed]
    t = _top(remain, s)
    if t is not None:
        rec["sub_row"], rec["sub_score"] = t, s[t]
    while True:
        t = _top(remain, s)
        if t is None or s[t] < rec["sub_score"] - band:
            break
        rec["n_sub"] += 1
        removed |= {j for j in remain if same_locus(w[j], w[t], span)}
        remain = [j for j in remain if j not in removed]
    return rec, locus0


def hit_one(ids, scores, cnt, head, full, span, min_score, band):
    rec, _ = locus_scan(ids, scores, cnt, head, span, band)
    if rec["status"] == 0:
        rec["mapq"] = mapq_value(rec["best_score"], rec["sub_score"], rec["n_sub"], full, min_score)
    return rec


def hit_all(ids, scores, cnt, full, ref_len, head=None, locus_span=None, min_score=39, sub_band=2):
    """hit_one over a batch laid out as deepreadmapper_amd.hit_mapq takes it: a list of dicts, one per read."""
    span = ref_len if locus_span is None else locus_span
    return [hit_one(ids[r], scores[r], cnt[r], -1 if head is None else head[r], full[r], span, min_score, sub_band)
            for r in range(len(cnt))]


def pair_one(ids1, scores1, cnt1, ids2, scores2, cnt2, full1, full2, pair, ref_len, min_tlen, max_tlen,
             unpaired_penalty, span, min_score, band):
    """The drm_pair_mapq record of one pair; `pair` is its drm_pair_hits record as a dict."""
    out = dict.fromkeys(PAIR_FIELDS, 0)
    st = int(pair["status"])
    if st == 4:
        return out
    assert 0 <= st <= 3
    loci = []
    for m, (ids, sc, cnt, full, j) in enumerate(((ids1, scores1, cnt1, full1, int(pair["j1"])),
                                                 (ids2, scores2, cnt2, full2, int(pair["j2"])))):
        rec, locus0 = ({"status": 1}, set()) if j == -1 else locus_scan(ids, sc, cnt, j, span, band)
        q = mapq_value(rec["best_score"], rec["sub_score"], rec["n_sub"], full, min_score) if rec["status"] == 0 else 0
        out["q_se%d" % (m + 1)] = q
        loci.append(locus0)
    out["mapq1"], out["mapq2"] = out["q_se1"], out["q_se2"]
    if st != 0:
        return out
    k = len(ids1)
    c1, c2 = min(max(int(cnt1), 0), k), min(max(int(cnt2), 0), k)
    w1, s1 = [int(x) for x in ids1[:c1]], [int(x) for x in scores1[:c1]]
    w2, s2 = [int(x) for x in ids2[:c2]], [int(x) for x in scores2[:c2]]
    sub_pair = 0
    for a in range(c1):
        if s1[a] <= 0:
            continue
        for b in range(c2):
            if s2[b] <= 0 or (w1[a] & 1) == (w2[b] & 1) or (a in loci[0] and b in loci[1]):
                continue
            if s1[a] + s2[b] > sub_pair and P.is_proper(w1[a], s1[a], w2[b], s2[b], ref_len, min_tlen, max_tlen)[0]:
                sub_pair = s1[a] + s2[b]
    tops = max(x for x in s1 if x > 0) + max(x for x in s2 if x > 0)
    subo = max(sub_pair, tops - unpaired_penalty)
    q_pe = min(max(6 * (int(pair["score"]) - subo), 0), 60)
    out["sub_pair"], out["q_pe"] = sub_pair, q_pe
    for m in ("1", "2"):
        q = out["q_se" + m]
        out["mapq" + m] = q if q > q_pe else min(q_pe, q + 40)
    return out


def pair_all(ids1, scores1, cnt1, ids2, scores2, cnt2, full1, full2, pairs, ref_len, min_tlen=0, max_tlen=1000,
             unpaired_penalty=17, row_step=1, locus_span=None, min_score=39, sub_band=2):
    """pair_one over a batch laid out as deepreadmapper_amd.pair_mapq takes it; pairs[p] indexable by field name."""
    span = ref_len if locus_span is None else locus_span
    npairs = (len(cnt1) + row_step - 1) // row_step
    out = []
    for p in range(npairs):
        r = p * row_step
        out.append(pair_one(ids1[r], scores1[r], cnt1[r], ids2[r], scores2[r], cnt2[r], full1[r], full2[r],
                            {f: int(pairs[p][f]) for f in P.FIELDS}, ref_len, min_tlen, max_tlen, unpaired_penalty,
                            span, min_score, sub_band))
    return out


def rescued_one(status, rec, rescue_score, full1, full2, min_score):
    """drm_pair_mapq_rescued on one pair: the record (a dict over PAIR_FIELDS) after the rule."""
    out = dict(rec)
    if status == 5:
        out["mapq2"] = min(out["mapq1"], mapq_value(rescue_score, 0, 0, full2, min_score))
    elif status == 6:
        out["mapq1"] = min(out["mapq2"], mapq_value(rescue_score, 0, 0, full1, min_score))
    return out


def as_dicts(records, fields):
    return [{f: int(records[f][p]) for f in fields} for p in range(len(records))]


def assert_equal(got, want, what=""):
    """Every field of every record; names the first differing one."""
    if isinstance(got, np.ndarray):
        got = as_dicts(got, got.dtype.names)
    assert len(got) == len(want), (what, len(got), len(want))
    for p, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, p, g, w)
