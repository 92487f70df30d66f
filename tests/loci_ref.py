"""The locus-list definition of include/drm_hip.h (drm_hit_loci) restated in plain Python: loops over Python integers
with an explicit list of the rows that remain, no packed keys and no code shared with the kernel. "Same locus", the
top of a set and the MAPQ formula are mapq_ref's."""
import numpy as np

import mapq_ref as M

EMPTY_ID = 2**64 - 1
EMPTY = (EMPTY_ID, 0, -1, 0)  # (id, score, row, size) of a slot at or beyond n_loci


def loci_one(ids, scores, cnt, head, full, span, min_score, band, max_loci, drop_pct):
    """(MAPQ record as a dict, n_loci, n_pass, [(id, score, row, size)] * max_loci) of one list."""
    k = len(ids)
    c = min(max(int(cnt), 0), k)
    w = [int(x) for x in ids[:c]]
    s = [int(x) for x in scores[:c]]
    live = [j for j in range(c) if s[j] > 0]
    head = int(head)
    if head == -1:
        head = M._top(live, s)
    if head is None or head not in live:
        return dict(M.NOTHING), 0, 0, [EMPTY] * max_loci
    locus0 = [j for j in live if M.same_locus(w[j], w[head], span)]
    best_score = s[head]
    slots = [(w[head], best_score, head, len(locus0))]
    n_pass = 1
    remain = [j for j in live if j not in locus0]
    rec = dict(best=head, best_score=best_score, locus_rows=len(locus0), sub_row=-1, sub_score=0, n_sub=0, mapq=0,
               status=0)
    first = True
    while remain:
        t = M._top(remain, s)
        if first:
            rec["sub_row"], rec["sub_score"] = t, s[t]
            first = False
        counts_sub = s[t] >= rec["sub_score"] - band
        passes = s[t] >= min_score and 100 * s[t] >= drop_pct * best_score
        if not counts_sub and not passes:
            break
        gone = [j for j in remain if M.same_locus(w[j], w[t], span)]
        if counts_sub:
            rec["n_sub"] += 1
        if passes:
            n_pass += 1
            if len(slots) < max_loci:
                slots.append((w[t], s[t], t, len(gone)))
        remain = [j for j in remain if j not in gone]
    rec["mapq"] = M.mapq_value(best_score, rec["sub_score"], rec["n_sub"], full, min_score)
    n_loci = len(slots)
    return rec, n_loci, n_pass, slots + [EMPTY] * (max_loci - n_loci)


def loci_all(ids, scores, cnt, full, ref_len, max_loci, drop_pct=80, head=None, locus_span=None, min_score=39,
             sub_band=2):
    """loci_one over a batch laid out as deepreadmapper_amd.hit_loci takes it: one tuple per read."""
    span = ref_len if locus_span is None else locus_span
    return [loci_one(ids[r], scores[r], cnt[r], -1 if head is None else head[r], full[r], span, min_score, sub_band,
                     max_loci, drop_pct) for r in range(len(cnt))]


def assert_equal(got, want, what=""):
    """got = hit_loci's seven arrays, want = loci_all's list: every field of every record, both counts and every slot
    of every read; names the first difference."""
    rec, n_loci, n_pass, l_ids, l_sc, l_rows, l_size = got
    assert len(rec) == len(want) == len(n_loci) == len(n_pass), (what, len(rec), len(want))
    assert rec.dtype.names == M.FIELDS
    for r, (wrec, wn, wp, wslots) in enumerate(want):
        grec = {f: int(rec[f][r]) for f in M.FIELDS}
        assert grec == wrec, (what, r, grec, wrec)
        assert (int(n_loci[r]), int(n_pass[r])) == (wn, wp), (what, r, int(n_loci[r]), int(n_pass[r]), wn, wp)
        gslots = [(int(l_ids[r, j]), int(l_sc[r, j]), int(l_rows[r, j]), int(l_size[r, j]))
                  for j in range(l_ids.shape[1])]
        assert gslots == wslots, (what, r, gslots, wslots)
    assert l_ids.dtype == np.uint64 and l_sc.dtype == l_rows.dtype == l_size.dtype == np.int32
