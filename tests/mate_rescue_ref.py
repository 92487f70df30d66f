"""Plain Python/numpy restatement of the mate rescue defined in include/drm_hip.h (drm_mate_rescue,
drm_mate_rescue_region, drm_mate_rescue_window, drm_pair_rescue_choose) -- a helper for the tests, not a test.
Written from the header text with Python integers; it shares nothing with the C++ or HIP code. The recurrence is
sw_align_affine_ref's restatement of drm_sw_align_affine's, which the header says it is."""
import numpy as np

from sw_align_affine_ref import dp_matrices
from sw_align_ref import revcomp

FIELDS = ("region_start", "region_len", "reverse", "score", "ref_end", "q_end", "status")
PAIR_FIELDS = ("j1", "j2", "score", "tlen", "n_proper", "status")
MAX_ROWS = 2048


def d_range(ref_len, min_tlen, max_tlen):
    return max(0, min_tlen - ref_len), max_tlen - ref_len


def supported(ref_len, min_tlen, max_tlen):
    dlo, dhi = d_range(ref_len, min_tlen, max_tlen)
    return dhi - dlo + ref_len <= MAX_ROWS


def region(glen, ref_len, anchor, min_tlen=0, max_tlen=1000):
    """(start, length, reverse) of the rescue region of anchor id `anchor` on a genome of glen bases."""
    anchor = int(anchor)
    a, rev = anchor >> 1, 1 - (anchor & 1)
    dlo, dhi = d_range(ref_len, min_tlen, max_tlen)
    if a + ref_len > glen or dhi < dlo:
        return 0, 0, rev
    if anchor & 1 == 0:
        s, e = min(glen, a + dlo), min(glen, a + dhi + ref_len)
    else:
        s, e = max(0, a - dhi), min(glen, a - dlo + ref_len)
    if e <= s:
        return 0, 0, rev
    return s, e - s, rev


def region_bytes(genome, ref_len, anchor, min_tlen=0, max_tlen=1000):
    g = bytes(genome)
    s, n, rev = region(len(g), ref_len, anchor, min_tlen, max_tlen)
    r = g[s:s + n]
    return revcomp(r) if rev else r


def scan(w, q, scoring):
    """(score, ref_end, q_end) of the query q over the oriented region bytes w: the largest H, and among the cells
    that hold it the smallest row, then the smallest column; (0, 0, 0) when nothing scores."""
    if len(w) == 0 or len(q) == 0:
        return 0, 0, 0
    H, _, _ = dp_matrices(w, q, scoring)
    score = int(H.max())
    if score == 0:
        return 0, 0, 0
    cells = np.argwhere(H == score)  # row-major: smallest i first, then smallest j
    return score, int(cells[0][0]), int(cells[0][1])


def rescue_one(genome, ref_len, anchor, query, scoring=(1, 1, 0, 1), min_tlen=0, max_tlen=1000):
    """The record of one task as a dict over FIELDS; query = None stands for a task_query outside [0, nq)."""
    g = bytes(genome)
    s, n, rev = region(len(g), ref_len, anchor, min_tlen, max_tlen)
    rec = dict(region_start=s, region_len=n, reverse=rev, score=0, ref_end=0, q_end=0, status=1)
    if query is None:
        return rec
    score, i, j = scan(region_bytes(g, ref_len, anchor, min_tlen, max_tlen), bytes(query), scoring)
    if score > 0:
        rec.update(score=score, ref_end=i, q_end=j, status=0)
    return rec


def window(rec, ref_len, glen):
    """The window id under which the aligners find a status-0 record."""
    assert rec["status"] == 0
    if rec["reverse"]:
        p = rec["region_start"] + rec["region_len"] - rec["ref_end"]
    else:
        p = rec["region_start"] + rec["ref_end"] - ref_len
    p = min(max(p, 0), glen - ref_len)
    return 2 * p + (1 if rec["reverse"] else 0)


def choose(pair, s1, s2, anchor1, anchor2, rA, rB, ref_len, glen, unpaired_penalty=17, min_score=0):
    """(pair record dict, rescued window id) by drm_pair_rescue_choose's rules; rA / rB are record dicts or None."""
    out = dict(pair)

    def valid(r):
        return r is not None and r["status"] == 0 and r["score"] >= min_score
    cands = []  # (sum, record, anchor, status); rA first, so that it wins a tie
    if pair["status"] == 1:
        need = s1 + s2 - unpaired_penalty
        if valid(rA) and s1 + rA["score"] >= need:
            cands.append((s1 + rA["score"], rA, anchor1, 5))
        if valid(rB) and rB["score"] + s2 >= need:
            cands.append((rB["score"] + s2, rB, anchor2, 6))
    elif pair["status"] == 2 and valid(rA):
        cands.append((s1 + rA["score"], rA, anchor1, 5))
    elif pair["status"] == 3 and valid(rB):
        cands.append((rB["score"] + s2, rB, anchor2, 6))
    if not cands:
        return out, 0
    total, r, anchor, status = max(cands, key=lambda c: c[0])  # max keeps the first of equal sums
    wr = window(r, ref_len, glen)
    anchor = int(anchor)
    f, rv = (wr, anchor) if anchor & 1 else (anchor, wr)
    out.update(status=status, score=total, tlen=(rv >> 1) + ref_len - (f >> 1))
    out["j2" if status == 5 else "j1"] = -1
    return out, wr


def as_dicts(records, fields=FIELDS):
    return [{f: int(records[f][p]) for f in fields} for p in range(len(records))]


def assert_equal(got, want, what=""):
    """Every field of every record; names the first differing task."""
    got = as_dicts(got) if isinstance(got, np.ndarray) else got
    assert len(got) == len(want), (what, len(got), len(want))
    for p, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, p, g, w)
