"""The mate-pairing definition of include/drm_hip.h (drm_pair_hits) restated in plain Python: loops over the k x k
table of combinations with Python integers, no packed keys and no code shared with the kernel."""
import numpy as np

FIELDS = ("j1", "j2", "score", "tlen", "n_proper", "status")


def _clamp(c, k):
    return min(max(int(c), 0), k)


def _top(scores, cnt):
    """The live row of largest score, the smallest row among equals; None when no row is live."""
    top = None
    for j in range(cnt):
        if int(scores[j]) > 0 and (top is None or int(scores[j]) > int(scores[top])):
            top = j
    return top


def is_proper(w1, s1, w2, s2, ref_len, min_tlen, max_tlen):
    """(proper, T) of one combination of hit (w1, s1) of mate 1 with hit (w2, s2) of mate 2."""
    w1, w2 = int(w1), int(w2)
    if int(s1) <= 0 or int(s2) <= 0 or (w1 & 1) == (w2 & 1):
        return False, 0
    f, r = (w2, w1) if w1 & 1 else (w1, w2)
    pf, pr = f >> 1, r >> 1
    if pf > pr:
        return False, 0
    t = pr + ref_len - pf
    return min_tlen <= t <= max_tlen, t


def pair_one(ids1, scores1, cnt1, ids2, scores2, cnt2, ref_len, min_tlen=0, max_tlen=1000, unpaired_penalty=17):
    """The record of one pair as a dict over FIELDS; ids / scores are the k rows of each mate's list."""
    k = len(ids1)
    c1, c2 = _clamp(cnt1, k), _clamp(cnt2, k)
    n_proper, best = 0, None  # best = (sum, j1, j2, T)
    # Python integers once per list (the k = 1024 table has 2^20 cells); the cell test below is is_proper's
    w1s, s1s = [int(x) for x in ids1[:c1]], [int(x) for x in scores1[:c1]]
    w2s, s2s = [int(x) for x in ids2[:c2]], [int(x) for x in scores2[:c2]]
    for j1 in range(c1):
        w1, s1 = w1s[j1], s1s[j1]
        if s1 <= 0:
            continue
        for j2 in range(c2):
            w2, s2 = w2s[j2], s2s[j2]
            if s2 <= 0 or (w1 & 1) == (w2 & 1):
                continue
            pf, pr = (w2 >> 1, w1 >> 1) if w1 & 1 else (w1 >> 1, w2 >> 1)
            t = pr + ref_len - pf
            if pf > pr or t < min_tlen or t > max_tlen:
                continue
            n_proper += 1
            if best is None or s1 + s2 > best[0]:  # row order: the first of equal sums has the smallest j1, then j2
                best = (s1 + s2, j1, j2, t)
    t1, t2 = _top(scores1, c1), _top(scores2, c2)
    rec = dict(j1=-1, j2=-1, score=0, tlen=0, n_proper=n_proper, status=4)
    if t1 is not None and t2 is not None:
        tops = int(scores1[t1]) + int(scores2[t2])
        if best is not None and best[0] >= tops - unpaired_penalty:
            rec.update(j1=best[1], j2=best[2], score=best[0], tlen=best[3], status=0)
        else:
            rec.update(j1=t1, j2=t2, score=tops, status=1)
    elif t1 is not None:
        rec.update(j1=t1, score=int(scores1[t1]), status=2)
    elif t2 is not None:
        rec.update(j2=t2, score=int(scores2[t2]), status=3)
    return rec


def pair_all(ids1, scores1, cnt1, ids2, scores2, cnt2, ref_len, min_tlen=0, max_tlen=1000, unpaired_penalty=17,
             row_step=1):
    """pair_one over a batch laid out as deepreadmapper_amd.pair_hits takes it: list of dicts, one per pair."""
    npairs = (len(cnt1) + row_step - 1) // row_step
    return [pair_one(ids1[p * row_step], scores1[p * row_step], cnt1[p * row_step], ids2[p * row_step],
                     scores2[p * row_step], cnt2[p * row_step], ref_len, min_tlen, max_tlen, unpaired_penalty)
            for p in range(npairs)]


def as_dicts(records):
    """A structured result array of the package as the list of dicts pair_all returns."""
    return [{f: int(records[f][p]) for f in FIELDS} for p in range(len(records))]


def assert_equal(got, want, what=""):
    """Every field of every record; names the first differing pair."""
    got = as_dicts(got) if isinstance(got, np.ndarray) else got
    assert len(got) == len(want), (what, len(got), len(want))
    for p, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, p, g, w)
