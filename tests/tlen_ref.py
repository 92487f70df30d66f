"""The template-length definitions of include/drm_hip.h (drm_tlen_scan, drm_tlen_estimate) restated in plain Python:
the per-pair class and template length on top of mapq_ref's hit_one (the locus scan and the MAPQ of one list from its
top hit), and the estimator on Python's big integers with math.isqrt, from the sorted samples themselves where the C
code walks the histogram."""
import math

import numpy as np

import mapq_ref as M

SAMPLE_FIELDS = ("cls", "tlen", "mapq1", "mapq2")
ESTIMATE_FIELDS = ("n", "n_trim", "p25", "p50", "p75", "trim_lo", "trim_hi", "mean", "sd", "low", "high", "status")


def scan_one(ids1, scores1, cnt1, ids2, scores2, cnt2, full1, full2, ref_len, min_mapq, max_scan, span, min_score,
             band):
    """The drm_tlen_sample of one pair as a dict."""
    recs = [M.hit_one(ids, sc, cnt, -1, full, span, min_score, band)
            for ids, sc, cnt, full in ((ids1, scores1, cnt1, full1), (ids2, scores2, cnt2, full2))]
    out = dict(cls=0, tlen=0, mapq1=recs[0]["mapq"], mapq2=recs[1]["mapq"])
    if not all(r["status"] == 0 and r["mapq"] >= min_mapq for r in recs):
        return out
    w1, w2 = int(ids1[recs[0]["best"]]), int(ids2[recs[1]["best"]])
    if (w1 & 1) == (w2 & 1):
        cls, t = 3, abs((w1 >> 1) - (w2 >> 1)) + ref_len
    else:
        f, r = (w2, w1) if w1 & 1 else (w1, w2)
        d = (r >> 1) - (f >> 1)
        cls, t = (1, d + ref_len) if d >= 0 else (2, -d + ref_len)
    if t > max_scan:
        cls, t = 4, 0
    out["cls"], out["tlen"] = cls, t
    return out


def scan_all(ids1, scores1, cnt1, ids2, scores2, cnt2, full1, full2, ref_len, min_mapq=20, max_scan=None, row_step=1,
             locus_span=None, min_score=39, sub_band=2):
    """scan_one over a batch laid out as deepreadmapper_amd.tlen_scan takes it: (samples as a list of dicts, the
    histogram [3, max_scan + 1] of Python-counted bins)."""
    span = ref_len if locus_span is None else locus_span
    max_scan = max(ref_len, 10000) if max_scan is None else max_scan
    npairs = (len(cnt1) + row_step - 1) // row_step
    hist = np.zeros((3, max_scan + 1), dtype=np.uint32)
    out = []
    for p in range(npairs):
        r = p * row_step
        s = scan_one(ids1[r], scores1[r], cnt1[r], ids2[r], scores2[r], cnt2[r], full1[r], full2[r], ref_len, min_mapq,
                     max_scan, span, min_score, sub_band)
        if 1 <= s["cls"] <= 3:
            hist[s["cls"] - 1, s["tlen"]] += 1
        out.append(s)
    return out, hist


def estimate(hist_row, min_samples=10):
    """drm_tlen_estimate as a dict over ESTIMATE_FIELDS."""
    nbins = len(hist_row)
    count = {t: int(hist_row[t]) for t in range(1, nbins) if int(hist_row[t])}
    n = sum(count.values())
    if n < min_samples:
        return dict.fromkeys(ESTIMATE_FIELDS, 0) | dict(status=1)

    def at(idx):  # a[idx] of the ascending samples
        for t in sorted(count):
            idx -= count[t]
            if idx < 0:
                return t
    p25, p50, p75 = (at(min(n - 1, q * n // 4)) for q in (1, 2, 3))
    iqr = p75 - p25
    trim_lo, trim_hi = max(1, p25 - 2 * iqr), min(nbins - 1, p75 + 2 * iqr)
    kept = {t: c for t, c in count.items() if trim_lo <= t <= trim_hi}
    x, s1, s2 = sum(kept.values()), sum(t * c for t, c in kept.items()), sum(t * t * c for t, c in kept.items())
    v = x * s2 - s1 * s1
    assert x >= 1 and v >= 0
    r = math.isqrt(v)
    return dict(n=n, n_trim=x, p25=p25, p50=p50, p75=p75, trim_lo=trim_lo, trim_hi=trim_hi,
                mean=(2 * s1 + x) // (2 * x), sd=(2 * r + x) // (2 * x),
                low=max(1, min(p25 - 3 * iqr, (s1 - 4 * r) // x)),  # // floors toward minus infinity
                high=max(p75 + 3 * iqr, -((-(s1 + 4 * r)) // x)), status=0)
