"""drm_tlen_estimate (host only) against the Python restatement (tests/tlen_ref.py): hand-worked histograms -- one
spike, two spikes, a tight peak with far outliers, a spread so wide that S1 - 4R is negative, the sample threshold, the
first and the last bin, sums beyond 64 bits -- then 2,000 random sparse and dense histograms, every argument error, and
the parameter errors of drm_tlen_scan that are decided before any device is touched. No GPU."""
import numpy as np
import pytest

import tlen_ref as T


def _hist(nbins, counts):
    h = np.zeros(nbins, np.uint32)
    for t, c in counts.items():
        h[t] = c
    return h


def _both(h, min_samples=10):
    """The library's estimate, checked against the restatement's."""
    from deepreadmapper_amd import TLEN_ESTIMATE_FIELDS, tlen_estimate
    got = tlen_estimate(h, min_samples)
    assert tuple(TLEN_ESTIMATE_FIELDS) == T.ESTIMATE_FIELDS
    assert got == T.estimate(h, min_samples), (got, T.estimate(h, min_samples))
    return got


def test_all_samples_at_one_length():
    e = _both(_hist(1001, {300: 50}))
    assert e == dict(n=50, n_trim=50, p25=300, p50=300, p75=300, trim_lo=300, trim_hi=300, mean=300, sd=0, low=300,
                     high=300, status=0)


def test_two_spikes():
    # a[0..10) = 200, a[10..20) = 400: quartile indices 5, 10, 15; iqr 200; S1 = 6000, S2 = 2 * 10^6,
    # V = 20 * 2 * 10^6 - 36 * 10^6 = 4 * 10^6, R = 2000; mean 300.5 and sd 100.5 round half up to 300 and 100
    e = _both(_hist(1001, {200: 10, 400: 10}))
    assert e == dict(n=20, n_trim=20, p25=200, p50=400, p75=400, trim_lo=1, trim_hi=800, mean=300, sd=100, low=1,
                     high=1000, status=0)


def test_a_tight_peak_with_far_outliers():
    # quartile indices 50, 101, 152 of 203: 300, 300, 301; the trim [298, 303] drops the three at 9000; S1 = 60000,
    # S2 = 18000100, V = 20000, R = 141; low = min(297, floor(59436 / 200)), high = max(304, ceil(60564 / 200))
    e = _both(_hist(10001, {299: 50, 300: 100, 301: 50, 9000: 3}))
    assert e == dict(n=203, n_trim=200, p25=300, p50=300, p75=301, trim_lo=298, trim_hi=303, mean=300, sd=1, low=297,
                     high=304, status=0)


def test_low_is_clamped_where_the_spread_passes_the_mean():
    # S1 = 1010, V = 20 * 100010 - 1010^2 = 990^2, S1 - 4R = -2950: floor(-2950 / 20) = -148 where truncation gives
    # -147; either way below p25 - 3 * iqr's clamp at 1
    e = _both(_hist(1001, {1: 10, 100: 10}))
    assert e == dict(n=20, n_trim=20, p25=1, p50=100, p75=100, trim_lo=1, trim_hi=298, mean=51, sd=50, low=1,
                     high=397, status=0)
    assert (1010 - 4 * 990) // 20 == -148


def test_the_sample_threshold():
    nothing = dict.fromkeys(T.ESTIMATE_FIELDS, 0) | dict(status=1)
    assert _both(_hist(100, {5: 9})) == nothing
    assert _both(_hist(100, {5: 10}))["status"] == 0
    assert _both(_hist(100, {5: 3, 7: 4}), min_samples=8) == nothing
    assert _both(_hist(100, {5: 3, 7: 4}), min_samples=7)["n"] == 7
    assert _both(_hist(100, {5: 1}), min_samples=1)["low"] == 5
    # bin 0 is no template length: its count is not a sample
    assert _both(_hist(100, {0: 1000, 5: 9})) == nothing
    assert _both(_hist(100, {0: 1000, 5: 10}))["n"] == 10


def test_first_and_last_bin():
    for nbins in (2, 3, 1000, 2**16 + 1):
        e = _both(_hist(nbins, {1: 12}))
        assert (e["low"], e["high"], e["mean"], e["sd"], e["trim_lo"], e["trim_hi"]) == (1, 1, 1, 0, 1, 1)
        t = nbins - 1
        e = _both(_hist(nbins, {t: 12}))
        assert (e["low"], e["high"], e["mean"], e["sd"], e["trim_lo"], e["trim_hi"]) == (t, t, t, 0, t, t)


def test_sums_beyond_64_bits():
    c = 2**20
    e = _both(_hist(2**16 + 1, {1: c, 65535: c}))
    assert 2 * c * (c * (1 + 65535**2)) > 2**64  # x * S2
    # V = x^2 * 32767^2 exactly: R = 2^21 * 32767; mean 32768, sd 32767.5 rounded half up... of an exact half: 32767
    assert e == dict(n=2 * c, n_trim=2 * c, p25=1, p50=65535, p75=65535, trim_lo=1, trim_hi=65536, mean=32768,
                     sd=32767, low=1, high=65535 + 3 * 65534, status=0)
    # every bin full: n just below 2^48 and x * S2 close to 2^127
    full = np.full(2**16 + 1, 2**32 - 1, np.uint32)
    e = _both(full)
    assert e["n"] == 2**16 * (2**32 - 1) and e["status"] == 0


def test_random_histograms():
    rng = np.random.default_rng(2024)
    seen = set()
    for case in range(2000):
        kind = case % 4
        if kind == 0:    # dense, small counts: many ties at the quartiles
            nbins = int(rng.integers(2, 300))
            h = rng.integers(0, 4, size=nbins).astype(np.uint32)
        elif kind == 1:  # sparse over a long row
            nbins = int(rng.integers(2, 2**16 + 2))
            h = np.zeros(nbins, np.uint32)
            at = rng.integers(0, nbins, size=int(rng.integers(1, 12)))
            h[at] = rng.integers(1, 50, size=len(at))
        elif kind == 2:  # a library: a peak with a tail and a few outliers
            nbins = 10001
            h = np.zeros(nbins, np.uint32)
            t = np.clip(rng.normal(rng.integers(200, 600), rng.integers(1, 80), size=400).astype(np.int64), 0, nbins - 1)
            np.add.at(h, t, 1)
            np.add.at(h, rng.integers(0, nbins, size=int(rng.integers(0, 20))), 1)
        else:            # counts up to 2^32 - 1
            nbins = int(rng.integers(2, 2000))
            h = np.zeros(nbins, np.uint32)
            at = rng.integers(0, nbins, size=int(rng.integers(1, 30)))
            h[at] = rng.integers(1, 2**32, size=len(at), dtype=np.uint64).astype(np.uint32)
        e = _both(h, int(rng.integers(1, 30)))
        seen.add((e["status"], e["low"] == 1, e["sd"] == 0))
    assert len(seen) >= 4  # both statuses, clamped and unclamped low, zero and non-zero sd


def test_estimate_argument_errors():
    from deepreadmapper_amd import DrmError, tlen_estimate
    from deepreadmapper_amd._native import DRM_ERR_ARG, lib, ptr
    h = _hist(100, {50: 20})
    out = np.zeros(16, np.int64)
    for args in ((None, 100, 10, ptr(out)), (ptr(h), 100, 10, None), (ptr(h), 1, 10, ptr(out)),
                 (ptr(h), 0, 10, ptr(out)), (ptr(h), -5, 10, ptr(out)), (ptr(h), 2**16 + 2, 10, ptr(out)),
                 (ptr(h), 100, 0, ptr(out)), (ptr(h), 100, -1, ptr(out))):
        assert lib().drm_tlen_estimate(*args) == DRM_ERR_ARG, args
        assert lib().drm_last_error()
        assert not out.any()  # nothing written
    with pytest.raises(DrmError) as e:
        tlen_estimate(h[:1])
    assert e.value.code == DRM_ERR_ARG
    with pytest.raises(DrmError):
        tlen_estimate(h, 0)
    assert tlen_estimate(h)["mean"] == 50  # a valid call right after them


def test_scan_parameter_errors_need_no_device():
    from deepreadmapper_amd import DrmError, tlen_scan
    from deepreadmapper_amd._native import DRM_ERR_ARG, DRM_ERR_UNSUPPORTED, lib, ptr
    ids, sc = np.full((1, 2), 200, np.uint64), np.full((1, 2), 50, np.int32)
    cnt, full = np.array([2], np.int32), np.array([50], np.int32)
    args = (ids, sc, cnt, ids, sc, cnt, full, full)
    for bad in (dict(min_mapq=-1), dict(min_mapq=61), dict(max_scan=149), dict(max_scan=2**16 + 1), dict(ref_len=0),
                dict(ref_len=2**20 + 1), dict(locus_span=0), dict(min_score=-1), dict(min_score=2**20 + 1),
                dict(sub_band=-1), dict(sub_band=2**20 + 1)):
        prm = dict(dict(ref_len=150), **bad)
        with pytest.raises(DrmError) as e:
            tlen_scan(*args, **prm)
        assert e.value.code == DRM_ERR_ARG, (bad, str(e.value))
    wide = (np.zeros((1, 1025), np.uint64), np.zeros((1, 1025), np.int32), cnt)
    with pytest.raises(DrmError) as e:
        tlen_scan(*wide, *wide, full, full, 150)
    assert e.value.code == DRM_ERR_UNSUPPORTED
    # the scores of counted rows are checked on the host, before any upload
    for s in (-1, 2**20 + 1):
        bad_sc = sc.copy()
        bad_sc[0, 1] = s
        for a in ((ids, bad_sc, cnt, ids, sc, cnt), (ids, sc, cnt, ids, bad_sc, cnt)):
            with pytest.raises(DrmError) as e:
                tlen_scan(*a, full, full, 150)
            assert e.value.code == DRM_ERR_ARG
    # what the wrapper never passes: negative npairs, row_step 0, null parameters, null lists, a null histogram
    mp, tp = np.array([150, 150, 39, 2], np.int32), np.array([20, 10000], np.int32)
    hist = np.full(3 * 10001, 7, np.uint32)
    good = [ptr(mp), ptr(tp), ptr(ids), ptr(sc), ptr(cnt), ptr(ids), ptr(sc), ptr(cnt), ptr(full), ptr(full), 1, 2, 1,
            None, ptr(hist)]
    for at, value in ((0, None), (1, None), (10, -1), (12, 0), (14, None), (2, None), (3, None), (4, None), (5, None),
                      (6, None), (7, None), (8, None), (9, None)):
        a = list(good)
        a[at] = value
        assert lib().drm_tlen_scan(*a) == DRM_ERR_ARG, at
        assert (hist == 7).all()
    # no pairs: valid without a device, and the host form zeroes the histogram
    a = list(good)
    a[10] = 0
    assert lib().drm_tlen_scan(*a) == 0 and not hist.any()
    samples, h = tlen_scan(np.zeros((0, 4)), np.zeros((0, 4)), [], np.zeros((0, 4)), np.zeros((0, 4)), [], [], [], 150)
    assert len(samples) == 0 and h.shape == (3, 10001) and not h.any()
