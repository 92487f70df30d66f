"""CPU tests of the mate rescue's host-only entry points (include/drm_hip.h): drm_mate_rescue_region,
drm_mate_rescue_window and drm_pair_rescue_choose against the plain restatement of tests/mate_rescue_ref.py, which is
itself pinned to hand-worked cases first. (The scan runs on the GPU: tests/test_gpu_mate_rescue.py.)"""
import itertools

import numpy as np
import pytest

import mate_rescue_ref as R
from deepreadmapper_amd import DrmError, mate_rescue_region, mate_rescue_window, pair_rescue_choose
from deepreadmapper_amd._native import DRM_ERR_ARG, DRM_ERR_UNSUPPORTED

REF_LEN = 150


def F(pos):
    """Window id of a forward hit at genome position pos."""
    return 2 * pos


def Rv(pos):
    return 2 * pos + 1


def _codes():
    return DRM_ERR_ARG, DRM_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------ 1. the restatement
def test_ref_region_hand_worked():
    # forward anchor at 1000, default 0..1000: the mate is a reverse hit at 1000 .. 1850, region [1000, 2000)
    assert R.region(10_000, 150, F(1000)) == (1000, 1000, 1)
    # reverse anchor at 1000: the mate is a forward hit at 150 .. 1000, region [150, 1150)
    assert R.region(10_000, 150, Rv(1000)) == (150, 1000, 0)
    # min_tlen above ref_len moves the near edge: dlo = 50
    assert R.region(10_000, 150, F(1000), 200, 1000) == (1050, 950, 1)
    assert R.region(10_000, 150, Rv(1000), 200, 1000) == (150, 950, 0)
    # min_tlen below ref_len does not: dlo = 0
    assert R.region(10_000, 150, F(1000), 100, 1000) == (1000, 1000, 1)
    # clamped at either genome end
    assert R.region(1500, 150, F(1000)) == (1000, 500, 1)
    assert R.region(10_000, 150, Rv(300)) == (0, 450, 0)
    # empty: anchor past the end, dhi < dlo, a forward anchor whose near edge is the genome end
    assert R.region(1100, 150, F(1000)) == (0, 0, 1)
    assert R.region(1100, 150, Rv(1000)) == (0, 0, 0)
    assert R.region(10_000, 150, F(1000), 0, 149) == (0, 0, 1)
    assert R.region(1150, 150, F(1000), 300, 1000) == (0, 0, 1)


def test_ref_window_hand_worked():
    # forward region [150, 1150), the alignment ends in row 400: its last base is genome[549], the window 400 .. 549
    rec = dict(region_start=150, region_len=1000, reverse=0, score=100, ref_end=400, q_end=151, status=0)
    assert R.window(rec, 150, 10_000) == F(400)
    # reversed region [1000, 2000), oriented row 400 is genome[1599]: the window starts there
    rec = dict(region_start=1000, region_len=1000, reverse=1, score=100, ref_end=400, q_end=151, status=0)
    assert R.window(rec, 150, 10_000) == Rv(1600)
    # clamped at 0 and at glen - ref_len
    rec = dict(region_start=0, region_len=450, reverse=0, score=100, ref_end=100, q_end=101, status=0)
    assert R.window(rec, 150, 10_000) == F(0)
    rec = dict(region_start=1000, region_len=500, reverse=1, score=100, ref_end=40, q_end=41, status=0)
    assert R.window(rec, 150, 1500) == Rv(1350)


def test_ref_choose_hand_worked():
    glen = 10_000
    pair = dict(j1=3, j2=4, score=250, tlen=0, n_proper=0, status=1)
    rA = dict(region_start=1000, region_len=1000, reverse=1, score=140, ref_end=400, q_end=151, status=0)
    # anchored on mate 1's forward hit at 1000: mate 2 rescued at 1600 on the reverse strand, T = 1600 + 150 - 1000
    out, w = R.choose(pair, 130, 120, F(1000), Rv(7000), rA, None, 150, glen)
    assert (out, w) == (dict(j1=3, j2=-1, score=270, tlen=750, n_proper=0, status=5), Rv(1600))
    rB = dict(region_start=5850, region_len=1000, reverse=0, score=150, ref_end=300, q_end=151, status=0)
    # anchored on mate 2's reverse hit at 7000: mate 1 rescued at 6000 forward, T = 7000 + 150 - 6000
    out, w = R.choose(pair, 130, 120, F(1000), Rv(7000), None, rB, 150, glen)
    assert (out, w) == (dict(j1=-1, j2=4, score=270, tlen=1150, n_proper=0, status=6), F(6000))
    # equal sums: rA
    assert R.choose(pair, 130, 120, F(1000), Rv(7000), rA, rB, 150, glen)[0]["status"] == 5
    rB["score"] = 151
    assert R.choose(pair, 130, 120, F(1000), Rv(7000), rA, rB, 150, glen)[0]["status"] == 6


# ------------------------------------------------------------------------------------------ 2. drm_mate_rescue_region
REGION_CASES = [(glen, ref_len, mn, mx)
                for glen in (0, 149, 150, 151, 1100, 1149, 1150, 1151, 2000, 10_000)
                for ref_len, mn, mx in ((150, 0, 1000), (150, 100, 1000), (150, 200, 1000), (150, 150, 150),
                                        (150, 0, 149), (150, 400, 2047), (150, 0, 2048), (150, 2048, 2048),
                                        (1, 0, 2048), (256, 300, 1300), (64, 0, 64))]


@pytest.mark.parametrize("glen,ref_len,mn,mx", REGION_CASES)
def test_region_against_the_restatement(glen, ref_len, mn, mx):
    assert R.supported(ref_len, mn, mx)
    pos = sorted({0, 1, 2, ref_len, 299, 300, 849, 850, 851, 999, 1000, 1001, max(glen - ref_len - 1, 0),
                  max(glen - ref_len, 0), max(glen - ref_len + 1, 0), glen, glen + 1, 2 ** 40, 2 ** 63 - 1})
    for p, strand in itertools.product(pos, (0, 1)):
        w = 2 * p + strand
        assert mate_rescue_region(glen, ref_len, w, mn, mx) == R.region(glen, ref_len, w, mn, mx), (p, strand)


def test_region_cap_is_2048_rows():
    arg, unsupported = _codes()
    # dhi - dlo + ref_len = max_tlen at min_tlen <= ref_len
    assert mate_rescue_region(10_000, 150, F(1000), 0, 2048) == (1000, 2048, 1)
    with pytest.raises(DrmError) as e:
        mate_rescue_region(10_000, 150, F(1000), 0, 2049)
    assert e.value.code == unsupported
    # ... and max_tlen - min_tlen + ref_len at min_tlen above ref_len
    assert mate_rescue_region(10_000, 150, Rv(4000), 400, 2298) == R.region(10_000, 150, Rv(4000), 400, 2298)
    assert R.region(10_000, 150, Rv(4000), 400, 2298)[1] == 2048
    with pytest.raises(DrmError) as e:
        mate_rescue_region(10_000, 150, Rv(4000), 400, 2299)
    assert e.value.code == unsupported
    assert not R.supported(150, 400, 2299) and not R.supported(150, 0, 2049) and R.supported(150, 400, 2298)


@pytest.mark.parametrize("ref_len,mn,mx,glen", [(0, 0, 1000, 5000), (2 ** 20 + 1, 0, 1000, 5000), (150, -1, 1000, 5000),
                                                (150, 1001, 1000, 5000), (150, 0, 2 ** 30 + 1, 5000),
                                                (150, 0, 1000, -1)])
def test_region_argument_errors(ref_len, mn, mx, glen):
    with pytest.raises(DrmError) as e:
        mate_rescue_region(glen, ref_len, F(10), mn, mx)
    assert e.value.code == _codes()[0]


# ------------------------------------------------------------------------------------------ 3. drm_mate_rescue_window
def test_window_against_the_restatement():
    rng = np.random.default_rng(5)
    n = 0
    for glen, ref_len in ((10_000, 150), (1500, 150), (700, 150), (150, 150), (300, 64)):
        for _ in range(300):
            strand = int(rng.integers(2))
            a = int(rng.integers(0, glen - ref_len + 1))
            s, ln, rev = R.region(glen, ref_len, 2 * a + strand)
            if ln == 0:
                continue
            rec = dict(region_start=s, region_len=ln, reverse=rev, score=int(rng.integers(1, 200)),
                       ref_end=int(rng.integers(1, ln + 1)), q_end=int(rng.integers(1, 153)), status=0)
            assert mate_rescue_window(rec, ref_len, glen) == R.window(rec, ref_len, glen), rec
            n += 1
    assert n > 1000
    # the region's corners, both orientations
    for rev, ref_end in itertools.product((0, 1), (1, 149, 150, 151, 999, 1000)):
        for s, glen in ((0, 1000), (0, 5000), (4000, 5000)):
            rec = dict(region_start=s, region_len=1000, reverse=rev, score=9, ref_end=ref_end, q_end=9, status=0)
            assert mate_rescue_window(rec, 150, glen) == R.window(rec, 150, glen), rec


def test_window_argument_errors():
    arg = _codes()[0]
    rec = dict(region_start=0, region_len=0, reverse=0, score=0, ref_end=0, q_end=0, status=1)
    ok = dict(rec, status=0, score=5, region_len=10, ref_end=5)
    assert mate_rescue_window(ok, 150, 1000) == F(0)
    for r, ref_len, glen in ((rec, 150, 1000), (ok, 150, 149), (ok, 0, 100), (dict(ok, ref_end=0), 150, 1000),
                             (dict(ok, ref_end=11), 150, 1000), (dict(ok, region_start=-1), 150, 1000),
                             (dict(ok, region_start=991), 150, 1000), (dict(ok, region_start=2 ** 63 - 1), 150, 1000)):
        with pytest.raises(DrmError) as e:
            mate_rescue_window(r, ref_len, glen)
        assert e.value.code == arg


# ------------------------------------------------------------------------------------------ 4. drm_pair_rescue_choose
GLEN = 10_000
A1, A2 = F(1000), Rv(7000)


def _rA(score, status=0, ref_end=400):
    return dict(region_start=1000, region_len=1000, reverse=1, score=score, ref_end=ref_end, q_end=151, status=status)


def _rB(score, status=0, ref_end=300):
    return dict(region_start=5850, region_len=1000, reverse=0, score=score, ref_end=ref_end, q_end=151, status=status)


def _pair(status, j1=3, j2=4, score=250, tlen=0, n_proper=2):
    if status == 2:
        j2 = -1
    if status == 3:
        j1 = -1
    if status == 4:
        j1 = j2 = -1
    return dict(j1=j1, j2=j2, score=score, tlen=tlen, n_proper=n_proper, status=status)


def _both(pair, s1, s2, rA, rB, penalty=17, min_score=0, a1=A1, a2=A2, glen=GLEN):
    got_rec, got_w = pair_rescue_choose(pair, s1, s2, a1, a2, rA, rB, REF_LEN, glen, penalty, min_score)
    want_rec, want_w = R.choose(pair, s1, s2, a1, a2, rA, rB, REF_LEN, glen, penalty, min_score)
    got = {f: int(got_rec[f]) for f in R.PAIR_FIELDS}
    assert (got, got_w) == (want_rec, want_w), (pair, s1, s2, rA, rB, penalty, min_score)
    return got, got_w


def test_choose_every_pair_status():
    for status in range(5):
        pair = _pair(status, tlen=420 if status == 0 else 0)
        s1 = 130 if status in (0, 1, 2) else 0
        s2 = 120 if status in (0, 1, 3) else 0
        for rA, rB in itertools.product((None, _rA(140), _rA(140, status=1)), (None, _rB(150), _rB(150, status=1))):
            got, w = _both(pair, s1, s2, rA, rB)
            if status in (0, 4):
                assert got == pair and w == 0
    # the expected outcomes, stated once by hand
    assert _both(_pair(1), 130, 120, _rA(140), None)[0]["status"] == 5
    assert _both(_pair(1), 130, 120, None, _rB(150))[0]["status"] == 6
    assert _both(_pair(2), 130, 0, _rA(140), _rB(150)) == (dict(j1=3, j2=-1, score=270, tlen=750, n_proper=2,
                                                                 status=5), Rv(1600))
    assert _both(_pair(3), 0, 120, _rA(140), _rB(150)) == (dict(j1=-1, j2=4, score=270, tlen=1150, n_proper=2,
                                                                 status=6), F(6000))
    assert _both(_pair(2), 130, 0, None, _rB(150))[0]["status"] == 2
    assert _both(_pair(3), 0, 120, _rA(140), None)[0]["status"] == 3


def test_choose_penalty_threshold():
    # s1 + s2 = 250; sumA = 130 + rA: qualifies from 250 - 17 = 233, i.e. rA >= 103
    assert _both(_pair(1), 130, 120, _rA(103), None)[0]["status"] == 5
    assert _both(_pair(1), 130, 120, _rA(102), None)[0]["status"] == 1
    # sumB = rB + 120: rB >= 113
    assert _both(_pair(1), 130, 120, None, _rB(113))[0]["status"] == 6
    assert _both(_pair(1), 130, 120, None, _rB(112))[0]["status"] == 1
    assert _both(_pair(1), 130, 120, _rA(102), _rB(113))[0]["status"] == 6
    assert _both(_pair(1), 130, 120, _rA(140), None, penalty=0)[0]["status"] == 5
    assert _both(_pair(1), 130, 120, _rA(119), None, penalty=0)[0]["status"] == 1
    # the penalty does not apply to a pair with one live mate
    assert _both(_pair(2), 130, 0, _rA(1), None, penalty=0)[0]["status"] == 5


def test_choose_min_score_threshold():
    for status, s1, s2 in ((1, 130, 120), (2, 130, 0)):
        assert _both(_pair(status), s1, s2, _rA(140), None, min_score=140)[0]["status"] == 5
        assert _both(_pair(status), s1, s2, _rA(139), None, min_score=140)[0]["status"] == status
    for status, s1, s2 in ((1, 130, 120), (3, 0, 120)):
        assert _both(_pair(status), s1, s2, None, _rB(150), min_score=150)[0]["status"] == 6
        assert _both(_pair(status), s1, s2, None, _rB(149), min_score=150)[0]["status"] == status
    # an invalid rA leaves the field to rB
    assert _both(_pair(1), 130, 120, _rA(139), _rB(140), min_score=140)[0]["status"] == 6


def test_choose_tie_and_larger_sum():
    # sumA = 130 + 140 = sumB = 150 + 120: rA
    got, w = _both(_pair(1), 130, 120, _rA(140), _rB(150))
    assert got["status"] == 5 and got["score"] == 270 and w == Rv(1600)
    got, w = _both(_pair(1), 130, 120, _rA(140), _rB(151))
    assert got["status"] == 6 and got["score"] == 271 and w == F(6000)
    got, w = _both(_pair(1), 130, 120, _rA(141), _rB(150))
    assert got["status"] == 5 and got["score"] == 271


def test_choose_both_anchor_strands_and_clamped_windows():
    # mate 1's hit reverse at 7000, mate 2's forward at 1000: the records swap their regions
    rA = dict(_rB(140))
    rB = dict(_rA(150))
    got, w = _both(_pair(1), 130, 120, _rA(0, status=1), None, a1=Rv(7000), a2=F(1000))
    assert got["status"] == 1
    got, w = _both(_pair(1), 130, 120, rA, None, a1=Rv(7000), a2=F(1000))
    assert (got["status"], got["tlen"], w) == (5, 1150, F(6000))
    got, w = _both(_pair(1), 130, 120, None, rB, a1=Rv(7000), a2=F(1000))
    assert (got["status"], got["tlen"], w) == (6, 750, Rv(1600))
    # a rescued window clamped at either genome end still gives tlen >= ref_len
    lo = dict(region_start=0, region_len=450, reverse=0, score=150, ref_end=100, q_end=151, status=0)
    got, w = _both(_pair(3), 0, 120, None, lo, a2=Rv(300))
    assert (got["tlen"], w) == (450, F(0))
    hi = dict(region_start=1000, region_len=500, reverse=1, score=150, ref_end=40, q_end=151, status=0)
    got, w = _both(_pair(2), 130, 0, hi, None, a1=F(1000), glen=1500)
    assert (got["tlen"], w) == (500, Rv(1350))


def test_choose_argument_errors():
    arg = _codes()[0]
    for status in (-1, 5, 6):
        with pytest.raises(DrmError) as e:
            pair_rescue_choose(_pair(1) | {"status": status}, 130, 120, A1, A2, _rA(140), None, REF_LEN, GLEN)
        assert e.value.code == arg
