"""CPU tests of the paired-end path: the Python restatement of the pairing definition (tests/pair_ref.py) is pinned
to hand-worked cases of every status and tie rule, and the host-only drm_sam_pair_fields gives the pair flags, PNEXT
and TLEN by the rules of include/drm_hip.h. (The paired SAM writer has no host-only entry point: it is covered by
tests/test_gpu_pair_cli.py.)"""
import pytest

import pair_ref as P

REF_LEN = 150


def F(pos):
    """Window id of a forward hit at genome position pos."""
    return 2 * pos


def R(pos):
    return 2 * pos + 1


def _one(h1, h2, cnt1=None, cnt2=None, **kw):
    """pair_one on two lists of (window id, score) rows."""
    k = max(len(h1), len(h2), 1)
    pad = lambda h: ([w for w, _ in h] + [0] * (k - len(h)), [s for _, s in h] + [0] * (k - len(h)))  # noqa: E731
    (i1, s1), (i2, s2) = pad(h1), pad(h2)
    return P.pair_one(i1, s1, len(h1) if cnt1 is None else cnt1, i2, s2, len(h2) if cnt2 is None else cnt2,
                      kw.pop("ref_len", REF_LEN), **kw)


# ------------------------------------------------------------------------------------------ 1. the restatement
def test_ref_status_0_proper_pair_and_tlen():
    # forward at 100, reverse at 300: T = 300 + 150 - 100
    assert _one([(F(100), 150)], [(R(300), 140)]) == dict(j1=0, j2=0, score=290, tlen=350, n_proper=1, status=0)
    # mate 1 may be the reverse one
    assert _one([(R(300), 150)], [(F(100), 140)]) == dict(j1=0, j2=0, score=290, tlen=350, n_proper=1, status=0)


def test_ref_status_1_when_nothing_proper_or_too_far_below_the_tops():
    # same strand
    assert _one([(F(100), 150)], [(F(300), 140)]) == dict(j1=0, j2=0, score=290, tlen=0, n_proper=0, status=1)
    # reverse hit left of the forward hit
    assert _one([(F(300), 150)], [(R(100), 140)])["status"] == 1
    # proper (row 1 of mate 1 with row 0 of mate 2) but 18 below the top hits' sum at penalty 17 ...
    h1, h2 = [(F(5000), 150), (F(100), 132)], [(R(300), 140)]
    assert _one(h1, h2) == dict(j1=0, j2=0, score=290, tlen=0, n_proper=1, status=1)
    # ... and exactly 17 below: chosen
    h1[1] = (F(100), 133)
    assert _one(h1, h2) == dict(j1=1, j2=0, score=273, tlen=350, n_proper=1, status=0)


def test_ref_status_2_3_4_and_liveness():
    assert _one([(F(100), 150)], []) == dict(j1=0, j2=-1, score=150, tlen=0, n_proper=0, status=2)
    assert _one([], [(R(300), 140)]) == dict(j1=-1, j2=0, score=140, tlen=0, n_proper=0, status=3)
    assert _one([], []) == dict(j1=-1, j2=-1, score=0, tlen=0, n_proper=0, status=4)
    # a zero-score row is not live: not a top hit, not paired, not counted
    assert _one([(F(100), 0), (F(100), 7)], [(R(300), 0)]) == dict(j1=1, j2=-1, score=7, tlen=0, n_proper=0, status=2)
    # counts are clamped to [0, k]: negative is 0, beyond k is k
    assert _one([(F(100), 150)], [(R(300), 140)], cnt1=-3)["status"] == 3
    assert _one([(F(100), 150)], [(R(300), 140)], cnt1=99, cnt2=99)["status"] == 0
    # a row past the count does not exist
    assert _one([(F(100), 150), (F(100), 151)], [(R(300), 140)], cnt1=1)["score"] == 290


def test_ref_tie_rules():
    # all rows equal and proper: (0, 0)
    h1, h2 = [(F(100), 9)] * 3, [(R(200), 9)] * 3
    assert _one(h1, h2) == dict(j1=0, j2=0, score=18, tlen=250, n_proper=9, status=0)
    # the largest sum wins wherever it sits: sums (0,0) = 13, (0,1) = 10, (1,0) = 16, (1,1) = 13
    r = _one([(F(100), 5), (F(100), 8)], [(R(200), 8), (R(200), 5)])
    assert (r["j1"], r["j2"], r["score"], r["n_proper"]) == (1, 0, 16, 4)
    # equal sums on one row of mate 1: the smallest j2
    r = _one([(F(100), 8)], [(R(200), 3), (R(200), 8), (R(200), 8)])
    assert (r["j1"], r["j2"], r["score"]) == (0, 1, 16)
    # the top hit is the largest score, the smallest row among equals, in an unsorted list
    assert _one([(F(100), 3), (F(100), 9), (F(100), 9)], [])["j1"] == 1


def test_ref_equal_sums_prefer_smaller_j1_then_j2():
    # only (0, 1) and (1, 0) are proper, both with sum 13
    h1 = [(F(100), 5), (F(1000), 8)]
    h2 = [(R(1100), 5), (R(200), 8)]
    r = _one(h1, h2, max_tlen=300)
    assert r["n_proper"] == 2 and (r["j1"], r["j2"], r["score"], r["status"]) == (0, 1, 13, 0)


def test_ref_bounds_are_inclusive():
    for t, ok in ((199, False), (200, True), (400, True), (401, False)):
        r = _one([(F(1000), 50)], [(R(1000 + t - REF_LEN), 50)], min_tlen=200, max_tlen=400)
        assert (r["status"] == 0) == ok and r["n_proper"] == int(ok), t
        assert r["tlen"] == (t if ok else 0)
    # pos(f) == pos(r) is allowed (T = ref_len), pos(f) == pos(r) + 1 is not
    assert _one([(F(1000), 50)], [(R(1000), 50)])["tlen"] == REF_LEN
    assert _one([(F(1001), 50)], [(R(1000), 50)])["status"] == 1
    assert P.is_proper(F(1000), 50, R(1000), 50, REF_LEN, 0, 1000) == (True, REF_LEN)
    assert P.is_proper(F(1001), 50, R(1000), 50, REF_LEN, 0, 1000)[0] is False


def test_ref_wide_ids_need_64_bits():
    a = 2**32 - 4
    assert _one([(a, 50)], [(a + 2 * 200 + 1, 50)])["tlen"] == 350          # crosses 2^32 as a window id
    assert _one([(2 * (2**32 - 10), 50)], [(2 * (2**32 + 90) + 1, 50)])["tlen"] == 250  # crosses 2^32 as a position
    assert _one([(2**64 - 2, 50)], [(2**64 - 1, 50)])["tlen"] == REF_LEN
    assert _one([(2, 50)], [(2**64 - 1, 50)])["status"] == 1               # 2^63 apart: no 32-bit wrap-around


# ------------------------------------------------------------------------------------------ 2. drm_sam_pair_fields
def _fields(m1, m2, proper):
    from deepreadmapper_amd import sam_pair_fields
    return sam_pair_fields(m1, m2, proper)


def test_pair_fields_both_mapped_flags_and_tlen():
    a, b = _fields((1, 0, 101, 150), (1, 1, 301, 150), True)
    assert a == dict(flag=0x1 | 0x2 | 0x20 | 0x40, has_rname=1, pos=101, pnext=301, tlen=350)
    assert b == dict(flag=0x1 | 0x2 | 0x10 | 0x80, has_rname=1, pos=301, pnext=101, tlen=-350)
    # not proper: the same without 0x2
    a, b = _fields((1, 0, 101, 150), (1, 1, 301, 150), False)
    assert (a["flag"], b["flag"]) == (0x1 | 0x20 | 0x40, 0x1 | 0x10 | 0x80) and a["tlen"] == 350
    # mate 2 leftmost: it gets +L; mate 1 reverse sets 0x10 on its own line and 0x20 on the mate's
    a, b = _fields((1, 1, 301, 148), (1, 0, 101, 150), True)
    assert a == dict(flag=0x1 | 0x2 | 0x10 | 0x40, has_rname=1, pos=301, pnext=101, tlen=-348)
    assert b == dict(flag=0x1 | 0x2 | 0x20 | 0x80, has_rname=1, pos=101, pnext=301, tlen=348)
    # both forward / both reverse (never proper, but the strand bits are independent)
    a, b = _fields((1, 0, 10, 5), (1, 0, 20, 5), False)
    assert (a["flag"], b["flag"]) == (0x1 | 0x40, 0x1 | 0x80)
    a, b = _fields((1, 1, 10, 5), (1, 1, 20, 5), False)
    assert (a["flag"], b["flag"]) == (0x1 | 0x10 | 0x20 | 0x40, 0x1 | 0x10 | 0x20 | 0x80)


def test_pair_fields_equal_pos_and_containment():
    # equal pos1: mate 1 gets +L, L from the longer span
    a, b = _fields((1, 0, 500, 100), (1, 1, 500, 150), True)
    assert (a["tlen"], b["tlen"]) == (150, -150)
    a, b = _fields((1, 1, 500, 150), (1, 0, 500, 100), True)
    assert (a["tlen"], b["tlen"]) == (150, -150)
    # mate 2 lies inside mate 1: the rightmost end is mate 1's, so L is mate 1's span, not 520 + 20 - 500
    a, b = _fields((1, 0, 500, 150), (1, 1, 520, 20), True)
    assert (a["tlen"], b["tlen"]) == (150, -150)
    a, b = _fields((1, 1, 520, 20), (1, 0, 500, 150), True)
    assert (a["tlen"], b["tlen"]) == (-150, 150)


def test_pair_fields_one_or_none_mapped():
    a, b = _fields((1, 1, 77, 150), None, True)  # `proper` without two mapped mates never sets 0x2
    assert a == dict(flag=0x1 | 0x8 | 0x10 | 0x40, has_rname=1, pos=77, pnext=77, tlen=0)
    assert b == dict(flag=0x1 | 0x4 | 0x20 | 0x80, has_rname=1, pos=77, pnext=77, tlen=0)
    a, b = _fields((0, 1, 5, 5), (1, 0, 42, 150), False)  # an unmapped mate's other fields are ignored
    assert a == dict(flag=0x1 | 0x4 | 0x40, has_rname=1, pos=42, pnext=42, tlen=0)
    assert b == dict(flag=0x1 | 0x8 | 0x80, has_rname=1, pos=42, pnext=42, tlen=0)
    a, b = _fields(None, None, True)
    assert a == dict(flag=0x1 | 0x4 | 0x8 | 0x40, has_rname=0, pos=0, pnext=0, tlen=0)
    assert b == dict(flag=0x1 | 0x4 | 0x8 | 0x80, has_rname=0, pos=0, pnext=0, tlen=0)


def test_pair_fields_argument_errors():
    from deepreadmapper_amd import DrmError
    from deepreadmapper_amd._native import DRM_ERR_ARG, lib
    for m1, m2 in (((1, 0, 0, 150), (1, 1, 10, 150)), ((1, 0, 10, 150), (1, 1, 10, 0)), ((1, 0, -5, 150), None),
                   (None, (1, 0, 10, -1))):
        with pytest.raises(DrmError) as e:
            _fields(m1, m2, True)
        assert e.value.code == DRM_ERR_ARG
    assert lib().drm_sam_pair_fields(None, 1, None) == DRM_ERR_ARG
    assert _fields((1, 0, 1, 1), (1, 1, 1, 1), True)[0]["tlen"] == 1  # a valid call after the errors


def test_version_has_the_pairing_api():
    from deepreadmapper_amd._native import lib
    assert lib().drm_version() >= 400
