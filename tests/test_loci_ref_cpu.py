"""CPU tests of the locus-list definition (include/drm_hip.h, drm_hit_loci): the Python restatement
(tests/loci_ref.py) is pinned to hand-worked cases -- the header's example, equal scores, a given head that is not the
top, a dead or out-of-range head, drop_pct 0 / 80 / 100, truncation at max_loci -- and its MAPQ part equals
mapq_ref.hit_one on random lists. No device is needed."""
import numpy as np
import pytest

import loci_ref as L
import mapq_ref as M


def F(pos):
    return 2 * pos


def R(pos):
    return 2 * pos + 1


def loci(hits, head=-1, full=150, span=150, min_score=39, band=2, max_loci=5, drop_pct=80, cnt=None):
    ids, sc = [w for w, _ in hits], [s for _, s in hits]
    return L.loci_one(ids, sc, len(hits) if cnt is None else cnt, head, full, span, min_score, band, max_loci, drop_pct)


def slots_of(result):
    """The recorded slots as (row, score, size), and the check that the rest are empty."""
    _, n_loci, _, slots = result
    assert all(s == L.EMPTY for s in slots[n_loci:])
    return [(row, score, size) for _, score, row, size in slots[:n_loci]]


def test_the_headers_example():
    hits = [(F(0), 100), (F(100), 90), (F(200), 80)]
    rec, n_loci, n_pass, slots = loci(hits)
    assert (n_loci, n_pass) == (2, 2)
    assert slots[:2] == [(F(0), 100, 0, 2), (F(200), 80, 2, 1)] and slots[2:] == [L.EMPTY] * 3
    assert rec == M.hit_one([w for w, _ in hits], [s for _, s in hits], 3, -1, 150, 150, 39, 2)
    assert (rec["best"], rec["locus_rows"], rec["sub_row"], rec["sub_score"], rec["n_sub"]) == (0, 2, 2, 80, 1)
    # one point more and the second locus no longer passes; it still counts for the MAPQ
    rec81, n_loci, n_pass, slots = loci(hits, drop_pct=81)
    assert (n_loci, n_pass) == (1, 1) and slots[1] == L.EMPTY and rec81 == rec


def test_equal_scores_the_smallest_row_wins():
    hits = [(F(9000), 70), (F(1000), 70), (R(1000), 70), (F(5000), 70), (F(1010), 70)]
    res = loci(hits)
    assert slots_of(res) == [(0, 70, 1), (1, 70, 2), (2, 70, 1), (3, 70, 1)]
    assert res[0]["sub_row"] == 1 and res[0]["n_sub"] == 3 and res[2] == 4


def test_a_given_head_that_is_not_the_top():
    hits = [(F(0), 100), (F(1000), 60), (F(2000), 90), (F(1100), 95)]
    # head row 1: its locus holds row 3 (95, above the head); the others follow by score, and both exceed 80 % of 60
    res = loci(hits, head=1)
    assert slots_of(res) == [(1, 60, 2), (0, 100, 1), (2, 90, 1)]
    assert res[0]["best"] == 1 and res[0]["best_score"] == 60 and res[0]["sub_row"] == 0 and res[0]["sub_score"] == 100
    assert res[0] == M.hit_one([w for w, _ in hits], [s for _, s in hits], 4, 1, 150, 150, 39, 2)


def test_a_dead_or_out_of_range_head_gives_nothing():
    hits = [(F(0), 0), (F(1000), 50), (F(2000), 45)]
    for kw in (dict(head=0), dict(head=3), dict(head=-2), dict(head=2, cnt=2), dict(cnt=0), dict(cnt=-4), dict(cnt=1)):
        rec, n_loci, n_pass, slots = loci(hits, **kw)
        assert rec == M.NOTHING and (n_loci, n_pass) == (0, 0) and slots == [L.EMPTY] * 5, kw
    assert slots_of(loci(hits)) == [(1, 50, 1), (2, 45, 1)]
    assert slots_of(loci(hits, cnt=99)) == [(1, 50, 1), (2, 45, 1)]  # clamped to k


def test_drop_pct_0_80_100():
    hits = [(F(0), 100), (F(1000), 100), (F(2000), 80), (F(3000), 79), (F(4000), 40), (F(5000), 38)]
    # 0: everything at or above min_score; the row at 38 is below it
    res = loci(hits, drop_pct=0, max_loci=8)
    assert slots_of(res) == [(0, 100, 1), (1, 100, 1), (2, 80, 1), (3, 79, 1), (4, 40, 1)] and res[2] == 5
    # and with min_score 0 the last one as well
    assert slots_of(loci(hits, drop_pct=0, max_loci=8, min_score=0))[-1] == (5, 38, 1)
    # 80: 100 * 80 >= 80 * 100 holds exactly, 79 fails
    res = loci(hits, drop_pct=80, max_loci=8)
    assert slots_of(res) == [(0, 100, 1), (1, 100, 1), (2, 80, 1)] and res[2] == 3
    # 100: only loci that score what the head scores
    res = loci(hits, drop_pct=100, max_loci=8)
    assert slots_of(res) == [(0, 100, 1), (1, 100, 1)] and res[2] == 2
    # n_sub is drm_hit_mapq's in every case: only the row at 100 is within the band of the competitor
    for pct in (0, 80, 100):
        assert loci(hits, drop_pct=pct)[0]["n_sub"] == 1
    # locus 0 is recorded even below min_score, and counts in n_pass; nothing else passes then
    res = loci([(F(0), 30), (F(1000), 30)], drop_pct=0)
    assert slots_of(res) == [(0, 30, 1)] and res[2] == 1 and res[0]["n_sub"] == 1 and res[0]["mapq"] == 0


def test_truncation_reports_n_pass_above_n_loci():
    hits = [(F(1000 * j), 90) for j in range(7)]
    for max_loci, want in ((1, 1), (2, 2), (5, 5), (7, 7), (64, 7)):
        rec, n_loci, n_pass, slots = loci(hits, max_loci=max_loci)
        assert (n_loci, n_pass) == (want, 7) and len(slots) == max_loci
        assert [s[2] for s in slots[:n_loci]] == list(range(want))
        assert rec["n_sub"] == 6  # the scan goes on past the last slot


@pytest.mark.parametrize("k", [1, 3, 8])
def test_the_mapq_part_equals_hit_one_on_random_lists(k):
    rng = np.random.default_rng(200 + k)
    seen = set()
    for _ in range(1500):
        ids = rng.integers(0, 2 * 40, size=k).astype(np.uint64)
        sc = rng.choice([0, 5, 6, 8], size=k).astype(np.int32)
        cnt, head, full = int(rng.integers(-1, k + 2)), int(rng.integers(-2, k + 1)), int(rng.integers(6, 10))
        min_score, band = int(rng.choice([0, 4, 6])), int(rng.choice([0, 2]))
        max_loci, pct = int(rng.choice([1, 2, 5])), int(rng.choice([0, 80, 100]))
        rec, n_loci, n_pass, slots = L.loci_one(ids, sc, cnt, head, full, 10, min_score, band, max_loci, pct)
        assert rec == M.hit_one(ids, sc, cnt, head, full, 10, min_score, band)
        assert n_loci == min(n_pass, max_loci) and len(slots) == max_loci
        assert (n_loci == 0) == (rec["status"] == 1)
        if n_loci:
            assert slots[0][1:] == (rec["best_score"], rec["best"], rec["locus_rows"])
            assert all(a[1] >= b[1] for a, b in zip(slots[1:n_loci], slots[2:n_loci]))  # non-increasing after slot 0
        seen.add((n_loci, n_pass > n_loci))
    if k == 8:
        assert {(0, False), (1, False), (2, False), (2, True), (5, False)} <= seen
