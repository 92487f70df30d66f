"""CPU tests of the mapping-quality definition (include/drm_hip.h): the Python restatement (tests/mapq_ref.py) is
pinned to hand-worked cases first; the host-only entry points drm_mapq_value and drm_pair_mapq_rescued then equal it
over a full grid, at 2^20 everywhere, for every status, and for every argument error; and the two claims the definition
makes by construction hold on the restatement. No device is needed."""
import ctypes as C

import numpy as np
import pytest

import mapq_ref as M


def F(pos):
    return 2 * pos


def R(pos):
    return 2 * pos + 1


def scan(hits, head=-1, span=150, band=2, cnt=None):
    ids, sc = [w for w, _ in hits], [s for _, s in hits]
    rec, locus0 = M.locus_scan(ids, sc, len(hits) if cnt is None else cnt, head, span, band)
    return tuple(rec[f] for f in ("best", "best_score", "locus_rows", "sub_row", "sub_score", "n_sub", "status")), locus0


NOTHING = (-1, 0, 0, -1, 0, 0, 1)


# ------------------------------------------------------------------------------------------ 1. the restatement
def test_restatement_greedy_suppression_is_not_transitive():
    rec, locus0 = scan([(F(0), 100), (F(100), 90), (F(200), 80)])
    assert rec == (0, 100, 2, 2, 80, 1, 0) and locus0 == {0, 1}
    # with the middle row as the head all three are one locus
    rec, locus0 = scan([(F(0), 100), (F(100), 90), (F(200), 80)], head=1)
    assert rec == (1, 90, 3, -1, 0, 0, 0) and locus0 == {0, 1, 2}


def test_restatement_span_boundary_and_strands():
    # |dpos| = span - 1 is the same locus, |dpos| = span is not, on either side of the head
    assert scan([(F(1000), 50), (F(1149), 40)])[0] == (0, 50, 2, -1, 0, 0, 0)
    assert scan([(F(1000), 50), (F(1150), 40)])[0] == (0, 50, 1, 1, 40, 1, 0)
    assert scan([(F(1000), 50), (F(851), 40)])[0] == (0, 50, 2, -1, 0, 0, 0)
    assert scan([(F(1000), 50), (F(850), 40)])[0] == (0, 50, 1, 1, 40, 1, 0)
    assert scan([(F(7), 50), (F(7), 40)], span=1)[0] == (0, 50, 2, -1, 0, 0, 0)
    assert scan([(F(7), 50), (F(8), 40)], span=1)[0] == (0, 50, 1, 1, 40, 1, 0)
    # opposite strands at one position are two loci
    assert scan([(F(1000), 50), (R(1000), 50)])[0] == (0, 50, 1, 1, 50, 1, 0)


def test_restatement_dead_rows_counts_and_heads():
    hits = [(F(0), 0), (F(1000), 30), (F(5000), 0), (F(2000), 20), (F(3000), 20)]
    assert scan(hits)[0] == (1, 30, 1, 3, 20, 2, 0)  # dead rows are neither head, locus row nor competitor
    assert scan(hits, cnt=4)[0] == (1, 30, 1, 3, 20, 1, 0)  # only the first `count` rows
    assert scan(hits, cnt=1)[0] == NOTHING and scan(hits, cnt=0)[0] == NOTHING and scan(hits, cnt=-3)[0] == NOTHING
    assert scan(hits, cnt=99)[0] == scan(hits)[0]  # clamped to k
    # a head that is not the top: the top becomes the competitor
    assert scan(hits, head=3)[0] == (3, 20, 1, 1, 30, 1, 0)
    # a head that is dead, past the count, or not a row at all
    assert scan(hits, head=0)[0] == NOTHING and scan(hits, head=4, cnt=4)[0] == NOTHING
    assert scan(hits, head=5)[0] == NOTHING and scan(hits, head=-2)[0] == NOTHING
    assert scan([(F(0), 0)] * 3)[0] == NOTHING and scan([])[0] == NOTHING


def test_restatement_ties_and_the_band():
    # ties in score are decided by row: head, competitor, and the order in which loci are taken
    assert scan([(F(0), 9), (F(1000), 9), (F(2000), 9)])[0] == (0, 9, 1, 1, 9, 2, 0)
    # rows 1 and 2 tie; row 1 is taken first and swallows row 3 (100 away) but not row 2 (200 away from it)
    assert scan([(F(0), 9), (F(1000), 5), (F(1200), 5), (F(1100), 5)])[0] == (0, 9, 1, 1, 5, 2, 0)
    # taken in the other order the middle row would merge all three: row order matters
    assert scan([(F(0), 9), (F(1100), 5), (F(1200), 5), (F(1000), 5)])[0] == (0, 9, 1, 1, 5, 1, 0)
    # the band: s(t) == sub_score - band counts, one below does not, and the scan stops there
    hits = [(F(0), 50), (F(1000), 40), (F(2000), 38), (F(3000), 37), (F(4000), 38)]
    assert scan(hits, band=2)[0] == (0, 50, 1, 1, 40, 3, 0)
    assert scan(hits, band=1)[0] == (0, 50, 1, 1, 40, 1, 0)
    assert scan(hits, band=3)[0] == (0, 50, 1, 1, 40, 4, 0)
    assert scan(hits, band=0)[0] == (0, 50, 1, 1, 40, 1, 0)


def test_restatement_wide_ids():
    # ids across 2^32 (positions across 2^31), positions across 2^32, and up to 2^64 - 1
    for base in (2**32, 2**33, 2**64 - 2):
        lo = base - 2 * 100  # 100 positions below the one `base` names
        assert scan([(base & ~1, 50), (lo & ~1, 40)])[0] == (0, 50, 2, -1, 0, 0, 0)
        assert scan([(base & ~1, 50), ((lo & ~1) - 2 * 50, 40)])[0] == (0, 50, 1, 1, 40, 1, 0)
    assert scan([(2**64 - 1, 50), (2**64 - 3, 40), (2**64 - 2, 45)])[0] == (0, 50, 2, 2, 45, 1, 0)
    assert scan([(2**64 - 1, 50), (1, 50)])[0] == (0, 50, 1, 1, 50, 1, 0)  # 2^63 apart: never one locus


# ------------------------------------------------------------------------------------------ 2. drm_mapq_value
def test_mapq_value_worked_values():
    from deepreadmapper_amd import mapq_value
    for f in (mapq_value, M.mapq_value):
        assert f(150, 0, 0, 150, 39) == 60   # a perfect unique read
        assert f(130, 0, 0, 150, 39) == 52   # a unique read at 130 of 150
        assert f(130, 0, 0, 150, 0) == 52
        assert f(150, 150, 1, 150, 39) == 0  # a competitor that scores the same
        assert f(150, 149, 1, 150, 39) == 0  # floor(60 * 1 * 150 / (111 * 150)) = 0, less 3
        assert f(150, 100, 1, 150, 39) == 24  # floor(60 * 50 / 111) = 27, less 3 * floor(log2(2))
        assert f(150, 100, 3, 150, 39) == 21 and f(150, 100, 7, 150, 39) == 18
        assert f(0, 0, 0, 150, 39) == 0 and f(150, 0, 0, 0, 39) == 0 and f(39, 0, 0, 150, 39) == 0
        assert f(200, 0, 0, 150, 39) == 60  # s1 above full counts as full


def test_mapq_value_equals_the_restatement_over_the_grid():
    from deepreadmapper_amd._native import lib
    fn, q = lib().drm_mapq_value, C.c_int32(0)
    ref, seen, n = M.mapq_value, set(), 0
    for full in (1, 150, 152):
        for min_score in (0, 39, 160):
            for n_sub in (0, 1, 2, 3, 7, 8, 1023):
                for s1 in range(161):
                    for sub in range(161):
                        assert fn(s1, sub, n_sub, full, min_score, C.byref(q)) == 0
                        if q.value != ref(s1, sub, n_sub, full, min_score):
                            raise AssertionError((s1, sub, n_sub, full, min_score, q.value))
                        seen.add(q.value)
                        n += 1
    assert n == 161 * 161 * 7 * 9 and seen >= {0, 1, 30, 59, 60}


def test_mapq_value_at_two_to_the_twenty():
    from deepreadmapper_amd import mapq_value
    big = 2**20
    for s1 in (big, big - 1, 1):
        for sub in (big, big - 1, 0):
            for n_sub in (0, big):
                for full in (big, big - 1, 1):
                    for min_score in (0, big - 1, big):
                        assert mapq_value(s1, sub, n_sub, full, min_score) == M.mapq_value(s1, sub, n_sub, full,
                                                                                           min_score)
    assert mapq_value(big, 0, 0, big, 0) == 60 and mapq_value(big, 0, 0, big, big - 1) == 60
    assert mapq_value(big, big - 1, 0, big, 0) == 0 and mapq_value(big, big // 2, 0, big, 0) == 30
    assert mapq_value(-5, 0, 0, 150, 39) == 0 and mapq_value(150, -5, 0, 150, 39) == 60
    assert mapq_value(150, 0, 0, -1, 39) == 0


# ------------------------------------------------------------------------------------------ 3. rescued pairs
def _pairs(statuses):
    from deepreadmapper_amd import PAIR_RESULT_DTYPE
    p = np.zeros(len(statuses), dtype=PAIR_RESULT_DTYPE)
    p["status"] = statuses
    return p


def test_pair_mapq_rescued_every_status_and_the_min_at_equality():
    from deepreadmapper_amd import PAIR_MAPQ_RESULT_DTYPE, pair_mapq_rescued
    # (status, mapq1, mapq2 before, rescue score): value(130, 0, 0, 150, 39) = 52, value(150, ..) = 60, value(39, ..) = 0
    cases = [(0, 60, 60, 150), (1, 40, 30, 150), (2, 50, 0, 150), (3, 0, 50, 150), (4, 0, 0, 150),
             (5, 60, 0, 130), (5, 52, 0, 130), (5, 51, 0, 130), (5, 53, 7, 130), (5, 0, 9, 150), (5, 60, 1, 39),
             (6, 0, 60, 130), (6, 0, 52, 130), (6, 0, 51, 130), (6, 7, 53, 130), (6, 9, 0, 150), (6, 1, 60, 39)]
    before = np.zeros(len(cases), dtype=PAIR_MAPQ_RESULT_DTYPE)
    before["mapq1"], before["mapq2"] = [c[1] for c in cases], [c[2] for c in cases]
    before["q_se1"], before["q_se2"], before["q_pe"], before["sub_pair"] = 11, 12, 13, 14
    full = np.full(len(cases), 150, np.int32)
    rs = np.array([c[3] for c in cases], np.int32)
    keep = before.copy()
    got = pair_mapq_rescued(_pairs([c[0] for c in cases]), before, rs, full, full, 150)
    assert before.tobytes() == keep.tobytes()
    want = [M.rescued_one(c[0], {f: int(before[f][i]) for f in M.PAIR_FIELDS}, c[3], 150, 150, 39)
            for i, c in enumerate(cases)]
    M.assert_equal(got, want)
    assert list(zip(got["mapq1"].tolist(), got["mapq2"].tolist())) == [
        (60, 60), (40, 30), (50, 0), (0, 50), (0, 0),
        (60, 52), (52, 52), (51, 51), (53, 52), (0, 0), (60, 0),
        (52, 60), (52, 52), (51, 51), (52, 53), (0, 0), (0, 60)]
    # the rescued mate's own length is the one that counts, through row_step as drm_pair_mapq indexes it
    full1, full2 = np.array([150, 0, 100, 0], np.int32), np.array([130, 0, 150, 0], np.int32)
    b = np.zeros(2, dtype=PAIR_MAPQ_RESULT_DTYPE)
    b["mapq1"], b["mapq2"] = [60, 0], [0, 60]
    got = pair_mapq_rescued(_pairs([5, 6]), b, [130, 100], full1, full2, 150, row_step=2)
    assert got["mapq2"][0] == 60 and got["mapq1"][1] == 60  # 130 of 130 and 100 of 100
    got = pair_mapq_rescued(_pairs([5, 6]), b, [130, 100], full2, full1, 150, row_step=2)
    assert got["mapq2"][0] == 52 and got["mapq1"][1] == M.mapq_value(100, 0, 0, 150, 39) == 40
    assert len(pair_mapq_rescued(_pairs([]), b[:0], [], [], [], 150)) == 0


# ------------------------------------------------------------------------------------------ 4. argument errors
def test_argument_errors_of_the_host_only_functions():
    from deepreadmapper_amd import PAIR_MAPQ_RESULT_DTYPE, DrmError, mapq_value, pair_mapq_rescued
    from deepreadmapper_amd._native import DRM_ERR_ARG, lib

    def fails(f, *a, **kw):
        with pytest.raises(DrmError) as e:
            f(*a, **kw)
        assert e.value.code == DRM_ERR_ARG, str(e.value)
        assert mapq_value(150, 0, 0, 150, 39) == 60  # a valid call right after it
    assert lib().drm_mapq_value(150, 0, 0, 150, 39, None) == DRM_ERR_ARG
    fails(mapq_value, 150, 0, -1, 150, 39)
    fails(mapq_value, 150, 0, 2**20 + 1, 150, 39)
    fails(mapq_value, 150, 0, 0, 150, -1)
    fails(mapq_value, 150, 0, 0, 150, 2**20 + 1)
    fails(mapq_value, 2**20 + 1, 0, 0, 150, 39)
    fails(mapq_value, 150, 2**20 + 1, 0, 150, 39)
    fails(mapq_value, 150, 0, 0, 2**20 + 1, 39)
    fails(mapq_value, -2**20 - 1, 0, 0, 150, 39)
    b = np.zeros(1, dtype=PAIR_MAPQ_RESULT_DTYPE)
    b["mapq1"] = 60
    ok = dict(pairs=_pairs([5]), mapq=b, rescue_score=[130], full1=[150], full2=[150], ref_len=150)
    assert int(pair_mapq_rescued(**ok)["mapq2"][0]) == 52
    for st in (-1, 7):
        fails(pair_mapq_rescued, **dict(ok, pairs=_pairs([st])))
    for bad in (dict(ref_len=0), dict(ref_len=2**20 + 1), dict(locus_span=0), dict(locus_span=2**20 + 1),
                dict(min_score=-1), dict(min_score=2**20 + 1), dict(sub_band=-1), dict(sub_band=2**20 + 1),
                dict(rescue_score=[2**20 + 1]), dict(full2=[2**20 + 1])):
        fails(pair_mapq_rescued, **dict(ok, **bad))
    # a bad record anywhere leaves every record as it was
    two = np.zeros(2, dtype=PAIR_MAPQ_RESULT_DTYPE)
    two["mapq1"] = 60
    L = lib()
    prm = np.array([150, 150, 39, 2], np.int32)
    p = _pairs([5, 9])
    z = np.array([130, 130], np.int32)
    f = np.array([150, 150], np.int32)
    assert L.drm_pair_mapq_rescued(prm.ctypes.data, p.ctypes.data, z.ctypes.data, f.ctypes.data, f.ctypes.data, 2, 1,
                                   two.ctypes.data) == DRM_ERR_ARG
    assert two["mapq2"].tolist() == [0, 0]
    assert L.drm_pair_mapq_rescued(prm.ctypes.data, None, z.ctypes.data, f.ctypes.data, f.ctypes.data, 2, 1,
                                   two.ctypes.data) == DRM_ERR_ARG
    assert L.drm_pair_mapq_rescued(None, p.ctypes.data, z.ctypes.data, f.ctypes.data, f.ctypes.data, 2, 1,
                                   two.ctypes.data) == DRM_ERR_ARG
    assert L.drm_pair_mapq_rescued(prm.ctypes.data, p.ctypes.data, z.ctypes.data, f.ctypes.data, f.ctypes.data, 2, 0,
                                   two.ctypes.data) == DRM_ERR_ARG
    assert L.drm_pair_mapq_rescued(prm.ctypes.data, p.ctypes.data, z.ctypes.data, f.ctypes.data, f.ctypes.data, -1, 1,
                                   two.ctypes.data) == DRM_ERR_ARG


# ------------------------------------------------------------------------------------------ 5. by construction
def test_an_exact_duplicate_in_the_list_gives_zero():
    rng = np.random.default_rng(1)
    for _ in range(300):
        k = int(rng.integers(2, 12))
        pos = rng.integers(0, 5000, size=k)
        ids = [int(2 * p + rng.integers(2)) for p in pos]
        sc = [int(x) for x in rng.integers(1, 151, size=k)]
        best = max(sc)
        a = sc.index(best)
        # a second locus (a span away or on the other strand) with the same score
        dup = (ids[a] ^ 1) if rng.integers(2) else ids[a] + 2 * int(rng.integers(150, 1000))
        ids.append(dup)
        sc.append(best)
        rec = M.hit_one(ids, sc, len(ids), -1, 150, 150, int(rng.integers(0, 60)), 2)
        assert rec["status"] == 0 and rec["sub_score"] == rec["best_score"] == best and rec["mapq"] == 0, (ids, sc)


def test_stride_one_neighbours_never_lower_the_mapq():
    rng = np.random.default_rng(2)
    lowered_naively = 0
    for _ in range(300):
        k = int(rng.integers(1, 8))
        ids = [int(2 * p + rng.integers(2)) for p in rng.integers(0, 5000, size=k)]
        sc = [int(x) for x in rng.integers(1, 140, size=k)]
        ids.insert(0, 2 * 10000)
        sc.insert(0, 150)  # the best window, far from the others
        alone = M.hit_one(ids, sc, len(ids), -1, 150, 150, 39, 2)
        # its stride-1 neighbours on either side, each a little lower, anywhere in the list
        near = [(2 * (10000 + d), 150 - 2 * abs(d)) for d in (-3, -2, -1, 1, 2, 3)]
        ids2, sc2 = list(ids), list(sc)
        for w, s in near:
            at = int(rng.integers(1, len(ids2) + 1))
            ids2.insert(at, w)
            sc2.insert(at, s)
        crowded = M.hit_one(ids2, sc2, len(ids2), -1, 150, 150, 39, 2)
        assert crowded["mapq"] == alone["mapq"] and crowded["locus_rows"] == 7, (ids2, sc2)
        assert crowded["sub_score"] == alone["sub_score"] and crowded["n_sub"] == alone["n_sub"]
        lowered_naively += M.mapq_value(150, 148, 1, 150, 39) < alone["mapq"]
    assert lowered_naively > 250  # what a plain runner-up would have done to the same reads
