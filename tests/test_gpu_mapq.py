"""GPU tests of the mapping-quality kernels (mapq.hip: drm_hit_mapq, drm_pair_mapq and their device forms): every field
of every record equals the Python restatement of the definition (tests/mapq_ref.py) -- on random tie-heavy lists whose
loci merge and split, with the head, the competitor and a suppressed row at the lane and per-lane-row boundaries for
k = 63 ... 129 and 1024, on one-locus lists and lists of k singleton loci, with given heads and the top hit, with dead
rows and clamped counts, with more reads than launched waves; for pairs on small tables full of ties, with the
second-best proper combination planted inside and outside the chosen loci and at the table's corners, at the q_pe and
+40 thresholds, for statuses 1 to 4 and the interleaved layout; through the device forms, also chained on the rerank's
and the pairing's device outputs; and for every argument error."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import mapq_ref as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_LEN = 150


def F(pos):
    return 2 * pos


def R(pos):
    return 2 * pos + 1


def _arrays(lists, k):
    """[[(window id, score), ...], ...] as (ids [n, k] u64, scores [n, k] i32, counts [n] i32)."""
    ids, sc = np.zeros((len(lists), k), np.uint64), np.zeros((len(lists), k), np.int32)
    for r, h in enumerate(lists):
        for j, (w, s) in enumerate(h):
            ids[r, j], sc[r, j] = w, s
    return ids, sc, np.array([len(h) for h in lists], np.int32)


def _check_hits(ids, sc, cnt, full, head=None, what="", **prm):
    """The package's records on the batch equal the restatement's; returns them."""
    from deepreadmapper_amd import hit_mapq
    prm.setdefault("ref_len", REF_LEN)
    got = hit_mapq(ids, sc, cnt, full, head=head, **prm)
    M.assert_equal(got, M.hit_all(ids, sc, cnt, full, head=head, **prm), what)
    return got


def _check_pairs(ids1, s1, c1, ids2, s2, c2, full1, full2, what="", row_step=1, **prm):
    """pair_hits, then the package's pair MAPQ records equal the restatement's; returns (pairs, records)."""
    from deepreadmapper_amd import pair_hits, pair_mapq
    prm.setdefault("ref_len", REF_LEN)
    pair_prm = {f: prm[f] for f in ("ref_len", "min_tlen", "max_tlen", "unpaired_penalty") if f in prm}
    pairs = pair_hits(ids1, s1, c1, ids2, s2, c2, row_step=row_step, **pair_prm)
    got = pair_mapq(ids1, s1, c1, ids2, s2, c2, full1, full2, pairs, row_step=row_step, **prm)
    M.assert_equal(got, M.pair_all(ids1, s1, c1, ids2, s2, c2, full1, full2, pairs, row_step=row_step, **prm), what)
    return pairs, got


def _fields(rec, names=("best", "best_score", "locus_rows", "sub_row", "sub_score", "n_sub", "status")):
    return tuple(int(rec[f]) for f in names)


# ------------------------------------------------------------------------------------------ 1. random tie-heavy lists
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_random_lists_full_of_ties(k):
    """Positions from a range four spans wide on both strands, so loci merge and split; scores from four values, one
    of them dead, two of them exactly sub_band apart; every count from -1 to k + 1; the top hit and every given head,
    live, dead, past the count or no row at all."""
    rng = np.random.default_rng(100 + k)
    n = 4000
    ids = rng.integers(0, 2 * 40, size=(n, k)).astype(np.uint64)
    sc = rng.choice([0, 5, 6, 8], size=(n, k)).astype(np.int32)
    cnt = rng.integers(-1, k + 2, size=n).astype(np.int32)
    full = rng.integers(6, 10, size=n).astype(np.int32)
    prm = dict(ref_len=10, locus_span=10, min_score=4, sub_band=2)
    top = _check_hits(ids, sc, cnt, full, **prm)
    head = rng.integers(-2, k + 1, size=n).astype(np.int32)
    given = _check_hits(ids, sc, cnt, full, head=head, **prm)
    assert set(top["status"].tolist()) == {0, 1} and set(given["status"].tolist()) == {0, 1}
    if k == 8:
        assert top["n_sub"].max() >= 3 and top["locus_rows"].max() >= 3 and len(set(top["mapq"].tolist())) > 5
        assert ((given["status"] == 0) & (given["best"] != top["best"])).any()


# ------------------------------------------------------------------------------------------ 2. shapes
@pytest.mark.parametrize("k", [63, 64, 65, 127, 128, 129, 1024])
def test_list_shapes_at_the_lane_and_row_boundaries(k):
    rng = np.random.default_rng(k)
    lists, heads, want = [], [], []
    # (a) head (100), a suppressed row beside it (99, above the competitor: a plain runner-up would take it) and the
    # competitor (90) planted at rows 0, 1, 63, 64, k - 1; every other row a low singleton locus far away
    spots = sorted({r for r in (0, 1, 63, 64, k - 1) if r < k})
    for h, s, c in itertools.permutations(spots, 3):
        rows = [(F(10**6 + 1000 * j), 1 + j % 5) for j in range(k)]
        rows[h], rows[s], rows[c] = (F(5000), 100), (F(5010), 99), (R(5000), 90)
        lists.append(rows)
        heads.append(h if (h + s + c) % 2 else -1)
        want.append((h, 100, 2, c, 90, 1, 0))
    planted = len(lists)
    # (b) one locus: every row within the span of every head
    lists.append([(F(7000 + j % 100), int(rng.integers(1, 150))) for j in range(k)])
    heads.append(-1)
    lists.append([(R(7000 + j % 100), int(rng.integers(1, 150))) for j in range(k)])
    heads.append(k - 1)
    # (c) k singleton loci of equal score: n_sub = k - 1, the scan takes k iterations
    lists.append([(F(200 * j), 77) for j in range(k)])
    heads.append(-1)
    lists.append([(F(200 * (k - j)), 77) for j in range(k)])
    heads.append(k // 2)
    # (d) n_sub at 1, 2, 3, 4, where floor(log2(n_sub + 1)) steps, with rows below the band behind them
    for n_sub in (1, 2, 3, 4):
        rows = [(F(10**6 + 1000 * j), 57) for j in range(k)]
        rows[k - 1] = (F(0), 100)
        for x in range(n_sub):
            rows[x * (k // 5)] = (R(3000 * x), 60 - (x % 2) * 2)
        lists.append(rows)
        heads.append(-1)
    # (e) counts: empty, negative, above k, and one short of the planted rows
    tail = len(lists)
    lists += [lists[0], lists[0], lists[0], lists[planted - 1]]
    heads += [-1, -1, heads[0], heads[planted - 1]]
    ids, sc, cnt = _arrays(lists, k)
    cnt[tail:] = [0, -5, k + 9, k - 1]
    full = np.full(len(lists), 150, np.int32)
    got = _check_hits(ids, sc, cnt, full, head=np.array(heads, np.int32))
    assert [_fields(r) for r in got[:planted]] == want
    assert (got["mapq"][:planted] == M.mapq_value(100, 90, 1, 150, 39)).all()
    assert _fields(got[planted])[2:] == (k, -1, 0, 0, 0) and _fields(got[planted + 1])[2:] == (k, -1, 0, 0, 0)
    assert int(got["best"][planted + 1]) == k - 1
    assert _fields(got[planted + 2]) == (0, 77, 1, 1, 77, k - 1, 0)
    assert _fields(got[planted + 3]) == (k // 2, 77, 1, 0, 77, k - 1, 0)
    assert got["n_sub"][planted + 4:planted + 8].tolist() == [1, 2, 3, 4]
    assert got["mapq"][planted + 4:planted + 8].tolist() == [M.mapq_value(100, 60, n, 150, 39) for n in (1, 2, 3, 4)]
    q = got["mapq"][planted + 4:planted + 8].tolist()  # floor(log2(n_sub + 1)) is 1, 1, 2, 2
    assert q[0] == q[1] == q[2] + 3 == q[3] + 3
    assert got["status"][tail:].tolist() == [1, 1, 0, 0 if heads[planted - 1] != k - 1 else 1]
    # no head given at all: every list from its top hit
    _check_hits(ids, sc, cnt, full)


def _grid_waves():
    class Props(C.Structure):
        _fields_ = [("cu_count", C.c_int32), ("clock_khz", C.c_int32), ("total_mem", C.c_int64),
                    ("lds_per_cu", C.c_int32), ("arch", C.c_char * 64)]
    from deepreadmapper_amd._native import lib
    p = Props()
    assert lib().drm_device_get_props(0, C.byref(p)) == 0
    return 32 * p.cu_count  # the launchers' grid bound for lists this short


def test_more_reads_and_pairs_than_launched_waves():
    """A wave loops over reads / pairs and reuses its LDS: longer lists followed by shorter ones, the last one checked."""
    rng = np.random.default_rng(5)
    n, k = max(5000, _grid_waves() + 37), 6
    ids = rng.integers(0, 60, size=(2 * n, k)).astype(np.uint64)
    sc = rng.integers(0, 4, size=(2 * n, k)).astype(np.int32)
    cnt = rng.integers(0, k + 1, size=2 * n).astype(np.int32)
    full = np.full(2 * n, 3, np.int32)
    ids[-2, :2], sc[-2, :2], cnt[-2] = [F(3), F(29)], [3, 2], 2
    ids[-1, :2], sc[-1, :2], cnt[-1] = [R(4), R(5)], [3, 1], 2
    prm = dict(ref_len=4, locus_span=4, min_score=0, sub_band=1)
    got = _check_hits(ids, sc, cnt, full, **prm)
    assert len(got) == 2 * n > _grid_waves()
    assert _fields(got[-2]) == (0, 3, 1, 1, 2, 1, 0) and _fields(got[-1]) == (0, 3, 2, -1, 0, 0, 0)
    pairs, pq = _check_pairs(ids, sc, cnt, ids[1:], sc[1:], cnt[1:], full, full[1:], row_step=2, max_tlen=12,
                             unpaired_penalty=2, **prm)
    assert len(pq) == n and int(pairs["status"][-1]) == 0
    # F(3) + R(4) = 6 chosen; F(29) pairs with nothing (T = 4 + 4 - 29 < 0): sub_pair 0, subo = 6 - 2
    # mate 1's F(29) competes with F(3): floor(60 * 1 * 3 / (3 * 3)) - 3 = 17 > q_pe; mate 2 is one locus
    assert tuple(int(pq[f][-1]) for f in M.PAIR_FIELDS) == (17, 60, 17, 60, 12, 0)


# ------------------------------------------------------------------------------------------ 3. pairs
@pytest.mark.parametrize("prm", [dict(ref_len=3, min_tlen=0, max_tlen=7, unpaired_penalty=1, locus_span=2),
                                 dict(ref_len=2, min_tlen=4, max_tlen=6, unpaired_penalty=2, locus_span=3)])
def test_small_pair_tables_full_of_ties(prm):
    rng = np.random.default_rng(11)
    n, k = 2000, 8
    counts = np.array([0, 1, 2, 3, 5, 8], np.int32)
    c1, c2 = counts[np.arange(n) % 6], counts[(np.arange(n) // 6) % 6]
    ids1, ids2 = (rng.integers(0, 16, size=(n, k)).astype(np.uint64) for _ in range(2))
    s1, s2 = (rng.choice([0, 1, 1, 2, 2, 3, 3], size=(n, k)).astype(np.int32) for _ in range(2))
    full1, full2 = (rng.integers(2, 5, size=n).astype(np.int32) for _ in range(2))
    pairs, got = _check_pairs(ids1, s1, c1, ids2, s2, c2, full1, full2, min_score=0, sub_band=1, **prm)
    assert set(pairs["status"].tolist()) == {0, 1, 2, 3, 4}
    assert len(set(got["q_pe"].tolist())) >= 2 and (got["sub_pair"] > 0).any()
    assert (got["mapq1"] != got["q_se1"]).any() and (got["mapq2"] != got["q_se2"]).any()


@pytest.mark.parametrize("k", [64, 65, 128, 1024])
def test_second_best_combination_inside_and_outside_the_chosen_loci(k):
    """The chosen rows (100 + 100) and a second row of each mate (95) at the table's corners. Beside both chosen rows
    the second-best combinations are the chosen one shifted by a few bases and are excluded; with one of them outside
    its mate's chosen locus they count. Every other combination is improper by order."""
    rng = np.random.default_rng(k)
    lists1, lists2, want = [], [], []
    corners = [(0, k - 1, k - 1, 0), (k - 1, 0, 0, k - 1), (0, 0, k - 1, k - 1), (k - 1, k - 2, 63 if k > 64 else 1, 64 if k > 65 else 2)]
    shapes = [(10, 10, 0), (10, 300, 195), (300, 10, 195)] if k < 1024 else [(10, 10, 0), (10, 300, 195)]
    # (the restatement walks 2^20 cells per pair at k = 1024: two pairs there)
    for a, b, c, e in corners[:4 if k < 1024 else 1]:
        for d1, d2, sub in shapes:
            # mate 1: reverse hits low in the genome; mate 2: forward hits high in it -> opposite strands, wrong order
            h1 = [(R(int(rng.integers(0, 1000))), int(rng.integers(1, 60))) for _ in range(k)]
            h2 = [(F(int(rng.integers(10**6, 10**6 + 1000))), int(rng.integers(1, 60))) for _ in range(k)]
            h1[a], h1[c] = (F(5000), 100), (F(5000 - d1), 95)
            h2[b], h2[e] = (R(5200), 100), (R(5200 + d2), 95)
            lists1.append(h1)
            lists2.append(h2)
            want.append((a, b, sub))
    ids1, s1, c1 = _arrays(lists1, k)
    ids2, s2, c2 = _arrays(lists2, k)
    full = np.full(len(lists1), 150, np.int32)
    pairs, got = _check_pairs(ids1, s1, c1, ids2, s2, c2, full, full)
    assert [(int(p["j1"]), int(p["j2"])) for p in pairs] == [w[:2] for w in want]
    assert (pairs["status"] == 0).all() and (pairs["score"] == 200).all()
    assert got["sub_pair"].tolist() == [w[2] for w in want]
    # excluded: subo is the unpaired alternative, 200 - 17, and q_pe = 60; counted: 6 * (200 - 195) = 30
    assert got["q_pe"].tolist() == [60 if w[2] == 0 else 30 for w in want]


def test_pair_thresholds_and_statuses():
    unique1, unique2 = [(F(5000), 100)], [(R(5200), 100)]
    cases = [
        (unique1, unique2),                                                    # 0: q_pe = 6 * 17 -> 60
        ([(F(5000), 100), (F(9000), 99)], [(R(5200), 100), (R(9200), 100)]),    # 1: sub_pair 199 -> q_pe 6; both mates ambiguous alone
        ([(F(5000), 100), (F(9000), 100)], [(R(5200), 100), (R(9200), 100)]),   # 2: sub_pair 200 -> q_pe 0
        ([(R(90000), 110), (F(5000), 100)], [(R(5200), 100)]),                  # 3: subo from the unpaired tops; the chosen row is not mate 1's top
        ([(F(5000), 100), (F(20000), 100)], unique2),                           # 4: q_se1 = 0 lifted to 40
        (unique1, [(R(5200), 100), (R(20000), 100)]),                           # 5: the same for mate 2
        ([(F(5000), 100), (F(20000), 70)], unique2),                            # 6: q_se1 = 29, + 40 above q_pe
        ([(F(5000), 100), (F(9000), 100)], [(F(5200), 100)]),                   # 7: status 1, two loci of mate 1
        (unique1, [(R(300), 0)]),                                               # 8: status 2
        ([(F(100), 0)], unique2),                                               # 9: status 3
        ([(F(100), 0)], []),                                                    # 10: status 4
    ]
    k = 2
    ids1, s1, c1 = _arrays([c[0] for c in cases], k)
    ids2, s2, c2 = _arrays([c[1] for c in cases], k)
    full = np.full(len(cases), 100, np.int32)
    pairs, got = _check_pairs(ids1, s1, c1, ids2, s2, c2, full, full)
    assert pairs["status"].tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 2, 3, 4]
    want = {0: (60, 60, 60, 60, 60, 0), 1: (6, 6, 0, 0, 6, 199), 2: (0, 0, 0, 0, 0, 200),
            3: (40, 60, 0, 60, 42, 0), 4: (40, 60, 0, 60, 60, 0), 5: (60, 40, 60, 0, 60, 0),
            6: (60, 60, 26, 60, 60, 0), 7: (0, 60, 0, 60, 0, 0), 8: (60, 0, 60, 0, 0, 0), 9: (0, 60, 0, 60, 0, 0),
            10: (0, 0, 0, 0, 0, 0)}
    for p, w in want.items():
        assert tuple(int(got[f][p]) for f in M.PAIR_FIELDS) == w, (p, got[p], w)
    # the q_se of case 6: 100 against a competitor at 70, one competing locus
    assert M.mapq_value(100, 70, 1, 100, 39) == 26
    # q_se > q_pe keeps q_se: the same unique mates under a penalty of 0 (subo = the tops themselves, q_pe = 0)
    _, got = _check_pairs(ids1[:1], s1[:1], c1[:1], ids2[:1], s2[:1], c2[:1], full[:1], full[:1], unpaired_penalty=0)
    assert tuple(int(got[f][0]) for f in M.PAIR_FIELDS) == (60, 60, 60, 60, 0, 0)
    # +40 on the other side of q_pe: q_se1 = 0, q_pe = 6 * 5 = 30 -> 30, not 40
    _, got = _check_pairs(ids1[4:5], s1[4:5], c1[4:5], ids2[4:5], s2[4:5], c2[4:5], full[:1], full[:1],
                          unpaired_penalty=5)
    assert tuple(int(got[f][0]) for f in M.PAIR_FIELDS) == (30, 60, 0, 60, 30, 0)


def test_interleaved_layout_equals_two_arrays():
    from deepreadmapper_amd import pair_hits, pair_mapq
    rng = np.random.default_rng(6)
    n, k = 301, 9
    ids = rng.integers(0, 3000, size=(2 * n, k)).astype(np.uint64)
    sc = rng.integers(0, 100, size=(2 * n, k)).astype(np.int32)
    cnt = rng.integers(-1, k + 2, size=2 * n).astype(np.int32)
    full = rng.integers(90, 101, size=2 * n).astype(np.int32)
    prm = dict(ref_len=REF_LEN, min_tlen=100, max_tlen=900, unpaired_penalty=17)
    pairs = pair_hits(ids, sc, cnt, ids[1:], sc[1:], cnt[1:], row_step=2, **prm)
    inter = pair_mapq(ids, sc, cnt, ids[1:], sc[1:], cnt[1:], full, full[1:], pairs, row_step=2, min_score=20, **prm)
    _, split = _check_pairs(ids[0::2].copy(), sc[0::2].copy(), cnt[0::2].copy(), ids[1::2].copy(), sc[1::2].copy(),
                            cnt[1::2].copy(), full[0::2].copy(), full[1::2].copy(), min_score=20, **prm)
    assert len(inter) == n and inter.tobytes() == split.tobytes()
    assert set(pairs["status"].tolist()) >= {0, 1} and len(set(split["mapq1"].tolist())) > 5


# ------------------------------------------------------------------------------------------ 4. device forms
def test_device_forms_equal_host_forms():
    from deepreadmapper_amd import (MAPQ_RESULT_DTYPE, PAIR_MAPQ_RESULT_DTYPE, hit_mapq, hit_mapq_device, pair_hits,
                                    pair_hits_device, pair_mapq, pair_mapq_device)
    from deepreadmapper_amd.device import DeviceBuffer, Stream
    rng = np.random.default_rng(7)
    n, k = 500, 65
    ids = rng.integers(0, 5000, size=(2 * n, k)).astype(np.uint64)
    sc = rng.integers(0, 150, size=(2 * n, k)).astype(np.int32)
    cnt = rng.integers(0, k + 1, size=2 * n).astype(np.int32)
    full = rng.integers(140, 151, size=2 * n).astype(np.int32)
    head = rng.integers(-1, k, size=2 * n).astype(np.int32)
    st = Stream()
    d_ids, d_sc, d_cnt = DeviceBuffer.from_host(ids), DeviceBuffer.from_host(sc), DeviceBuffer.from_host(cnt)
    d_full, d_head = DeviceBuffer.from_host(full), DeviceBuffer.from_host(head)
    d_out = DeviceBuffer((2 * n,), MAPQ_RESULT_DTYPE)
    for h, d_h in ((None, None), (head, d_head)):
        want = hit_mapq(ids, sc, cnt, full, REF_LEN, head=h)
        hit_mapq_device(d_ids, d_sc, d_cnt, d_full, 2 * n, k, REF_LEN, d_head=d_h, d_out=d_out, stream=st)
        st.synchronize()
        assert d_out.download().tobytes() == want.tobytes()
        M.assert_equal(want, M.hit_all(ids, sc, cnt, full, REF_LEN, head=h))
    pairs = pair_hits(ids, sc, cnt, ids[1:], sc[1:], cnt[1:], row_step=2, ref_len=REF_LEN)
    want = pair_mapq(ids, sc, cnt, ids[1:], sc[1:], cnt[1:], full, full[1:], pairs, REF_LEN, row_step=2)
    d_pairs = pair_hits_device(d_ids, d_sc, d_cnt, d_ids.ptr + 8 * k, d_sc.ptr + 4 * k, d_cnt.ptr + 4, n, k, REF_LEN,
                               row_step=2, stream=st)
    d_pq = DeviceBuffer((n,), PAIR_MAPQ_RESULT_DTYPE)
    pair_mapq_device(d_ids, d_sc, d_cnt, d_ids.ptr + 8 * k, d_sc.ptr + 4 * k, d_cnt.ptr + 4, d_full, d_full.ptr + 4,
                     d_pairs, n, k, REF_LEN, row_step=2, d_out=d_pq, stream=st)
    st.synchronize()
    assert d_pq.download().tobytes() == want.tobytes()
    assert set(pairs["status"].tolist()) >= {0, 1}


def test_device_forms_chained_on_the_rerank_outputs():
    """drm_post_process_sw_dynamic_device -> drm_hit_mapq_device and drm_pair_hits_device -> drm_pair_mapq_device on
    its d_top_ids / d_top_scores / d_status, nothing copied in between; equal to the restatement on the downloaded
    arrays. The first two reads' true windows have their stride-1 neighbours beside them in the list."""
    from deepreadmapper_amd import GenomeTable, extract_fasta_sequence, hit_mapq_device, pair_hits_device, pair_mapq_device
    from deepreadmapper_amd._native import check, lib
    from deepreadmapper_amd.device import DeviceBuffer, Stream
    from deepreadmapper_amd.rerank import _COMP_TABLE, pack_queries
    g = np.frombuffer(extract_fasta_sequence(os.path.join(GOLDEN, "ecoli_150.fna")), dtype=np.uint8).copy()
    rng = np.random.default_rng(8)
    starts = [(20, 320), (100, 300), (400, 250), (250, 600)]  # (fragment start, template length); the third is swapped
    reads, nb = [], []
    for x, (p, t) in enumerate(starts):
        m1 = bytes(g[p:p + REF_LEN])
        m2 = bytes(_COMP_TABLE[g[p + t - REF_LEN:p + t][::-1]])
        w1, w2 = 2 * p, 2 * (p + t - REF_LEN) + 1
        if x == 2:
            m1, m2, w1, w2 = m2, m1, w2, w1
        reads += [b"<" + m1 + b">", b"<" + m2 + b">"]
        for w in (w1, w2):  # the true window among random ones, and one window past the genome end (score 0)
            row = rng.integers(0, 2 * (len(g) - REF_LEN), size=8)
            row[int(rng.integers(5))] = w
            row[7] = 2 * len(g)
            nb.append(row)
    nb = np.array(nb, dtype=np.int64)
    nb[0, 5:7] = [2 * 21, 2 * 22]  # the stride-1 neighbours of read 0's true window 2 * 20
    nb[1, 5:7] = [2 * (20 + 320 - REF_LEN + 1) + 1, 2 * (20 + 320 - REF_LEN - 1) + 1]  # and of read 1's, reverse
    nq, kk = nb.shape
    qbuf, qlen = pack_queries(reads)
    full = (qlen - 2).astype(np.int32)
    t = GenomeTable(g, REF_LEN)
    st = Stream()
    d_nb, d_q, d_ql = DeviceBuffer.from_host(nb), DeviceBuffer.from_host(qbuf), DeviceBuffer.from_host(qlen)
    d_full = DeviceBuffer.from_host(full)
    d_sc, d_ids, d_st = DeviceBuffer((nq, kk), np.int32), DeviceBuffer((nq, kk), np.uint64), DeviceBuffer(nq, np.int32)
    check(lib().drm_post_process_sw_dynamic_device(t.handle, d_nb.ptr, nq, kk, d_q.ptr, d_ql.ptr, qbuf.shape[1], 1, kk,
                                                   kk, d_sc.ptr, d_ids.ptr, d_st.ptr, st.handle))
    d_hit = hit_mapq_device(d_ids, d_sc, d_st, d_full, nq, kk, REF_LEN, stream=st)
    d_pairs = pair_hits_device(d_ids, d_sc, d_st, d_ids.ptr + 8 * kk, d_sc.ptr + 4 * kk, d_st.ptr + 4, nq // 2, kk,
                               REF_LEN, row_step=2, stream=st)
    d_pq = pair_mapq_device(d_ids, d_sc, d_st, d_ids.ptr + 8 * kk, d_sc.ptr + 4 * kk, d_st.ptr + 4, d_full,
                            d_full.ptr + 4, d_pairs, nq // 2, kk, REF_LEN, row_step=2, stream=st)
    st.synchronize()
    hit, pairs, pq = d_hit.download(), d_pairs.download(), d_pq.download()
    ids, sc, cnt = d_ids.download(), d_sc.download(), d_st.download()
    t.free()
    assert (cnt == kk).all() and (sc == 0).any() and (full == REF_LEN).all()
    M.assert_equal(hit, M.hit_all(ids, sc, cnt, full, REF_LEN))
    M.assert_equal(pq, M.pair_all(ids, sc, cnt, ids[1:], sc[1:], cnt[1:], full, full[1:], pairs, REF_LEN, row_step=2))
    assert (hit["best_score"] == REF_LEN).all() and (hit["status"] == 0).all()
    assert int(hit["locus_rows"][0]) >= 3 and int(hit["locus_rows"][1]) >= 3
    # the competitors are chance hits at or below min_score (at most 39 against a whole 1,000-base
    # region), so a read alone loses only the 3 * floor(log2(n_sub + 1)) of their number, and a pair nothing
    assert (hit["sub_score"] <= 39).all() and (hit["n_sub"] >= 1).all()
    assert hit["mapq"].tolist() == [60 - 3 * (int(n + 1).bit_length() - 1) for n in hit["n_sub"]]
    assert (pq["q_pe"] == 60).all() and (pq["mapq1"] == 60).all() and (pq["mapq2"] == 60).all()
    assert pairs["status"].tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------ 5. argument errors
def test_argument_errors_leave_the_library_usable():
    from deepreadmapper_amd import DrmError, PAIR_RESULT_DTYPE, hit_mapq, pair_hits, pair_mapq
    from deepreadmapper_amd._native import DRM_ERR_ARG, DRM_ERR_UNSUPPORTED
    ids, sc, cnt = _arrays([[(F(100), 50), (F(5000), 40)]], 2)
    ids2, sc2, cnt2 = _arrays([[(R(300), 50)]], 2)
    full = np.array([50], np.int32)
    pairs = pair_hits(ids, sc, cnt, ids2, sc2, cnt2, REF_LEN)

    def good():
        assert int(_check_hits(ids, sc, cnt, full)["mapq"][0]) == M.mapq_value(50, 40, 1, 50, 39) == 54 - 3
        _, got = _check_pairs(ids, sc, cnt, ids2, sc2, cnt2, full, full)
        assert int(got["mapq2"][0]) == 60

    def fails(code, f, *a, **prm):
        prm.setdefault("ref_len", REF_LEN)
        with pytest.raises(DrmError) as e:
            f(*a, **prm)
        assert e.value.code == code, (prm, str(e.value))
        good()  # a valid call right after it
    good()
    hit_args, pair_args = (ids, sc, cnt, full), (ids, sc, cnt, ids2, sc2, cnt2, full, full, pairs)
    for bad in (dict(ref_len=0), dict(ref_len=2**20 + 1), dict(locus_span=0), dict(locus_span=2**20 + 1),
                dict(min_score=-1), dict(min_score=2**20 + 1), dict(sub_band=-1), dict(sub_band=2**20 + 1)):
        fails(DRM_ERR_ARG, hit_mapq, *hit_args, **bad)
        fails(DRM_ERR_ARG, pair_mapq, *pair_args, **bad)
    for bad in (dict(min_tlen=500, max_tlen=499), dict(max_tlen=2**30 + 1), dict(unpaired_penalty=-1)):
        fails(DRM_ERR_ARG, pair_mapq, *pair_args, **bad)
    wide = _arrays([[(F(100), 50)]], 1025)
    fails(DRM_ERR_UNSUPPORTED, hit_mapq, *wide, full)
    fails(DRM_ERR_UNSUPPORTED, pair_mapq, *wide, *wide, full, full, pairs)
    for s in (2**20 + 1, -1):
        bad_sc = sc.copy()
        bad_sc[0, 1] = s
        fails(DRM_ERR_ARG, hit_mapq, ids, bad_sc, cnt, full)
        fails(DRM_ERR_ARG, pair_mapq, ids, bad_sc, cnt, ids2, sc2, cnt2, full, full, pairs)
        fails(DRM_ERR_ARG, pair_mapq, ids2, sc2, cnt2, ids, bad_sc, cnt, full, full, pairs)
    # a score out of range in a row past the count is not looked at
    past = sc2.copy()
    past[0, 1] = -7
    _check_pairs(ids, sc, cnt, ids2, past, cnt2, full, full)
    _check_hits(ids2, past, cnt2, full)
    # pair records outside statuses 0 to 4
    for st in (-1, 5, 6):
        bad_pairs = pairs.copy()
        bad_pairs["status"] = st
        fails(DRM_ERR_ARG, pair_mapq, ids, sc, cnt, ids2, sc2, cnt2, full, full, bad_pairs)
    # k = 0 and nothing at all are valid
    z = np.zeros((3, 0))
    got = hit_mapq(z, z, np.zeros(3), np.full(3, 150), REF_LEN)
    assert got["status"].tolist() == [1, 1, 1] and got["best"].tolist() == [-1, -1, -1] and not got["mapq"].any()
    p4 = np.zeros(3, dtype=PAIR_RESULT_DTYPE)
    p4["status"], p4["j1"], p4["j2"] = 4, -1, -1
    got = pair_mapq(z, z, np.zeros(3), z, z, np.zeros(3), np.full(3, 150), np.full(3, 150), p4, REF_LEN)
    assert not got.view(np.int32).any()
    e = np.zeros((0, 4))
    assert len(hit_mapq(e, e, [], [], REF_LEN)) == 0
    assert len(pair_mapq(e, e, [], e, e, [], [], [], p4[:0], REF_LEN)) == 0
