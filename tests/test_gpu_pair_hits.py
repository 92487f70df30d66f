"""GPU tests of the mate-pairing kernel (pair_hits.hip, drm_pair_hits / drm_pair_hits_device): every field of every
record equals the Python restatement of the definition (tests/pair_ref.py) -- on small exhaustive tables full of
ties, at the lane and list edges, at the template-length and penalty bounds, with dead rows and clamped counts, with
window ids past 2^32 and near 2^64, with more pairs than launched waves, in the interleaved layout, through the
device entry point (also chained on the rerank's device outputs), and for every argument error."""
import ctypes as C
import os

import numpy as np
import pytest

import pair_ref as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_LEN = 150


def _check(ids1, s1, c1, ids2, s2, c2, what="", **prm):
    """The package's result on the batch equals the restatement's; returns the result."""
    from deepreadmapper_amd import pair_hits
    prm.setdefault("ref_len", REF_LEN)
    got = pair_hits(ids1, s1, c1, ids2, s2, c2, **prm)
    P.assert_equal(got, P.pair_all(ids1, s1, c1, ids2, s2, c2, **prm), what)
    return got


def _lists(h, k):
    """One list of (window id, score) rows as (ids [k] u64, scores [k] i32, count)."""
    ids, sc = np.zeros(k, np.uint64), np.zeros(k, np.int32)
    for j, (w, s) in enumerate(h):
        ids[j], sc[j] = w, s
    return ids, sc, len(h)


def _batch(pairs, k):
    """[(hits of mate 1, hits of mate 2), ...] as the six arrays of pair_hits."""
    a = [_lists(h1, k) for h1, _ in pairs]
    b = [_lists(h2, k) for _, h2 in pairs]
    st = lambda x, i, dt: np.array([r[i] for r in x], dtype=dt).reshape(len(x), *([k] if i < 2 else []))  # noqa: E731
    return (st(a, 0, np.uint64), st(a, 1, np.int32), st(a, 2, np.int32), st(b, 0, np.uint64), st(b, 1, np.int32),
            st(b, 2, np.int32))


def F(pos):
    return 2 * pos


def R(pos):
    return 2 * pos + 1


# ------------------------------------------------------------------------------------------ 1. small exhaustive
@pytest.mark.parametrize("prm", [dict(ref_len=3, min_tlen=0, max_tlen=7, unpaired_penalty=1),
                                 dict(ref_len=2, min_tlen=4, max_tlen=6, unpaired_penalty=0)])
def test_small_tables_full_of_ties(prm):
    """Counts 0, 1, 2, 3, 5 for either mate, positions from a range of 8 on both strands, scores 1..3 with a few
    zeros: equal sums, equal scores and equal positions everywhere; 4000 pairs in one launch."""
    rng = np.random.default_rng(11)
    n, k = 4000, 5
    counts = np.array([0, 1, 2, 3, 5], np.int32)
    c1, c2 = counts[np.arange(n) % 5], counts[(np.arange(n) // 5) % 5]
    ids1, ids2 = (rng.integers(0, 16, size=(n, k)).astype(np.uint64) for _ in range(2))
    s1, s2 = (rng.choice([0, 1, 1, 2, 2, 3, 3], size=(n, k)).astype(np.int32) for _ in range(2))
    got = _check(ids1, s1, c1, ids2, s2, c2, **prm)
    assert set(got["status"].tolist()) == {0, 1, 2, 3, 4}
    assert got["n_proper"].max() > 3


# ------------------------------------------------------------------------------------------ 2. lane and list edges
@pytest.mark.parametrize("k", [63, 64, 65, 127, 128, 129, 1024])
def test_single_proper_combination_at_the_edges(k):
    """One proper combination planted at the corners of the table and at mate-2 rows 63 / 64; every other
    combination is improper by strand or by order, whatever its scores. Counts equal to k and below it."""
    rng = np.random.default_rng(k)
    pairs, planted = [], []
    # (the restatement walks 2^20 cells per pair at k = 1024: two count shapes there, three below)
    for cnt1, cnt2 in ((k, k), (k - 1, k - 2), (k - 7, k))[:2 if k == 1024 else 3]:
        spots = [(0, cnt2 - 1), (cnt1 - 1, 0), (cnt1 - 1, cnt2 - 1), (cnt1 // 2, min(63, cnt2 - 1))]
        if cnt2 > 64:
            spots += [(min(64, cnt1 - 1), 64), (min(63, cnt1 - 1), 64)]
        for j1, j2 in spots:
            # mate 1: reverse hits low in the genome; mate 2: forward hits high in it -> opposite strands, wrong order
            h1 = [(R(int(rng.integers(0, 1000))), int(rng.integers(1, 60))) for _ in range(cnt1)]
            h2 = [(F(int(rng.integers(10**6, 10**6 + 1000))), int(rng.integers(1, 60))) for _ in range(cnt2)]
            h1[j1] = (F(5000), 7)
            h2[j2] = (R(5200), 9)
            pairs.append((h1, h2))
            planted.append((j1, j2))
    got = _check(*_batch(pairs, k), unpaired_penalty=1 << 20)
    assert [(int(r["j1"]), int(r["j2"])) for r in got] == planted
    assert (got["n_proper"] == 1).all() and (got["status"] == 0).all() and (got["score"] == 16).all()
    assert (got["tlen"] == 350).all()


# ------------------------------------------------------------------------------------------ 3. tie rules
def test_tie_rules():
    k = 130  # three 64-row chunks of mate 1, three strides of mate 2
    same = ([(F(100), 9)] * k, [(R(200), 9)] * k)
    # only (0, 1) and (1, 0) are proper, sum 13 each: (lo, hi) at the smaller j1 against (hi, lo) at the larger
    cross = ([(F(100), 5), (F(1000), 8)], [(R(1100), 5), (R(200), 8)])
    # the same two rows far apart, past a chunk border of mate 1 and a stride of mate 2
    far1 = [(F(100), 5)] + [(R(0), 1)] * 99 + [(F(1000), 8)]
    far2 = [(R(1100), 5)] + [(F(10**6), 1)] * 69 + [(R(200), 8)]
    # one row of mate 1 against equal scores of mate 2: the smallest j2, in the same lane (rows 1 and 65) or not
    j2a = ([(F(100), 8)], [(R(200), 3), (R(200), 8)] + [(R(200), 2)] * 63 + [(R(200), 8), (R(200), 8)])
    # unsorted lists: the top hit is the largest score, the smallest row among equals, not row 0
    tops = ([(F(100), 3)] + [(F(100), 2)] * 70 + [(F(100), 9), (F(100), 9)], [(F(100), 1), (F(100), 4), (F(100), 4)])
    got = _check(*_batch([same, cross, (far1, far2), j2a, tops], k), max_tlen=300)
    want = [(0, 0, 18, 0, k * k), (0, 1, 13, 0, 2), (0, 70, 13, 0, 2), (0, 1, 16, 0, 67), (71, 1, 13, 1, 0)]
    assert [tuple(int(r[f]) for f in ("j1", "j2", "score", "status", "n_proper")) for r in got] == want


# ------------------------------------------------------------------------------------------ 4. bounds
def test_template_length_and_penalty_bounds():
    lo, hi = 200, 400
    pairs = [([(F(1000), 50)], [(R(1000 + t - REF_LEN), 50)]) for t in (lo - 1, lo, hi, hi + 1)]
    pairs += [([(R(1000 + t - REF_LEN), 50)], [(F(1000), 50)]) for t in (lo - 1, lo, hi, hi + 1)]
    got = _check(*_batch(pairs, 1), min_tlen=lo, max_tlen=hi)
    assert got["status"].tolist() == [1, 0, 0, 1] * 2 and got["tlen"].tolist() == [0, lo, hi, 0] * 2
    # pos(f) == pos(r) is allowed, pos(f) == pos(r) + 1 is not; same-strand combinations never are
    pairs = [([(F(1000), 50)], [(R(1000), 50)]), ([(F(1001), 50)], [(R(1000), 50)]),
             ([(R(1000), 50)], [(F(1000), 50)]), ([(R(1000), 50)], [(F(1001), 50)]),
             ([(F(1000), 50)], [(F(1100), 50)]), ([(R(1000), 50)], [(R(1100), 50)])]
    got = _check(*_batch(pairs, 1))
    assert got["status"].tolist() == [0, 1, 0, 1, 1, 1] and got["tlen"].tolist() == [REF_LEN, 0, REF_LEN, 0, 0, 0]
    # a window shorter than min_tlen - ref_len is no pair either, and max_tlen < ref_len accepts nothing
    assert _check(*_batch(pairs[:1], 1), min_tlen=REF_LEN + 1, max_tlen=1000)["status"][0] == 1
    assert _check(*_batch(pairs[:1], 1), min_tlen=0, max_tlen=REF_LEN - 1)["n_proper"][0] == 0
    # the penalty: best_sum == s(t1) + s(t2) - penalty is status 0, one below is status 1
    for s, status in ((133, 0), (132, 1)):
        got = _check(*_batch([([(F(5000), 150), (F(100), s)], [(R(300), 140)])], 2), unpaired_penalty=17)
        assert (int(got["status"][0]), int(got["n_proper"][0])) == (status, 1)
    got = _check(*_batch([([(F(5000), 150), (F(100), 150)], [(R(300), 140)])], 2), unpaired_penalty=0)
    assert tuple(int(got[f][0]) for f in ("j1", "j2", "status")) == (1, 0, 0)


# ------------------------------------------------------------------------------------------ 5. liveness and counts
def test_dead_rows_and_clamped_counts():
    k = 70
    live1, live2 = (F(100), 20), (R(300), 30)
    dead_pair = ([(F(100), 0)] * 66 + [live1], [(R(300), 0)] * 65 + [live2, (R(300), 0)])
    only1 = ([(F(100), 0), live1], [(R(300), 0)] * 3)
    only2 = ([(F(100), 0)] * 2, [(R(300), 0), live2])
    none = ([(F(100), 0)] * k, [(R(300), 0)] * k)
    empty = ([], [])
    ids1, s1, c1, ids2, s2, c2 = _batch([dead_pair, only1, only2, none, empty], k)
    got = _check(ids1, s1, c1, ids2, s2, c2)
    want = [(66, 65, 50, 350, 1, 0), (1, -1, 20, 0, 0, 2), (-1, 1, 30, 0, 0, 3), (-1, -1, 0, 0, 0, 4),
            (-1, -1, 0, 0, 0, 4)]
    assert [tuple(int(r[f]) for f in P.FIELDS) for r in got] == want
    # negative counts (the rerank's error statuses) are 0 rows; counts above k are k rows
    full = ([(F(100), 5)] * k, [(R(300), 6)] * k)
    ids1, s1, c1, ids2, s2, c2 = _batch([full] * 4, k)
    c1[:], c2[:] = [-1, k + 1, 2**31 - 1, -2**31], [k, 10 * k, -3, k]
    got = _check(ids1, s1, c1, ids2, s2, c2)
    assert got["status"].tolist() == [3, 0, 2, 3] and got["n_proper"].tolist() == [0, k * k, 0, 0]


# ------------------------------------------------------------------------------------------ 6. wide ids
@pytest.mark.parametrize("base", [2**32 - 4, 2**33 - 4, 2**64 - 3000])
def test_wide_window_ids(base):
    """Window ids that cross 2^32, positions that cross 2^32, and ids up to 2^64 - 1 (positions near 2^63): T is
    computed in 64 bits."""
    rng = np.random.default_rng(3)
    n, k = 600, 8
    lo = base - 1500
    ids1, ids2 = (np.array([[(lo + int(x)) % 2**64 for x in r] for r in rng.integers(0, 3000, size=(n, k))],
                           dtype=np.uint64) for _ in range(2))
    if base == 2**64 - 3000:  # one list at the other end of the id space: differences of about 2^63 never pair
        ids2[::7] = rng.integers(0, 3000, size=ids2[::7].shape).astype(np.uint64)
        ids1[0, 0], ids2[0, 0] = 2**64 - 2, 2**64 - 1
    s1, s2 = (rng.integers(1, 150, size=(n, k)).astype(np.int32) for _ in range(2))
    c = np.full(n, k, np.int32)
    got = _check(ids1, s1, c, ids2, s2, c, min_tlen=0, max_tlen=600)
    assert (got["status"] == 0).sum() > n // 4 and (got["status"] == 1).any()
    assert got["tlen"].max() > 300


def test_n_proper_of_a_full_table_is_exact():
    k = 1024
    rng = np.random.default_rng(9)
    ids1, ids2 = np.full((1, k), F(2**31 + 5), np.uint64), np.full((1, k), R(2**31 + 205), np.uint64)
    s1, s2 = (rng.integers(1, 150, size=(1, k)).astype(np.int32) for _ in range(2))
    c = np.full(1, k, np.int32)
    got = _check(ids1, s1, c, ids2, s2, c)
    assert int(got["n_proper"][0]) == 1024 * 1024 and int(got["tlen"][0]) == 350


# ------------------------------------------------------------------------------------------ 7. more pairs than waves
def _grid_waves():
    class Props(C.Structure):
        _fields_ = [("cu_count", C.c_int32), ("clock_khz", C.c_int32), ("total_mem", C.c_int64),
                    ("lds_per_cu", C.c_int32), ("arch", C.c_char * 64)]
    from deepreadmapper_amd._native import lib
    p = Props()
    assert lib().drm_device_get_props(0, C.byref(p)) == 0
    return 32 * p.cu_count  # launch_pair_hits' grid bound for lists this short


def test_more_pairs_than_launched_waves():
    """A wave loops over pairs and reuses its LDS: longer lists followed by shorter ones, the last pair checked."""
    rng = np.random.default_rng(5)
    n, k = max(5000, _grid_waves() + 37), 6
    ids1, ids2 = (rng.integers(0, 40, size=(n, k)).astype(np.uint64) for _ in range(2))
    s1, s2 = (rng.integers(0, 4, size=(n, k)).astype(np.int32) for _ in range(2))
    c1, c2 = (rng.integers(0, k + 1, size=n).astype(np.int32) for _ in range(2))
    ids1[-1, :2], s1[-1, :2], c1[-1] = [F(3), F(9)], [2, 3], 2
    ids2[-1, :2], s2[-1, :2], c2[-1] = [R(4), R(5)], [3, 1], 2
    got = _check(ids1, s1, c1, ids2, s2, c2, ref_len=4, max_tlen=12, unpaired_penalty=2)
    assert len(got) == n > _grid_waves()
    assert tuple(int(got[f][-1]) for f in P.FIELDS) == (0, 0, 5, 5, 2, 0)  # F(3) + R(4): T = 4 + 4 - 3


# ------------------------------------------------------------------------------------------ 8. layout
def test_interleaved_layout_equals_two_arrays():
    from deepreadmapper_amd import pair_hits
    rng = np.random.default_rng(6)
    n, k = 301, 9
    ids = rng.integers(0, 3000, size=(2 * n, k)).astype(np.uint64)
    sc = rng.integers(0, 100, size=(2 * n, k)).astype(np.int32)
    cnt = rng.integers(-1, k + 2, size=2 * n).astype(np.int32)
    prm = dict(ref_len=REF_LEN, min_tlen=100, max_tlen=900, unpaired_penalty=17)
    inter = pair_hits(ids, sc, cnt, ids[1:], sc[1:], cnt[1:], row_step=2, **prm)
    split = _check(ids[0::2].copy(), sc[0::2].copy(), cnt[0::2].copy(), ids[1::2].copy(), sc[1::2].copy(),
                   cnt[1::2].copy(), **prm)
    assert len(inter) == n and inter.tobytes() == split.tobytes()
    assert set(split["status"].tolist()) >= {0, 1}
    # any other step: every third row of two separate arrays
    step3 = pair_hits(ids, sc, cnt, ids[::-1].copy(), sc[::-1].copy(), cnt[::-1].copy(), row_step=3, **prm)
    P.assert_equal(step3, P.pair_all(ids, sc, cnt, ids[::-1], sc[::-1], cnt[::-1], row_step=3, **prm))


# ------------------------------------------------------------------------------------------ 9. device form
def test_device_form_equals_host_form():
    from deepreadmapper_amd import PAIR_RESULT_DTYPE, pair_hits, pair_hits_device
    from deepreadmapper_amd.device import DeviceBuffer, Stream
    rng = np.random.default_rng(7)
    n, k = 500, 65
    ids = rng.integers(0, 5000, size=(2 * n, k)).astype(np.uint64)
    sc = rng.integers(0, 150, size=(2 * n, k)).astype(np.int32)
    cnt = rng.integers(0, k + 1, size=2 * n).astype(np.int32)
    want = pair_hits(ids, sc, cnt, ids[1:], sc[1:], cnt[1:], row_step=2, ref_len=REF_LEN)
    st = Stream()
    d_ids, d_sc, d_cnt = DeviceBuffer.from_host(ids), DeviceBuffer.from_host(sc), DeviceBuffer.from_host(cnt)
    d_out = DeviceBuffer((n,), PAIR_RESULT_DTYPE)
    pair_hits_device(d_ids, d_sc, d_cnt, d_ids.ptr + 8 * k, d_sc.ptr + 4 * k, d_cnt.ptr + 4, n, k, REF_LEN, row_step=2,
                     d_out=d_out, stream=st)
    st.synchronize()
    assert d_out.download().tobytes() == want.tobytes()
    assert set(want["status"].tolist()) >= {0, 1}


def test_device_form_chained_on_the_rerank_outputs():
    """drm_post_process_sw_dynamic_device -> drm_pair_hits_device on its d_top_ids / d_top_scores / d_status, nothing
    copied in between; equals the host call on the downloaded arrays."""
    from deepreadmapper_amd import GenomeTable, extract_fasta_sequence, pair_hits, pair_hits_device
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
            row = rng.integers(0, 2 * (len(g) - REF_LEN), size=6)
            row[int(rng.integers(5))] = w
            row[5] = 2 * len(g)
            nb.append(row)
    nb = np.array(nb, dtype=np.int64)
    nq, kk = nb.shape
    qbuf, qlen = pack_queries(reads)
    t = GenomeTable(g, REF_LEN)
    st = Stream()
    d_nb, d_q, d_ql = DeviceBuffer.from_host(nb), DeviceBuffer.from_host(qbuf), DeviceBuffer.from_host(qlen)
    d_sc, d_ids, d_st = DeviceBuffer((nq, kk), np.int32), DeviceBuffer((nq, kk), np.uint64), DeviceBuffer(nq, np.int32)
    check(lib().drm_post_process_sw_dynamic_device(t.handle, d_nb.ptr, nq, kk, d_q.ptr, d_ql.ptr, qbuf.shape[1], 1, kk,
                                                   kk, d_sc.ptr, d_ids.ptr, d_st.ptr, st.handle))
    d_out = pair_hits_device(d_ids, d_sc, d_st, d_ids.ptr + 8 * kk, d_sc.ptr + 4 * kk, d_st.ptr + 4, nq // 2, kk,
                             REF_LEN, row_step=2, stream=st)
    st.synchronize()
    got, ids, sc, cnt = d_out.download(), d_ids.download(), d_sc.download(), d_st.download()
    t.free()
    assert (cnt == kk).all() and (sc == 0).any()
    want = pair_hits(ids, sc, cnt, ids[1:], sc[1:], cnt[1:], row_step=2, ref_len=REF_LEN)
    assert got.tobytes() == want.tobytes()
    P.assert_equal(got, P.pair_all(ids, sc, cnt, ids[1:], sc[1:], cnt[1:], REF_LEN, row_step=2))
    assert got["status"].tolist() == [0, 0, 0, 0] and got["tlen"].tolist() == [t for _, t in starts]
    assert (got["score"] == 2 * REF_LEN).all()


# ------------------------------------------------------------------------------------------ 10. argument errors
def test_argument_errors_leave_the_library_usable():
    from deepreadmapper_amd import DrmError, pair_hits
    from deepreadmapper_amd._native import DRM_ERR_ARG, DRM_ERR_UNSUPPORTED
    good = _batch([([(F(100), 50)], [(R(300), 50)])], 2)

    def fails(code, arrays=good, **prm):
        prm.setdefault("ref_len", REF_LEN)
        with pytest.raises(DrmError) as e:
            pair_hits(*arrays, **prm)
        assert e.value.code == code, (prm, str(e.value))
        assert int(_check(*good)["status"][0]) == 0  # a valid call right after it
    wide = _batch([([(F(100), 50)], [(R(300), 50)])], 1025)
    fails(DRM_ERR_UNSUPPORTED, wide)
    fails(DRM_ERR_ARG, min_tlen=500, max_tlen=499)
    fails(DRM_ERR_ARG, ref_len=0)
    fails(DRM_ERR_ARG, ref_len=2**20 + 1)
    fails(DRM_ERR_ARG, min_tlen=-1)
    fails(DRM_ERR_ARG, max_tlen=2**30 + 1)
    fails(DRM_ERR_ARG, unpaired_penalty=-1)
    fails(DRM_ERR_ARG, unpaired_penalty=2**20 + 1)
    for bad in (2**20 + 1, -1):
        arrays = _batch([([(F(100), 50)], [(R(300), bad)])], 2)
        fails(DRM_ERR_ARG, arrays)
    # a score out of range in a row past the count is not looked at
    arrays = _batch([([(F(100), 50)], [(R(300), 50)])], 2)
    arrays[1][0, 1] = -7
    assert int(_check(*arrays)["status"][0]) == 0
    # k = 0 and no pairs at all are valid
    z = np.zeros((3, 0))
    got = pair_hits(z, z, np.zeros(3), z, z, np.zeros(3), ref_len=REF_LEN)
    assert got["status"].tolist() == [4, 4, 4]
    assert len(pair_hits(np.zeros((0, 4)), np.zeros((0, 4)), [], np.zeros((0, 4)), np.zeros((0, 4)), [], REF_LEN)) == 0
