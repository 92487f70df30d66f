"""GPU tests of the template-length scan (tlen_scan.hip: drm_tlen_scan and its device form): every field of every sample
and the whole histogram equal the Python restatement of the definition (tests/tlen_ref.py) -- on random tie-heavy lists
with dead rows and clamped counts, with the top hit and its competitor at the lane and per-lane-row boundaries for
k = 63 ... 129 and 1024 in either mate, at every class boundary (d = 0, +1, -1, equal strands at one position,
T = max_scan and one beyond, max_scan = ref_len, a MAPQ at the threshold and one below it, a dead mate under a threshold
of 0), with ids across 2^32 and at the top of the u64 range, with 20,000 pairs in one bin and more pairs than launched
waves, in the interleaved layout, through the device form adding into a filled histogram with and without samples and
chained on the rerank's device outputs, and for every argument error."""
import itertools
import os

import numpy as np
import pytest

import mapq_ref as M
import tlen_ref as T
from test_gpu_mapq import F, R, _arrays, _grid_waves

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_LEN = 150


def _check(ids1, s1, c1, ids2, s2, c2, full1, full2, what="", **prm):
    """The package's samples and histogram on the batch equal the restatement's; returns them."""
    from deepreadmapper_amd import tlen_scan
    prm.setdefault("ref_len", REF_LEN)
    got, hist = tlen_scan(ids1, s1, c1, ids2, s2, c2, full1, full2, **prm)
    want, want_hist = T.scan_all(ids1, s1, c1, ids2, s2, c2, full1, full2, **prm)
    M.assert_equal(got, want, what)
    assert hist.shape == want_hist.shape and hist.dtype == np.uint32
    assert (hist == want_hist).all(), (what, np.argwhere(hist != want_hist)[:5])
    placed = sum(1 for s in want if 1 <= s["cls"] <= 3)
    assert int(hist.sum(dtype=np.int64)) == placed
    return got, hist


def _pairs(cases, k, **prm):
    """cases = [(mate 1's rows, mate 2's rows), ...], rows as (window id, score); full = 100 for every read."""
    ids1, s1, c1 = _arrays([c[0] for c in cases], k)
    ids2, s2, c2 = _arrays([c[1] for c in cases], k)
    full = np.full(len(cases), 100, np.int32)
    return _check(ids1, s1, c1, ids2, s2, c2, full, full, **prm)


# ------------------------------------------------------------------------------------------ 1. random tie-heavy lists
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_random_lists_full_of_ties(k):
    """Positions from a range four spans wide on both strands, scores from four values, one of them dead, every count
    from -1 to k + 1; max_scan inside the range of template lengths, so every class occurs."""
    rng = np.random.default_rng(300 + k)
    n = 4000
    ids1, ids2 = (rng.integers(0, 2 * 40, size=(n, k)).astype(np.uint64) for _ in range(2))
    s1, s2 = (rng.choice([0, 5, 6, 8], size=(n, k)).astype(np.int32) for _ in range(2))
    c1, c2 = (rng.integers(-1, k + 2, size=n).astype(np.int32) for _ in range(2))
    full1, full2 = (rng.integers(6, 10, size=n).astype(np.int32) for _ in range(2))
    prm = dict(ref_len=10, locus_span=10, min_score=4, sub_band=2, max_scan=30)
    for min_mapq in (0, 20):
        got, hist = _check(ids1, s1, c1, ids2, s2, c2, full1, full2, f"min_mapq {min_mapq}", min_mapq=min_mapq, **prm)
        assert set(got["cls"].tolist()) == {0, 1, 2, 3, 4}
        assert (hist.sum(axis=1) > 0).all() and len(set(got["mapq1"].tolist())) > 2


# ------------------------------------------------------------------------------------------ 2. placement
@pytest.mark.parametrize("k", [63, 64, 65, 127, 128, 129, 1024])
def test_top_hit_and_competitor_at_the_lane_and_row_boundaries(k):
    """One mate's top hit (100) and its competitor at rows 0, 1, 63, 64, k - 1, every other row a low singleton locus far
    away; the other mate unique. A competitor of 70 leaves the mate confident (MAPQ 26 of a self score 100), one of 99
    does not: a scan that misses it, or takes another row for the top hit, changes the class or the template length."""
    spots = sorted({r for r in (0, 1, 63, 64, k - 1) if r < k})
    cases, want = [], []
    for (h, c), sub, mate in itertools.product(itertools.permutations(spots, 2), (70, 99), (0, 1)):
        rows = [(F(10**6 + 1000 * j), 1 + j % 5) for j in range(k)]
        rows[h], rows[c] = (F(5000), 100), (F(9000), sub)
        other = [(R(5200), 100)]
        cases.append((rows, other) if mate == 0 else (other, rows))
        q = M.mapq_value(100, sub, 1, 100, 39)
        want.append((1, 350, q, 60) if sub == 70 else (0, 0, q, 60))
        if mate == 1:
            want[-1] = want[-1][:2] + (60, q)
    got, hist = _pairs(cases, k, min_mapq=26)
    assert M.mapq_value(100, 70, 1, 100, 39) == 26 and M.mapq_value(100, 99, 1, 100, 39) < 26
    assert [tuple(int(s[f]) for f in T.SAMPLE_FIELDS) for s in got] == want
    assert int(hist[0, 350]) == len(cases) // 2 == int(hist.sum())


# ------------------------------------------------------------------------------------------ 3. class boundaries
def test_class_boundaries():
    u = lambda w: [(w, 100)]  # noqa: E731  a unique hit: MAPQ 60
    amb = lambda w: [(w, 100), (w + 2 * 4000, 70)]  # noqa: E731  MAPQ 26
    tie = lambda w: [(w, 100), (w + 2 * 4000, 100)]  # noqa: E731  status 0, MAPQ 0
    dead = [(F(777), 0)]
    cases = [
        (u(F(5000)), u(R(5000))),    # 0: d = 0: FR at T = ref_len
        (u(F(5000)), u(R(5001))),    # 1: d = +1
        (u(F(5001)), u(R(5000))),    # 2: d = -1: RF, T = ref_len + 1
        (u(R(5000)), u(F(5000))),    # 3: the same three with mate 1 the reverse hit
        (u(R(5001)), u(F(5000))),    # 4
        (u(R(5000)), u(F(5001))),    # 5
        (u(F(5000)), u(F(5000))),    # 6: equal strands, equal positions
        (u(R(5000)), u(R(5300))),    # 7: equal strands
        (u(F(5000)), u(R(14850))),   # 8: T = max_scan
        (u(F(5000)), u(R(14851))),   # 9: T = max_scan + 1
        (u(R(5000)), u(F(14851))),   # 10: RF one beyond
        (u(F(5000)), u(F(14851))),   # 11: same strand one beyond
        (amb(F(5000)), u(R(5200))),  # 12: mapq1 = 26
        (u(F(5000)), amb(R(5200))),  # 13: mapq2 = 26
        (amb(F(5000)), amb(R(5200))),  # 14: both
        (tie(F(5000)), u(R(5200))),  # 15: mapq1 = 0 with status 0
        (dead, u(R(5200))),          # 16: mate 1 without a live row: status 1
        (u(F(5000)), []),            # 17: mate 2 empty
        (dead, []),                  # 18
    ]
    cls = lambda got: got["cls"].tolist()  # noqa: E731
    got, hist = _pairs(cases, 2, min_mapq=26)
    assert cls(got) == [1, 1, 2, 1, 1, 2, 3, 3, 1, 4, 4, 4, 1, 1, 1, 0, 0, 0, 0]
    assert got["tlen"].tolist() == [150, 151, 151, 150, 151, 151, 150, 450, 10000, 0, 0, 0, 350, 350, 350, 0, 0, 0, 0]
    assert got["mapq1"].tolist()[12:17] == [26, 60, 26, 0, 0] and got["mapq2"].tolist()[12:18] == [60, 26, 26, 60, 60, 0]
    assert int(hist[0, 10000]) == 1 and hist.shape == (3, 10001)
    # one below the threshold, for either mate
    got, _ = _pairs(cases, 2, min_mapq=27)
    assert cls(got)[12:15] == [0, 0, 0] and cls(got)[:12] == [1, 1, 2, 1, 1, 2, 3, 3, 1, 4, 4, 4]
    # a threshold of 0 admits the tie (status 0) and still not the dead mate (status 1)
    got, _ = _pairs(cases, 2, min_mapq=0)
    assert cls(got)[12:] == [1, 1, 1, 1, 0, 0, 0]
    # the smallest max_scan: ref_len, one bin above bin 0 in use
    got, hist = _pairs(cases, 2, min_mapq=26, max_scan=REF_LEN)
    assert cls(got) == [1, 4, 4, 1, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4, 4, 0, 0, 0, 0]
    assert hist.shape == (3, 151) and hist[:, 150].tolist() == [2, 0, 1] and int(hist.sum()) == 3


# ------------------------------------------------------------------------------------------ 4. wild ids
def test_ids_across_2_32_and_at_the_top_of_the_range():
    """No histogram write for a pair that is far, however the ids would truncate; the restatement computes in Python
    integers."""
    top, u = 2**64 - 1, lambda w: [(w, 100)]  # noqa: E731
    cases = [
        (u(F(2**31 + 5)), u(R(2**31 + 205))),  # 0: ids beyond 2^32: FR at 350
        (u(F(100)), u(R(100 + 2**32))),         # 1: positions 2^32 apart: far, 150 after a 32-bit truncation
        (u(F(100)), u(R(100 + 2**31))),         # 2: ids 2^32 apart
        (u(R(100)), u(F(100 + 2**32))),         # 3: RF, far
        (u(F(100 + 2**32)), u(F(100))),         # 4: same strand, far
        (u(top), u(0)),                         # 5: reverse at 2^63 - 1 and forward at 0: FR, d = 2^63 - 1
        (u(top - 1), u(1)),                     # 6: forward at 2^63 - 1 and reverse at 0: RF
        (u(top), u(top - 1)),                   # 7: the same position on both strands: FR at ref_len
        (u(top - 1), u(top)),                   # 8
        (u(top), u(top)),                       # 9: same strand at ref_len
        (u(top - 1), u(0)),                     # 10: same strand, |d| = 2^63 - 1: T passes 2^63
        (u(top), u(1)),                         # 11
        ([(top, 100), (top - 2, 90), (1, 80)], [(0, 100), (top - 1, 100)]),  # 12: loci at the range's end; mate 2 ambiguous
    ]
    got, hist = _pairs(cases, 3, min_mapq=20)
    assert got["cls"].tolist() == [1, 4, 4, 4, 4, 4, 4, 1, 1, 3, 4, 4, 0]
    assert got["tlen"].tolist() == [350, 0, 0, 0, 0, 0, 0, 150, 150, 150, 0, 0, 0]
    assert int(hist.sum()) == 4 and hist[:, 150].tolist() == [2, 0, 1] and int(hist[0, 350]) == 1
    got, _ = _pairs(cases, 3, min_mapq=0)
    assert got["cls"].tolist()[12] == 4


# ------------------------------------------------------------------------------------------ 5. pairs and layout
def test_many_pairs_in_one_bin_and_more_pairs_than_waves():
    """Every pair adds to the same bin: 20,000 atomics on one address, from waves that loop over several pairs and reuse
    their LDS; then the same pairs with a few others among them, interleaved (row_step 2) and as two arrays."""
    from deepreadmapper_amd import tlen_scan
    n, k = max(20000, _grid_waves() + 37), 3
    one = ([(F(5000), 100), (F(5003), 90), (F(90000), 30)], [(R(5200), 100), (F(90000), 35)])
    ids1, s1, c1 = _arrays([one[0]] * n, k)
    ids2, s2, c2 = _arrays([one[1]] * n, k)
    full = np.full(n, 100, np.int32)
    got, hist = tlen_scan(ids1, s1, c1, ids2, s2, c2, full, full, REF_LEN)
    want, _ = T.scan_all(ids1[:1], s1[:1], c1[:1], ids2[:1], s2[:1], c2[:1], full, full, REF_LEN)
    assert want[0]["cls"] == 1 and want[0]["tlen"] == 350
    assert all(got[f].tolist() == [want[0][f]] * n for f in T.SAMPLE_FIELDS)
    assert int(hist[0, 350]) == n == int(hist.sum(dtype=np.int64)) and n > _grid_waves()
    # interleaved: read 2p is mate 1, read 2p + 1 mate 2; every seventh pair RF, every eleventh ambiguous
    rng = np.random.default_rng(9)
    ids, sc, cnt = np.zeros((2 * n, k), np.uint64), np.zeros((2 * n, k), np.int32), np.zeros(2 * n, np.int32)
    ids[0::2], sc[0::2], cnt[0::2] = ids1, s1, c1
    ids[1::2], sc[1::2], cnt[1::2] = ids2, s2, c2
    ids[1::14, 0] = R(4000 + rng.integers(300, 400, size=len(ids[1::14])))
    sc[0::22, 1] = 100
    ids[0::22, 1] = F(70000)
    full2 = rng.integers(100, 104, size=2 * n).astype(np.int32)
    inter, hist_i = _check(ids, sc, cnt, ids[1:], sc[1:], cnt[1:], full2, full2[1:], "interleaved", row_step=2)
    split, hist_s = tlen_scan(ids[0::2].copy(), sc[0::2].copy(), cnt[0::2].copy(), ids[1::2].copy(), sc[1::2].copy(),
                              cnt[1::2].copy(), full2[0::2].copy(), full2[1::2].copy(), REF_LEN)
    assert len(inter) == n and inter.tobytes() == split.tobytes() and (hist_i == hist_s).all()
    assert set(inter["cls"].tolist()) == {0, 1, 2} and int(inter["cls"][-1]) == int(split["cls"][-1])


# ------------------------------------------------------------------------------------------ 6. device form
def test_device_form_adds_into_the_histogram():
    from deepreadmapper_amd import TLEN_SAMPLE_DTYPE, tlen_scan, tlen_scan_device
    from deepreadmapper_amd.device import DeviceBuffer, Stream
    rng = np.random.default_rng(7)
    n, k = 500, 65
    ids = rng.integers(0, 5000, size=(2 * n, k)).astype(np.uint64)
    sc = rng.integers(0, 60, size=(2 * n, k)).astype(np.int32)
    sc[:, 0] = 150  # a read with any row at all maps uniquely
    cnt = rng.integers(0, k + 1, size=2 * n).astype(np.int32)
    full = rng.integers(140, 151, size=2 * n).astype(np.int32)
    want, want_hist = _check(ids, sc, cnt, ids[1:], sc[1:], cnt[1:], full, full[1:], row_step=2, max_scan=3000)
    assert set(want["cls"].tolist()) == {0, 1, 2, 3} and want_hist.shape == (3, 3001)
    st = Stream()
    d_ids, d_sc, d_cnt = DeviceBuffer.from_host(ids), DeviceBuffer.from_host(sc), DeviceBuffer.from_host(cnt)
    d_full = DeviceBuffer.from_host(full)
    before = rng.integers(0, 1000, size=want_hist.shape).astype(np.uint32)
    d_hist = DeviceBuffer.from_host(before)
    d_samples = DeviceBuffer((n,), TLEN_SAMPLE_DTYPE)
    lists = (d_ids, d_sc, d_cnt, d_ids.ptr + 8 * k, d_sc.ptr + 4 * k, d_cnt.ptr + 4, d_full, d_full.ptr + 4, n, k, REF_LEN)
    tlen_scan_device(*lists, d_hist, max_scan=3000, row_step=2, d_samples=d_samples, stream=st)
    st.synchronize()
    assert d_samples.download().tobytes() == want.tobytes()
    assert (d_hist.download() == before + want_hist).all()
    # without samples, accumulating a second time
    tlen_scan_device(*lists, d_hist, max_scan=3000, row_step=2, stream=st)
    st.synchronize()
    assert (d_hist.download() == before + 2 * want_hist).all()
    assert tlen_scan(ids, sc, cnt, ids[1:], sc[1:], cnt[1:], full, full[1:], REF_LEN, max_scan=3000, row_step=2,
                     samples=False)[0] is None


def test_device_form_chained_on_the_rerank_outputs():
    """drm_post_process_sw_dynamic_device -> drm_tlen_scan_device on its d_top_ids / d_top_scores / d_status, nothing
    copied in between; equal to the restatement on the downloaded arrays, and the simulated template lengths come out."""
    from deepreadmapper_amd import GenomeTable, TLEN_SAMPLE_DTYPE, extract_fasta_sequence, tlen_scan_device
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
    nb[0, 5:7] = [2 * 21, 2 * 22]  # the stride-1 neighbours of read 0's true window
    nq, kk = nb.shape
    qbuf, qlen = pack_queries(reads)
    full = (qlen - 2).astype(np.int32)
    t = GenomeTable(g, REF_LEN)
    st = Stream()
    d_nb, d_q, d_ql = DeviceBuffer.from_host(nb), DeviceBuffer.from_host(qbuf), DeviceBuffer.from_host(qlen)
    d_full = DeviceBuffer.from_host(full)
    d_sc, d_ids, d_st = DeviceBuffer((nq, kk), np.int32), DeviceBuffer((nq, kk), np.uint64), DeviceBuffer(nq, np.int32)
    d_hist = DeviceBuffer.from_host(np.zeros((3, 10001), np.uint32))
    d_samples = DeviceBuffer((nq // 2,), TLEN_SAMPLE_DTYPE)
    check(lib().drm_post_process_sw_dynamic_device(t.handle, d_nb.ptr, nq, kk, d_q.ptr, d_ql.ptr, qbuf.shape[1], 1, kk,
                                                   kk, d_sc.ptr, d_ids.ptr, d_st.ptr, st.handle))
    tlen_scan_device(d_ids, d_sc, d_st, d_ids.ptr + 8 * kk, d_sc.ptr + 4 * kk, d_st.ptr + 4, d_full, d_full.ptr + 4,
                     nq // 2, kk, REF_LEN, d_hist, row_step=2, d_samples=d_samples, stream=st)
    st.synchronize()
    got, hist = d_samples.download(), d_hist.download()
    ids, sc, cnt = d_ids.download(), d_sc.download(), d_st.download()
    t.free()
    want, want_hist = T.scan_all(ids, sc, cnt, ids[1:], sc[1:], cnt[1:], full, full[1:], REF_LEN, row_step=2)
    M.assert_equal(got, want)
    assert (hist == want_hist).all()
    assert got["cls"].tolist() == [1, 1, 1, 1] and got["tlen"].tolist() == [t for _, t in starts]


# ------------------------------------------------------------------------------------------ 7. argument errors
def test_argument_errors_leave_the_library_usable():
    from deepreadmapper_amd import DrmError, tlen_scan
    from deepreadmapper_amd._native import DRM_ERR_ARG, DRM_ERR_UNSUPPORTED
    ids, sc, cnt = _arrays([[(F(100), 50), (F(5000), 40)]], 2)
    ids2, sc2, cnt2 = _arrays([[(R(300), 50)]], 2)
    full = np.array([50], np.int32)
    args = (ids, sc, cnt, ids2, sc2, cnt2, full, full)

    def good():
        got, hist = _check(*args, min_mapq=20)
        assert (int(got["cls"][0]), int(got["tlen"][0]), int(got["mapq1"][0])) == (1, 350, 51) and int(hist[0, 350]) == 1

    def fails(code, *a, **prm):
        prm.setdefault("ref_len", REF_LEN)
        with pytest.raises(DrmError) as e:
            tlen_scan(*a, **prm)
        assert e.value.code == code, (prm, str(e.value))
        good()  # a valid call right after it
    good()
    for bad in (dict(ref_len=0), dict(ref_len=2**20 + 1), dict(locus_span=0), dict(locus_span=2**20 + 1),
                dict(min_score=-1), dict(min_score=2**20 + 1), dict(sub_band=-1), dict(sub_band=2**20 + 1),
                dict(min_mapq=-1), dict(min_mapq=61), dict(max_scan=REF_LEN - 1), dict(max_scan=2**16 + 1),
                dict(ref_len=2**16 + 1, max_scan=2**16)):
        fails(DRM_ERR_ARG, *args, **bad)
    wide = _arrays([[(F(100), 50)]], 1025)
    fails(DRM_ERR_UNSUPPORTED, *wide, *wide, full, full)
    for s in (2**20 + 1, -1):
        bad_sc = sc.copy()
        bad_sc[0, 1] = s
        fails(DRM_ERR_ARG, ids, bad_sc, cnt, ids2, sc2, cnt2, full, full)
        fails(DRM_ERR_ARG, ids2, sc2, cnt2, ids, bad_sc, cnt, full, full)
    # a score out of range in a row past the count is not looked at; max_scan at its bounds is accepted
    past = sc2.copy()
    past[0, 1] = -7
    _check(ids, sc, cnt, ids2, past, cnt2, full, full)
    _check(*args, max_scan=2**16)
    _check(*args, max_scan=REF_LEN)
    # k = 0 and nothing at all are valid
    z = np.zeros((3, 0))
    got, hist = tlen_scan(z, z, np.zeros(3), z, z, np.zeros(3), np.full(3, 150), np.full(3, 150), REF_LEN)
    assert not got.view(np.int32).any() and not hist.any()
    e = np.zeros((0, 4))
    got, hist = tlen_scan(e, e, [], e, e, [], [], [], REF_LEN)
    assert len(got) == 0 and not hist.any()
