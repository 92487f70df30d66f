"""GPU tests of the contig stage (contig_hits.hip: drm_contig_hits and its device form): every output array equals the
plain restatement of tests/contig_ref.py -- on random lists over contigs, gaps and the space past the genome, at every
boundary of a contig, for the stable compaction at the lane and chunk boundaries of k = 63 ... 129 and 1024, for tables
of 1 contig to 2^20 on both sides of the LDS threshold, with more reads than launched waves; composed with the pairing,
MAPQ and template-length kernels, which must stop relating two hits once a contig boundary lies between them; through
the device form chained on the rerank's device outputs; and for every argument error."""
import os

import numpy as np
import pytest

import contig_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("out_ids", "out_spread", "out_scores", "out_contig", "out_cnt")


def F(pos):
    return 2 * pos


def Rv(pos):
    return 2 * pos + 1


def _check(table, ids, sc, cnt, ref_len, what=""):
    """The package's five arrays on the batch equal the restatement's; returns them."""
    from deepreadmapper_amd import contig_hits
    ids, sc, cnt = np.asarray(ids, np.uint64), np.asarray(sc, np.int32), np.asarray(cnt, np.int32)
    got = contig_hits(table, ids, sc, cnt, ref_len)
    want = R.contig_hits(table.starts, table.lens, ids, sc, cnt, ref_len)
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    return got


# five contigs with gaps in front of the second to the fifth, one of exactly REF_LEN and one shorter
STARTS, LENS, REF_LEN = [0, 520, 700, 715, 1000], [500, 10, 7, 200, 300], 10
GLEN = 1300


@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_random_lists(k):
    from deepreadmapper_amd import ContigTable
    rng = np.random.default_rng(100 + k)
    n = 4000
    pos = rng.integers(0, GLEN + 40, size=(n, k))
    edge = rng.random((n, k)) < 0.3  # a third of the rows within two bases of a contig's start or last window
    t = rng.integers(0, 5, size=(n, k))
    at = np.where(rng.random((n, k)) < 0.5, np.array(STARTS)[t], (np.array(STARTS) + np.array(LENS) - REF_LEN)[t])
    pos = np.where(edge, np.maximum(at + rng.integers(-2, 3, size=(n, k)), 0), pos)
    ids = (2 * pos + rng.integers(0, 2, size=(n, k))).astype(np.uint64)
    sc = rng.integers(0, 4, size=(n, k)).astype(np.int32) * 3
    cnt = rng.integers(-1, k + 2, size=n).astype(np.int32)
    table = ContigTable(STARTS, LENS)
    got = _check(table, ids, sc, cnt, REF_LEN)
    table.free()
    assert set(np.unique(got[3]).tolist()) == {-1, 0, 1, 3, 4}  # never the contig shorter than a window
    assert (got[2][got[3] >= 0] == 0).any() and 0 < got[4].sum() < np.clip(cnt, 0, k).sum()


def test_boundaries():
    from deepreadmapper_amd import ContigTable
    table = ContigTable(STARTS, LENS)
    pos = [490, 491,        # ends exactly at contig 0's end; one base beyond
           715, 714,        # starts at contig 3's start; one base before
           505, 510,        # inside a gap; ends where contig 1 starts
           520, 519, 521,   # the contig of exactly REF_LEN
           700, 697, 705,   # the contig shorter than REF_LEN
           1290, 1291, 1300, 1301, 5000]  # the last window; past the genome's end
    ids = [s(p) for p in pos for s in (F, Rv)] + [2**63, 2**63 + 1, 2**64 - 2, 2**64 - 1, 2**41, 2**41 + 1]
    k = len(ids)
    ids = np.array([ids, ids[::-1]], dtype=np.uint64)
    sc = np.arange(1, 2 * k + 1, dtype=np.int32).reshape(2, k)
    got = _check(table, ids, sc, [k, k], REF_LEN)
    table.free()
    assert got[4].tolist() == [8, 8]
    assert got[0][0, :8].tolist() == [F(490), Rv(490), F(715), Rv(715), F(520), Rv(520), F(1290), Rv(1290)]
    assert got[0][1, :8].tolist() == got[0][0, :8].tolist()[::-1]
    assert got[3][0, :8].tolist() == [0, 0, 3, 3, 1, 1, 4, 4]
    assert got[1][0, 2] == F(715) + (3 << 33) and got[1][0, 7] == Rv(1290) + (4 << 33)


def test_boundaries_kept_rows_spelled_out():
    from deepreadmapper_amd import ContigTable
    table = ContigTable(STARTS, LENS)
    ids = np.array([[F(491), Rv(490), F(714), F(715), Rv(505), F(520), Rv(521), F(700), F(1290), Rv(1291), 2**63,
                     2**64 - 2, 2**64 - 1]], dtype=np.uint64)
    sc = np.array([[9, 0, 8, 7, 6, 0, 5, 4, 3, 2, 1, 1, 1]], dtype=np.int32)
    got = _check(table, ids, sc, [13], REF_LEN)
    table.free()
    assert got[4].tolist() == [4]
    assert got[0][0, :4].tolist() == [Rv(490), F(715), F(520), F(1290)]
    assert got[1][0, :4].tolist() == [Rv(490), F(715) + (3 << 33), F(520) + (1 << 33), F(1290) + (4 << 33)]
    assert got[2][0].tolist() == [0, 7, 0, 3] + [0] * 9 and got[3][0].tolist() == [0, 3, 1, 4] + [-1] * 9  # dead rows stay
    assert (got[0][0, 4:] == 2**64 - 1).all() and (got[1][0, 4:] == 2**64 - 1).all()


@pytest.mark.parametrize("k", [63, 64, 65, 127, 128, 129, 1024])
def test_stable_compaction(k):
    """One read per keep pattern; the score is the row number + 1, so order and scores show at once."""
    from deepreadmapper_amd import ContigTable
    table = ContigTable([100], [100])
    marks = [j for j in (0, 63, 64, k - 1) if j < k]
    only = np.zeros(k, bool)
    only[marks] = True
    pats = [only, ~only, np.arange(k) % 2 == 0, np.arange(k) % 2 == 1, np.zeros(k, bool), np.ones(k, bool)]
    rng = np.random.default_rng(k)
    pats.append(rng.random(k) < 0.5)
    keep = np.array(pats)
    ids = np.where(keep, 2 * (100 + np.arange(k) % 91), 2 * 300).astype(np.uint64) + (np.arange(k) % 2).astype(np.uint64)
    sc = np.tile(np.arange(1, k + 1, dtype=np.int32), (len(pats), 1))
    cnt = np.full(len(pats), k, np.int32)
    got = _check(table, ids, sc, cnt, 10, what=k)
    # a short count cuts the pattern, one beyond k is clamped
    got2 = _check(table, ids, sc, [k - 1, k + 1, k // 2, 1, 0, -1, k], 10, what=(k, "counts"))
    table.free()
    assert got[4].tolist() == [int(p.sum()) for p in pats]
    for r, p in enumerate(pats):
        m = int(p.sum())
        assert got[2][r, :m].tolist() == (np.flatnonzero(p) + 1).tolist()
        assert not got[2][r, m:].any() and (got[3][r, m:] == -1).all() and (got[0][r, m:] == R.FILL).all()
    assert got2[4][4] == 0 and got2[4][5] == 0 and got2[4][0] == int(only[:k - 1].sum())


def _sizes():
    from deepreadmapper_amd.contigs import lds_max
    lim = lds_max()
    return sorted({1, 2, 3, 65536, 2**20, lim - 1, lim, lim + 1})


def test_table_sizes_on_both_sides_of_the_lds_threshold():
    """Contig t is [3 t, 3 t + 2), ref_len 2: a window fits at the contig's start only. Hits in the first, a middle and
    the last contig, beside windows that touch the gap behind them and random ones."""
    from deepreadmapper_amd import ContigTable
    from deepreadmapper_amd.contigs import lds_max
    assert 1 < lds_max() < 65536  # so the sizes below sit on both sides
    rng = np.random.default_rng(7)
    for n in _sizes():
        table = ContigTable(np.arange(n, dtype=np.int64) * 3, np.full(n, 2, np.int64))
        mid = n // 2
        marks = [0, mid, n - 1]
        row = [F(3 * t) for t in marks] + [Rv(3 * t + 1) for t in marks] + [Rv(3 * t) for t in marks] + [F(3 * n)]
        rnd = rng.integers(0, 2 * 3 * n + 8, size=(40, len(row)))
        ids = np.concatenate([[row], rnd]).astype(np.uint64)
        sc = rng.integers(0, 5, size=ids.shape).astype(np.int32)
        got = _check(table, ids, sc, np.full(len(ids), len(row)), 2, what=n)
        table.free()
        assert got[4][0] == 6 and got[3][0, :6].tolist() == marks + marks
        assert got[1][0, 2] == F(3 * (n - 1)) + ((n - 1) << 33)
        assert got[4][1:].sum() > 0


def _grid_waves():
    from deepreadmapper_amd.device import device_props
    return 32 * device_props(0)["cu_count"]  # the launcher's grid bound for a table this small


def test_more_reads_than_launched_waves():
    """A wave loops over reads: a full list followed by shorter ones, the last read checked by hand."""
    from deepreadmapper_amd import ContigTable
    rng = np.random.default_rng(5)
    n, k = max(5000, _grid_waves() + 37), 5
    table = ContigTable(STARTS, LENS)
    ids = (2 * rng.integers(0, GLEN + 20, size=(n, k)) + rng.integers(0, 2, size=(n, k))).astype(np.uint64)
    sc = rng.integers(0, 50, size=(n, k)).astype(np.int32)
    cnt = rng.integers(0, k + 1, size=n).astype(np.int32)
    ids[-1], sc[-1], cnt[-1] = [F(495), Rv(1000), F(2000), Rv(100), F(3)], [1, 2, 3, 4, 5], 4
    got = _check(table, ids, sc, cnt, REF_LEN)
    table.free()
    assert len(got[4]) == n > _grid_waves()
    assert got[4][-1] == 2 and got[0][-1, :2].tolist() == [Rv(1000), Rv(100)] and got[3][-1].tolist() == [4, 0, -1, -1, -1]


# ------------------------------------------------------------------------ composition with the pair-level kernels
def test_spread_ids_keep_the_pair_level_kernels_inside_a_contig():
    """Two hits 100 bases apart: on one contig the pairing, the locus scan and the template-length scan relate them as
    they do with the real ids; with a contig boundary between them they no longer do."""
    from deepreadmapper_amd import ContigTable, contig_hits, hit_mapq, pair_hits, tlen_scan
    rl = 50
    table = ContigTable([0, 2000], [2000, 2000])  # adjoining: nothing but the table separates positions 1999 and 2000
    full = np.array([rl], np.int32)

    def lists(w1, w2):
        """(mate 1, mate 2) one-row lists and the two-row list of both hits, real and spread"""
        out = []
        for ids, sc in (([[w1]], [[rl]]), ([[w2]], [[rl]]), ([[w1, w2 - (w2 & 1)]], [[rl, rl - 5]])):
            ids, sc = np.array(ids, np.uint64), np.array(sc, np.int32)
            oi, osp, osc, oc, ocnt = contig_hits(table, ids, sc, [ids.shape[1]], rl)
            assert np.array_equal(oi, ids) and np.array_equal(osc, sc) and ocnt[0] == ids.shape[1]
            out.append((oi, osp, osc, ocnt))
        return out

    for (w1, w2), same in (((F(1800), Rv(1900)), True), ((F(1900), Rv(2000)), False)):
        m1, m2, both = lists(w1, w2)
        for use in (0, 1):  # the real ids, then the spread ids
            pr = pair_hits(m1[use], m1[2], m1[3], m2[use], m2[2], m2[3], rl, max_tlen=1000)
            hm = hit_mapq(both[use], both[2], both[3], full, rl, locus_span=150)
            smp, hist = tlen_scan(m1[use], m1[2], m1[3], m2[use], m2[2], m2[3], full, full, rl)
            related = same or use == 0
            assert int(pr["n_proper"][0]) == (1 if related else 0), (same, use)
            assert int(pr["status"][0]) == (0 if related else 1) and int(pr["tlen"][0]) == (150 if related else 0)
            assert int(hm["locus_rows"][0]) == (2 if related else 1), (same, use)
            assert int(hm["n_sub"][0]) == (0 if related else 1) and int(hm["sub_score"][0]) == (0 if related else rl - 5)
            assert int(smp["cls"][0]) == (1 if related else 4) and int(smp["tlen"][0]) == (150 if related else 0)
            assert int(hist.sum()) == (1 if related else 0)
    table.free()


def test_device_form_chained_on_the_rerank_outputs():
    """drm_post_process_sw_dynamic_device -> drm_contig_hits_device -> drm_hit_mapq_device on the spread ids, nothing
    copied in between; equal to the restatement on the downloaded arrays."""
    import mapq_ref as M
    from deepreadmapper_amd import ContigTable, GenomeTable, contig_hits_device, extract_fasta_sequence, hit_mapq_device
    from deepreadmapper_amd._native import check, lib
    from deepreadmapper_amd.device import DeviceBuffer, Stream
    from deepreadmapper_amd.rerank import pack_queries
    rl = 150
    g = np.frombuffer(extract_fasta_sequence(os.path.join(GOLDEN, "ecoli_150.fna")), dtype=np.uint8).copy()
    starts, lens = [0, 340, 640], [300, 300, len(g) - 640]  # a gap, then two adjoining contigs
    rng = np.random.default_rng(8)
    true = [20, 149, 150, 151, 340, 489, 491, 640, len(g) - rl]  # 151 and 491 straddle a contig's end
    reads = [b"<" + bytes(g[p:p + rl]) + b">" for p in true]
    nb = rng.integers(0, 2 * (len(g) - rl), size=(len(true), 8))
    nb[:, 3] = [2 * p for p in true]
    nb[:, 7] = 2 * len(g)  # a window past the genome end
    nb = nb.astype(np.int64)
    nq, kk = nb.shape
    qbuf, qlen = pack_queries(reads)
    full = (qlen - 2).astype(np.int32)
    t, table = GenomeTable(g, rl), ContigTable(starts, lens)
    st = Stream()
    d_nb, d_q, d_ql = DeviceBuffer.from_host(nb), DeviceBuffer.from_host(qbuf), DeviceBuffer.from_host(qlen)
    d_full = DeviceBuffer.from_host(full)
    d_sc, d_ids, d_st = DeviceBuffer((nq, kk), np.int32), DeviceBuffer((nq, kk), np.uint64), DeviceBuffer(nq, np.int32)
    check(lib().drm_post_process_sw_dynamic_device(t.handle, d_nb.ptr, nq, kk, d_q.ptr, d_ql.ptr, qbuf.shape[1], 1, kk,
                                                   kk, d_sc.ptr, d_ids.ptr, d_st.ptr, st.handle))
    d_out = contig_hits_device(table, d_ids, d_sc, d_st, nq, kk, rl, stream=st)
    d_hit = hit_mapq_device(d_out[1], d_out[2], d_out[4], d_full, nq, kk, rl, stream=st)
    st.synchronize()
    ids, sc, cnt = d_ids.download(), d_sc.download(), d_st.download()
    got = [b.download() for b in d_out]
    hit = d_hit.download()
    t.free()
    table.free()
    assert (cnt == kk).all()
    want = R.contig_hits(starts, lens, ids, sc, cnt, rl)
    for name, a, b in zip(NAMES, got, want):
        assert np.array_equal(a, b), name
    M.assert_equal(hit, M.hit_all(got[1], got[2], got[4], full, rl))
    top = [int(got[0][r, hit["best"][r]]) if hit["status"][r] == 0 else None for r in range(nq)]
    for r, p in enumerate(true):
        if p in (151, 491):
            assert 2 * p not in got[0][r].tolist() and (top[r] is None or hit["best_score"][r] < rl)
        else:
            assert top[r] == 2 * p and hit["best_score"][r] == rl
    assert (got[4] < kk).all()  # the window past the end is gone from every list


# ------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_leave_the_library_usable():
    from deepreadmapper_amd import ContigTable, DrmError, contig_hits
    from deepreadmapper_amd._native import DRM_ERR_ARG, DRM_ERR_UNSUPPORTED, lib, ptr
    table = ContigTable(STARTS, LENS)
    ids, sc, cnt = np.array([[F(3), F(600)]], np.uint64), np.array([[4, 5]], np.int32), np.array([2], np.int32)

    def good():
        got = _check(table, ids, sc, cnt, REF_LEN)
        assert got[4].tolist() == [1] and got[0][0].tolist() == [F(3), 2**64 - 1]
    good()

    class NoTable:
        handle = None
    for code, args in ((DRM_ERR_ARG, (NoTable, ids, sc, cnt, REF_LEN)), (DRM_ERR_ARG, (table, ids, sc, cnt, 0)),
                       (DRM_ERR_ARG, (table, ids, sc, cnt, 2**20 + 1)),
                       (DRM_ERR_UNSUPPORTED, (table, np.zeros((1, 1025)), np.zeros((1, 1025)), [1], REF_LEN))):
        with pytest.raises(DrmError) as e:
            contig_hits(*args)
        assert e.value.code == code, str(e.value)
        good()
    # the raw entry point: a negative nreads, null pointers, outputs that overlap an input or each other
    oi, osp = np.zeros_like(ids), np.zeros_like(ids)
    osc, oc, ocnt = np.zeros_like(sc), np.zeros_like(sc), np.zeros_like(cnt)
    h = table.handle

    def call(nreads=1, k=2, a_ids=ids, a_sc=sc, a_cnt=cnt, o=(oi, osp, osc, oc, ocnt)):
        return lib().drm_contig_hits(h, REF_LEN, ptr(a_ids), ptr(a_sc), ptr(a_cnt), nreads, k, *[ptr(x) for x in o])
    assert call() == 0 and ocnt[0] == 1
    assert call(nreads=-1) == DRM_ERR_ARG
    assert call(k=-1) == DRM_ERR_UNSUPPORTED
    for miss in range(5):
        assert call(o=[None if x == miss else b for x, b in enumerate((oi, osp, osc, oc, ocnt))]) == DRM_ERR_ARG
    assert call(a_ids=None) == DRM_ERR_ARG and call(a_sc=None) == DRM_ERR_ARG and call(a_cnt=None) == DRM_ERR_ARG
    assert call(o=(ids, osp, osc, oc, ocnt)) == DRM_ERR_ARG   # in place
    assert call(o=(oi, osp, sc, oc, ocnt)) == DRM_ERR_ARG
    assert call(o=(oi, osp, osc, oc, cnt)) == DRM_ERR_ARG
    assert call(o=(oi, oi, osc, oc, ocnt)) == DRM_ERR_ARG     # two outputs in one array
    assert call(o=(oi, osp, osc, osc, ocnt)) == DRM_ERR_ARG
    assert lib().drm_contig_hits_device(None, REF_LEN, None, None, None, 1, 2, None, None, None, None, None,
                                        None) == DRM_ERR_ARG
    assert lib().drm_contig_hits_device(h, REF_LEN, None, None, None, 1, 2, None, None, None, None, None,
                                        None) == DRM_ERR_ARG
    good()
    # k = 0 and nothing at all are valid
    z = np.zeros((3, 0))
    got = contig_hits(table, z, z, np.ones(3), REF_LEN)
    assert got[4].tolist() == [0, 0, 0] and got[0].shape == (3, 0)
    e = np.zeros((0, 4))
    assert len(contig_hits(table, e, e, [], REF_LEN)[4]) == 0
    table.free()
