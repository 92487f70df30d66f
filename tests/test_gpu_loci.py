"""GPU tests of the locus-list kernel (hit_loci.hip: drm_hit_loci and its device form): every field of every MAPQ
record, both counts and every slot of every read equal the Python restatement of the definition (tests/loci_ref.py),
over the grid k in {0, 1, 2, 63, 64, 65, 128, 1024} x max_loci in {1, 2, 5, 64} x drop_pct in {0, 80, 100} x sub_band
in {0, 2} x min_score in {0, 39} -- on random windows of both strands of a genome four spans long (loci collide), with
ids near 2^64 - 1 and spread ids, with dead rows, counts below 0 and above k, heads -1 / live / dead / out of range,
on k singleton loci of one score and on lists without a live row; the MAPQ records equal drm_hit_mapq's byte for byte,
GPU against GPU; the device form on a stream equals the host form over poisoned output buffers; every argument error
returns its code and nreads = 0 is fine."""
import numpy as np
import pytest

import loci_ref as L
import mapq_ref as M

pytestmark = pytest.mark.gpu

REF_LEN = 150
SCORES = np.array([0, 0, 30, 38, 39, 40, 75, 79, 80, 81, 98, 99, 100, 100, 120, 150], np.int32)
GRID = [(pct, band, mn) for pct in (0, 80, 100) for band in (0, 2) for mn in (0, 39)]
MAX_LOCI = (1, 2, 5, 64)


def _inputs(k):
    """(ids, scores, cnt, full, head, first singleton read, first dead read) of the batch for one k."""
    rng = np.random.default_rng(7000 + k)
    n = 6 if k == 1024 else 120 if k >= 63 else 300
    pos = rng.integers(0, 4 * REF_LEN, size=(n, k)).astype(np.uint64)
    strand = rng.integers(0, 2, size=(n, k)).astype(np.uint64)
    ids = 2 * pos + strand
    third = n // 3
    ids[third:2 * third] = 2 * (np.uint64(2**63 - 1) - pos[third:2 * third]) + strand[third:2 * third]  # up to 2^64 - 1
    contig = rng.integers(0, 3, size=(n - 2 * third, k)).astype(np.uint64)
    ids[2 * third:] += contig << np.uint64(33)  # spread ids: id + (contig << 33)
    sc = SCORES[rng.integers(0, len(SCORES), size=(n, k))]
    cnt = np.full(n, k, np.int32)
    odd = rng.random(n) < 0.3
    cnt[odd] = rng.integers(-2, k + 3, size=int(odd.sum()))
    # k singleton loci of one score (the scan takes k iterations), forward and reverse, and lists without a live row
    single = np.stack([2 * REF_LEN * np.arange(k, dtype=np.uint64), 2 * REF_LEN * np.arange(k, dtype=np.uint64)[::-1] + 1])
    ids = np.concatenate([ids, single, ids[:2]])
    sc = np.concatenate([sc, np.full((2, k), 77, np.int32), np.zeros((2, k), np.int32)])
    cnt = np.concatenate([cnt, [k, k + 5, k, k]]).astype(np.int32)
    total = len(cnt)
    full = rng.integers(140, 151, size=total).astype(np.int32)
    head = rng.integers(-3, k + 2, size=total).astype(np.int32)  # -1, live, dead, past the count, no row at all
    head[rng.random(total) < 0.4] = -1
    head[n:n + 2] = [-1, k // 2] if k else [-1, -1]
    return ids, sc, cnt, full, head, n, n + 2


def _want_arrays(want64, max_loci):
    """The restatement's result at max_loci = 64 cut to max_loci slots (n_loci = min(n_pass, max_loci): the truncation
    rule of the definition), as the arrays hit_loci returns without the records."""
    n = len(want64)
    n_pass = np.array([w[2] for w in want64], np.int32)
    slots = np.array([w[3][:max_loci] for w in want64], dtype=object).reshape(n, max_loci, 4)
    return (np.minimum(n_pass, max_loci).astype(np.int32), n_pass, slots[:, :, 0].astype(np.uint64),
            slots[:, :, 1].astype(np.int32), slots[:, :, 2].astype(np.int32), slots[:, :, 3].astype(np.int32))


def _records(want64):
    rec = np.zeros(len(want64), dtype=np.dtype([(f, np.int32) for f in M.FIELDS]))
    for r, w in enumerate(want64):
        for f in M.FIELDS:
            rec[f][r] = w[0][f]
    return rec


@pytest.mark.parametrize("k", [0, 1, 2, 63, 64, 65, 128, 1024])
def test_kernel_equals_the_restatement_over_the_grid(k):
    from deepreadmapper_amd import hit_loci, hit_mapq
    all_ids, all_sc, all_cnt, all_full, all_head, single, dead = _inputs(k)
    ids, sc, cnt, full, head = all_ids, all_sc, all_cnt, all_full, all_head
    if k == 1024:  # the restatement takes k^2 / 2 steps on k singletons: there once, below, and hand-worked on the grid
        sel = np.r_[0:single, dead:len(cnt)]
        ids, sc, cnt, full, head = ids[sel], sc[sel], cnt[sel], full[sel], head[sel]
    seen_trunc = seen_multi = False
    for with_head in (True, False):
        h = head if with_head else None
        for pct, band, mn in GRID if with_head else GRID[5:7]:
            prm = dict(ref_len=REF_LEN, min_score=mn, sub_band=band)
            want64 = L.loci_all(ids, sc, cnt, full, max_loci=64, drop_pct=pct, head=h, **prm)
            wrec = _records(want64)
            mapq = hit_mapq(ids, sc, cnt, full, head=h, **prm)  # GPU against GPU, byte for byte
            for ml in MAX_LOCI:
                got = hit_loci(ids, sc, cnt, full, max_loci=ml, drop_pct=pct, head=h, **prm)
                want = _want_arrays(want64, ml)
                what = dict(k=k, max_loci=ml, drop_pct=pct, sub_band=band, min_score=mn, head=with_head)
                same = got[0].tobytes() == wrec.tobytes() and all(
                    g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got[1:], want))
                if not same:  # name the first difference
                    L.assert_equal(got, L.loci_all(ids, sc, cnt, full, max_loci=ml, drop_pct=pct, head=h, **prm), what)
                    raise AssertionError(("the cut of the 64-slot restatement differs from the restatement", what))
                assert got[0].tobytes() == mapq.tobytes(), what
                seen_trunc |= bool((got[2] > got[1]).any())
                seen_multi |= bool((got[1] >= 3).any())
        # the cut above is the definition's own truncation: the restatement run at 5 slots says the same
        sample = slice(0, 12)
        L.assert_equal(tuple(a[sample] for a in hit_loci(ids, sc, cnt, full, max_loci=5, drop_pct=80, head=h,
                                                         ref_len=REF_LEN)),
                       L.loci_all(ids[sample], sc[sample], cnt[sample], full[sample], REF_LEN, 5, head=None if h is None
                                  else h[sample]), "direct")
    if k == 0:
        rec, n_loci, n_pass, l_ids, l_sc, l_rows, l_size = hit_loci(ids, sc, cnt, full, REF_LEN, 5)
        assert (rec["status"] == 1).all() and not n_loci.any() and not n_pass.any()
        assert (l_ids == L.EMPTY_ID).all() and not l_sc.any() and (l_rows == -1).all() and not l_size.any()
        return
    # hand-worked: the k singletons of score 77 all pass whatever the parameters; the slots are rows 0 .. in order
    ids, sc, cnt, full = all_ids, all_sc, all_cnt, all_full
    if k == 1024:
        rows = slice(single, single + 2)
        L.assert_equal(tuple(a[rows] for a in hit_loci(ids, sc, cnt, full, REF_LEN, 64, head=all_head)),
                       L.loci_all(ids[rows], sc[rows], cnt[rows], full[rows], REF_LEN, 64, head=all_head[rows]), "single")
    for ml, (pct, band, mn) in [(ml, g) for ml in MAX_LOCI for g in GRID]:
        rec, n_loci, n_pass, l_ids, l_sc, l_rows, l_size = hit_loci(ids, sc, cnt, full, REF_LEN, ml, drop_pct=pct,
                                                                    sub_band=band, min_score=mn)
        kept = min(k, ml)
        assert int(n_pass[single]) == k and int(n_loci[single]) == kept and int(rec["n_sub"][single]) == k - 1
        assert l_rows[single, :kept].tolist() == list(range(kept)) and (l_size[single, :kept] == 1).all()
        assert (l_sc[single, :kept] == 77).all() and (l_rows[single, kept:] == -1).all()
        assert l_ids[single, :kept].tolist() == ids[single, :kept].tolist()
        assert int(rec["status"][dead]) == 1 and int(n_loci[dead]) == 0 and (l_ids[dead] == L.EMPTY_ID).all()
    if k >= 63:
        assert seen_trunc and seen_multi


def test_device_form_on_a_stream_equals_the_host_form_over_poison():
    from deepreadmapper_amd import MAPQ_RESULT_DTYPE, hit_loci, hit_loci_device
    from deepreadmapper_amd.device import DeviceBuffer, Stream
    k = 65
    ids, sc, cnt, full, head, _, _ = _inputs(k)
    n = len(cnt)
    st = Stream()
    d_ids, d_sc, d_cnt = DeviceBuffer.from_host(ids), DeviceBuffer.from_host(sc), DeviceBuffer.from_host(cnt)
    d_full, d_head = DeviceBuffer.from_host(full), DeviceBuffer.from_host(head)
    for ml, (h, d_h) in ((1, (None, None)), (5, (head, d_head)), (64, (head, d_head))):
        want = hit_loci(ids, sc, cnt, full, REF_LEN, ml, head=h)
        poison = [np.full(n, 0x5A, np.uint8).repeat(MAPQ_RESULT_DTYPE.itemsize).view(MAPQ_RESULT_DTYPE),
                  np.full(n, 0x5A5A5A5A, np.int32), np.full(n, 0x5A5A5A5A, np.int32),
                  np.full((n, ml), 0x5A5A5A5A5A5A5A5A, np.uint64), np.full((n, ml), 0x5A5A5A5A, np.int32),
                  np.full((n, ml), 0x5A5A5A5A, np.int32), np.full((n, ml), 0x5A5A5A5A, np.int32)]
        bufs = [DeviceBuffer.from_host(p) for p in poison]
        out = hit_loci_device(d_ids, d_sc, d_cnt, d_full, n, k, REF_LEN, ml, d_head=d_h, d_out=bufs[0], d_n_loci=bufs[1],
                              d_n_pass=bufs[2], d_loci_ids=bufs[3], d_loci_scores=bufs[4], d_loci_rows=bufs[5],
                              d_loci_size=bufs[6], stream=st)
        st.synchronize()
        for name, b, w in zip(("records", "n_loci", "n_pass", "ids", "scores", "rows", "size"), out, want):
            assert b.download().tobytes() == w.tobytes(), (ml, name)
        L.assert_equal(want, L.loci_all(ids, sc, cnt, full, REF_LEN, ml, head=h), ml)
    # outputs left to the wrapper are allocated by it
    out = hit_loci_device(d_ids, d_sc, d_cnt, d_full, n, k, REF_LEN, 2, stream=st)
    st.synchronize()
    for b, w in zip(out, hit_loci(ids, sc, cnt, full, REF_LEN, 2)):
        assert b.download().tobytes() == w.tobytes()


def test_argument_errors_leave_the_library_usable():
    from deepreadmapper_amd import DrmError, hit_loci
    from deepreadmapper_amd._native import DRM_ERR_ARG, DRM_ERR_UNSUPPORTED
    ids = np.array([[2 * 0, 2 * 100, 2 * 200]], np.uint64)
    sc = np.array([[100, 90, 80]], np.int32)
    cnt, full = np.array([3], np.int32), np.array([150], np.int32)

    def good():
        rec, n_loci, n_pass, l_ids, l_sc, l_rows, l_size = hit_loci(ids, sc, cnt, full, REF_LEN, 5)
        assert (int(n_loci[0]), int(n_pass[0])) == (2, 2)  # the header's example
        assert l_rows[0].tolist() == [0, 2, -1, -1, -1] and l_size[0].tolist() == [2, 1, 0, 0, 0]
        assert l_sc[0].tolist() == [100, 80, 0, 0, 0] and l_ids[0].tolist() == [0, 400] + [L.EMPTY_ID] * 3

    def fails(code, *a, **prm):
        prm.setdefault("ref_len", REF_LEN)
        prm.setdefault("max_loci", 5)
        with pytest.raises(DrmError) as e:
            hit_loci(*a, **prm)
        assert e.value.code == code, (prm, str(e.value))
        good()  # a valid call right after it
    good()
    args = (ids, sc, cnt, full)
    for bad in (dict(max_loci=0), dict(max_loci=-3), dict(drop_pct=-1), dict(drop_pct=101), dict(ref_len=0),
                dict(ref_len=2**20 + 1), dict(locus_span=0), dict(locus_span=2**20 + 1), dict(min_score=-1),
                dict(min_score=2**20 + 1), dict(sub_band=-1), dict(sub_band=2**20 + 1)):
        fails(DRM_ERR_ARG, *args, **bad)
    fails(DRM_ERR_UNSUPPORTED, *args, max_loci=65)
    wide = np.zeros((1, 1025))
    fails(DRM_ERR_UNSUPPORTED, wide, wide, cnt, full)
    for s in (2**20 + 1, -1):
        bad_sc = sc.copy()
        bad_sc[0, 1] = s
        fails(DRM_ERR_ARG, ids, bad_sc, cnt, full)
    past = sc.copy()  # a score out of range in a row past the count is not looked at
    past[0, 2] = -7
    rec, n_loci, *_ = hit_loci(ids, past, np.array([2], np.int32), full, REF_LEN, 5)
    assert int(n_loci[0]) == 1 and int(rec["locus_rows"][0]) == 2
    # nothing at all is valid, and touches nothing
    e = np.zeros((0, 4))
    out = hit_loci(e, e, [], [], REF_LEN, 5)
    assert len(out[0]) == 0 and out[3].shape == (0, 5)
    good()
