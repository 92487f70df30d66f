"""Every kernel `launch_l2_rerank` (l2_rerank.hip) can pick, each compared bit for bit with the oracle (0-ulp distances
and ids in order, as test_gpu_l2.py does) on one embedded table of 3,000 windows. The launcher chooses by the number
of candidates per query: up to 128 the fused kernel, more the staged distance kernel (64 candidates per block, the
last block partial) and a register sort of 4, 8 or 16 keys per lane (switching at 256 and 512), up to 1024. A query
whose first k + 1 sorted distances hold an exact tie is handed to the heap replay, which strides over its list.
* dense lists of 127 to 1024 labels on both sides of every switch, for k = 1, 64, 65, kk - 1, kk; 1025 refused, an
  invalid label in the last partial block reported;
* one exact tie placed at the sorted positions around each register boundary (63 | 64, 127 | 128, 255 | 256,
  511 | 512), where the tie test reads lane 0 of the next register;
* more tied queries than one pass of the replay grid holds, at 1024 and at 300 candidates;
* sparse lists of 129 and 400 candidates through the 4- and 8-key sorts."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

N_WIN = 3000
EQ_A, EQ_B = 5, 6  # two equal windows: equal embeddings, an exact tie between different ids


@pytest.fixture(scope="module")
def enc():
    from deepreadmapper_amd import Encoder
    e = Encoder()
    yield e
    e.free()


def _download_table(t):
    from deepreadmapper_amd._native import lib
    from deepreadmapper_amd.rerank import window_embeddings_ptr
    p, d = window_embeddings_ptr(t)
    assert p and d == 128
    out = np.empty((t.n_ref, d), dtype=np.float32)
    assert lib().drm_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), out.nbytes) == 0
    return out


@pytest.fixture(scope="module")
def table(enc):
    """(handle, its embedding rows, a pool of 640 query embeddings), shared and left unchanged"""
    from deepreadmapper_amd.rerank import WindowTable, embed_windows
    rng = np.random.default_rng(11)
    win = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(N_WIN, 150))]
    win[EQ_A] = win[EQ_B]
    t = WindowTable(win)
    embed_windows(t, enc)
    emb = _download_table(t)
    assert np.array_equal(emb[EQ_A], emb[EQ_B])
    pool = enc.vectorize([bytes(win[i][::-1]) for i in rng.integers(0, N_WIN, size=640)])
    yield t, emb, pool
    t.free()


def _both(table, nb, qe, stride, kc):
    from deepreadmapper_amd.rerank import l2_rerank_arrays
    t, emb, _ = table
    d, ids, counts = l2_rerank_arrays(t, nb, qe, stride, kc)
    rc, wd, wi, st = O.post_process_l2_static(emb, nb, qe, stride, kc)
    assert rc == 0 and (counts == kc).all()
    bad = np.flatnonzero((d.view(np.uint32) != wd.view(np.uint32)).any(axis=1) | (ids != wi).any(axis=1))
    assert bad.size == 0, f"{bad.size} queries differ from the oracle, first {bad[:8]}"
    return wd, wi


def _raises(code, text, fn):
    from deepreadmapper_amd._native import DrmError
    with pytest.raises(DrmError) as e:
        fn()
    assert e.value.code == code and text in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------ 9. switch points
def _dense_lists(rng, kk):
    """18 lists of kk labels: 6 drawn with repeats, 6 of distinct windows, each with the last label repeating the
    first (an exact tie, handed to the replay once it lies among the first k + 1); 6 of distinct windows without any
    repeat (no tie: the sorted rows are written by the sort kernel itself)"""
    free = np.setdiff1d(np.arange(N_WIN), [EQ_B])
    nb = np.stack([rng.integers(0, N_WIN, size=kk) for _ in range(6)] +
                  [rng.choice(free, size=kk, replace=False) for _ in range(12)]).astype(np.int64)
    nb[:12, -1] = nb[:12, 0]
    return nb


@pytest.mark.parametrize("kk", [127, 128, 129, 192, 193, 256, 257, 512, 513, 1023, 1024])
def test_dense_switch_points(table, kk):
    """127 | 128 | 129: the fused kernel and the staged one with a last block of one row; 256 | 257 and 512 | 513: the
    4-, 8- and 16-key sorts; 192 | 193 and 1023 | 1024: a full and a partial last block of 64 candidates"""
    rng = np.random.default_rng(9000 + kk)
    nb = _dense_lists(rng, kk)
    qe = table[2][rng.integers(0, 640, size=len(nb))]
    for kc in sorted({1, 64, 65, kk - 1, kk}):
        _both(table, nb, qe, 1, kc)


def test_dense_limits(table):
    """1025 labels are refused (DRM_ERR_UNSUPPORTED). 129 labels with an invalid one at position 128 -- the only row of
    the staged kernel's last block, reported through ncand -- or at position 0: "Invalid mapping index" (DRM_ERR_ARG),
    as the reference throws. The handle stays usable after each."""
    from deepreadmapper_amd._native import DRM_ERR_ARG, DRM_ERR_UNSUPPORTED
    from deepreadmapper_amd.rerank import l2_rerank_arrays
    t, emb, pool = table
    rng = np.random.default_rng(9100)
    qe = pool[:6]
    nb = rng.integers(0, N_WIN, size=(6, 1025)).astype(np.int64)
    _raises(DRM_ERR_UNSUPPORTED, "1024", lambda: l2_rerank_arrays(t, nb, qe, 1, 5))
    _both(table, nb[:, :1024], qe, 1, 5)
    good = np.ascontiguousarray(nb[:, :129])
    for pos, label in ((128, -1), (0, -1), (128, N_WIN), (64, 1 << 40)):
        bad = good.copy()
        bad[4, pos] = label
        _raises(DRM_ERR_ARG, "Invalid mapping index", lambda: l2_rerank_arrays(t, bad, qe, 1, 5))
        _both(table, good, qe, 1, 129)


# ------------------------------------------------------------------------------------------ 10. ties at the boundaries
# One exact tie at sorted positions (t, t + 1). The sort kernels see it when t < k and hand the query to the replay;
# at t = b - 1 the tied neighbour is lane 0 of the next register (sorted_tie's nx_wrap). If that were missed, the row
# would come out in (distance, list position) order, so each (boundary, candidates) case needs a query whose
# partial_sort row differs from that order: the seeds below were searched (from 0 up) until one does for k = b and
# for k = b + 1; the order depends only on the permutation drawn from the seed, not on the distances' values, and the
# test checks it again before it runs.
TIE_SEEDS = {(64, 128): 0, (64, 129): 0, (128, 130): 0, (256, 258): 0, (512, 514): 0}
TIE_QUERIES = 6  # per tied position: 4 with the two equal windows as the pair, 2 with one label twice


def _tie_designs(b, nc):
    """(t, perm, twice) per designed query: list position p holds the window of sorted rank perm[p]; the ranks t and
    t + 1 are the tied pair"""
    rng = np.random.default_rng(TIE_SEEDS[b, nc])
    return [(t, rng.permutation(nc), j >= 4) for t in (b - 2, b - 1, b) for j in range(TIE_QUERIES)]


def _stable_order(dist, k):
    return np.lexsort((np.arange(len(dist)), dist))[:k]


def _tie_shows(perm, t, k):
    """libstdc++'s partial_sort of a list with this rank pattern differs from the (distance, position) order"""
    r = perm.astype(np.float32)
    r[perm == t + 1] = t
    return not np.array_equal(O.stl_partial_sort_asc_f32(r, k), _stable_order(r, k))


def _tie_lists(table, designs, nc):
    """the designed lists on the real distances: per query the windows sorted by their distance to it, all distinct
    but the pair, taken around the pair's own distance"""
    _, emb, pool = table
    every = np.arange(N_WIN, dtype=np.int64)[None]
    nb, qe = [], []
    cursor = 0
    for t, perm, twice in designs:
        while True:  # the next query of the pool that has enough windows on either side of the pair
            assert cursor < len(pool), "query pool exhausted"
            q = pool[cursor:cursor + 1]
            cursor += 1
            _, wd, wi, _ = O.post_process_l2_static(emb, every, q, 1, N_WIN)
            order = np.lexsort((wi[0], wd[0].view(np.uint32)))
            d, w = wd[0][order].view(np.uint32), wi[0][order].astype(np.int64)
            pair = (int(w[N_WIN // 2]),) * 2 if twice else (EQ_A, EQ_B)
            d_pair = d[w == pair[0]][0]
            _, first, counts = np.unique(d, return_index=True, return_counts=True)
            keep = first[counts == 1]  # windows whose distance no other window shares
            keep = keep[(d[keep] != d_pair) & ~np.isin(w[keep], pair)]
            at = int(np.searchsorted(d[keep], d_pair))
            if at >= t and len(keep) - at >= nc - 2 - t:
                break
        ranked = np.concatenate([w[keep[at - t:at]], pair, w[keep[at:at + nc - 2 - t]]])
        assert len(ranked) == nc
        nb.append(ranked[perm])
        qe.append(q[0])
    return np.array(nb, np.int64), np.array(qe, np.float32)


@pytest.mark.parametrize("b,nc", sorted(TIE_SEEDS))
def test_tie_at_register_boundary(table, b, nc):
    """b = 64 in the fused kernel (128 candidates) and in l2_sort_kernel<4> (129); 128, 256 and 512 at the smallest
    count that holds positions up to b + 1: <4> at 130, <8> at 258, <16> at 514. For the tie at (b - 2, b - 1),
    (b - 1, b) and (b, b + 1): k = b + 1 and k = b see the tie at (b - 1, b) (positions [0, k] are checked), k = b - 1
    does not."""
    designs = _tie_designs(b, nc)
    for k in (b, b + 1):
        assert any(_tie_shows(perm, t, k) for t, perm, twice in designs if t == b - 1 and not twice), (b, nc, k)
    nb, qe = _tie_lists(table, designs, nc)
    dist = [np.array([O.calc_l2_dist(table[1][w], qe[q]) for w in nb[q]], np.float32) for q in range(len(nb))]
    for k in (b - 1, b, b + 1):
        wd, wi = _both(table, nb, qe, 1, k)
        ties = [(np.diff(wd_q.view(np.uint32)) == 0).sum() for wd_q in wd]
        shows = 0
        for q, (t, perm, twice) in enumerate(designs):
            assert ties[q] == (1 if t + 1 < k else 0), (q, t, k)  # exactly the designed tie, when both are among the k
            shows += t == b - 1 and not np.array_equal(nb[q][_stable_order(dist[q], k)], wi[q].astype(np.int64))
        assert k == b - 1 or shows > 0, (b, nc, k)  # a missed tie at the register boundary would change a row


# ------------------------------------------------------------------------------------------ 11. replay at scale
@pytest.mark.parametrize("kk,n_tied,n_free", [(1024, 600, 0), (300, 200, 20)])
def test_replay_past_one_grid_pass(table, kk, n_tied, n_free):
    """Labels drawn from 6 windows (two of them equal): every such query is full of exact ties and goes to the replay.
    At 1024 candidates the replay runs 4 threads per block (its heap is LDS) in at most 128 blocks, so one pass holds
    512 queries and 600 force the stride; at 300 candidates 200 tied queries mix with 20 tie-free ones."""
    rng = np.random.default_rng(9200 + kk)
    nb = rng.choice(np.arange(EQ_A, EQ_A + 6), size=(n_tied + n_free, kk)).astype(np.int64)
    free = np.setdiff1d(np.arange(N_WIN), [EQ_B])
    for q in range(n_free):
        nb[q * (n_tied // max(n_free, 1))] = rng.choice(free, size=kk, replace=False)
    qe = table[2][rng.integers(0, 640, size=len(nb))]
    for kc in (kk, 37):
        _both(table, nb, qe, 1, kc)


# ------------------------------------------------------------------------------------------ 12. sparse lists
@pytest.mark.parametrize("stride,kk", [(3, 43), (2, 200)])
def test_sparse_through_sort_kernels(table, stride, kk):
    """kk * stride = 129 and 400 stream entries per query: l2_sort_kernel<4> and <8> on the reference's global
    expansion stream"""
    rng = np.random.default_rng(9300 + stride)
    nq = 60
    nb = rng.integers(0, N_WIN // stride, size=(nq, kk)).astype(np.int64)
    qe = table[2][rng.integers(0, 640, size=nq)]
    for kc in (kk * stride, 50, 1):
        _both(table, nb, qe, stride, kc)
