"""CPU checks of what the exhaustive scans' GPU tests lean on: the numpy restatements of the two distances
(tests/exact_ref.py) against the oracle, and recall_at_k on hand-made arrays."""
import numpy as np
import pytest

import exact_ref as R
from oracle import oracle as O


def test_l2_restatement_equals_oracle_avx_order():
    """200 random pairs at d = 16, 48, 128, 144: the 8-accumulator restatement has the bits of oracle.l2_avx
    (hnswlib's L2SqrSIMD16ExtAVX), and the index-order sum differs on at least one pair, so a kernel with the wrong
    order would be caught."""
    rng = np.random.default_rng(8)
    differs = 0
    for d in (16, 48, 128, 144):
        x = rng.standard_normal((50, d)).astype(np.float32)
        y = rng.standard_normal((50, d)).astype(np.float32)
        for i in range(50):
            want = np.float32(O.l2_avx(x[i], y[i]))
            got = R.l2sqr8(y[i:i + 1], x[i])[0]
            assert got.view(np.uint32) == want.view(np.uint32), (d, i)
            differs += int(R.l2sqr_plain(y[i:i + 1], x[i])[0].view(np.uint32) != want.view(np.uint32))
    assert differs > 0


def test_adc_restatement_equals_oracle_bruteforce(c1):
    """On C1 adc_topk equals the brute force inside test_oracle_exhaustive_search_equals_bruteforce, and through it
    the oracle's exhaustive graph search (ids outside the tie group at the k-th distance)."""
    fx = c1["fx"]
    q = c1["q"][:30]
    s = O.make_index(fx)
    codes = fx.codes.reshape(fx.ntotal, -1)
    D, I = R.adc_topk(lambda x: O.pq_distance_table(s, x), codes, q, 50)
    for i in range(len(q)):
        lut = O.pq_distance_table(s, q[i])
        dist = np.zeros(fx.ntotal, dtype=np.float32)
        for m in range(fx.pq_M):
            dist = (dist + lut[m][codes[:, m]]).astype(np.float32)
        order = np.lexsort((np.arange(fx.ntotal), dist))[:50]
        assert np.array_equal(I[i], order) and np.array_equal(D[i].view(np.uint32), dist[order].view(np.uint32))
    Do, Io, _, _ = O.hnswpq_search(fx, q, 50, 4096)
    assert np.array_equal(Do.view(np.uint32), D.view(np.uint32))
    strict = D < D[:, -1:]
    assert np.array_equal(Io[strict], I[strict])


def test_topk_pads_short_results():
    base = np.zeros((3, 16), dtype=np.float32)
    base[:, 0] = [2, 1, 1]
    D, I = R.l2sqr8_topk(base, np.zeros((1, 16), np.float32), 5)
    assert I[0].tolist() == [1, 2, 0, -1, -1] and D[0, :3].tolist() == [1, 1, 4] and np.isinf(D[0, 3:]).all()


def test_recall_at_k_hand_made():
    from deepreadmapper_amd import recall_at_k
    inf = np.inf
    De = np.array([[1, 2, 3, 4]], dtype=np.float32)
    Ie = np.array([[10, 11, 12, 13]], dtype=np.int64)
    # full
    r = recall_at_k(De, Ie, De, Ie)
    assert r["id_recall"] == 1.0 and r["dist_recall"] == 1.0 and r["k"] == 4
    # none
    r = recall_at_k(np.array([[5, 6, 7, 8]], np.float32), np.array([[20, 21, 22, 23]]), De, Ie)
    assert r["id_recall"] == 0.0 and r["dist_recall"] == 0.0
    # a tie at the boundary: the approximate side returned another member of the k-th distance's tie group
    De2 = np.array([[1, 2, 3, 3]], dtype=np.float32)
    Ie2 = np.array([[10, 11, 12, 13]])
    Da2 = np.array([[1, 2, 3, 3]], dtype=np.float32)
    Ia2 = np.array([[10, 11, 13, 14]])
    r = recall_at_k(Da2, Ia2, De2, Ie2)
    assert r["id_recall"] == 0.75 and r["dist_recall"] == 1.0
    # k smaller than the row width: only the first k columns of both sides count
    r = recall_at_k(Da2, Ia2, De2, Ie2, k=2)
    assert r["id_recall"] == 1.0 and r["dist_recall"] == 1.0 and r["k"] == 2
    r = recall_at_k(Da2, Ia2, De2, Ie2, k=3)
    assert r["id_recall"] == pytest.approx(2 / 3) and r["dist_recall"] == 1.0
    # padded rows: the exact side holds 2 valid rows of 4; padding never counts as a hit on either side
    De3 = np.array([[1, 2, inf, inf], [1, 2, 3, 4]], dtype=np.float32)
    Ie3 = np.array([[10, 11, -1, -1], [1, 2, 3, 4]])
    Da3 = np.array([[1, inf, inf, inf], [1, 2, inf, inf]], dtype=np.float32)
    Ia3 = np.array([[10, -1, -1, -1], [1, 2, -1, -1]])
    r = recall_at_k(Da3, Ia3, De3, Ie3)
    assert r["id_recall_per_query"].tolist() == [0.5, 0.5]
    assert r["dist_recall_per_query"].tolist() == [0.25, 0.5]
    assert r["id_recall"] == 0.5 and r["dist_recall"] == 0.375
    # uint64 labels with the flat search's padding 2^64-1
    La = np.array([[10, 2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1]], dtype=np.uint64)
    Le = np.array([[10, 11, 2 ** 64 - 1, 2 ** 64 - 1]], dtype=np.uint64)
    r = recall_at_k(Da3[:1], La, De3[:1], Le)
    assert r["id_recall"] == 0.5 and r["dist_recall"] == 0.25
    with pytest.raises(ValueError):
        recall_at_k(De, Ie, De, Ie, k=5)
