"""Numpy restatements of the exhaustive scans' definition -- TEST INFRASTRUCTURE ONLY.

adc_topk:    PQ-ADC, the sequential fp32 sum of the query's distance-table entries, then the k smallest under
             (distance, id).
l2sqr8_topk: squared L2 in hnswlib's L2SqrSIMD16ExtAVX order (8 accumulators over dims i, i + 8, ..., added left
             to right, no fusion), then the k smallest under (distance, row).
Both pad a short result with (+inf, -1)."""
import numpy as np


def _topk(dist, k):
    n = dist.shape[0]
    order = np.lexsort((np.arange(n), dist))[:k]
    D = np.full(k, np.inf, dtype=np.float32)
    I = np.full(k, -1, dtype=np.int64)
    D[:len(order)] = dist[order]
    I[:len(order)] = order
    return D, I


def adc_dist(lut, codes):
    """dist(i) = (((lut[0][c_i0] + lut[1][c_i1]) + ...) + lut[M-1][c_i,M-1]) in fp32, from +0.0."""
    lut = np.asarray(lut, dtype=np.float32)
    dist = np.zeros(codes.shape[0], dtype=np.float32)
    for m in range(lut.shape[0]):
        dist = (dist + lut[m][codes[:, m]]).astype(np.float32)
    return dist


def adc_topk(lut_fn, codes, q, k):
    """lut_fn(x) -> [M][ksub] f32 distance table of one query; codes [ntotal][M] sub-quantizer indices."""
    q = np.asarray(q, dtype=np.float32)
    D = np.empty((len(q), k), dtype=np.float32)
    I = np.empty((len(q), k), dtype=np.int64)
    for i in range(len(q)):
        D[i], I[i] = _topk(adc_dist(lut_fn(q[i]), codes), k)
    return D, I


def l2sqr8(base, x):
    """The distance of one query x [d] to every row of base [n][d], d % 16 == 0."""
    base = np.asarray(base, dtype=np.float32)
    x = np.asarray(x, dtype=np.float32)
    n, d = base.shape
    assert d % 16 == 0 and x.shape == (d,)
    acc = np.zeros((n, 8), dtype=np.float32)
    for j in range(0, d, 8):
        df = (x[None, j:j + 8] - base[:, j:j + 8]).astype(np.float32)
        acc = (acc + (df * df).astype(np.float32)).astype(np.float32)
    r = acc[:, 0]
    for i in range(1, 8):
        r = (r + acc[:, i]).astype(np.float32)
    return r


def l2sqr_plain(base, x):
    """The same terms summed in index order (one accumulator): what a kernel with the wrong order would compute."""
    base = np.asarray(base, dtype=np.float32)
    x = np.asarray(x, dtype=np.float32)
    r = np.zeros(base.shape[0], dtype=np.float32)
    for j in range(base.shape[1]):
        df = (x[j] - base[:, j]).astype(np.float32)
        r = (r + (df * df).astype(np.float32)).astype(np.float32)
    return r


def l2sqr8_topk(base, q, k):
    q = np.asarray(q, dtype=np.float32)
    D = np.empty((len(q), k), dtype=np.float32)
    I = np.empty((len(q), k), dtype=np.int64)
    for i in range(len(q)):
        D[i], I[i] = _topk(l2sqr8(base, q[i]), k)
    return D, I
