"""GPU tests of the exhaustive scans (exact_scan.hip) against the numpy restatements of their
definition (tests/exact_ref.py). Every comparison is exact: D by bit pattern, I by value."""
import numpy as np
import pytest

import exact_ref as R
import tie_graphs as TG
from oracle import faiss_file, oracle as O

pytestmark = pytest.mark.gpu

U64_PAD = np.uint64(2 ** 64 - 1)


def same(D, I, Dr, Ir):
    assert D.dtype == np.float32 and D.shape == Dr.shape and I.shape == Ir.shape
    assert np.array_equal(I.astype(np.int64), Ir), np.argwhere(I.astype(np.int64) != Ir)[:5]
    assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32))


# ------------------------------------------------------------------ 1. designed integer indexes
NTOTALS = [1, 5, 63, 64, 65, 255, 256, 257, 1000, 4099]
KS = [1, 2, 63, 64, 65, 128, 1000, 1024]


def designed_queries(rng, n):
    """Zero except integer values in [0, 15] at dims 16 * m: with tie_graphs' centroids every ADC distance is the
    exact small integer sum_m (x[16 m] - code_m)^2."""
    q = np.zeros((n, TG.D), dtype=np.float32)
    q[:, ::TG.DSUB] = rng.integers(0, 16, size=(n, TG.M_PQ)).astype(np.float32)
    return q


def designed_index(directory, ntotal, hi, seed):
    """An IHNp file whose codes are random over all 8 bytes in [0, hi); the rows only make the file valid."""
    rng = np.random.default_rng(seed)
    rows, _, entry, max_level = TG.random_tie_graph(rng, ntotal)
    codes = rng.integers(0, hi, size=(ntotal, TG.M_PQ)).astype(np.uint8)
    path = TG.write_ihnp(str(directory / f"int_{ntotal}_{hi}.index"), rows, codes, entry, max_level)
    return path, codes


def integer_topk(codes, q, k):
    """The expected result in integer numpy."""
    xi = q[:, ::TG.DSUB].astype(np.int64)
    D = np.full((len(q), k), np.inf, dtype=np.float32)
    I = np.full((len(q), k), -1, dtype=np.int64)
    dist = []
    for i in range(len(q)):
        di = ((codes.astype(np.int64) - xi[i][None, :]) ** 2).sum(axis=1)
        order = np.lexsort((np.arange(len(codes)), di))
        dist.append(di[order])
        D[i, :min(k, len(order))] = di[order][:k].astype(np.float32)
        I[i, :min(k, len(order))] = order[:k]
    return D, I, dist


@pytest.mark.parametrize("ntotal", NTOTALS)
@pytest.mark.parametrize("hi", [4, 256])
def test_designed_integer_indexes(tmp_path, ntotal, hi):
    from deepreadmapper_amd import read_index
    path, codes = designed_index(tmp_path, ntotal, hi, seed=1000 * hi + ntotal)
    q = designed_queries(np.random.default_rng(ntotal + hi), 9)
    ix = read_index(path)
    try:
        for k in KS:
            Dr, Ir, _ = integer_topk(codes, q, k)
            D, I = ix.exact_search(q, k)
            same(D, I, Dr, Ir)
        if hi == 4:
            # the first k >= 2 whose cut falls inside a group of equal distances: the tie must be cut by id
            _, _, dist = integer_topk(codes, q, 1)
            for i in range(len(q)):
                cut = np.flatnonzero(dist[i][1:-1] == dist[i][2:]) + 2 if ntotal >= 3 else np.array([], np.int64)
                if ntotal == 1000:  # pigeonhole: 1,000 nodes, far fewer distinct sums of 8 squares below 16^2
                    assert len(cut) and cut[0] <= 128
                if len(cut) and cut[0] <= 1024:
                    k = int(cut[0])
                    Dr, Ir, di = integer_topk(codes, q[i:i + 1], k)
                    assert di[0][k - 1] == di[0][k]
                    D, I = ix.exact_search(q[i:i + 1], k)
                    same(D, I, Dr, Ir)
    finally:
        ix.free()


# ------------------------------------------------------------------ shared C1 references
@pytest.fixture(scope="module")
def c1_adc(c1):
    """adc_topk at k = 1024 for the 150 C1 reads with the oracle's distance table (its prefixes serve smaller k)."""
    fx = c1["fx"]
    s = O.make_index(fx)
    codes = fx.codes.reshape(fx.ntotal, -1)
    D, I = R.adc_topk(lambda x: O.pq_distance_table(s, x), codes, c1["q"], 1024)
    D.setflags(write=False)
    I.setflags(write=False)
    return D, I


@pytest.fixture(scope="module")
def c1_l2(c1):
    D, I = R.l2sqr8_topk(c1["x"], c1["q"], 1024)
    D.setflags(write=False)
    I.setflags(write=False)
    return D, I


@pytest.fixture(scope="module")
def c1_ix(c1):
    from deepreadmapper_amd import read_index
    ix = read_index(c1["index"])
    yield ix
    ix.free()


# ------------------------------------------------------------------ 2. C1 on real floats
@pytest.mark.parametrize("k", [128, 1024])
def test_c1_equals_adc_reference(c1, c1_ix, c1_adc, k):
    """All 150 reads: the LUT order and the sequential sum at 0 ulp on real floats."""
    D, I = c1_ix.exact_search(c1["q"], k)
    same(D, I, c1_adc[0][:, :k], c1_adc[1][:, :k])


# ------------------------------------------------------------------ 3. graph against scan
def test_graph_search_against_scan(c1, c1_ix):
    from deepreadmapper_amd import recall_at_k
    q = c1["q"][:40]
    Dg, Ig, _ = c1_ix.search(q, 50, 2048)
    De, Ie = c1_ix.exact_search(q, 1024)
    assert np.array_equal(Dg.view(np.uint32), De[:, :50].view(np.uint32))
    strict = Dg < Dg[:, -1:]
    assert np.array_equal(Ig[strict], Ie[:, :50][strict])
    assert (De[:, 1023] > De[:, 49]).all()  # the scan's 1,024 rows hold the whole tie group at the 50th distance
    for i in range(len(q)):  # the remaining ids lie inside that group
        group = set(Ie[i][De[i] == De[i, 49]].tolist())
        assert set(Ig[i][~strict[i]].tolist()) <= group
        assert len(set(Ig[i].tolist())) == 50
    r = recall_at_k(Dg, Ig, De, Ie, k=50)
    assert r["dist_recall"] == 1.0 and (r["dist_recall_per_query"] == 1.0).all()


# ------------------------------------------------------------------ 4. tiling invariance
def test_slice_rows_do_not_change_the_result(tmp_path):
    from deepreadmapper_amd import read_index, set_slice_rows
    path, codes = designed_index(tmp_path, 4099, 4, seed=77)
    q = designed_queries(np.random.default_rng(5), 9)
    Dr, Ir, _ = integer_topk(codes, q, 128)
    ix = read_index(path)
    try:
        outs = []
        for rows in (64, 100, 1000, 0):
            set_slice_rows(rows)
            D, I = ix.exact_search(q, 128)
            same(D, I, Dr, Ir)
            outs.append((D.tobytes(), I.tobytes()))
        assert all(o == outs[0] for o in outs)
    finally:
        set_slice_rows(0)
        ix.free()


def test_query_batch_edges(c1, c1_ix, c1_adc):
    """Every n from 1 to 2 * QUERY_TILE + 1 gives the rows of the n = 150 call."""
    from deepreadmapper_amd import QUERY_TILE
    from deepreadmapper_amd._native import lib
    assert QUERY_TILE == lib().drm_exact_query_tile() and QUERY_TILE >= 1
    Dall, Iall = c1_ix.exact_search(c1["q"], 128)
    same(Dall, Iall, c1_adc[0][:, :128], c1_adc[1][:, :128])
    for n in range(1, 2 * QUERY_TILE + 2):
        D, I = c1_ix.exact_search(c1["q"][:n], 128)
        assert D.tobytes() == Dall[:n].tobytes() and I.tobytes() == Iall[:n].tobytes(), n


# ------------------------------------------------------------------ 5. device entry point
def test_device_entry_on_a_stream(c1, c1_ix, c1_adc):
    from deepreadmapper_amd.device import DeviceBuffer, Stream
    q = c1["q"]
    n = len(q)
    s = Stream()
    d_x = DeviceBuffer.from_host(q)
    bufs = []
    try:
        for k in (128, 37):  # back to back on one handle
            d_D, d_I = DeviceBuffer((n, k), np.float32), DeviceBuffer((n, k), np.int64)
            bufs += [d_D, d_I]
            c1_ix.exact_search_device(d_x, n, k, d_D, d_I, stream=s)
            D, I = d_D.download(), d_I.download()
            same(D, I, c1_adc[0][:, :k], c1_adc[1][:, :k])
            Dh, Ih = c1_ix.exact_search(q, k)
            assert D.tobytes() == Dh.tobytes() and I.tobytes() == Ih.tobytes()
    finally:
        for b in bufs + [d_x]:
            b.free()


def test_device_entry_unaligned_queries(c1, c1_ix, c1_adc):
    """d_x four bytes past a 16-byte boundary: the scan's fast8 switch needs aligned queries, so an 8 x 8 index then
    takes the generic kernel (QT = 1, LUT in dynamic LDS) -- with the same rows."""
    from deepreadmapper_amd.device import DeviceBuffer
    q = c1["q"][:37]
    n, d = q.shape
    host = np.zeros(n * d + 4, dtype=np.float32)
    host[1:1 + n * d] = q.ravel()
    buf = DeviceBuffer.from_host(host)
    assert buf.ptr % 16 == 0

    class _At:
        ptr = buf.ptr + 4

    bufs = [buf]
    try:
        for k in (128, 1024):
            d_D, d_I = DeviceBuffer((n, k), np.float32), DeviceBuffer((n, k), np.int64)
            bufs += [d_D, d_I]
            c1_ix.exact_search_device(_At, n, k, d_D, d_I)
            same(d_D.download(), d_I.download(), c1_adc[0][:n, :k], c1_adc[1][:n, :k])
    finally:
        for b in bufs:
            b.free()


# ------------------------------------------------------------------ 6. generic PQ shape
def test_generic_pq_shape(c1, tmp_path):
    from deepreadmapper_amd import read_index, synth
    x = np.ascontiguousarray(c1["x"][:600])
    path = str(tmp_path / "m4.index")
    synth.build_index(x, path, M_pq=4, nbits=8, M_hnsw=8, efc=40, nthreads=1)
    fx = faiss_file.read(path)
    assert fx.pq_M == 4 and fx.ntotal == 600
    s = O.make_index(fx)
    codes = fx.codes.reshape(fx.ntotal, -1)
    q = c1["q"][:20]
    ix = read_index(path)
    try:
        for k in (1, 100, 1024):
            Dr, Ir = R.adc_topk(lambda v: O.pq_distance_table(s, v), codes, q, k)
            D, I = ix.exact_search(q, k)
            same(D, I, Dr, Ir)
    finally:
        ix.free()


# ------------------------------------------------------------------ 7. fp32
@pytest.mark.parametrize("k", [1, 64, 65, 128, 1024])
def test_l2_c1(c1, c1_l2, k):
    from deepreadmapper_amd import exact_search_l2
    D, I = exact_search_l2(c1["x"], c1["q"], k)
    same(D, I, c1_l2[0][:, :k], c1_l2[1][:, :k])


@pytest.mark.parametrize("d", [16, 48, 144])
def test_l2_random_shapes(d):
    from deepreadmapper_amd import exact_search_l2
    rng = np.random.default_rng(d)
    q = rng.standard_normal((9, d)).astype(np.float32)
    for n_base in (1, 63, 64, 65, 1000):
        base = rng.standard_normal((n_base, d)).astype(np.float32)
        for k in (1, 70):
            Dr, Ir = R.l2sqr8_topk(base, q, k)
            D, I = exact_search_l2(base, q, k)
            same(D, I, Dr, Ir)


def test_l2_designed_ties_and_device_buffers():
    """300 random rows, each 3 times, shuffled: k = 1, 2, 4, 100 cut groups of equal distance, so rows come back in
    ascending row order inside a group. Also through DeviceBuffers on a stream."""
    from deepreadmapper_amd import exact_search_l2
    from deepreadmapper_amd.device import DeviceBuffer, Stream
    rng = np.random.default_rng(31)
    base = np.repeat(rng.standard_normal((300, 32)).astype(np.float32), 3, axis=0)
    base = np.ascontiguousarray(base[np.random.default_rng(7).permutation(len(base))])
    q = rng.standard_normal((9, 32)).astype(np.float32)
    d_b, d_q, s = DeviceBuffer.from_host(base), DeviceBuffer.from_host(q), Stream()
    try:
        for k in (1, 2, 4, 100):
            Dr, Ir = R.l2sqr8_topk(base, q, k)
            if k > 1:
                assert (Dr[:, 0] == Dr[:, 1]).all() and (Ir[:, 0] < Ir[:, 1]).all()
            D, I = exact_search_l2(base, q, k)
            same(D, I, Dr, Ir)
            Dd, Id = exact_search_l2(d_b, d_q, k, stream=s)
            assert Dd.tobytes() == D.tobytes() and Id.tobytes() == I.tobytes()
    finally:
        d_b.free()
        d_q.free()


# ------------------------------------------------------------------ 8. flat handle
def test_flat_handle(c1_flat, tmp_path):
    from deepreadmapper_amd import HnswFlatIndex, synth
    fx = c1_flat["fx"]
    q = c1_flat["q"]
    ix = HnswFlatIndex(c1_flat["index"])
    try:
        Dr, Ir = R.l2sqr8_topk(fx["vec"], q, 128)
        D, L = ix.exact_search(q, 128)
        assert L.dtype == np.uint64
        assert np.array_equal(L, fx["labels"].astype(np.uint64)[Ir])
        assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32))
        # the graph search never reports a pair at other bits than the scan's: every (label, distance) it returns
        # is the scan's distance of that label
        Dg, Lg, _ = ix.search(q, 30, int(ix.ntotal) + 10)
        Dall, Lall = ix.exact_search(q, 1024)
        for i in range(len(q)):
            at = {int(l): j for j, l in enumerate(Lall[i])}
            for j in range(30):
                if int(Lg[i, j]) in at:
                    assert Dg[i, j].view(np.uint32) == Dall[i, at[int(Lg[i, j])]].view(np.uint32)
    finally:
        ix.free()
    # k > ntotal: padding (+inf, 2^64-1)
    from oracle import hnswlib_file
    small = str(tmp_path / "small.hnsw")
    synth.build_flat_index(c1_flat["x"][:40], small, M=8, efc=40, nthreads=1)
    sfx = hnswlib_file.read(small)
    ix = HnswFlatIndex(small)
    try:
        Dr, Ir = R.l2sqr8_topk(sfx["vec"], q[:9], 64)
        D, L = ix.exact_search(q[:9], 64)
        assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32))
        assert np.array_equal(L[:, :40], sfx["labels"].astype(np.uint64)[Ir[:, :40]])
        assert (L[:, 40:] == U64_PAD).all() and np.isinf(D[:, 40:]).all()
    finally:
        ix.free()


def level0_unreachable(fx):
    """Nodes that no path of level-0 links reaches from the entry point."""
    n, l0 = fx["n"], fx["l0"]
    seen = np.zeros(n, dtype=bool)
    seen[fx["ep"]] = True
    stack = [int(fx["ep"])]
    while stack:
        u = stack.pop()
        for v in l0[u, 1:1 + (int(l0[u, 0]) & 0xFFFF)]:
            if not seen[v]:
                seen[v] = True
                stack.append(int(v))
    return int((~seen).sum())


def test_flat_graph_search_against_scan(c1_flat):
    """Against drm_flat_search(k = 30, ef = ntotal + 10), D is equal and dist_recall == 1.0: a graph search that may
    keep the whole index finds what the scan finds, provided every node can be reached. The c1_flat graph is built
    with 4 threads; the builder used to overwrite links that concurrently inserted elements had made to a node
    still being inserted, which left 14 to 39 of the 1,702 nodes without any path to them (469 to 798 of the
    150 x 30 distances then differed, dist_recall 0.982 to 0.991). tests/test_flat_builder_cpu.py holds the builder
    to it without a GPU. The figures are printed before the assertions."""
    from deepreadmapper_amd import HnswFlatIndex, recall_at_k
    q = c1_flat["q"]
    ix = HnswFlatIndex(c1_flat["index"])
    try:
        D, L = ix.exact_search(q, 128)
        Dg, Lg, _ = ix.search(q, 30, int(ix.ntotal) + 10)
        r = recall_at_k(Dg, Lg, D, L, k=30)
        print("flat graph vs scan: differing distances", int((Dg.view(np.uint32) != D[:, :30].view(np.uint32)).sum()),
              "of", Dg.size, "dist_recall", r["dist_recall"], "id_recall", r["id_recall"],
              "level-0 unreachable nodes", level0_unreachable(c1_flat["fx"]), "of", c1_flat["fx"]["n"])
        assert np.array_equal(Dg.view(np.uint32), D[:, :30].view(np.uint32))
        assert r["dist_recall"] == 1.0
    finally:
        ix.free()


# ------------------------------------------------------------------ 9. errors
def test_errors_leave_the_handle_usable(c1, c1_ix, c1_flat, c1_adc):
    from deepreadmapper_amd import DrmError, HnswFlatIndex, exact_search_l2
    from deepreadmapper_amd._native import DRM_ERR_ARG, DRM_ERR_UNSUPPORTED
    q = c1["q"][:4]
    fix = HnswFlatIndex(c1_flat["index"])

    def code(fn):
        with pytest.raises(DrmError) as e:
            fn()
        return e.value.code, str(e.value)

    try:
        for k in (0, 1025):
            assert code(lambda: c1_ix.exact_search(q, k))[0] == DRM_ERR_UNSUPPORTED
            assert code(lambda: fix.exact_search(q, k))[0] == DRM_ERR_UNSUPPORTED
            assert code(lambda: exact_search_l2(c1["x"], q, k))[0] == DRM_ERR_UNSUPPORTED
        empty = np.zeros((0, 128), np.float32)
        for fn in (lambda: c1_ix.exact_search(empty, 10), lambda: fix.exact_search(empty, 10),
                   lambda: exact_search_l2(c1["x"], empty, 10)):
            c, msg = code(fn)
            assert c == DRM_ERR_ARG and "Query data is empty" in msg
        wrong = np.zeros((2, 64), np.float32)
        assert code(lambda: c1_ix.exact_search(wrong, 10))[0] == DRM_ERR_ARG
        assert code(lambda: fix.exact_search(wrong, 10))[0] == DRM_ERR_ARG
        assert code(lambda: exact_search_l2(c1["x"], wrong, 10))[0] == DRM_ERR_ARG
        b24 = np.zeros((10, 24), np.float32)
        assert code(lambda: exact_search_l2(b24, b24[:2], 3))[0] == DRM_ERR_UNSUPPORTED
        # the handles still answer
        D, I = c1_ix.exact_search(q, 128)
        same(D, I, c1_adc[0][:4, :128], c1_adc[1][:4, :128])
        D, L = fix.exact_search(q, 5)
        Dr, Ir = R.l2sqr8_topk(c1_flat["fx"]["vec"], q, 5)
        assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32))
        assert np.array_equal(L, c1_flat["fx"]["labels"].astype(np.uint64)[Ir])
    finally:
        fix.free()
