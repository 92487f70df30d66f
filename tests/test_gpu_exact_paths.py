"""The paths of the exhaustive scans (exact_scan.hip) that tests/test_gpu_exact.py leaves out:
slices for the fp32 and the generic PQ kernel, the merge with labels, the query-chunk loop, the clamp to 1,024
slices, the default split into several slices, adversarial arrival orders, k with cap == k + step, the packed PQ
shapes, an empty base and the 64 KB lookup-table limit. Every comparison is exact, as in test_gpu_exact.same: D by
bit pattern, I by value, against pq_graphs.adc_reference / exact_ref.l2sqr8 sorted by (distance, id). The inputs
come from tests/exact_cases.py; tests/test_exact_cases_cpu.py proves what each does to the selection. Each test
reads the plan the library itself would run with (drm_debug_exact_plan) and asserts that it reaches what it names.

Which test reaches which path:
  exact_l2_kernel with slices > 1, a 3-row last slice, slices shorter than k      test_l2_slices
  exact_merge_kernel with labels over 11 slices, lists padded inside              test_l2_slices_with_labels
  exact_pq_kernel<1, false> with slices; nbits 5 / 6 / 10, 16-byte codes          test_generic_pq_slices
  the same kernel on an 8 x 8 index (unaligned queries) with slices               test_8x8_unaligned_slices
  run_scan's second chunk (9 queries: a full tile and one of a single query)      test_chunked, test_query_batch_edges_across_chunks
  a merge over 1,024 slices                                                       test_chunked
  the clamp to kMaxSlices (rows raised to 128, 547 slices)                        test_max_slices_clamp
  the default split giving 4 slices                                               test_default_multi_slice
  a compaction at every step, the fill exactly at cap, cap == k + step            test_arrival_orders
  the cut inside a group of equal distances that spans slices                     test_ties_at_the_cut
  n_base == 0                                                                     test_empty_base
  a 64 KB LUT beside the 16 KB sort buffer; the refusal past it                   test_lut_limit"""
import numpy as np
import pytest

import exact_cases as E

pytestmark = pytest.mark.gpu

U64_PAD = np.uint64(2 ** 64 - 1)
_TOPK = {}


def same(D, I, Dr, Ir):
    assert D.dtype == np.float32 and D.shape == Dr.shape and I.shape == Ir.shape
    assert np.array_equal(I.astype(np.int64), Ir), np.argwhere(I.astype(np.int64) != Ir)[:5]
    assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32))


def expected(tag, case, k, n=None):
    """The case's reference top-k, computed once per (case, k) and left unchanged; its first n rows."""
    if (tag, k) not in _TOPK:
        _TOPK[tag, k] = E._frozen(*E.topk_of(case["dist"], k))
    Dr, Ir = _TOPK[tag, k]
    return (Dr, Ir) if n is None else (Dr[:n], Ir[:n])


def plan(kind, n, n_base, k):
    from deepreadmapper_amd.exact import scan_plan
    p = scan_plan(kind, n, n_base, k)
    assert (p["qt"], p["step"], p["cap"]) == (E.QT[kind], E.STEP[kind], E.cap_of(kind, k))
    assert p["slices"] == max(1, -(-n_base // p["slice_rows"])) and p["chunks"] == -(-n // p["chunk"])
    return p


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    return tmp_path_factory.mktemp("exact_paths")


def open_pq(directory, name, case):
    from deepreadmapper_amd import read_index
    return read_index(E.write_pq_index(directory / f"{name}.index", case))


# ------------------------------------------------------------------ slices
def test_l2_slices():
    from deepreadmapper_amd import exact_search_l2, set_slice_rows
    c = E.l2_gauss(4099, 32)
    n = len(c["q"])
    try:
        for k in (1, 70, 128):
            Dr, Ir = expected("l2_4099", c, k)
            outs = []
            for rows, slices in ((64, 65), (100, 33), (1000, 5), (0, 1)):
                set_slice_rows(rows)
                p = plan("l2", n, 4099, k)
                assert p["slices"] == slices
                if rows == 64:
                    assert 4099 - 64 * p["slice_rows"] == 3 and (k == 1 or p["slice_rows"] < k)
                D, I = exact_search_l2(c["base"], c["q"], k)
                same(D, I, Dr, Ir)
                outs.append((D.tobytes(), I.tobytes()))
            assert all(o == outs[0] for o in outs)
    finally:
        set_slice_rows(0)


def test_l2_slices_with_labels(directory):
    from deepreadmapper_amd import HnswFlatIndex, set_slice_rows, synth
    c = E.l2_gauss(700, 32)
    built = str(directory / "built700.hnsw")
    synth.build_flat_index(c["base"], built, M=8, efc=40, nthreads=1)
    fx = E.write_flat_shuffled(directory / "shuffled700.hnsw", built)
    labels = fx["labels"].astype(np.uint64)
    assert fx["n"] == 700 and len(np.unique(labels)) == 700 and (labels != np.arange(700)).all()
    dist = np.stack([E.R.l2sqr8(fx["vec"], x) for x in c["q"]])
    ix = HnswFlatIndex(str(directory / "shuffled700.hnsw"))
    try:
        for k in (5, 64, 128):
            Dr, Ir = E.topk_of(dist, k)
            outs = []
            for rows, slices in ((64, 11), (0, 1)):
                set_slice_rows(rows)
                assert plan("l2", len(c["q"]), 700, k)["slices"] == slices  # k = 128: every slice's list is padded
                D, L = ix.exact_search(c["q"], k)
                assert L.dtype == np.uint64 and np.array_equal(L, labels[Ir])
                assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32))
                outs.append((D.tobytes(), L.tobytes()))
            assert outs[0] == outs[1]
        set_slice_rows(64)  # k > ntotal: the merged list itself ends in padding
        Dr, Ir = E.topk_of(dist, 1024)
        D, L = ix.exact_search(c["q"], 1024)
        assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32)) and np.array_equal(L[:, :700], labels[Ir[:, :700]])
        assert (L[:, 700:] == U64_PAD).all() and np.isinf(D[:, 700:]).all()
    finally:
        set_slice_rows(0)
        ix.free()


@pytest.mark.parametrize("shape", ["4x8d32", "16x8", "8x6", "8x5", "8x10"])
def test_generic_pq_slices(directory, shape):
    from deepreadmapper_amd import set_slice_rows
    c = E.pq_gauss(shape, 1000)
    n = len(c["q"])
    ix = open_pq(directory, f"gauss_{shape}", c)
    try:
        assert (ix.info.pq_M, ix.info.pq_nbits, ix.ntotal) == (c["M"], c["nbits"], 1000)
        for k in (1, 100, 256, 768, 1024):  # 1,024 > ntotal: padding
            Dr, Ir = expected(f"gauss_{shape}", c, k)
            outs = []
            for rows, slices in ((64, 16), (0, 1)):
                set_slice_rows(rows)
                p = plan("pq", n, 1000, k)
                assert p["slices"] == slices and p["qt"] == 1 and p["chunks"] == 1
                if k in (256, 768):
                    assert p["cap"] == k + 256
                D, I = ix.exact_search(c["q"], k)
                same(D, I, Dr, Ir)
                outs.append((D.tobytes(), I.tobytes()))
            assert outs[0] == outs[1]
    finally:
        set_slice_rows(0)
        ix.free()


def test_8x8_unaligned_slices(directory):
    """d_x four bytes past a 16-byte boundary: an 8 x 8 index then takes the generic kernel (test_gpu_exact's
    test_device_entry_unaligned_queries), here with 16 slices."""
    from deepreadmapper_amd import set_slice_rows
    from deepreadmapper_amd.device import DeviceBuffer
    c = E.pq_gauss("8x8", 1000)
    n, d = c["q"].shape
    host = np.zeros(n * d + 4, dtype=np.float32)
    host[1:1 + n * d] = c["q"].ravel()
    buf = DeviceBuffer.from_host(host)
    assert buf.ptr % 16 == 0

    class _At:
        ptr = buf.ptr + 4

    bufs = [buf]
    ix = open_pq(directory, "gauss_8x8", c)
    try:
        set_slice_rows(64)
        for k in (128, 768, 1024):
            assert plan("pq", n, 1000, k)["slices"] == 16
            d_D, d_I = DeviceBuffer((n, k), np.float32), DeviceBuffer((n, k), np.int64)
            bufs += [d_D, d_I]
            ix.exact_search_device(_At, n, k, d_D, d_I)
            D, I = d_D.download(), d_I.download()
            same(D, I, *expected("gauss_8x8", c, k))
            Da, Ia = ix.exact_search(c["q"], k)  # aligned: the tiled kernel, 16 slices too
            assert plan("pq8", n, 1000, k)["slices"] == 16
            assert D.tobytes() == Da.tobytes() and I.tobytes() == Ia.tobytes()
    finally:
        set_slice_rows(0)
        ix.free()
        for b in bufs:
            b.free()


# ------------------------------------------------------------------ chunks, 1,024 slices, the default split
class _Big:
    """The two 65,536-row inputs of the chunked cases behind one search(q, k): an fp32 base, and the designed 8 x 8
    index (opened once per module)."""

    def __init__(self, kind, directory):
        self.kind = kind
        self.case = E.l2_gauss(E.N_BIG, 16, nq=25) if kind == "l2" else E.pq8_big()
        self.ix = open_pq(directory, "pq8_big", self.case) if kind == "pq8" else None
        self.q = self.case["q"]

    def search(self, n, k):
        from deepreadmapper_amd import exact_search_l2
        if self.kind == "l2":
            return exact_search_l2(self.case["base"], self.q[:n], k)
        return self.ix.exact_search(self.q[:n], k)

    def expected(self, k, n=None):
        return expected("big_" + self.kind, self.case, k, n)


@pytest.fixture(scope="module", params=["l2", "pq8"])
def big(request, directory):
    b = _Big(request.param, directory)
    yield b
    if b.ix is not None:
        b.ix.free()


def test_chunked(big):
    """25 queries at k = 1,024 over 1,024 slices: 16 MB of lists per query, so the 256 MB workspace takes 16 queries
    and run_scan goes round twice; the second chunk holds 9 queries = a full tile and a tile of one real query."""
    from deepreadmapper_amd import set_slice_rows
    try:
        set_slice_rows(64)
        p = plan(big.kind, 25, E.N_BIG, 1024)
        assert (p["slices"], p["cap"], p["chunk"], p["chunks"]) == (1024, 2048, 16, 2)
        assert p["slices"] * p["cap"] * 8 * p["chunk"] == 256 << 20
        D, I = big.search(25, 1024)
        same(D, I, *big.expected(1024))
    finally:
        set_slice_rows(0)


def test_query_batch_edges_across_chunks(big):
    """Every n around the chunk (16) and the tile (8) boundaries gives the first n rows of the n = 25 answer."""
    from deepreadmapper_amd import set_slice_rows
    try:
        set_slice_rows(64)
        Dall, Iall = big.search(25, 1024)
        same(Dall, Iall, *big.expected(1024))
        for n in (15, 16, 17, 24, 25):
            assert plan(big.kind, n, E.N_BIG, 1024)["chunks"] == (1 if n <= 16 else 2)
            D, I = big.search(n, 1024)
            assert D.tobytes() == Dall[:n].tobytes() and I.tobytes() == Iall[:n].tobytes(), n
    finally:
        set_slice_rows(0)


def test_default_multi_slice(big):
    """The default split of 65,536 rows for 9 queries (2 tiles): min(one round of workgroups / 2 tiles, 65,536 / 16 Ki)
    = 4 slices on any device with two or more CUs. Equal to the 1,024-slice result byte for byte."""
    from deepreadmapper_amd import set_slice_rows
    try:
        for k in (128, 1024):
            set_slice_rows(0)
            p = plan(big.kind, 9, E.N_BIG, k)
            assert p["slices"] == 4 and p["slice_rows"] == 16384 and p["chunks"] == 1
            D, I = big.search(9, k)
            same(D, I, *big.expected(k, 9))
            set_slice_rows(64)
            assert plan(big.kind, 9, E.N_BIG, k)["slices"] == 1024
            D2, I2 = big.search(9, k)
            assert D.tobytes() == D2.tobytes() and I.tobytes() == I2.tobytes()
    finally:
        set_slice_rows(0)


def test_max_slices_clamp():
    """70,001 rows at 64 rows per slice would be 1,094 slices: the rows are raised to 128, 547 slices, the last of
    113 rows."""
    from deepreadmapper_amd import exact_search_l2, set_slice_rows
    c = E.l2_gauss(70001, 16)
    try:
        set_slice_rows(64)
        p = plan("l2", len(c["q"]), 70001, 128)
        assert p["slice_rows"] == 128 and p["slices"] == 547 and 70001 - 546 * 128 == 113
        D, I = exact_search_l2(c["base"], c["q"], 128)
        same(D, I, *expected("l2_70001", c, 128))
    finally:
        set_slice_rows(0)


# ------------------------------------------------------------------ selection
def _search(kind, directory, name, case):
    """(search(k) -> D, I; close()) for a case of either sort."""
    if kind == "l2":
        from deepreadmapper_amd import exact_search_l2
        return (lambda k: exact_search_l2(case["base"], case["q"], k)), (lambda: None)
    ix = open_pq(directory, name, case)
    return (lambda k: ix.exact_search(case["q"], k)), ix.free


@pytest.mark.parametrize("order", E.ORDERS)
@pytest.mark.parametrize("kind", ["pq8", "pq", "l2"])
def test_arrival_orders(directory, kind, order):
    """8,192 rows in one slice, in an order made for query 0 (test_exact_cases_cpu: descending -- every row of every
    step passes, a compaction follows every (cap - k) / step steps with a tighter threshold each time, and at
    cap == k + step the buffer fills to exactly cap at every step; ascending and sawtooth -- nothing passes after
    the first compaction). The other 8 queries see the same rows in an order that means nothing to them."""
    from deepreadmapper_amd import set_slice_rows
    c = E.order_case(kind, order)
    search, close = _search(kind, directory, f"order_{kind}_{order}", c)
    try:
        set_slice_rows(E.N_ORDER)
        for k in E.ORDER_KS[kind]:
            p = plan(kind, len(c["q"]), E.N_ORDER, k)
            assert p["slices"] == 1 and p["slice_rows"] == E.N_ORDER and p["chunks"] == 1
            if k in E.tight_ks(kind):
                assert p["cap"] == k + p["step"]
            D, I = search(k)
            same(D, I, *expected(f"order_{kind}_{order}", c, k))
    finally:
        set_slice_rows(0)
        close()


@pytest.mark.parametrize("kind", ["pq8", "pq", "l2"])
def test_ties_at_the_cut(directory, kind):
    """8 groups of about 1,024 equal rows, descending for query 0, k inside a group (test_exact_cases_cpu: for some
    query the group at the cut lies in several slices, so the merge decides which of its ids are returned)."""
    from deepreadmapper_amd import set_slice_rows
    c = E.tie_case(kind)
    search, close = _search(kind, directory, f"ties_{kind}", c)
    try:
        for k in E.tie_ks(c["dist"]):
            Dr, Ir = expected(f"ties_{kind}", c, k)
            D1 = expected(f"ties_{kind}", c, k + 1)[0]
            assert D1[0, k - 1] == D1[0, k] and (D1[:, k - 1] == D1[:, k]).sum() >= 2  # the cut is inside a group
            outs = []
            for rows, slices in zip(E.TIE_SLICE_ROWS, (2, 64)):
                set_slice_rows(rows)
                assert plan(kind, len(c["q"]), E.N_ORDER, k)["slices"] == slices
                D, I = search(k)
                same(D, I, Dr, Ir)
                outs.append((D.tobytes(), I.tobytes()))
            assert outs[0] == outs[1]
    finally:
        set_slice_rows(0)
        close()


# ------------------------------------------------------------------ edges of the entry points
def test_empty_base(directory):
    from deepreadmapper_amd import HnswFlatIndex, exact_search_l2
    q = E.l2_gauss(64, 16)["q"][:3]
    p = plan("l2", 3, 0, 5)
    assert p["slices"] == 1 and p["chunks"] == 1
    D, I = exact_search_l2(np.zeros((0, 16), np.float32), q, 5)
    assert D.shape == (3, 5) and np.isposinf(D).all() and I.dtype == np.int64 and (I == -1).all()
    ix = HnswFlatIndex(E.write_flat_empty(directory / "empty.hnsw", 16))
    try:
        assert ix.ntotal == 0
        D, L = ix.exact_search(q, 5)
        assert D.shape == (3, 5) and np.isposinf(D).all() and L.dtype == np.uint64 and (L == U64_PAD).all()
    finally:
        ix.free()


def test_lut_limit(directory):
    """M * ksub * 4 == 65,536: the largest lookup table launch_exact_pq takes; the generic kernel then asks for 64 KB
    of dynamic LDS beside its static 16 KB sort buffer. One bit more per index (128 KB) is refused, and the handle
    lives on."""
    from deepreadmapper_amd import DrmError
    from deepreadmapper_amd._native import DRM_ERR_UNSUPPORTED
    c = E.pq_lut(10)
    assert c["M"] * (1 << c["nbits"]) * 4 == 65536
    ix = open_pq(directory, "lut64k", c)
    try:
        for k in (1, 300, 301):
            D, I = ix.exact_search(c["q"], k)
            same(D, I, *expected("lut64k", c, k))
    finally:
        ix.free()
    c = E.pq_lut(11)
    assert c["M"] * (1 << c["nbits"]) * 4 == 131072
    ix = open_pq(directory, "lut128k", c)
    try:
        for _ in range(2):
            with pytest.raises(DrmError) as e:
                ix.exact_search(c["q"], 5)
            assert e.value.code == DRM_ERR_UNSUPPORTED and "lookup table larger than 64 KB" in str(e.value)
        assert (ix.ntotal, ix.info.pq_M, ix.info.pq_nbits) == (300, 16, 11) and ix.search_errors() == 0
    finally:
        ix.free()
