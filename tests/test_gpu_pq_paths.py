"""The paths of the three HNSW-PQ search kernels (hnsw_pq_fast.hip, hnsw_search.hip, hnsw_search_lds.hip) that no
d = 128 / PQ 8 x 8 / M_hnsw = 16 index reaches, each against the oracle exactly as tests/test_gpu_parity.py compares:
ids, fp32 distances as bit patterns (0 ulp), nhops, and ndis (always for the general and the LDS-heap kernel, with
exact statistics for the lean one). The indices come from tests/pq_graphs.py; tests/test_pq_graphs_cpu.py proves,
from the oracle alone, that each fixture reaches the path named here.

Which test reaches which instantiation: hnsw_pq_search_kernel<1|2|4|8, false> test_generic_shapes_general_kernel;
<R, true> at deg0 = 8 / 24 / 64 test_lean_kernel_degrees[..-0]; hnsw_pq_search_lds_kernel<false>
test_generic_shapes_lds_kernel; <true> with a full heap test_lds_kernel_8x8; the lean kernel's variants at
deg0 = 64 test_lean_kernel_degrees[8x8m32-1], test_lean_kernel_full_rows and test_full_reset_lean_kernel."""
import ctypes as C

import numpy as np
import pytest

import pq_graphs as P
from oracle import oracle as O

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _oracle(f, q, k, ef):
    """The oracle's (D, I, ndis, nhops), computed once per (index, queries, k, ef) and left unchanged."""
    key = (f["index"], hash(q.tobytes()), q.shape, k, ef)
    if key not in _ORACLE:
        r = O.hnswpq_search(f["fx"], q, k, ef)
        for a in r:
            a.setflags(write=False)
        _ORACLE[key] = r
    return _ORACLE[key]


def _open(f):
    from deepreadmapper_amd import read_index
    return read_index(f["index"])


def _check(ix, f, k, ef, q=None, ndis=True):
    """One search on an open handle against the oracle. ndis=False: the lean kernel without exact statistics (it
    reports the distances it computed, not faiss's count)."""
    q = f["q"] if q is None else q
    fx = f["fx"]
    D, I, st = ix.search(q, k, ef)
    Do, Io, nd, nh = _oracle(f, q, k, ef)
    what = f"{fx.pq_M}x{fx.pq_nbits} d={fx.d} n={fx.ntotal} nq={len(q)} k={k} ef={ef}"
    bad = np.flatnonzero((I != Io).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[:8]}"
    assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)), what  # 0 ulp
    assert st.nhops == int(nh.sum()), what
    if ndis:
        assert st.ndis == int(nd.sum()), what
    assert ix.search_errors() == 0, what
    return Do, Io, nd, nh


def _check_both_stats(ix, f, k, ef, q=None):
    """test_gpu_parity._search_both on an open handle: the default statistics, then the exact ones."""
    ix.set_exact_stats(False)
    _check(ix, f, k, ef, q, ndis=False)
    ix.set_exact_stats(True)
    r = _check(ix, f, k, ef, q)
    ix.set_exact_stats(False)
    return r


def _device_search(ix, q, k, ef, offset):
    """drm_search_device_ex with the queries `offset` floats past a 16-byte boundary. Returns D, I, ndis, nhops."""
    from deepreadmapper_amd.device import DeviceBuffer, synchronize
    n, d = q.shape
    host = np.zeros(n * d + 4, dtype=np.float32)
    host[offset:offset + n * d] = q.ravel()
    buf = DeviceBuffer.from_host(host)
    assert buf.ptr % 16 == 0

    class _At:
        ptr = buf.ptr + 4 * offset

    dD, dI = DeviceBuffer((n, k), np.float32), DeviceBuffer((n, k), np.int64)
    nd, nh = DeviceBuffer(n, np.int32), DeviceBuffer(n, np.int32)
    try:
        ix.search_device(_At, n, k, ef, dD, dI, nd, nh)
        synchronize()
        return dD.download(), dI.download(), nd.download(), nh.download()
    finally:
        for b in (buf, dD, dI, nd, nh):
            b.free()


def _device_bytes(ix):
    from deepreadmapper_amd._native import IndexInfo, check, lib
    info = IndexInfo()
    check(lib().drm_index_get_info(ix.handle, C.byref(info)))
    return int(info.device_bytes)


def _unsupported(call):
    from deepreadmapper_amd._native import DRM_ERR_UNSUPPORTED, DrmError
    with pytest.raises(DrmError) as e:
        call()
    assert e.value.code == DRM_ERR_UNSUPPORTED, (e.value.code, str(e.value))
    return str(e.value)


# ------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("pqpaths")


@pytest.fixture(scope="module")
def built(workdir):
    """The 2,902-node builder-made indices of every shape, made on first use."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = P.make_built(workdir, name)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def rnd4x12(workdir):
    return P.make_random(workdir, "4x12", 64, 4, 12, 16, 1500)


@pytest.fixture(scope="module")
def fans(workdir):
    return {n: P.make_fan(workdir, n) for n in (P.FAN_N_LDS, P.FAN_N_GENERAL)}


@pytest.fixture(scope="module")
def ramp(workdir):
    return P.make_ramp(workdir)


def _shape_fixture(built, rnd4x12, name):
    return rnd4x12 if name == "4x12" else built(name)


# ------------------------------------------------------------------------------------------ a, b: generic shapes
@pytest.mark.parametrize("name", list(P.BUILT_SHAPES) + ["4x12"])
def test_generic_shapes_general_kernel(built, rnd4x12, name):
    """hnsw_pq_search_kernel<R, false>, R = 1, 2, 4, 8 (test_pq_graphs_cpu.test_case_lists_reach_every_instantiation):
    the bit-packed decode of pq_common.h (nbits 5, 6, 10, 12), the scalar LUT build (dsub = 8, or ksub 32 / 64: no
    multiple of 128), the vector LUT build with M = 4 (4 x 8 at d = 64, 4 x 12), deg0 = 8 with seven levels (8 x 5)
    and deg0 = 64 (8 x 6). 4 x 12 is a hand-written random graph (holes, a repeated link) at the LUT limit of 16384
    entries = 64 KB of dynamic LDS."""
    f = _shape_fixture(built, rnd4x12, name)
    ix = _open(f)
    for k, ef in P.GENERAL_KEF:
        _check(ix, f, k, ef)
    ix.free()


@pytest.mark.parametrize("name", list(P.BUILT_SHAPES) + ["4x12"])
def test_generic_shapes_lds_kernel(built, rnd4x12, name):
    """hnsw_pq_search_lds_kernel<false> and its own bit-packed decode: the heap fills, evicts and the walk ends on
    `below >= efSearch` at ef = 600 (test_built_indices_fill_the_heap_and_stop), k > 512 sorts kpad = 1024 keys in
    LDS, (513, 16) and (1024, 16) have efSearch far below the heap size max(ef, k), (1024, 4096) is both limits at
    once (on 4 x 12: 64 KB of LUT + 40 KB of heaps in one workgroup's LDS)."""
    f = _shape_fixture(built, rnd4x12, name)
    ix = _open(f)
    for k, ef in P.LDS_KEF:
        _check(ix, f, k, ef)
    ix.free()


@pytest.mark.parametrize("name", ["8x5", "8x10", "4x8d64", "8x8"])
def test_forced_lds_kernel_small_ef(built, name, monkeypatch):
    """DRM_SEARCH_LDS_KERNEL=1: the LDS-heap kernel at the small (k, ef) the other kernels normally serve."""
    monkeypatch.setenv("DRM_SEARCH_LDS_KERNEL", "1")
    f = built(name)
    ix = _open(f)
    for k, ef in ((10, 16), (1, 1), (64, 100), (128, 128)):
        _check(ix, f, k, ef)
    ix.free()


def test_lds_kernel_8x8(built):
    """hnsw_pq_search_lds_kernel<true> with a full heap, on the 8 x 8 built index."""
    f = built("8x8")
    ix = _open(f)
    for k, ef in P.LDS_KEF:
        _check(ix, f, k, ef)
    ix.free()


def test_lds_kernel_tie_heavy_index(repeats):
    """The same on the tie-heavy `repeats` index (identical PQ codes): pop_min and the `>=` rejection among equal
    distances on a full heap."""
    ix = _open(repeats)
    for k, ef in P.LDS_KEF:
        _check(ix, repeats, k, ef)
    ix.free()


@pytest.mark.parametrize("M_pq,nbits,d", [(8, 8, 128), (8, 6, 128)])
def test_lds_kernel_ties_straddle_k(workdir, M_pq, nbits, d):
    """make_tie: the k-th and (k + 1)-th distances are equal at k = 513 and k = 1024
    (test_tie_fixtures_straddle_k), so the result heap's choice among tied ids and the order of the bitonic sort by
    (distance, id) are both visible; efSearch = 16 stops the walk early, 2048 > ntotal never fills the heap."""
    f = P.make_tie(workdir, f"tie{M_pq}x{nbits}", d, M_pq, nbits, 16, 1500)
    ix = _open(f)
    for k, ef in ((513, 2048), (1024, 2048), (513, 16), (1024, 16), (514, 600), (600, 600), (10, 600)):
        _check(ix, f, k, ef)
    ix.free()


@pytest.mark.parametrize("M_pq,nbits,d", [(8, 8, 128), (8, 6, 128), (4, 8, 32)])
def test_padding_and_empty_index(workdir, M_pq, nbits, d):
    """ntotal = 300 < k: the result heap keeps (+inf, -1) entries and the sort pads (LDS kernel at k = 513 / 1024,
    general kernel at k = 400, lean kernel on 8 x 8 at (128, 128) is not short: k = 64 of a walk that stops early
    is). ntotal = 0 with entry_point = -1: only padding, ndis = nhops = 0, through every kernel."""
    f = P.make_chain(workdir, f"c{M_pq}x{nbits}", d, M_pq, nbits, 8, 300)
    ix = _open(f)
    for k, ef in ((513, 16), (1024, 16), (513, 600), (400, 400), (400, 16), (128, 128), (64, 8), (10, 16)):
        Do, Io, _, _ = _check_both_stats(ix, f, k, ef)
        if k >= 400:
            assert ((Io >= 0).sum(axis=1) < k).all()
    ix.free()
    e = P.make_chain(workdir, f"e{M_pq}x{nbits}", d, M_pq, nbits, 8, 0)
    ix = _open(e)
    for k, ef in ((10, 600), (1024, 16), (300, 512), (10, 16), (128, 128)):
        Do, Io, nd, nh = _check_both_stats(ix, e, k, ef)
        assert (Io == -1).all() and np.isinf(Do).all() and not nd.any() and not nh.any()
    ix.free()


# ------------------------------------------------------------------------------------------ c: visited-set reset
def test_full_reset_lds_kernel(fans, monkeypatch):
    """fan_graph(20,000) at ef = 2048: every query lists more than clear_cap = 16384 visited ids
    (test_fan_graphs_pass_the_clear_list), so the LDS-heap kernel clears its whole bitmap. The (10, 16) search that
    follows on the handle runs in the general kernel (DRM_SEARCH_FAST=0), which shares the bitmaps: a bit that
    survived would change its ndis and neighbours. Then the other way round."""
    monkeypatch.setenv("DRM_SEARCH_FAST", "0")
    f = fans[P.FAN_N_LDS]
    ix = _open(f)
    _, _, nd, _ = _check(ix, f, 10, 2048)
    assert nd.min() > 16384
    _check(ix, f, 10, 16)
    _check(ix, f, 600, 2048)
    _check(ix, f, 10, 16)
    ix.free()


def test_full_reset_general_kernel(fans, monkeypatch):
    """fan_graph(24,000) at ef = 512 through hnsw_pq_search_kernel<8, true> (DRM_SEARCH_FAST=0 keeps the follow-up
    (10, 16) in the general kernel too): more than 16384 distances per query, then the list reset."""
    monkeypatch.setenv("DRM_SEARCH_FAST", "0")
    f = fans[P.FAN_N_GENERAL]
    ix = _open(f)
    _, _, nd, _ = _check(ix, f, 10, 512)
    assert nd.min() > 16384
    _, _, nd, _ = _check(ix, f, 10, 16)
    assert nd.max() <= 16384
    _check(ix, f, 300, 512)
    ix.free()


def test_full_reset_lean_kernel(ramp):
    """The lean kernel keeps a bitmap only to count faiss's ndis (exact statistics). No fan graph takes it past
    clear_cap at ef <= 128 (about 7,000 distances); the ramp's sweep queries compute ntotal - 1 = 16,999 at any ef
    (test_ramp_graph_passes_the_clear_list_at_any_ef), on full 64-link rows. Sweep and stall queries alternate, so
    a full reset is followed by a list reset and the reverse; then the same through the other two kernels."""
    rng = np.random.default_rng(3)
    q = np.empty((24, 128), dtype=np.float32)
    q[0::2], q[1::2] = P.ramp_queries(rng, 12), P.ramp_queries(rng, 12, stall=True)
    ix = _open(ramp)
    for k, ef in P.LEAN_KEF + [(1, 1)]:
        _, _, nd, _ = _check_both_stats(ix, ramp, k, ef, q)
        assert (nd[0::2] > 16384).all() and (nd[1::2] <= 16384).all()
    # switching the statistics off releases the bitmaps; with them left on, every call starts on the bitmaps the
    # call before it reset (the stall queries walk ids that every sweep query has marked)
    ix.set_exact_stats(True)
    for k, ef in P.LEAN_KEF:
        _check(ix, ramp, k, ef, q)
        _check(ix, ramp, k, ef, q[1::2])
    _check(ix, ramp, 300, 512, q)
    _check(ix, ramp, 10, 600, q)
    _check(ix, ramp, 128, 128, q)
    ix.free()


@pytest.mark.parametrize("kernel", ["lean", "general", "lds"])
def test_full_reset_then_reuse_within_one_launch(fans, ramp, kernel, monkeypatch):
    """More queries than resident wave slots, so a slot serves several queries of one launch and starts each on the
    bitmap the one before it reset, with no wait in between; full and list resets alternate (lean) or follow in the
    next call (general, LDS). The slot count is the launcher's: CUs x waves per CU, one with
    DRM_SEARCH_WAVES_PER_CU=1 (lean, general), min(16, 160 KB / LDS bytes) for the LDS-heap kernel."""
    from deepreadmapper_amd.device import device_props
    cus = device_props()["cu_count"]
    monkeypatch.setenv("DRM_SEARCH_WAVES_PER_CU", "1")
    rng = np.random.default_rng(8)
    if kernel == "lean":
        f, k, ef, slots = ramp, 128, 128, cus
        n = 2 * slots + 38
        q = np.empty((n, 128), dtype=np.float32)
        q[0::2], q[1::2] = P.ramp_queries(rng, n // 2), P.ramp_queries(rng, n // 2, stall=True)
    elif kernel == "general":
        monkeypatch.setenv("DRM_SEARCH_FAST", "0")
        f, k, ef, slots = fans[P.FAN_N_GENERAL], 10, 512, cus
        q = P.fan_queries(rng, 2 * slots + 37)
    else:
        monkeypatch.setenv("DRM_SEARCH_FAST", "0")
        f, k, ef = fans[P.FAN_N_LDS], 10, 2048
        lds = 4 * 8 * 256 + 4 * 128 + 8 * ((ef + 1) & ~1) + 8 * 64 + 8 * 64  # plan_search: LUT, query, heaps
        slots = cus * max(1, min(16, (160 * 1024) // lds))
        q = P.fan_queries(rng, slots + 101)
    assert len(q) > slots
    ix = _open(f)
    ix.set_exact_stats(True)
    _, _, nd, _ = _check(ix, f, k, ef, q)
    assert (nd > 16384).sum() >= len(q) // 2
    _, _, nd, _ = _check(ix, f, 10, 16, q[:2 * cus + 37][1::2] if kernel == "lean" else q[:2 * cus + 37])
    assert nd.max() <= 16384
    ix.free()


# ------------------------------------------------------------------------------------------ d: lean kernel degrees
@pytest.mark.parametrize("fast", ["1", "0"])
@pytest.mark.parametrize("name", list(P.LEAN_DEGREES))
def test_lean_kernel_degrees(built, name, fast, monkeypatch):
    """8 x 8 built indices with M_hnsw = 4, 12, 32: level-0 rows of 8, 24 and 64 links (inline rows of 1, 3 and 6
    128-byte lines; at 64 every lane of the wave holds a link and a full row has no -1 for `jmax` to find), through
    the lean kernel with and without exact statistics, and through the general kernel (DRM_SEARCH_FAST=0)."""
    monkeypatch.setenv("DRM_SEARCH_FAST", fast)
    f = built(name)
    assert f["fx"].cum_nneighbor_per_level[1] == 2 * P.LEAN_DEGREES[name][3]
    ix = _open(f)
    for k, ef in P.LEAN_KEF + [(1, 1), (10, 16)]:
        _check_both_stats(ix, f, k, ef)
    ix.free()


@pytest.mark.parametrize("fast", ["1", "0"])
def test_lean_kernel_full_rows(workdir, fast, monkeypatch):
    """random_graph(hole_p = 0) at deg0 = 64: no level-0 row has a -1 (test_full_rows_graph), so every row load is
    the full-wave row and `jmax` its fallback; a hand-written graph has no neighbourhood structure, so the walk
    revisits and evicts far more than on a built index."""
    monkeypatch.setenv("DRM_SEARCH_FAST", fast)
    f = P.make_random(workdir, "full64", 128, 8, 8, 32, 3000, hole_p=0.0, dup=False)
    ix = _open(f)
    for k, ef in P.LEAN_KEF + [(10, 16), (300, 512), (10, 600)]:
        _check_both_stats(ix, f, k, ef)
    ix.free()


# ------------------------------------------------------------------------------------------ e: unaligned queries
@pytest.mark.parametrize("name,kefs", [("8x8", [(128, 128), (5, 128), (300, 512), (10, 600)]),
                                       ("4x8d64", [(10, 16), (100, 128), (300, 512), (10, 600)])])
def test_unaligned_queries(built, name, kefs):
    """drm_search_device_ex with d_x four bytes past a 16-byte boundary (x_aligned16 = 0): the lean kernel falls
    back from build_lut_m8 to build_lut, the general kernel from its float4 LUT build to the scalar one (8 x 8 and
    4 x 8 at d = 64 both have dsub = 16), the LDS-heap kernel reads the query scalar either way. Same rows as the
    aligned call and as the oracle."""
    f = built(name)
    ix = _open(f)
    ix.set_exact_stats(True)
    for k, ef in kefs:
        Do, Io, nd, nh = _oracle(f, f["q"], k, ef)
        for offset in (0, 1):
            D, I, gnd, gnh = _device_search(ix, f["q"], k, ef, offset)
            what = (name, k, ef, offset)
            assert np.array_equal(I, Io) and np.array_equal(D.view(np.uint32), Do.view(np.uint32)), what
            assert np.array_equal(gnd, nd) and np.array_equal(gnh, nh), what
    ix.free()


# ------------------------------------------------------------------------------------------ f: limits
def test_k_and_ef_limits(built):
    """k = 1024 and max(ef, k) = 4096 work (test_generic_shapes_lds_kernel runs (1024, 4096) too); k = 1025 and
    ef = 4097 are DRM_ERR_UNSUPPORTED, and the handle still answers afterwards."""
    for name in ("8x8", "8x6"):
        f = built(name)
        ix = _open(f)
        _check(ix, f, 1024, 4096)
        assert "k must be in [1, 1024]" in _unsupported(lambda: ix.search(f["q"], 1025, 16))
        _check(ix, f, 128, 128, ndis=False)
        assert "<= 4096" in _unsupported(lambda: ix.search(f["q"], 10, 4097))
        _check(ix, f, 10, 16, ndis=False)
        _unsupported(lambda: ix.search(f["q"], 1025, 4097))
        _check(ix, f, 10, 600)
        ix.free()


def test_degree_limits(workdir):
    """M_hnsw = 32 (deg0 = 64) works (test_lean_kernel_degrees); M_hnsw = 33 (deg0 = 66) is DRM_ERR_UNSUPPORTED from
    every search, and so is an upper-level degree of 65 under a level-0 degree of 32."""
    rng = np.random.default_rng(5)
    q = rng.standard_normal((4, 128)).astype(np.float32)
    f = P.make_random(workdir, "m33", 128, 8, 8, 33, 200, n_levels=2)
    ix = _open(f)
    for k, ef in ((10, 16), (300, 512), (10, 600)):
        assert "level-0 degree" in _unsupported(lambda: ix.search(q, k, ef))
    ix.free()
    # level 0 of M_hnsw = 16 (32 slots), upper levels 65 slots wide
    rows, entry, max_level = P.random_graph(200, 16, 2, rng)
    rows = [[r[0]] + [lv + [-1] * (65 - len(lv)) for lv in r[1:]] for r in rows]
    assert max_level == 1
    path = str(workdir / "upper65.index")
    P.write_ihnp(path, 128, 8, 8, 16, P.gauss_centroids(rng, 128, 8, 8), P.random_codes(rng, 200, 8, 8), rows, entry,
                 max_level, cum=[0, 32, 97])
    ix = _open({"index": path})
    for k, ef in ((10, 16), (300, 512), (10, 600)):
        assert "upper-level degree" in _unsupported(lambda: ix.search(q, k, ef))
    ix.free()


def test_lut_size_limits(workdir, rnd4x12):
    """M * 2^nbits = 16384 (4 x 12) works through both kernels -- 64 KB of dynamic LDS in the general kernel, more in
    the LDS-heap kernel, with no raw HIP launch error -- and 32768 (4 x 13), like 2 x 16, is DRM_ERR_UNSUPPORTED from
    both."""
    ix = _open(rnd4x12)
    _check(ix, rnd4x12, 10, 16)
    _check(ix, rnd4x12, 10, 600)
    _check(ix, rnd4x12, 1024, 4096)
    ix.free()
    for name, M_pq, nbits in (("4x13", 4, 13), ("2x16", 2, 16)):
        f = P.make_random(workdir, name, 32, M_pq, nbits, 8, 120, n_levels=2, nq=4)
        ix = _open(f)
        for k, ef in ((10, 16), (10, 600)):
            assert "PQ LUT" in _unsupported(lambda: ix.search(f["q"], k, ef))
        ix.free()


# ------------------------------------------------------------------------------------------ g: one handle
def test_one_handle_many_calls(built):
    """lean -> LDS -> general -> lean with exact statistics -> LDS with a larger k -> lean on one handle: the
    visited bitmaps, the clear lists and the lean kernel's log are shared, and ensure_visited / ensure_log
    (re)allocate them for each kernel's own slot count."""
    f = built("8x8")
    ix = _open(f)
    _check(ix, f, 128, 128, ndis=False)
    _check(ix, f, 10, 600)
    _check(ix, f, 300, 512)
    ix.set_exact_stats(True)
    _check(ix, f, 128, 128)
    _check(ix, f, 5, 128)
    _check(ix, f, 1024, 2048)
    ix.set_exact_stats(False)
    _check(ix, f, 128, 128, ndis=False)
    _check(ix, f, 64, 64, ndis=False)
    _check(ix, f, 10, 600)
    ix.free()


def test_device_bytes_after_lds_reallocation(built):
    """Two handles that end with the same allocations report the same device_bytes. A: one LDS-heap search of more
    queries than CUs, which allocates the bitmaps and clear lists (an 8 x 8 index loads without them). B: first an
    exact-statistics lean search at one wave per CU, which allocates CUs x 1 slots, then the same LDS-heap search,
    which needs more slots and reallocates (both in ensure_visited)."""
    from deepreadmapper_amd._native import check, lib
    from deepreadmapper_amd.device import device_props
    f = built("8x8")
    cus = device_props()["cu_count"]
    q = np.ascontiguousarray(np.resize(f["q"], (2 * cus + 5, 128)))
    a = _open(f)
    loaded = _device_bytes(a)
    _check(a, f, 10, 600, q)
    b = _open(f)
    assert _device_bytes(b) == loaded
    check(lib().drm_index_set_search_waves(b.handle, 1))
    b.set_exact_stats(True)
    _check(b, f, 10, 16, q)
    small = _device_bytes(b)
    check(lib().drm_index_set_search_waves(b.handle, 0))
    _check(b, f, 10, 600, q)
    words = (f["fx"].ntotal + 31) // 32
    assert small - loaded == cus * (4 * words + 4 * 16384)  # ensure_visited: CUs x 1 slots
    assert _device_bytes(a) > loaded and (_device_bytes(a) - loaded) % (4 * words + 4 * 16384) == 0
    assert _device_bytes(a) == _device_bytes(b)
    a.free()
    b.free()


def _search_rows(ix, f, k, ef, n, ndis=True):
    """One search of n queries (the fixture's 64, repeated) on an open handle; the first 64 rows against the oracle."""
    q = np.ascontiguousarray(np.resize(f["q"], (n, f["q"].shape[1])))
    D, I, _ = ix.search(q, k, ef)
    Do, Io, _, _ = _oracle(f, f["q"], k, ef)
    m = len(f["q"])
    assert np.array_equal(I[:m], Io) and np.array_equal(D[:m].view(np.uint32), Do.view(np.uint32)), (k, ef, n)
    assert np.array_equal(I[-m:], np.roll(Io, -((n - m) % m), axis=0)) and ix.search_errors() == 0, (k, ef, n)


def test_device_bytes_is_path_independent(built, monkeypatch):
    """device_bytes follows the workspace, whatever order the kernels came in. Three handles of the 8 x 8 index are
    driven to the same final workspace: (i) LDS-heap, general, lean with exact statistics; (ii) the reverse order;
    (iii) first a lean search at drm_index_set_search_waves(.., 1), then restored and as (i). Every search has more
    queries than a full grid of any kernel has slots (CUs x 20), so each step's slot count is plan_search's full
    grid: CUs x 11 for the LDS-heap kernel at ef = 600 (160 KB / 14,528 B of LDS), CUs x 20 for the other two, CUs
    x 1 at one wave per CU. After each step the difference from the loaded value is exactly slots x (4 x words +
    4 x 16384) for the bitmaps and clear lists plus 8 x slots x (cap - loaded cap) for the lean kernel's log, whose
    cap is max(DRM_SEARCH_LOG_CAP, efc + max(efc, 64)): with the request at 64 the log is reallocated at 80 entries
    for (10, 16) and back at 256 for (128, 128). Then a shape without inline rows (8 x 5): its loaded device_bytes is
    its index arrays plus what reserve_search_scratch allocates, CUs x per_cu x (4 x words + 4 x 16384) of bitmaps
    and clear lists and 8 x CUs x per_cu x cap of log -- cap = 256, the ef = 128 need, once the request
    (DRM_SEARCH_LOG_CAP, 512 unless set) is no larger, and 512 by default."""
    from deepreadmapper_amd._native import check, lib
    from deepreadmapper_amd.device import device_props
    cus = device_props()["cu_count"]
    monkeypatch.delenv("DRM_SEARCH_WAVES_PER_CU", raising=False)
    monkeypatch.setenv("DRM_SEARCH_LOG_CAP", "64")
    f = built("8x8")
    n = 20 * cus + 5
    words = (f["fx"].ntotal + 31) // 32
    per_slot = 4 * words + 4 * 16384
    lds = 4 * 8 * 256 + 4 * 128 + 8 * ((600 + 1) & ~1) + 8 * 64 + 8 * 64  # plan_search: LUT, query, heaps
    lds_per_cu = max(1, min(16, (160 * 1024) // lds))
    assert lds_per_cu == 11
    log80 = 8 * 20 * cus * (80 - 256)  # the log of a full grid, reallocated at cap 80 instead of the loaded 256

    def lds_step(ix):
        _search_rows(ix, f, 10, 600, n)

    def general_step(ix):
        _search_rows(ix, f, 300, 512, n)

    def lean_step(ix, after_1016, after_128):
        _search_rows(ix, f, 10, 16, n)
        assert _device_bytes(ix) - loaded == after_1016
        _search_rows(ix, f, 128, 128, n)
        assert _device_bytes(ix) - loaded == after_128

    handles = [_open(f) for _ in range(3)]
    loaded = _device_bytes(handles[0])
    for ix in handles:
        assert _device_bytes(ix) == loaded
        ix.set_exact_stats(True)
    full = 20 * cus * per_slot
    # (i)
    a = handles[0]
    lds_step(a)
    assert _device_bytes(a) - loaded == lds_per_cu * cus * per_slot
    general_step(a)
    assert _device_bytes(a) - loaded == full
    lean_step(a, full + log80, full)
    # (ii)
    b = handles[1]
    lean_step(b, full + log80, full)
    general_step(b)
    assert _device_bytes(b) - loaded == full
    lds_step(b)
    assert _device_bytes(b) - loaded == full
    # (iii)
    c = handles[2]
    check(lib().drm_index_set_search_waves(c.handle, 1))
    _search_rows(c, f, 10, 16, n)
    assert _device_bytes(c) - loaded == cus * per_slot + log80  # CUs x 1 slots of bitmaps; the log keeps its slots
    check(lib().drm_index_set_search_waves(c.handle, 0))
    lds_step(c)
    assert _device_bytes(c) - loaded == lds_per_cu * cus * per_slot + log80
    general_step(c)
    assert _device_bytes(c) - loaded == full + log80
    lean_step(c, full + log80, full)
    for ix in handles:
        d = _device_bytes(ix) - loaded
        assert d == full and d % per_slot == 0
    assert _device_bytes(a) == _device_bytes(b) == _device_bytes(c)
    for ix in handles:  # statistics off releases the bitmaps and clear lists of an index with inline rows
        ix.set_exact_stats(False)
        assert _device_bytes(ix) == loaded
        ix.free()

    # no inline rows: the whole workspace is reserved at load
    g = built("8x5")
    fx = g["fx"]
    cum = fx.cum_nneighbor_per_level
    upper = int(sum(cum[lv] - cum[1] for lv in fx.levels if lv > 1))
    arrays = (4 * len(fx.centroids) + len(fx.codes) + 4 * fx.ntotal * int(cum[1]) + 4 * fx.ntotal + 4 * max(upper, 1))
    per_cu = max(1, min(20, (160 * 1024) // (4 * 8 * 32)))  # the LUT of 8 x 2^5 entries is the only LDS
    gwords = (fx.ntotal + 31) // 32
    for request, cap in (("256", 256), (None, 512)):
        if request is None:
            monkeypatch.delenv("DRM_SEARCH_LOG_CAP")
        else:
            monkeypatch.setenv("DRM_SEARCH_LOG_CAP", request)
        ix = _open(g)
        scratch = _device_bytes(ix) - arrays
        print(f"8x5 loaded: request {request} scratch {scratch} = {cus} CUs x {per_cu} x ({4 * gwords} + {4 * 16384})"
              f" + 8 x {cus} x {per_cu} x {cap}")
        assert scratch == cus * per_cu * (4 * gwords + 4 * 16384) + 8 * cus * per_cu * cap, (request, cap)
        _check(ix, g, 10, 16)
        assert _device_bytes(ix) - arrays == scratch
        ix.free()
