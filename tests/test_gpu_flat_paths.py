"""The paths of the fp32 hnswlib kernel (hnsw_flat_search.hip) that no builder-made d = 128 index reaches, each
against the oracle restatement (oracle/hnswlib_oracle.cpp) exactly as tests/test_gpu_flat.py compares: labels,
fp32 distances as bit patterns, summed ndis / nhops, no search errors. The graphs come from tests/hnswlib_graphs.py;
tests/test_flat_graphs_cpu.py asserts, from oracle diagnostics, that each fixture reaches the path named here."""
import numpy as np
import pytest

import hnswlib_graphs as G
from oracle import oracle as O

pytestmark = pytest.mark.gpu

PAD = np.uint64(2 ** 64 - 1)
KEF = [(10, 64), (128, 128)]  # plus (30, n + 10): exhaustive, top_candidates in global memory
TIE_GRAPHS = [(600, 128, 64, 128, False), (600, 128, 64, 128, True), (400, 16, 4, 8, True),
              (900, 32, 100, 200, True), (40, 64, 8, 16, True)]


def _open(path):
    from deepreadmapper_amd import HnswFlatIndex
    return HnswFlatIndex(path)


def _check(ix, fx, q, k, ef):
    """test_gpu_flat._both on an already open handle."""
    D, L, st = ix.search(q, k, ef)
    Do, Io, nd, nh = O.hnswlib_search(fx, q, k, ef)
    what = f"n={fx['n']} d={fx['d']} maxM0={fx['maxM0']} nq={len(q)} k={k} ef={ef}"
    pad = Io < 0
    assert np.array_equal(L.astype(np.int64)[~pad], Io[~pad]) and (L[pad] == PAD).all(), what
    assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)), what  # 0 ulp
    assert st.ndis == int(nd.sum()) and st.nhops == int(nh.sum()), what
    assert ix.search_errors() == 0, what
    return Io


def _sweep(path, fx, q, kefs):
    """One fresh handle per (k, ef), as test_gpu_flat does."""
    for k, ef in kefs:
        ix = _open(path)
        _check(ix, fx, q, k, ef)
        ix.free()


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """Builder-made d = 128, M = 64, n = 2000 index (the C3 shape) + 32 queries."""
    path = str(tmp_path_factory.mktemp("built") / "b.hnsw")
    fx, x = G.build_and_read(path, 2000, 128, 64)
    q = np.random.default_rng(2).standard_normal((32, 128)).astype(np.float32)
    return {"index": path, "fx": fx, "q": q}


@pytest.fixture(scope="module")
def ties(tmp_path_factory):
    """The random tie graphs, keyed by their parameters, + 48 queries each."""
    d = tmp_path_factory.mktemp("ties")
    out = {}
    for n, dim, maxM, maxM0, dup in TIE_GRAPHS:
        path = str(d / f"t{n}_{dim}_{int(dup)}.hnsw")
        fx = G.write_and_read(path, G.random_tie_graph(np.random.default_rng(n + dim), n, dim, maxM, maxM0, dup))
        out[(n, dim, maxM, maxM0, dup)] = {"index": path, "fx": fx,
                                           "q": G.tie_queries(np.random.default_rng(1), 48, dim)}
    return out


@pytest.fixture(scope="module")
def stars(tmp_path_factory):
    d = tmp_path_factory.mktemp("stars")
    out = {}
    for hubs in (64, 70):
        path = str(d / f"s{hubs}.hnsw")
        out[hubs] = {"index": path, "fx": G.write_and_read(path, G.star_graph(hubs))}
    out["q"] = G.star_queries(np.random.default_rng(5), 300)
    return out


@pytest.mark.parametrize("d", [16, 32, 64, 256])
def test_dimensions(tmp_path, d):
    """NV = 0 generic kernel (l2_items, query in LDS): d != 128. 64 Gaussian queries + 16 stored vectors
    (distance 0), at the parallel heaps and at ef > ntotal (top_candidates continued in global memory)."""
    n = 2000
    path = str(tmp_path / "d.hnsw")
    fx, x = G.build_and_read(path, n, d, 16)
    assert fx["d"] == d
    q = np.concatenate([np.random.default_rng(d).standard_normal((64, d)).astype(np.float32), x[::125]])
    assert len(q) == 80
    _sweep(path, fx, q, KEF + [(30, n + 10)])


@pytest.mark.parametrize("d,n", [(16, 3000), (128, 1500)])
def test_wide_rows(tmp_path, d, n):
    """expand_row with maxM0 = 192 > 128: a second 128-slot pass, counts from l0cnt (test_flat_graphs_cpu:
    some row holds more than 128 links), in the generic and in the d = 128 kernel."""
    path = str(tmp_path / "w.hnsw")
    fx, x = G.build_and_read(path, n, d, 96)
    q = np.concatenate([np.random.default_rng(d).standard_normal((64, d)).astype(np.float32), x[::n // 16][:16]])
    _sweep(path, fx, q, KEF + [(30, n + 10)])


@pytest.mark.parametrize("n,d,maxM,maxM0,dup", TIE_GRAPHS)
def test_tie_graphs(ties, n, d, maxM, maxM0, dup):
    """Designed ties (tie_queries()[2] != 0), 64-bit labels, and with `dup` rows that list an id twice (check_dups).
    The first graph at (128, 128) is the MODE = 1 kernel on ties; the second differs only by the repeats and takes
    MODE = 0. (1, 1) and (10, 20) are one-group heaps, (400, 400) the three-group pop and the staged rank-by-count
    order by (distance, 64-bit label) -- on the 400- and 40-node graphs k > ntotal, so padding -- and ef = n + 5
    the serial top heap in LDS (600 + 5, 900 + 5), whose survivors are ranked by counting too."""
    t = ties[(n, d, maxM, maxM0, dup)]
    _sweep(t["index"], t["fx"], t["q"], [(128, 128), (10, 20), (1, 1), (400, 400), (16, n + 5)])


@pytest.mark.parametrize("which", ["built", "ties"])
def test_ef_boundaries(built, ties, which):
    """k = 16 at every ef where the heap code changes: par_pop_any's group edges (heap lengths 129/130 and 385/386
    are ef = 128/129 and 384/385; the first heap node a too small group would miss has its child at ef = 132 and
    386), the interrupted hop (candidate_set past 376 entries with ef <= 512:
    test_flat_graphs_cpu.test_interrupted_hop), parallel -> serial top heap (512/513), LDS -> global top heap
    (1023/1024)."""
    t = built if which == "built" else ties[TIE_GRAPHS[0]]
    efs = (127, 128, 129, 130, 131, 132, 383, 384, 385, 386, 387, 388, 511, 512, 513, 1022, 1023, 1024, 1025)
    _sweep(t["index"], t["fx"], t["q"][:32], [(16, ef) for ef in efs])


@pytest.mark.parametrize("which", ["built", "ties"])
def test_k_boundaries(built, ties, which):
    """ef = 64 at every k where the output order changes: bitonic128 (k <= 128), rank-by-count with labels staged
    in LDS (129 .. 376), unstaged with a wave-parallel top heap (377), unstaged from the global top heap (1500)."""
    t = built if which == "built" else ties[TIE_GRAPHS[0]]
    _sweep(t["index"], t["fx"], t["q"][:32], [(k, 64) for k in (127, 128, 129, 376, 377, 1500)])


def test_k_limit(ties):
    """k = 4096 is the largest supported (heavy padding on 600 nodes); k = 4097 is DRM_ERR_UNSUPPORTED."""
    from deepreadmapper_amd._native import DrmError, DRM_ERR_UNSUPPORTED
    t = ties[TIE_GRAPHS[0]]
    ix = _open(t["index"])
    Io = _check(ix, t["fx"], t["q"][:32], 4096, 64)
    assert ((Io >= 0).sum(axis=1) <= 600).all()
    with pytest.raises(DrmError) as e:
        ix.search(t["q"][:32], 4097, 64)
    assert e.value.code == DRM_ERR_UNSUPPORTED
    _check(ix, t["fx"], t["q"][:32], 10, 20)
    ix.free()


@pytest.mark.parametrize("d,maxM,maxM0", [(16, 4, 8), (128, 64, 128)])
@pytest.mark.parametrize("n", [0, 1, 5])
def test_tiny_indexes(tmp_path, n, d, maxM, maxM0):
    """ntotal in {0, 1, 5} with maxlevel = 0, in the generic kernel and in the C3 shape (where (128, 128) is the
    MODE = 1 kernel): ntotal < k pads, ntotal = 0 returns only padding and ndis = nhops = 0."""
    path = str(tmp_path / "tiny.hnsw")
    fx = G.write_and_read(path, G.tiny_graph(np.random.default_rng(n), n, d, maxM, maxM0))
    assert fx["n"] == n and fx["maxlevel"] == 0
    q = G.tie_queries(np.random.default_rng(1), 70, d)
    ix = _open(path)
    for k, ef in [(1, 1), (10, 20), (128, 128)]:
        Io = _check(ix, fx, q, k, ef)
        assert ((Io >= 0).sum(axis=1) == min(n, k)).all()
    if n == 0:
        D, L, st = ix.search(q, 10, 20)
        assert (L == PAD).all() and np.isinf(D).all() and st.ndis == 0 and st.nhops == 0
    ix.free()


def test_empty_index_as_hnswlib_writes_it(tmp_path):
    """hnswlib's own empty index: maxlevel = -1 and entry point -1."""
    path = str(tmp_path / "empty.hnsw")
    g = G.tiny_graph(np.random.default_rng(0), 0, 16, 4, 8)
    g["ep"] = 0xFFFFFFFF
    fx = G.write_and_read(path, dict(g, maxlevel=-1))
    ix = _open(path)
    _check(ix, fx, G.tie_queries(np.random.default_rng(1), 6, 16), 10, 20)
    ix.free()


def test_small_graph_with_upper_levels(ties):
    """40 nodes on three levels: ntotal < k, ntotal < ef, upper-level descent among ties."""
    t = ties[TIE_GRAPHS[4]]
    assert t["fx"]["maxlevel"] > 0
    _sweep(t["index"], t["fx"], t["q"], [(1, 1), (10, 20), (128, 128)])


def test_one_handle_many_calls_star(stars):
    """One handle on star_graph(64), five searches in a row, each against the oracle:
    1. 300 queries at (10, 64): every query computes 16641 > clear_cap distances -> full-bitmap reset, in slots
       that the next calls use again;
    2. the same at (10, 8): list reset; a stale visited bit of call 1 would change ndis and the neighbours;
    3. 4 queries at ef = n + 1: top_candidates in global memory, candidate_set 16576 entries deep, within its
       376 + 16384 capacity (test_flat_graphs_cpu.test_star_graphs), serial heaps in global memory with ties;
    4. call 1 again, after call 3 grew top_ovf and so reallocated the whole workspace;
    5. one query: fewer slots than allocated."""
    s, q = stars[64], stars["q"]
    n = s["fx"]["n"]
    ix = _open(s["index"])
    _check(ix, s["fx"], q, 10, 64)
    _check(ix, s["fx"], q, 10, 8)
    _check(ix, s["fx"], q[:4], 10, n + 1)
    assert ix.overflows() == 0
    _check(ix, s["fx"], q, 10, 64)
    _check(ix, s["fx"], q[7:8], 10, 64)
    ix.free()


def test_full_reset_then_reuse_within_one_launch(stars, monkeypatch):
    """One wave slot per CU (DRM_SEARCH_WAVES_PER_CU = 1, read when the index is loaded) and 2000 queries, so every
    slot serves several queries of one launch: each resets its whole bitmap (16641 > clear_cap distances) and the
    next query of the slot starts on it without a wait in between. Then the list reset under the same reuse."""
    monkeypatch.setenv("DRM_SEARCH_WAVES_PER_CU", "1")
    s = stars[64]
    q = G.star_queries(np.random.default_rng(6), 2000)
    ix = _open(s["index"])
    _check(ix, s["fx"], q, 10, 64)
    _check(ix, s["fx"], q, 10, 8)
    ix.free()


def test_one_handle_many_calls_built(built):
    """The same on the C3 shape: exhaustive ef (global top heap, workspace grown), then a small ef, then a large
    k, then the MODE = 1 kernel, on one handle."""
    ix = _open(built["index"])
    for k, ef in [(10, 64), (10, 2010), (10, 8), (1500, 64), (128, 128), (10, 2010)]:
        _check(ix, built["fx"], built["q"], k, ef)
    ix.free()


def test_candidate_overflow_is_reported(stars):
    """star_graph(70) at ef = n + 1: candidate_set needs 18106 > 376 + 16384 entries. drm_flat_search returns
    DRM_ERR_UNSUPPORTED (include/drm_hip.h), overflows() counts the 4 queries, and the handle goes on working."""
    from deepreadmapper_amd._native import DrmError, DRM_ERR_UNSUPPORTED
    s, q = stars[70], stars["q"]
    ix = _open(s["index"])
    with pytest.raises(DrmError) as e:
        ix.search(q[:4], 10, s["fx"]["n"] + 1)
    assert e.value.code == DRM_ERR_UNSUPPORTED
    assert ix.overflows() == 4
    _check(ix, s["fx"], q, 10, 64)
    assert ix.overflows() == 0
    ix.free()
