"""CPU side of the hand-made HNSW-PQ fixtures (tests/pq_graphs.py): the writer is the exact inverse of the oracle's
reader, the packed codes mean what an independent numpy ADC says they mean, and every fixture that
tests/test_gpu_pq_paths.py puts in front of hnsw_search.hip, hnsw_search_lds.hip and hnsw_pq_fast.hip reaches the
kernel path it is meant for -- proved here from the oracle's own ndis / nhops / results, so a fixture that stops
reaching its path fails without a GPU."""
import numpy as np
import pytest

import pq_graphs as P
from oracle import oracle as O

# The thresholds of the launcher (deepreadmapper_amd/csrc/hnsw_search.hip):
CLEAR_CAP = 16384   # ensure_visited `const int32_t clear_cap = 16384`: visited ids a query lists before
#                     it resets its whole bitmap (`clear_n <= a.clear_cap` at the end of each kernel's query loop)
R_MAX = 8           # plan_search `if (R > 8 || ix.force_lds_kernel)`, R = ceil(max(ef, k) / 64):
LDS_ABOVE = 512     # ... so max(ef, k) > 512 goes to the LDS-heap kernel
LEAN_EF_MAX = 128   # hnsw_pq_fast.hip hnsw_pq_fast_supported: `efc <= 128 && (k == efc || k <= 64)`, PQ 8 x 8 only
LEAN_K_REG = 64
K_MAX = 1024        # check_search_limits: `k < 1 || k > 1024`
EFC_MAX = 4096      # check_search_limits, the LDS-heap kernel only: `efc > 4096`
DEG_MAX = 64        # check_search_limits: `ix.deg0 > 64`, `ix.cum[l + 1] - ix.cum[l] > 64`
LUT_MAX = 16384     # check_search_limits: `pq_M * ksub > 16384`


def kernel_of(M_pq, nbits, k, ef, fast=True, force_lds=False):
    """plan_search's choice: "lean", "lds", or the general kernel's R instantiation (1, 2, 4, 8)."""
    efc = max(ef, k)
    assert 1 <= k <= K_MAX and efc <= EFC_MAX and M_pq * (1 << nbits) <= LUT_MAX
    R = (efc + 63) // 64
    if R > R_MAX or force_lds:
        return "lds"
    if fast and (M_pq, nbits) == (8, 8) and efc <= LEAN_EF_MAX and (k == efc or k <= LEAN_K_REG):
        return "lean"
    return {1: 1, 2: 2, 3: 4, 4: 4}.get(R, 8)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("pqbuilt")
    return {name: P.make_built(d, name) for name in list(P.BUILT_SHAPES) + ["8x8"]}


@pytest.fixture(scope="module")
def rnd4x12(tmp_path_factory):
    return P.make_random(tmp_path_factory.mktemp("pq4x12"), "4x12", 64, 4, 12, 16, 1500)


def test_case_lists_reach_every_instantiation():
    """The (k, ef) lists of the GPU tests against the thresholds above: the general list takes R = 1, 2, 4 and 8 on a
    generic shape, the LDS list only the LDS-heap kernel with both k <= 512 < ef and k > 512 (kpad = 1024), the
    lean list only the lean kernel on 8 x 8 (and the general one with the lean kernel off)."""
    assert {kernel_of(4, 8, k, ef) for k, ef in P.GENERAL_KEF} == {1, 2, 4, 8}
    assert {kernel_of(8, 6, k, ef) for k, ef in P.LDS_KEF} == {"lds"}
    assert any(k > LDS_ABOVE for k, _ in P.LDS_KEF) and any(k <= LDS_ABOVE < ef for k, ef in P.LDS_KEF)
    assert max(max(k, ef) for k, ef in P.LDS_KEF) == EFC_MAX and max(k for k, _ in P.LDS_KEF) == K_MAX
    assert {kernel_of(8, 8, k, ef) for k, ef in P.LEAN_KEF} == {"lean"}
    assert {kernel_of(8, 8, k, ef, fast=False) for k, ef in P.LEAN_KEF} == {1, 2}
    assert any(k == ef for k, ef in P.LEAN_KEF) and any(k != ef and k <= LEAN_K_REG for k, ef in P.LEAN_KEF)
    for d, M_pq, nbits, M_hnsw in list(P.BUILT_SHAPES.values()) + list(P.LEAN_DEGREES.values()):
        assert 2 * M_hnsw <= DEG_MAX and M_pq * (1 << nbits) <= LUT_MAX
    assert 4 * (1 << 12) == LUT_MAX and 4 * (1 << 13) == 2 * LUT_MAX and 2 * (1 << 16) > LUT_MAX


@pytest.mark.parametrize("name", ["8x8", "4x8d32", "8x6", "8x10"])
def test_writer_round_trip(built, tmp_path, name):
    """A builder-made file, read with oracle/faiss_file.py and written again by pq_graphs.write_ihnp from the
    unpacked fields (link lists, centroid indices), is byte-identical."""
    b = built[name]
    dst = P.rewrite(b["fx"], str(tmp_path / "rewritten.index"))
    assert open(b["index"], "rb").read() == open(dst, "rb").read()
    assert b["fx"].ntotal == 2902 and b["fx"].max_level > 0


def test_packer_bit_layout():
    """Index m sits at bits [m * nbits, (m + 1) * nbits), least-significant first: worked by hand for 8 x 5 (the
    second index straddles bytes 0 / 1) and 2 x 10 (three bytes, the second index at shift 2 of byte 1)."""
    got = P.pack_codes([[0b10101, 0b11011, 0, 0, 0, 0, 0, 0b10000]], 5)
    assert got.tolist() == [[0b01110101, 0b00000011, 0, 0, 0b10000000]]
    assert P.pack_codes([[0x3FF, 0x201]], 10).tolist() == [[0xFF, 0x07, 0x08]]
    rng = np.random.default_rng(0)
    for M_pq, nbits in ((8, 5), (8, 6), (8, 10), (4, 12), (4, 13), (2, 16), (3, 7)):
        idx = rng.integers(0, 1 << nbits, size=(50, M_pq))
        assert np.array_equal(P.unpack_codes(P.pack_codes(idx, nbits), M_pq, nbits), idx)


@pytest.mark.parametrize("name", ["8x6", "8x5", "8x10", "4x12"])
def test_adc_reference(built, rnd4x12, name):
    """Independent of the oracle: the ADC distance of every id from the centroid indices BEFORE packing, in numpy
    float32 in the documented order, equals bit for bit the D the oracle returns for that id in an exhaustive
    search (ef >= ntotal). Ties the Python packer to the oracle's decoder (and, through the GPU tests, to the
    kernels')."""
    f = rnd4x12 if name == "4x12" else built[name]
    fx, q = f["fx"], f["q"][[0, 1, len(f["q"]) - 1]]
    n = fx.ntotal
    ref = P.adc_reference(f["centroids"], f["codes_idx"], q)
    D, I, _, _ = O.hnswpq_search(fx, q, n, n + 8)
    for i in range(len(q)):
        ok = I[i] >= 0
        assert ok.sum() > 0.9 * n  # the walk reaches (nearly) every id
        assert np.array_equal(D[i][ok].view(np.uint32), ref[i][I[i][ok]].view(np.uint32)), (name, i)


def test_fan_graphs_pass_the_clear_list(tmp_path):
    """fan_graph(n, 64), one level. n = 20,000 at ef = 2048 (LDS-heap kernel) and n = 24,000 at ef = 512 (general
    kernel): every query computes more than clear_cap distances -- the full-bitmap reset -- and, ndis - 1 being the
    pushes after the seed on a one-level graph, fills and evicts from the candidate heap. The small-ef search that
    follows on the same handle stays on the list reset."""
    for n, ef in ((P.FAN_N_LDS, 2048), (P.FAN_N_GENERAL, 512)):
        f = P.make_fan(tmp_path, n)
        assert f["fx"].max_level == 0 and kernel_of(8, 8, 10, ef) == ("lds" if ef > LDS_ABOVE else 8)
        _, _, nd, nh = O.hnswpq_search(f["fx"], f["q"], 10, ef)
        assert nd.min() > CLEAR_CAP and nd.min() - 1 > ef and nh.max() < n
        _, _, nd, _ = O.hnswpq_search(f["fx"], f["q"], 10, 16)
        assert 64 < nd.min() and nd.max() <= CLEAR_CAP


def test_ramp_graph_passes_the_clear_list_at_any_ef(tmp_path):
    """make_ramp: a sweep query computes n - 1 > clear_cap distances at the lean kernel's ef <= 128 (and at ef = 1),
    which no fan graph does (about 7,000 at ef = 128); a stall query stays on the list reset. Level-0 rows are full
    (no -1) except the last 64: the lean kernel's full-wave row."""
    f = P.make_ramp(tmp_path)
    n = f["fx"].ntotal
    assert n == P.RAMP_N > CLEAR_CAP and f["fx"].max_level == 0 and f["fx"].cum_nneighbor_per_level[1] == DEG_MAX
    rng = np.random.default_rng(3)
    sweep, stall = P.ramp_queries(rng, 12), P.ramp_queries(rng, 12, stall=True)
    for k, ef in P.LEAN_KEF + [(10, 16), (1, 1), (300, 512), (10, 600)]:
        _, _, nd, nh = O.hnswpq_search(f["fx"], sweep, k, ef)
        assert (nd == n - 1).all() and nd.min() - 1 > max(ef, k) and nh.max() < n, (k, ef)
        _, _, nd, _ = O.hnswpq_search(f["fx"], stall, k, ef)
        assert 64 <= nd.min() and nd.max() <= CLEAR_CAP, (k, ef)


@pytest.mark.parametrize("name", list(P.BUILT_SHAPES) + ["8x8"])
def test_built_indices_fill_the_heap_and_stop(built, name):
    """2,902-node built indices at the LDS kernel's (600, 600) and (10, 600): the walk ends on the stop condition
    (nhops < ntotal, and fewer distances than an exhaustive walk computes, so candidates were left over) on a full
    600-entry heap that rejected or evicted: the level-0 pushes are ndis less the upper levels' distances, which are
    the same at any ef and at most the whole ndis of a (1, 1) search -- more than ef of them."""
    b = built[name]
    fx = b["fx"]
    assert fx.ntotal == 2902
    _, _, nd_all, _ = O.hnswpq_search(fx, b["q"], 10, fx.ntotal + 8)
    _, _, nd_1, _ = O.hnswpq_search(fx, b["q"], 1, 1)
    for k, ef in ((600, 600), (10, 600)):
        _, _, nd, nh = O.hnswpq_search(fx, b["q"], k, ef)
        assert nh.max() < fx.ntotal and (nd < nd_all).all()
        assert (nd - nd_1 > ef).all()


def test_k_padding_fixtures(tmp_path):
    """ntotal < k: a 300-node chain at k = 513 / 1024 returns fewer than k ids and pads -- all 300 at ef = 600, fewer
    at efSearch = 16, where the walk stops among ties first; ntotal = 0 returns only padding."""
    for M_pq, nbits, d in ((8, 8, 128), (8, 6, 128), (4, 8, 32)):
        f = P.make_chain(tmp_path, f"c{M_pq}x{nbits}", d, M_pq, nbits, 8, 300)
        for k, ef in ((513, 16), (1024, 16), (513, 600)):
            D, I, nd, _ = O.hnswpq_search(f["fx"], f["q"], k, ef)
            valid = (I >= 0).sum(axis=1)
            assert (valid == 300).all() if ef == 600 else ((valid > 64) & (valid < 300)).all()
            for i in range(len(I)):
                assert (I[i, valid[i]:] == -1).all() and np.isinf(D[i, valid[i]:]).all()
            assert (D[:, 1:64] == D[:, :63]).any()  # ties inside the sorted part
        e = P.make_chain(tmp_path, f"e{M_pq}x{nbits}", d, M_pq, nbits, 8, 0)
        assert e["fx"].ntotal == 0 and e["fx"].entry_point == -1
        D, I, nd, nh = O.hnswpq_search(e["fx"], e["q"], 10, 600)
        assert (I == -1).all() and np.isinf(D).all() and not nd.any() and not nh.any()


@pytest.mark.parametrize("M_pq,nbits,d", [(8, 8, 128), (8, 6, 128)])
def test_tie_fixtures_straddle_k(tmp_path, M_pq, nbits, d):
    """make_tie (1,500 nodes, 8 distinct distances): at k = 513 and k = 1024 the k-th and (k + 1)-th smallest
    distances of every query are equal -- which of the tied ids the result heap keeps decides the output (seen with
    ef = 2048 for both k, so the walk is the same) -- and the graph has a repeated link (check_dups) and levels."""
    f = P.make_tie(tmp_path, "tie", d, M_pq, nbits, 16, 1500)
    assert f["fx"].max_level > 0
    rows = P.rows_of(f["fx"])
    assert any(len([v for v in r[0] if v >= 0]) != len({v for v in r[0] if v >= 0}) for r in rows)
    for k in (513, 1024):
        D, I, _, _ = O.hnswpq_search(f["fx"], f["q"], k + 1, 2048)
        assert (I[:, k] >= 0).all() and (D[:, k - 1] == D[:, k]).all()
        assert len(np.unique(D[np.isfinite(D)])) < 200


def test_full_rows_graph(tmp_path):
    """random_graph(hole_p = 0) at M_hnsw = 32: every level-0 row holds 64 links and no -1, so the lean kernel's
    `jmax` has no hole to find and takes its fallback."""
    f = P.make_random(tmp_path, "full64", 128, 8, 8, 32, 3000, hole_p=0.0, dup=False)
    rows = P.rows_of(f["fx"])
    assert all(len(r[0]) == DEG_MAX and min(r[0]) >= 0 for r in rows) and f["fx"].max_level > 0


def test_random_4x12_fixture(rnd4x12):
    """4 x 12 at d = 64: a LUT of exactly 16384 entries, 6-byte codes, holes, a repeated link, three levels."""
    fx = rnd4x12["fx"]
    assert fx.pq_M * (1 << fx.pq_nbits) == LUT_MAX and len(fx.codes) == 6 * fx.ntotal and fx.max_level == 2
    assert (fx.neighbors == -1).any()
    _, _, nd, nh = O.hnswpq_search(fx, rnd4x12["q"], 600, 600)
    assert nd.min() - 1 > 600 + 64 * 2 and nh.max() < fx.ntotal
