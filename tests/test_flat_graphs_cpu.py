"""CPU side of the hand-made fp32 index fixtures (tests/hnswlib_graphs.py): the writer is the exact inverse of the
oracle's reader, and every fixture that tests/test_gpu_flat_paths.py puts in front of hnsw_flat_search.hip reaches
the kernel path it is meant for -- proved here from the oracle's own diagnostics (largest candidate_set, queries
with tied heap operations, distances computed), so a fixture that stops reaching its path fails without a GPU."""
import numpy as np
import pytest

import hnswlib_graphs as G
from oracle import oracle as O

# The thresholds of the launcher (deepreadmapper_amd/csrc/hnsw_flat_search.hip, launch_hnsw_flat_search):
CAND_LDS = 376     # DRM_FLAT_CAND_LDS (#define near l2_items_reg): candidate_set entries held in LDS
OVF_CAP = 16384    # `const int64_t ovf_cap = 16384`: candidate_set entries per slot in global memory
CLEAR_CAP = 16384  # `ix.clear_cap = 16384`: visited ids a query may list before it resets the whole bitmap
TOP_PAR_MAX = 512  # `top_par = ef + 1 <= min(top_lds, 513)`: largest ef with wave-parallel top_candidates
TOP_LDS_MAX = 1024  # `top_lds = min(efc + 1, 1024)`: top_candidates entries in LDS, the rest in global memory
ROW_PASS = 128     # expand_row handles 128 link slots per pass

TIE_GRAPHS = [(600, 128, 64, 128, False), (600, 128, 64, 128, True), (400, 16, 4, 8, True),
              (900, 32, 100, 200, True), (40, 64, 8, 16, True)]


def _row_counts(fx):
    return fx["l0"][:, 0] & 0xFFFF


def _labels_need_64_bits(lab):
    """Neither 32-bit half orders the labels, and none is a node id."""
    n = len(lab)
    lo, hi = lab & np.uint64(0xFFFFFFFF), lab >> np.uint64(32)
    assert len(np.unique(lab)) == n and int(lab.min()) >= 2 ** 33 and int(lab.max()) < 2 ** 63
    assert not np.array_equal(np.argsort(lo, kind="stable"), np.argsort(lab, kind="stable"))
    assert 1 < len(np.unique(hi)) < n and len(np.unique(lo)) == n
    assert not (lab == np.arange(n, dtype=np.uint64)).any()


def test_writer_round_trip(tmp_path):
    """write_hnswlib(read(file)) is byte-identical to a builder-made file (d = 16, M = 8, n = 3000)."""
    src = str(tmp_path / "built.hnsw")
    fx, _ = G.build_and_read(src, 3000, 16, 8)
    assert fx["n"] == 3000 and fx["maxlevel"] > 0 and (fx["levels"] > 0).any()
    dst = G.rewrite(fx, str(tmp_path / "rewritten.hnsw"))
    assert open(src, "rb").read() == open(dst, "rb").read()


def test_writer_from_rows_reads_back(tmp_path):
    """The list form of the writer (link lists instead of raw records) reads back to the same graph."""
    g = G.random_tie_graph(np.random.default_rng(3), 40, 64, 8, 16, True)
    fx = G.write_and_read(str(tmp_path / "g.hnsw"), g)
    assert fx["n"] == 40 and fx["d"] == 64 and fx["maxM"] == 8 and fx["maxM0"] == 16 and fx["ep"] == g["ep"]
    assert np.array_equal(fx["vec"], g["vec"]) and np.array_equal(fx["labels"], g["labels"])
    for i in range(40):
        assert list(fx["l0"][i, 1:1 + fx["l0"][i, 0]]) == g["l0_rows"][i]
        assert fx["levels"][i] == len(g["up_rows"][i])
        for l, lst in enumerate(g["up_rows"][i]):
            b = fx["up_off"][i] + l * 9
            assert list(fx["up"][b + 1:b + 1 + fx["up"][b]]) == lst
    assert fx["maxlevel"] == fx["levels"][fx["ep"]] == fx["levels"].max()


@pytest.mark.parametrize("n,d,maxM,maxM0,dup", TIE_GRAPHS)
def test_tie_graphs_tie_and_repeat(tmp_path, n, d, maxM, maxM0, dup):
    """Designed ties: at (k, ef) = (128, 128) some query pops or evicts among equal keys (tie_queries()[2] != 0), so
    the heap layout decides the traversal. `dup` graphs hold a row that lists one id twice (has_dup_links = 1 in
    the loader, check_dups in expand_row), the others none; links respect the levels the reader enforces; labels
    need all 64 bits."""
    g = G.random_tie_graph(np.random.default_rng(n + d), n, d, maxM, maxM0, dup)
    fx = G.write_and_read(str(tmp_path / "t.hnsw"), g)
    q = G.tie_queries(np.random.default_rng(1), 48, d)
    O.hnswlib_search(fx, q, 128, 128)
    assert O.hnswlib_tie_queries()[2] > 0
    assert G.has_dup_row(fx) == dup
    _labels_need_64_bits(fx["labels"])
    assert fx["levels"][fx["ep"]] == fx["maxlevel"] == fx["levels"].max() > 0
    blk = 1 + maxM
    for i in np.flatnonzero(fx["levels"]):
        for l in range(1, fx["levels"][i] + 1):
            b = fx["up_off"][i] + (l - 1) * blk
            assert (fx["levels"][fx["up"][b + 1:b + 1 + fx["up"][b]]] >= l).all()


@pytest.mark.parametrize("n", [0, 1, 5])
def test_tiny_graphs(tmp_path, n):
    """ntotal in {0, 1, 5}, one level: the reader accepts the files and the search returns every element, ordered
    by (distance, label), then padding."""
    fx = G.write_and_read(str(tmp_path / "tiny.hnsw"), G.tiny_graph(np.random.default_rng(n), n, 16, 4, 8))
    assert fx["n"] == n and fx["maxlevel"] == 0 and not (fx["levels"] > 0).any()
    q = G.tie_queries(np.random.default_rng(1), 6, 16)
    Do, Io, nd, nh = O.hnswlib_search(fx, q, 10, 20)
    for i in range(len(q)):
        dist = ((fx["vec"].astype(np.float64) - q[i]) ** 2).sum(axis=1)  # exact: small multiples of 0.25
        order = sorted(range(n), key=lambda j: (dist[j], int(fx["labels"][j])))
        assert Io[i, :n].tolist() == [int(fx["labels"][j]) for j in order] and (Io[i, n:] == -1).all()
        assert Do[i, :n].tolist() == [dist[j] for j in order] and np.isinf(Do[i, n:]).all()
    assert (nd == n).all() and (nh == min(n, 1) * n).all()


@pytest.mark.parametrize("d,n", [(16, 3000), (128, 1500)])
def test_wide_rows_need_two_passes(tmp_path, d, n):
    """M = 96 (maxM0 = 192): some level-0 row holds more than 128 links, so expand_row takes a second 128-slot
    pass with the count from l0cnt."""
    fx, _ = G.build_and_read(str(tmp_path / "w.hnsw"), n, d, 96)
    assert fx["maxM0"] == 192 and int(_row_counts(fx).max()) > ROW_PASS


def test_interrupted_hop(tmp_path):
    """d = 128, M = 64, n = 2000 at ef = 400: candidate_set outgrows its LDS part (maxcand > 376) while
    top_candidates is still wave-parallel (ef <= 512), so the fast hop loop hands a hop over to slow_consider
    half-way. At k > 1024 the survivors fill top_candidates past its LDS part."""
    fx, x = G.build_and_read(str(tmp_path / "b.hnsw"), 2000, 128, 64)
    q = np.random.default_rng(2).standard_normal((32, 128)).astype(np.float32)
    ef = 400
    O.hnswlib_search(fx, q, 16, ef)
    assert ef <= TOP_PAR_MAX and O.hnswlib_maxcand() > CAND_LDS
    _, Io, _, _ = O.hnswlib_search(fx, q, 1500, 64)
    assert ((Io >= 0).sum(axis=1) == 1500).all() and 1500 > TOP_LDS_MAX


def test_star_graphs(tmp_path):
    """star_graph(64): an exhaustive search takes candidate_set deep into its global part but within capacity
    (16384 < maxcand <= 376 + 16384), and at ef = 64 every query computes more than clear_cap distances (the
    full-bitmap reset). star_graph(70): candidate_set outgrows the capacity (the defined overflow error)."""
    s64 = G.write_and_read(str(tmp_path / "s64.hnsw"), G.star_graph(64))
    q = G.star_queries(np.random.default_rng(5), 8)
    n = s64["n"]
    O.hnswlib_search(s64, q, 10, n + 1)
    assert O.hnswlib_maxcand() == 256 + 255 * 64 == 16576
    assert OVF_CAP < O.hnswlib_maxcand() <= CAND_LDS + OVF_CAP
    _, _, nd, _ = O.hnswlib_search(s64, q, 10, 64)
    assert (nd > CLEAR_CAP).all() and (nd == 1 + 256 + 256 * 64).all()
    _, _, nd, _ = O.hnswlib_search(s64, q, 10, 8)
    assert ((nd > 257) & (nd <= CLEAR_CAP)).all()  # node 0's children and a few hubs' leaves: the list reset
    s70 = G.write_and_read(str(tmp_path / "s70.hnsw"), G.star_graph(70))
    O.hnswlib_search(s70, q[:4], 10, s70["n"] + 1)
    assert O.hnswlib_maxcand() == 256 + 255 * 70 == 18106 > CAND_LDS + OVF_CAP


def test_load_rejects_upper_blocks_wider_than_level0_rows(tmp_path):
    """maxM > maxM0: the oracle's reader and the product's parser accept the file, but the kernel stages an
    upper-level block (up to maxM links) in the LDS area sized for a level-0 row (maxM0 slots), so the loader
    refuses it before anything is uploaded (no GPU needed). hnswlib itself always writes maxM0 = 2 * maxM."""
    from deepreadmapper_amd import DrmError
    from deepreadmapper_amd._native import DRM_ERR_UNSUPPORTED
    from deepreadmapper_amd.flat import HnswFlatIndex
    g = G.random_tie_graph(np.random.default_rng(9), 60, 16, 16, 8, False)
    assert max(len(b) for r in g["up_rows"] for b in r) > 8  # a block that would not fit
    path = str(tmp_path / "wide_upper.hnsw")
    fx = G.write_and_read(path, g)
    assert fx["maxM"] == 16 and fx["maxM0"] == 8
    with pytest.raises(DrmError) as e:
        HnswFlatIndex(path)
    assert e.value.code == DRM_ERR_UNSUPPORTED and "maxM > maxM0" in str(e.value)
