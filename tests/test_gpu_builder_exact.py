"""The GPU index builder's file (builder_gpu.hip, drm_build_hnswpq_device) equals its plain restatement
(tests/builder_ref.py, itself checked in tests/test_builder_ref_cpu.py), link for link: levels, offsets, entry point,
max_level, PQ codes and every list of every node on every level, ids and -1 padding. The centroids are read from the
built file (test_gpu_builder.py holds them equal to the host builder's); everything else is restated from x.
A recall ratio absorbs a few lost links; this does not.

What each case compared (nodes / levels / lists) and what its restatement cost on one CPU core:
    shipped configuration, C1 windows, M 16, efC 200    1702 / 3 / 1804                             1.9 s
    beam width, 600 Gaussian, M 16, each of 9 efC        600 / 3 / 631                              0.3 to 0.5 s each
    degree, 600 Gaussian, efC 40, M 2, 4, 12, 32         600 / 11, 6, 3, 3 / 1183, 796, 649, 614    0.2 to 0.3 s each
    ties, 4 x 150 integer rows, efC 200, M 4, 16         600 / 6, 3 / 796, 631                      0.5 s each
    few nodes, n = 1, 2, 3, 5, 33, 65, 257, M 16         n / 1, 1, 1, 1, 2, 2, 2 / 1, 2, 3, 5, 36, 70, 274    < 0.1 s
    knobs, 600 Gaussian, M 16, efC 64                    600 / 3 / 631                              0.5 s
The GPU builds themselves take 0.1 to 0.2 s each (C1: 0.9 s with its restatement).
Sensitivity, on scratch builds of the kernel: `<=` for `<` in the neighbour heuristic fails test_ties (both M) and
none of test_gpu_builder.py's tests; the beam's shift without its carry between registers fails every case with ef > 64;
without the per-level bitmap clear nearly every case here fails.
Few nodes: the host k-means takes fewer training points than centroids (it reuses points), so the list starts at
n = 1; sample_rate is 1.0 there, so that every point trains.
Knobs (computed from n, the knob values and the restatement's visited counts): the batches of n = 600 are 1, 2, 4,
..., 256, 88 nodes; with DRM_BUILD_SLOTS=3 three waves share each, so the busiest wave takes at least 86 items of the
256-node batch on its one bitmap slot (by default every node of these batches has a wave to itself); with
DRM_BUILD_CLEAR_CAP=8 a level ends in the full-bitmap clear when its beam visited more than 8 nodes: 597 of the
628 beams (the others are the first nodes' and upper-level beams); by default (16384) none does: a beam visits 392
nodes at the most."""
import os

import numpy as np
import pytest

import builder_ref as R

pytestmark = pytest.mark.gpu

_restated = {}


def _restate(key, x, centroids, M_hnsw, efc, seed=0):
    """One restatement per (vectors, M_hnsw, beam width), shared by the builds that must equal it."""
    key = (key, M_hnsw, max(min(efc, R.EF_CAP), 2 * M_hnsw), seed)
    if key not in _restated:
        _restated[key] = (R.build(x, centroids, M_hnsw, efc, seed), np.array(centroids))
    b, cen = _restated[key]
    assert np.array_equal(cen.view(np.uint32), np.asarray(centroids).view(np.uint32))  # same PQ, build after build
    return b


def _build_and_compare(tmp_path, key, x, M_hnsw, efc, sample_rate=0.5, seed=0, tag=""):
    """GPU build of x; asserts the file equals the restatement; returns the file's bytes."""
    from deepreadmapper_amd import synth
    from oracle import faiss_file
    path = str(tmp_path / f"{key}_M{M_hnsw}_efc{efc}{tag}.index")
    synth.build_index_gpu(x, path, M_hnsw=M_hnsw, efc=efc, sample_rate=sample_rate, seed=seed)
    fx = faiss_file.read(path)
    b = _restate(key, x, fx.centroids, M_hnsw, efc, seed)
    assert fx.ntotal == len(x) and fx.efConstruction == efc
    assert np.array_equal(fx.levels, b.levels) and np.array_equal(fx.offsets, b.offsets)
    assert fx.entry_point == b.entry_point and fx.max_level == b.max_level
    assert np.array_equal(fx.codes, b.codes.reshape(-1))
    diff, nlists = R.first_difference(fx, b)
    print(f"{key} M_hnsw {M_hnsw} efC {efc}{tag}: {len(x)} nodes, {b.max_level + 1} levels, {nlists} lists compared")
    assert diff is None, diff
    assert nlists == int(b.levels.sum()) and np.array_equal(fx.neighbors, b.neighbors)
    with open(path, "rb") as f:
        return f.read()


def test_shipped_configuration_c1(tmp_path, c1):
    """All 1702 C1 windows (k-mer embedding) at M_hnsw = 16, efConstruction = 200. Overlapping windows give many
    nodes with one PQ code, so (distance, id) ties are everywhere."""
    from deepreadmapper_amd import synth
    x = synth.embed(c1["refs"])
    assert len(x) == 1702
    _build_and_compare(tmp_path, "c1", x, 16, 200)


@pytest.mark.parametrize("efc", [10, 63, 64, 65, 128, 129, 200, 256, 300])
def test_beam_width(tmp_path, efc):
    """The two sides of each 64-slot register of the beam and of the <2> / <4> kernel instantiations (ef <= 128 and
    above); 10 is raised to deg0 = 32, 300 is capped at 256. At this size the beam fills at every width (it visits
    290 to 511 nodes), and the restated graphs of 63, 64 and 65 differ from one another."""
    _build_and_compare(tmp_path, "gauss600", R.gaussian_vectors(600), 16, efc)


def test_beam_width_cap(tmp_path):
    """efConstruction = 300 is capped at 256: the two files are the same byte for byte, but for the four bytes in
    which each records the efConstruction it was asked for (as the host builder's file does)."""
    import struct
    x = R.gaussian_vectors(600)
    f256, f300 = (_build_and_compare(tmp_path, "gauss600", x, 16, efc) for efc in (256, 300))
    b = _restated[("gauss600", 16, 256, 0)][0]
    # fourcc, index header, then the vectors (u64 length first) assign_probas f64, cum_nneighbor_per_level i32,
    # levels i32, offsets u64, neighbors i32, then entry_point, max_level, efConstruction
    n_probas = len(R.assign_probas(16))
    at = 4 + 33 + (8 + 8 * n_probas) + (8 + 4 * (n_probas + 1)) + (8 + 4 * 600) + (8 + 8 * 601) + \
        (8 + 4 * len(b.neighbors)) + 8
    assert struct.unpack_from("<i", f256, at)[0] == 256 and struct.unpack_from("<i", f300, at)[0] == 300
    assert len(f256) == len(f300) and f256[:at] == f300[:at] and f256[at + 4:] == f300[at + 4:]


@pytest.mark.parametrize("M_hnsw", [2, 4, 12, 32])
def test_degree(tmp_path, M_hnsw):
    """M = 2 gives many levels (the upper-list offsets), M = 32 makes the level-0 list the whole wave and ef = 64."""
    _build_and_compare(tmp_path, "gauss600", R.gaussian_vectors(600), M_hnsw, 40)


@pytest.mark.parametrize("M_hnsw", [1, 33])
def test_degree_out_of_range(tmp_path, M_hnsw):
    from deepreadmapper_amd import synth
    from deepreadmapper_amd._native import DrmError
    with pytest.raises(DrmError) as e:
        synth.build_index_gpu(R.gaussian_vectors(64), str(tmp_path / "bad.index"), M_hnsw=M_hnsw, efc=40)
    assert e.value.code == -1, str(e.value)  # DRM_ERR_ARG


@pytest.mark.parametrize("M_hnsw", [4, 16])
def test_ties(tmp_path, M_hnsw):
    """Integer rows, each present four times: distances are equal for whole groups, and only the id orders them."""
    x = R.tied_vectors(150)
    _build_and_compare(tmp_path, "tied600", x, M_hnsw, 200)
    b = _restated[("tied600", M_hnsw, max(200, 2 * M_hnsw), 0)][0]
    assert len(np.unique(b.codes, axis=0)) <= 150


@pytest.mark.parametrize("n", [1, 2, 3, 5, 33, 65, 257])
def test_few_nodes(tmp_path, n):
    """Fewer candidates than deg, fewer than the heuristic's 64, a last partial batch (33, 65, 257: one node past a
    full batch). The host k-means accepts fewer training points than centroids, so n starts at 1; sample_rate = 1.0."""
    _build_and_compare(tmp_path, f"gauss{n}", R.gaussian_vectors(n, seed=n), 16, 200, sample_rate=1.0)


def test_work_queue_and_bitmap_reuse(tmp_path, monkeypatch):
    """Default knobs; DRM_BUILD_SLOTS=3 (three resident waves: each takes dozens of items per batch, one after the
    other on one bitmap slot, so a bit left set by one item would hide a node from the next); the same with
    DRM_BUILD_CLEAR_CAP=8 (every beam that visited more than 8 nodes ends in the full-bitmap clear). All three files
    are the restatement's, byte for byte the same."""
    x = R.gaussian_vectors(600)
    files = [_build_and_compare(tmp_path, "gauss600", x, 16, 64, tag="_default")]
    monkeypatch.setenv("DRM_BUILD_SLOTS", "3")
    files.append(_build_and_compare(tmp_path, "gauss600", x, 16, 64, tag="_slots3"))
    monkeypatch.setenv("DRM_BUILD_CLEAR_CAP", "8")
    files.append(_build_and_compare(tmp_path, "gauss600", x, 16, 64, tag="_slots3_cap8"))
    assert files[0] == files[1] == files[2]
    b = _restated[("gauss600", 16, 64, 0)][0]
    busiest = max(-(-count // 3) for _, count in b.batches)
    full_clears = sum(1 for nvis in b.visited.values() if nvis > 8)
    print(f"batches {[c for _, c in b.batches]}: with 3 slots the busiest wave takes >= {busiest} items; "
          f"with a clear list of 8, {full_clears} of {len(b.visited)} beams end in the full clear "
          f"(most nodes visited by one beam: {max(b.visited.values())})")
    assert busiest >= 24 and full_clears > len(b.visited) // 2 and max(b.visited.values()) <= 16384


def test_build_bounds_fail_loudly(tmp_path, monkeypatch):
    """The insertion kernel bounds its loops: with the beam's hop bound lowered to 1 (DRM_BUILD_HOP_BOUND), and with
    one resident wave allowed one work item (DRM_BUILD_SLOTS=1, DRM_BUILD_ITEM_BOUND=1), the kernels run to completion
    and the build returns DRM_ERR_INTERNAL, writing no file; the natural bounds (n hops, the batch's items) never
    trigger, and the build after the failed ones is the restatement's again."""
    from deepreadmapper_amd import synth
    from deepreadmapper_amd._native import DrmError
    x = R.gaussian_vectors(600)
    for knobs in ({"DRM_BUILD_HOP_BOUND": "1"}, {"DRM_BUILD_SLOTS": "1", "DRM_BUILD_ITEM_BOUND": "1"}):
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)
        path = str(tmp_path / "bounded.index")
        with pytest.raises(DrmError) as e:
            synth.build_index_gpu(x, path, M_hnsw=16, efc=64)
        assert e.value.code == -8 and "build state broken" in str(e.value), str(e.value)  # DRM_ERR_INTERNAL
        assert not os.path.exists(path)
        for k in knobs:
            monkeypatch.delenv(k)
    _build_and_compare(tmp_path, "gauss600", x, 16, 64, tag="_after")
