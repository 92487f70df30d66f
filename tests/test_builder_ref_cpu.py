"""The restatement of the GPU index build (tests/builder_ref.py) checked where no GPU is needed, so that a
disagreement in tests/test_gpu_builder_exact.py points at the kernel:

* its levels, offsets, entry point and PQ codes equal the host builder's file (same RNG streams, same encoder);
* its fast beam equals the literal one;
* the graphs it builds have the properties the algorithm implies (degrees, no self links, no duplicates, levels,
  order, every chosen link kept on both sides unless a closer one took its place, no link from nowhere);
* the neighbour heuristic, the greedy step and the beam give the results worked out by hand below.

The restated builds here take 0.2 to 0.5 s each on one core (the host builds that supply the centroids the same)."""
import numpy as np
import pytest

import builder_ref as R


def _host_file(tmp_path, x, M_hnsw, seed=0, sample_rate=0.5):
    """The host builder's file over x: the GPU builder trains the same PQ on the same sample, so its centroids are
    the ones the GPU file will hold (test_gpu_builder.py holds the two equal)."""
    from deepreadmapper_amd import synth
    from oracle import faiss_file
    path = str(tmp_path / f"host_{len(x)}_{M_hnsw}_{seed}.index")
    synth.build_index(x, path, M_hnsw=M_hnsw, efc=8, sample_rate=sample_rate, nthreads=1, seed=seed)
    return faiss_file.read(path)


@pytest.mark.parametrize("n,M_hnsw,seed", [(1, 16, 0), (2, 16, 0), (33, 16, 3), (600, 16, 0), (600, 2, 0), (600, 4, 7),
                                           (1000, 32, 1), (777, 12, 123456789)])
def test_levels_order_and_codes_match_host_builder(tmp_path, n, M_hnsw, seed):
    x = R.gaussian_vectors(n, seed=n + seed)
    fx = _host_file(tmp_path, x, M_hnsw, seed, sample_rate=1.0 if n < 512 else 0.5)
    lev = R.assign_levels(n, M_hnsw, seed)
    assert np.array_equal(lev + 1, fx.levels)
    assert np.array_equal(R.list_offsets(lev, M_hnsw), fx.offsets)
    order = R.insertion_order(lev, seed)
    assert sorted(order) == list(range(n))
    assert order[0] == fx.entry_point and lev[order[0]] == fx.max_level  # the host builder's first insertion
    assert len(R.assign_probas(M_hnsw)) + 1 == len(fx.cum_nneighbor_per_level)
    # codes: the first minimum of the float32 sequential sub-distance
    lut = R.distance_tables(x, fx.centroids)
    assert np.array_equal(R.codes_from_tables(lut).reshape(-1), fx.codes)
    # and that table is the oracle's, entry for entry
    from oracle import oracle as O
    for v in (0, n // 2, n - 1):
        assert np.array_equal(lut[v].view(np.uint32), O.pq_distance_table(fx, x[v]).view(np.uint32))


def test_mt19937_stream():
    """RandomState's raw stream is std::mt19937's: the standard's check value (10000th draw of the default seed)
    and the first three."""
    raw = np.random.RandomState(5489)._bit_generator.random_raw(10000)
    assert raw[:3].tolist() == [3499211612, 581869302, 3890346734] and int(raw[-1]) == 4123659995


def test_distance_orders():
    """The sums are sequential float32, not pairwise and not float64: against a scalar loop on one entry each."""
    rng = np.random.default_rng(3)
    x = rng.normal(size=(3, 128)).astype(np.float32)
    cen = rng.normal(size=(8, 256, 16)).astype(np.float32)
    lut = R.distance_tables(x, cen)
    sdc = R.sdc_table(cen)
    codes = R.codes_from_tables(lut)
    A, S = R.adc_matrix(lut, codes), R.sd_matrix(sdc, codes)
    f = np.float32
    for v, m, c in ((0, 0, 0), (1, 7, 255), (2, 3, 100)):
        acc = f(0)
        for t in range(16):
            df = f(x[v, m * 16 + t] - cen[m, c, t])
            acc = f(acc + f(df * df))
        assert lut[v, m, c] == acc
        acc = f(0)
        for t in range(16):
            df = f(cen[m, c, t] - cen[m, v, t])
            acc = f(acc + f(df * df))
        assert sdc[m, c, v] == acc == sdc[m, v, c]
    for u, v in ((0, 1), (2, 0), (1, 1)):
        a = s = f(0)
        for m in range(8):
            a = f(a + lut[u, m, codes[v, m]])
            s = f(s + sdc[m, codes[u, m], codes[v, m]])
        assert A[u, v] == a and S[u, v] == s


def _pos2(points):
    """Squared distances between 2-D points with coordinates in halves: exact in float."""
    return lambda a, b: (points[a][0] - points[b][0]) ** 2 + (points[a][1] - points[b][1]) ** 2


def test_heuristic_by_hand():
    """Ten nodes in the plane, the new node 0 at the origin, d and sd both the squared distance. Candidates in
    (d, id) order, with deg = 4:
      1 (1, 0)     d 1     nothing kept yet                                   -> kept
      2 (.5, 1)    d 1.25  sd(1, 2) = .25 + 1 = 1.25, not < 1.25 (strict)      -> kept
      3 (1.5, 0)   d 2.25  sd(1, 3) = .25 < 2.25                               -> dropped
      4 (-1.5, 0)  d 2.25  (after 3: equal d, higher id) sd(1, 4) = 6.25,
                           sd(2, 4) = 4 + 1 = 5                                -> kept
      5 (0, 2)     d 4     sd(1, 5) = 5, sd(2, 5) = .25 + 1 = 1.25 < 4         -> dropped
      6 (0, -2)    d 4     sd(1, 6) = 5, sd(2, 6) = .25 + 9, sd(4, 6) = 6.25   -> kept, the 4th: stop at deg = 4
      7 (0, -2.5)  d 6.25  sd(6, 7) = .25 < 6.25                               -> dropped when deg lets it be reached
      8 (-3, 3)    d 18    sd(2, 8) = 12.25 + 4 = 16.25 < 18                   -> dropped
      9 (5, 0)     d 25    sd(1, 9) = 16 < 25                                  -> dropped
    3 does not shield anyone: a dropped candidate is not compared against."""
    pts = {0: (0, 0), 1: (1, 0), 2: (.5, 1), 3: (1.5, 0), 4: (-1.5, 0), 5: (0, 2), 6: (0, -2), 7: (0, -2.5),
           8: (-3, 3), 9: (5, 0)}
    sd = _pos2(pts)
    cand = sorted((sd(0, c), c) for c in range(1, 10))
    assert [c for _, c in cand] == [1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert R.heuristic(cand, sd, 4) == [(1, 1), (1.25, 2), (2.25, 4), (4, 6)]
    assert R.heuristic(cand, sd, 8) == [(1, 1), (1.25, 2), (2.25, 4), (4, 6)]  # fewer than deg: the rest are dropped
    assert [c for _, c in R.heuristic(cand, sd, 3)] == [1, 2, 4]
    assert [c for _, c in R.heuristic(cand, sd, 1)] == [1]
    # with 6 out of the way 7 is kept: sd(1, 7) = 1 + 6.25, sd(2, 7) = .25 + 12.25, sd(4, 7) = 2.25 + 6.25 = 8.5
    assert [c for _, c in R.heuristic([e for e in cand if e[1] != 6], sd, 4)] == [1, 2, 4, 7]
    # only the 64 nearest are looked at: 70 candidates none of which shields another
    far = [(float(i + 1), i) for i in range(70)]
    assert R.heuristic(far, lambda k, c: 1e9, 100) == far[:64]


def test_descend_and_beam_by_hand():
    """A path 0 - 1 - 2 - 3 - 4 with a chord 1 - 5; distances of the new node: 9, 7, 4, 4, 6, 4 for nodes 0..5.
    Greedy from 0: to 1 (7 < 9); 1's links 0, 2, 5 have minimum 4 at both 2 and 5 -> the lower id 2; 2's links 1, 3
    have minimum 4 at 3, not < 4 -> stay at 2.
    Beam from 0, ef = 3: W = [0]; expand 0 -> [1, 0]; expand 1 -> visits 2, 5: [2, 5, 1] (0 falls off, expanded);
    expand 2 (4, 2) -> visits 3: [2, 3, 5] ((4, 3) before (4, 5); 1 falls off); expand 3 -> visits 4 at 6: no room,
    yet visited; expand 5 -> nothing new. Six nodes visited."""
    links = {0: [1], 1: [0, 2, 5], 2: [1, 3], 3: [2, 4], 4: [3], 5: [1]}
    dist = [9.0, 7.0, 4.0, 4.0, 6.0, 4.0]
    assert R.descend(dist, links.__getitem__, 0, 1) == 2
    for fn in (R.beam, R.beam_literal):
        assert fn(dist, links.__getitem__, 0, 3) == ([(4.0, 2), (4.0, 3), (4.0, 5)], 6)
        assert fn(dist, links.__getitem__, 0, 2) == ([(4.0, 2), (4.0, 3)], 6)  # 5 falls off W before its turn
        assert fn(dist, links.__getitem__, 4, 8)[0] == sorted((d, v) for v, d in enumerate(dist))


CASES = {
    "gauss_M16_ef64": lambda: (R.gaussian_vectors(600), 16, 64),
    "gauss_M16_ef10": lambda: (R.gaussian_vectors(600), 16, 10),
    "gauss_M2": lambda: (R.gaussian_vectors(600), 2, 40),
    "gauss_M32": lambda: (R.gaussian_vectors(600), 32, 40),
    "tied_M4": lambda: (R.tied_vectors(150), 4, 200),
    "tied_M16": lambda: (R.tied_vectors(150), 16, 200),
    "few_65": lambda: (R.gaussian_vectors(65), 16, 200),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_restated_graph_properties(tmp_path, case):
    x, M, efc = CASES[case]()
    n = len(x)
    fx = _host_file(tmp_path, x, M, sample_rate=1.0 if n < 512 else 0.5)
    b = R.build(x, fx.centroids, M, efc)
    assert np.array_equal(b.codes.reshape(-1), fx.codes) and np.array_equal(b.levels, fx.levels)
    assert b.entry_point == fx.entry_point and b.max_level == fx.max_level
    assert sum(c for _, c in b.batches) == n - 1 and all(c <= s for s, c in b.batches)
    if case.startswith("tied"):  # the ties are there: whole groups at one distance
        assert len(np.unique(b.codes, axis=0)) <= n // 4
    for v in range(n):
        assert len(b.lists[v]) == b.levels[v]
        for l, L in enumerate(b.lists[v]):
            deg = 2 * M if l == 0 else M
            ids = [w for _, w in L]
            assert len(L) <= deg and v not in ids and len(set(ids)) == len(ids)
            assert all(b.levels[w] > l for w in ids)
            assert L == sorted(L)
            assert R.file_list(b, v, l, M) == ids + [-1] * (deg - len(ids))  # the faiss layout of the same lists
            if v != b.entry_point or n == 1:
                assert (len(L) > 0) == (n > 1)
            for d, w in L:  # no link from nowhere: v chose w, or w chose v, at this distance
                assert (d, w) in b.forward.get((v, l), ()) or (d, v) in b.forward.get((w, l), ())
    for (u, l), kept in b.forward.items():
        deg = 2 * M if l == 0 else M
        assert 1 <= len(kept) <= deg and kept == sorted(kept)
        assert b.visited[(u, l)] >= len(kept)
        for d, v in kept:
            mine, theirs = b.lists[u][l], b.lists[v][l]
            # kept on both sides unless the list is full of closer entries
            assert (d, v) in mine or (len(mine) == deg and mine[-1] < (d, v))
            assert (d, u) in theirs or (len(theirs) == deg and theirs[-1] < (d, u))
    # the literal beam builds the same graph
    if n <= 600 and efc <= 64:
        lit = R.build(x, fx.centroids, M, efc, beam_fn=R.beam_literal)
        assert np.array_equal(lit.neighbors, b.neighbors) and lit.visited == b.visited
