"""The lean search kernel's sift-ups (hnsw_pq_fast.hip): Heap::push_fill while the ef = 128 heap fills (the lane-mask
form: every climb depth in one straight line) and Heap::climb128 after every pop of the full heap (on the scalar unit:
the pushed value climbs level by level -- the father read with v_readlane, one scalar compare, the father written one
level down with v_writelane -- and stops at the first father not below it). A climb that stopped one level early or
late, took the wrong half of a lane (L / R) or the wrong lane, or mishandled the root (lane 63's R) leaves another
heap: pop_min's tie choice (the highest tied slot), the evictions and so ids, nhops and ndis show it.

Indices (tests/pq_graphs.py, PQ 8 x 8, d = 128), M_hnsw 4 and 16, ntotal 1, 2, 3, 100 (the heap never fills), 127,
128, 129, 130 (the first replaces), 1500:
  rise  chain graph from node 0, integer centroids, the distance strictly rising with the node id: every push while
        the heap fills is the new maximum and climbs to the root (depths 1 .. 6 and, at k = 128, 7);
  fall  the same with the distance strictly falling: no push moves, filling or full (the early exit at depth 0);
  tie   integer centroids with eight distinct distances at most on a random graph: a pushed value meets fathers of its
        own distance, and the node id decides whether it passes them;
  rand  Gaussian centroids, uniform codes, a random graph.
(k, ef): (128, 128) the log result set, (10, 128) and (64, 128) the register result set; (64, 64) on one index size
per family for the general push / pop, which shares nothing with the ef = 128 sift-ups. Each against the oracle as
tests/test_gpu_heap_popped_ties.py compares (ids, distances at 0 ulp, nhops; ndis with exact statistics), in the
default and the exact-statistics mode.

That the fixtures reach the situations is asserted on the CPU first, from tests/faiss_literal.py alone, by counting
inside heap_push (the compares that let the value pass a father = the climb's depth) over the literal search of the
1500-node index at k = ef = 128: a fill push is one into a heap that is not yet full (k < 128 below: the position it
enters at is at most 127, so its climb has at most 6 levels and ends at the root when depth = bitlen(k) - 1), a
full-heap push the heap_push(128) after MinimaxHeap::push's heap_pop, with h in 0 .. 7 (7: the value is the new root).
The generator seeds of the rand family are chosen so that the literal search shows every depth 0 .. 6 and the climb
to the root among the fill pushes and every h in 0 .. 7 among the full-heap ones."""
from collections import Counter

import numpy as np
import pytest

import faiss_literal as FL
import pq_graphs as P
from oracle import oracle as O

D_, M_PQ, NBITS = 128, 8, 8
EF = 128
NTOTALS = [1, 2, 3, 100, 127, 128, 129, 130, 1500]
KEF = [(128, 128), (10, 128), (64, 128)]
KINDS = ["rise", "fall", "tie", "rand"]
M_HNSWS = [16, 4]
NQ = 12
# the generator seed per family (default 0), chosen on the CPU so that the literal search alone meets what _reach
# requires of the family
SEEDS = {}
# chain families: (x_0, x_16) of the queries. Node of rank r has code (r mod 256, r / 256, 0, ...) under centroids
# (c, 0, ...) and (256 c, 0, ...), so its distance is (r mod 256 - x_0)^2 + (256 (r / 256) - x_16)^2: with x_0 = -t
# and x_16 = -256 m it rises strictly with r whenever t < 257 m + 1 (the step from r = 256 j + 255 to 256 (j + 1)
# gains 256^2 + 512 * 256 (j + m) and loses 255^2 + 510 t), and every term is an integer below 2^24
CHAIN_QUERIES = [(0, 0), (-1, 0), (0, -256), (-100, -256), (-200, -512), (-3, -768)]


def _chain(directory, name, M_hnsw, n, rising):
    r = np.arange(n) if rising else n - 1 - np.arange(n)
    codes = np.zeros((n, M_PQ), dtype=np.int64)
    codes[:, 0], codes[:, 1] = r % 256, r // 256
    cen = np.zeros((M_PQ, 1 << NBITS, D_ // M_PQ), dtype=np.float32)
    cen[0, :, 0] = np.arange(256, dtype=np.float32)
    cen[1, :, 0] = 256.0 * np.arange(256, dtype=np.float32)
    q = np.zeros((len(CHAIN_QUERIES), D_), dtype=np.float32)
    q[:, 0] = [a for a, _ in CHAIN_QUERIES]
    q[:, D_ // M_PQ] = [b for _, b in CHAIN_QUERIES]
    return P._fixture(str(directory / f"{name}.index"), D_, M_PQ, NBITS, M_hnsw, cen, codes,
                      P.chain_graph(n, M_hnsw), q)


def _make(directory, kind, M_hnsw, n):
    seed = SEEDS.get((kind, M_hnsw), 0)
    name = f"{kind}_m{M_hnsw}_n{n}"
    dup = n >= 100  # a repeated link needs a row with two links
    if kind in ("rise", "fall"):
        return _chain(directory, name, M_hnsw, n, kind == "rise")
    if kind == "rand":
        return P.make_random(directory, name, D_, M_PQ, NBITS, M_hnsw, n, dup=dup, seed=seed, nq=NQ)
    rng = np.random.default_rng([seed, M_hnsw, n, 13])
    return P._fixture(str(directory / f"{name}.index"), D_, M_PQ, NBITS, M_hnsw, P.int_centroids(D_, M_PQ, NBITS),
                      P.tie_codes(rng, n, M_PQ, NBITS, n_values=4), P.random_graph(n, M_hnsw, 2, rng, 0.2, dup),
                      P.int_queries(rng, NQ, D_, M_PQ))


@pytest.fixture(scope="module")
def fixtures(tmp_path_factory):
    d = tmp_path_factory.mktemp("heap_siftup")
    made = {}

    def get(kind, M_hnsw, n):
        key = (kind, M_hnsw, n)
        if key not in made:
            made[key] = _make(d, kind, M_hnsw, n)
        return made[key]
    return get


def _count_climbs(f, queries):
    """Over faiss_literal's search of the queries at k = ef = 128, counted inside heap_push: `fill` and `full`, the
    climb depths (the compares that let the value pass a father) of the pushes into a heap not yet full (positions
    k < 128) and of the full heap's pushes; `root`, the fill pushes that ended at the root; and `ties`, keyed by
    (full, passed): the compares of the value with a father of its own distance, which the node id decides."""
    out = {"fill": Counter(), "full": Counter(), "root": 0, "ties": Counter()}
    state = {"full": False, "depth": None}
    cmp2, hpush, mpush = FL.cmp2_max, FL.heap_push, FL.MinimaxHeap.push

    def counted_cmp2(a1, b1, a2, b2):
        r = cmp2(a1, b1, a2, b2)
        if state["depth"] is not None:
            state["depth"] += int(r)
            if a1 == b1:
                out["ties"][(state["full"], bool(r))] += 1
        return r

    def counted_heap_push(k, val, ids, v, idv):
        state["depth"] = 0
        try:
            hpush(k, val, ids, v, idv)
        finally:
            depth, state["depth"] = state["depth"], None
        if state["full"]:
            assert k == EF
            out["full"][depth] += 1
        elif k < EF:
            out["fill"][depth] += 1
            out["root"] += int(k > 1 and depth == k.bit_length() - 1)

    def counted_push(self, i, v):  # MinimaxHeap::push: on a full heap heap_pop, then heap_push at k = n
        state["full"] = self.k == self.n
        try:
            return mpush(self, i, v)
        finally:
            state["full"] = False

    FL.cmp2_max, FL.heap_push, FL.MinimaxHeap.push = counted_cmp2, counted_heap_push, counted_push
    try:
        ix = FL.LiteralIndex(f["fx"])
        for x in queries:
            FL.search_one(ix, x, EF, EF)
    finally:
        FL.cmp2_max, FL.heap_push, FL.MinimaxHeap.push = cmp2, hpush, mpush
    return out


_REACH = {}


def _reach(fixtures, kind, M_hnsw):
    """Asserts, once per family, what the literal faiss search alone meets on the family's 1500-node index."""
    key = (kind, M_hnsw)
    if key not in _REACH:
        f = fixtures(kind, M_hnsw, 1500)
        _REACH[key] = _count_climbs(f, f["q"])
    c = _REACH[key]
    fill, full, what = c["fill"], c["full"], f"{kind} M_hnsw={M_hnsw}: fill {dict(c['fill'])} root {c['root']} " \
                                             f"full {dict(c['full'])} ties {dict(c['ties'])}"
    nfill = sum(fill.values())
    assert nfill >= EF - 1, what  # a heap was filled
    assert kind == "rise" or sum(full.values()) >= 1, what
    if kind == "rise":  # every fill push climbs to the root; the full heap takes nothing (all beyond its root)
        assert c["root"] == nfill - fill[0] and set(fill) >= set(range(1, 7)), what
        assert fill[0] == len(CHAIN_QUERIES), what  # the entry point's own push (k = 1)
    elif kind == "fall":  # nothing moves
        assert set(fill) == {0} and set(full) == {0}, what
    elif kind == "tie":  # equal distances against a father, passed and not passed, filling and full
        assert all(c["ties"][(fl, ps)] >= 1 for fl in (False, True) for ps in (False, True)), what
    else:
        assert set(fill) >= set(range(0, 7)) and c["root"] >= 1 and set(full) >= set(range(0, 8)), what
    return c


@pytest.mark.parametrize("M_hnsw", M_HNSWS)
@pytest.mark.parametrize("kind", KINDS)
def test_fixture_families_reach_the_climbs(fixtures, kind, M_hnsw):
    _reach(fixtures, kind, M_hnsw)


@pytest.mark.parametrize("M_hnsw", M_HNSWS)
@pytest.mark.parametrize("rising", [True, False])
def test_chain_distances_are_strictly_monotone(fixtures, rising, M_hnsw):
    """The chain families' premise, from the indices before packing (adc_reference): distances to every query
    strictly rising (falling) with the node id, and exact integers."""
    f = fixtures("rise" if rising else "fall", M_hnsw, 1500)
    d = P.adc_reference(f["centroids"], f["codes_idx"], f["q"])
    step = np.diff(d.astype(np.float64), axis=1)
    assert (step > 0).all() if rising else (step < 0).all()
    assert np.array_equal(d, np.rint(d)) and d.max() < 2 ** 24


def test_union_of_families_covers_every_depth(fixtures):
    """All the families together, per M_hnsw: every fill depth 0 .. 6, the climb to the root, every full-heap h."""
    for M_hnsw in M_HNSWS:
        fill, full, root = Counter(), Counter(), 0
        for kind in KINDS:
            c = _reach(fixtures, kind, M_hnsw)
            fill, full, root = fill + c["fill"], full + c["full"], root + c["root"]
        assert set(fill) >= set(range(0, 7)) and set(full) >= set(range(0, 8)) and root >= 1, (M_hnsw, fill, full)


_ORACLE = {}


def _oracle(f, k, ef):
    key = (f["index"], k, ef)
    if key not in _ORACLE:
        r = O.hnswpq_search(f["fx"], f["q"], k, ef)
        for a in r:
            a.setflags(write=False)
        _ORACLE[key] = r
    return _ORACLE[key]


def _check(ix, f, k, ef, ndis):
    fx, q = f["fx"], f["q"]
    D, I, st = ix.search(q, k, ef)
    Do, Io, nd, nh = _oracle(f, k, ef)
    what = f"n={fx.ntotal} k={k} ef={ef} exact_stats={ndis}"
    bad = np.flatnonzero((I != Io).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[:8]}"
    assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)), what  # 0 ulp
    assert st.nhops == int(nh.sum()), what
    if ndis:
        assert st.ndis == int(nd.sum()), what
    assert ix.search_errors() == 0, what


def _run(f, kefs):
    from deepreadmapper_amd import read_index
    ix = read_index(f["index"])
    try:
        for k, ef in kefs:
            ix.set_exact_stats(False)
            _check(ix, f, k, ef, ndis=False)
            ix.set_exact_stats(True)
            _check(ix, f, k, ef, ndis=True)
    finally:
        ix.free()


@pytest.mark.gpu
@pytest.mark.parametrize("n", NTOTALS)
@pytest.mark.parametrize("M_hnsw", M_HNSWS)
@pytest.mark.parametrize("kind", KINDS)
def test_siftup_against_oracle(fixtures, kind, M_hnsw, n):
    _reach(fixtures, kind, M_hnsw)
    _run(fixtures(kind, M_hnsw, n), KEF)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_general_push_pop_untouched(fixtures, kind):
    """(k, ef) = (64, 64): Heap::push / Heap::pop, on an index where the 64-slot heap fills and replaces."""
    _run(fixtures(kind, 16, 130), [(64, 64)])
