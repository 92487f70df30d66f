"""The lean search kernel's heap with popped slots that tie (hnsw_pq_fast.hip, struct Heap): a heap slot's key holds
its node id once, live (id | 2^31) or popped (id), and faiss's order -- where every popped slot has id -1, so two
popped slots of one distance are equal -- is kept by comparing through N(w) = max(w, 2^31 - 1) wherever both sides
can be popped. A kernel that ordered popped slots by their node ids would take other sift paths, leave other slots
for pop_min's tie choice (the highest tied slot) and so walk the graph in another order: ids, nhops and ndis show it.

Indices (tests/pq_graphs.py, PQ 8 x 8, d = 128): integer centroids with tie codes of n_values 1 and 2 (two and four
distinct distances per query at most, all exact), and Gaussian centroids on a random graph with a repeated link;
M_hnsw 16 and 4; ntotal 100 (the ef = 128 heap never fills), 128, 129, 130 (the first replaces), 1500.
(k, ef): (128, 128) the log result set with replace128; (10, 128) and (64, 128) the register result set;
(64, 64) and (100, 100) the general pop / push. Each against the oracle as tests/test_gpu_pq_paths.py compares (ids,
distances at 0 ulp, nhops; ndis with exact statistics), in the default and the exact-statistics mode.

That the fixtures reach the situation is asserted on the CPU first, from tests/faiss_literal.py alone, with cmp2_max
counted inside MinimaxHeap's heap_pop: each tie family (n_values x M_hnsw) must show compares of two popped slots
(both ids -1) of equal distance. The Gaussian family cannot: its distances are sums of eight Gaussian LUT entries
under uniform codes, so two nodes at one distance would need equal codes (1500^2 / 2 pairs against 2^64 codes); for
it the count required is that of compares of two popped slots of any distance, the case where the raw keys' low
words differ from faiss's and only the high words may decide."""
import numpy as np
import pytest

import faiss_literal as FL
import pq_graphs as P
from oracle import oracle as O

D_, M_PQ, NBITS = 128, 8, 8
NTOTALS = [100, 128, 129, 130, 1500]
KEF = [(128, 128), (10, 128), (64, 128), (64, 64), (100, 100)]
KINDS = ["tie1", "tie2", "rand"]
M_HNSWS = [16, 4]
NQ = 12
# the generator seed per family (default 0): chosen on the CPU so that the literal search alone reaches the counts
# that _reach requires (seeds 0, 1 and 3 of tie1 / M_hnsw 16 meet no tie of two popped slots at ef = 128)
SEEDS = {("tie1", 16): 2}


def _make(directory, kind, M_hnsw, n):
    seed = SEEDS.get((kind, M_hnsw), 0)
    name = f"{kind}_m{M_hnsw}_n{n}"
    if kind == "rand":
        return P.make_random(directory, name, D_, M_PQ, NBITS, M_hnsw, n, dup=True, seed=seed, nq=NQ)
    n_values = {"tie1": 1, "tie2": 2}[kind]
    rng = np.random.default_rng([seed, n_values, M_hnsw, n, 11])
    # the graph and the queries as make_tie draws them
    return P._fixture(str(directory / f"{name}.index"), D_, M_PQ, NBITS, M_hnsw, P.int_centroids(D_, M_PQ, NBITS),
                      P.tie_codes(rng, n, M_PQ, NBITS, n_values=n_values),
                      P.random_graph(n, M_hnsw, 2, rng, 0.2, True), P.int_queries(rng, NQ, D_, M_PQ))


@pytest.fixture(scope="module")
def fixtures(tmp_path_factory):
    d = tmp_path_factory.mktemp("popped_ties")
    made = {}

    def get(kind, M_hnsw, n):
        key = (kind, M_hnsw, n)
        if key not in made:
            made[key] = _make(d, kind, M_hnsw, n)
        return made[key]
    return get


def _count_popped_compares(f, ef, queries):
    """(compares of two different popped slots with equal distances, compares of two popped slots) inside
    MinimaxHeap's heap_pop, over faiss_literal's search of the given queries at k = ef."""
    counts = {"equal": 0, "any": 0, "on": False}
    cmp2, push = FL.cmp2_max, FL.MinimaxHeap.push

    def counted(a1, b1, a2, b2):
        if counts["on"] and a2 == -1 and b2 == -1:
            counts["any"] += 1
            # heap_pop also compares slot k with itself when it is the last child on the path (one object twice):
            # no tie between two slots
            counts["equal"] += int(a1 == b1 and a1 is not b1)
        return cmp2(a1, b1, a2, b2)

    def counted_push(self, i, v):  # a full MinimaxHeap's push: heap_pop, then heap_push of a live id
        counts["on"] = True
        try:
            return push(self, i, v)
        finally:
            counts["on"] = False

    FL.cmp2_max, FL.MinimaxHeap.push = counted, counted_push
    try:
        ix = FL.LiteralIndex(f["fx"])
        for x in queries:
            FL.search_one(ix, x, ef, ef)
    finally:
        FL.cmp2_max, FL.MinimaxHeap.push = cmp2, push
    return counts["equal"], counts["any"]


_REACH = {}


def _reach(fixtures, kind, M_hnsw):
    """Asserts, once per family, that the literal faiss search alone meets popped ties on the family's fixtures: at
    ef = 128 on the 1500-node index (replace128) and at ef = 64 on the 130-node one (the general pop)."""
    key = (kind, M_hnsw)
    if key not in _REACH:
        out = []
        for n, ef in [(1500, 128), (130, 64)]:
            f = fixtures(kind, M_hnsw, n)
            out.append(_count_popped_compares(f, ef, f["q"]))
        _REACH[key] = out
    for (equal, anyd), what in zip(_REACH[key], ["n=1500 ef=128", "n=130 ef=64"]):
        got = anyd if kind == "rand" else equal
        assert got >= 1, f"{kind} M_hnsw={M_hnsw} {what}: the literal search compares no two popped slots " \
                         f"{'at all' if kind == 'rand' else 'of equal distance'} ({equal} equal, {anyd} in all)"
    return _REACH[key]


@pytest.mark.parametrize("M_hnsw", M_HNSWS)
@pytest.mark.parametrize("kind", KINDS)
def test_fixture_families_reach_popped_ties(fixtures, kind, M_hnsw):
    _reach(fixtures, kind, M_hnsw)


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


@pytest.mark.gpu
@pytest.mark.parametrize("n", NTOTALS)
@pytest.mark.parametrize("M_hnsw", M_HNSWS)
@pytest.mark.parametrize("kind", KINDS)
def test_popped_ties_against_oracle(fixtures, kind, M_hnsw, n):
    from deepreadmapper_amd import read_index
    _reach(fixtures, kind, M_hnsw)
    f = fixtures(kind, M_hnsw, n)
    ix = read_index(f["index"])
    try:
        for k, ef in KEF:
            ix.set_exact_stats(False)
            _check(ix, f, k, ef, ndis=False)
            ix.set_exact_stats(True)
            _check(ix, f, k, ef, ndis=True)
    finally:
        ix.free()
