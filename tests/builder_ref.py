"""The GPU index build (deepreadmapper_amd/csrc/builder_gpu.hip) restated in numpy and plain Python, from the
algorithm in that file's header comment: tuples (distance, id) in Python lists, sets for the visited and expanded
marks, no packed keys, no registers, no batching of waves and no code shared with the kernel.

The build is a pure function of (x, centroids, M_hnsw, efConstruction, seed):
  * distances are float32 sums in a fixed order (distance_tables, adc_matrix, sdc_table, sd_matrix below), every
    comparison is on the pair (distance, id);
  * levels and the insertion order come from two std::mt19937 streams (RandomState's random_raw is that stream);
  * batch b holds order[2^b, 2^(b+1)); a batch member sees only the graph as it stood before its batch, so the members
    are independent of one another; the reverse links of a batch are added after it, each list keeping its `deg`
    smallest (distance, id), which does not depend on the order they arrive in;
  * the file holds every list sorted by (distance, id).
So `build` predicts the file of drm_build_hnswpq_device link for link (tests/test_gpu_builder_exact.py); the
restatement itself is checked without a GPU in tests/test_builder_ref_cpu.py.

Cost of `build` on one CPU core (measured; the distance matrices are numpy, the graph walk is Python):
    C1 windows   n = 1702  M = 16  efConstruction = 200    1.9 s
    Gaussian     n =  600  M = 16  efConstruction = 10 ... 300    0.3 to 0.5 s
    Gaussian     n =  600  M =  2 / 4 / 12 / 32, efC = 40  0.2 / 0.2 / 0.2 / 0.3 s
    tied rows    n =  600  M = 4 / 16  efConstruction = 200    0.5 s
    n <= 257                                               under 0.1 s
"""
import bisect
import heapq
import math

import numpy as np

MAX_BATCH = 1 << 21   # nodes of one batch at the most
EF_CAP = 256          # the beam is at most this wide
HEURISTIC_WIDTH = 64  # the neighbour heuristic looks at this many nearest candidates
KSUB, DSUB, M_PQ = 256, 16, 8


# ------------------------------------------------------------------------------------------ levels and order
def assign_probas(M):
    """HNSW::set_default_probas(M, 1 / log(M)): the probability of each level."""
    mult = 1.0 / math.log(M)
    out = []
    level = 0
    while True:
        p = math.exp(-level / mult) * (1 - math.exp(-1 / mult))
        if p < 1e-9:
            return out
        out.append(p)
        level += 1


def assign_levels(n, M, seed):
    """Level of each node, 0 = lowest (the file stores level + 1): std::mt19937(12345 + seed), one draw per node,
    f = raw / 4294967295.0 walked down the level probabilities."""
    probas = assign_probas(M)
    raw = np.random.RandomState((12345 + seed) & 0xFFFFFFFF)._bit_generator.random_raw(n) if n else []
    lev = np.zeros(n, dtype=np.int64)
    for i in range(n):
        f = int(raw[i]) / 4294967295.0
        level = len(probas) - 1
        for l, p in enumerate(probas):
            if f < p:
                level = l
                break
            f -= p
        lev[i] = level
    return lev


def insertion_order(lev, seed):
    """Levels descending; each level's nodes (ascending ids) shuffled by std::mt19937(789 + seed): for j < size - 1,
    swap bk[j] with bk[j + raw % (size - j)]. One stream runs through all the levels."""
    bits = np.random.RandomState((789 + seed) & 0xFFFFFFFF)._bit_generator
    out = []
    for level in range(int(lev.max()), -1, -1):
        bk = [int(i) for i in np.nonzero(lev == level)[0]]
        for j in range(len(bk) - 1):
            r = int(bits.random_raw()) % (len(bk) - j)
            bk[j], bk[j + r] = bk[j + r], bk[j]
        out += bk
    return out


def list_offsets(lev, M):
    """faiss's offsets: node i owns 2M slots for level 0 and M for each level above, offsets[i] is where they start."""
    per_node = 2 * M + np.asarray(lev, dtype=np.int64) * M
    return np.concatenate([[0], np.cumsum(per_node)]).astype(np.uint64)


# ------------------------------------------------------------------------------------------ distances
def distance_tables(x, centroids):
    """LUT[v][m][c] = sum_t (x[v][16 m + t] - cen[m][c][t])^2: float32, t = 0..15 in order from 0, no FMA."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, M_PQ, 1, DSUB)
    cen = np.asarray(centroids, dtype=np.float32).reshape(1, M_PQ, KSUB, DSUB)
    acc = np.zeros((x.shape[0], M_PQ, KSUB), dtype=np.float32)
    for t in range(DSUB):
        df = x[..., t] - cen[..., t]
        acc = acc + df * df
    return acc


def codes_from_tables(lut):
    """PQ code of each vector: per sub-quantizer the first centroid at the minimum sub-distance."""
    return np.argmin(lut, axis=2).astype(np.uint8)


def adc_matrix(lut, codes):
    """A[u][v] = d(u, v) = sum_m LUT[u][m][code[v][m]], float32, m = 0..7 in order: the distance the node u being
    inserted sees to v. Not symmetric: u's own vector against v's code."""
    n = len(codes)
    a = np.zeros((n, n), dtype=np.float32)
    for m in range(M_PQ):
        a = a + lut[:, m, :][:, codes[:, m]]
    return a


def sdc_table(centroids):
    """sdc[m][a][b] = sum_t (cen[m][a][t] - cen[m][b][t])^2, float32 in order."""
    cen = np.asarray(centroids, dtype=np.float32).reshape(M_PQ, KSUB, DSUB)
    acc = np.zeros((M_PQ, KSUB, KSUB), dtype=np.float32)
    for t in range(DSUB):
        df = cen[:, :, None, t] - cen[:, None, :, t]
        acc = acc + df * df
    return acc


def sd_matrix(sdc, codes):
    """S[k][c] = sd(k, c) = sum_m sdc[m][code_k[m]][code_c[m]], float32, m = 0..7 in order: code against code."""
    n = len(codes)
    s = np.zeros((n, n), dtype=np.float32)
    for m in range(M_PQ):
        cm = codes[:, m].astype(np.int64)
        s = s + sdc[m][cm[:, None], cm[None, :]]
    return s


# ------------------------------------------------------------------------------------------ one insertion
def descend(dist, links, cur, level):
    """Greedy step on one level: while some link of `cur` is nearer than `cur`, move to the lowest id among the
    nearest links. dist[v] is the new node's distance to v, links(v) the ids v links to on this level."""
    while True:
        ids = links(cur)
        if not ids:
            return cur
        nearest = min(dist[v] for v in ids)
        if nearest >= dist[cur]:
            return cur
        cur = min(v for v in ids if dist[v] == nearest)


def beam_literal(dist, links, start, ef):
    """The beam as the header comment says it, nothing clever: W is the sorted list of the ef nearest (d, id) seen.
    Take W's first entry not yet expanded, mark it, visit those of its links not visited before (they stay visited
    even when W has no room for them), merge, cut to ef; until every entry of W is expanded.
    Returns (W, number of nodes visited)."""
    W = [(dist[start], start)]
    visited = {start}
    expanded = set()
    while True:
        first = next((e for e in W if e[1] not in expanded), None)
        if first is None:
            return W, len(visited)
        expanded.add(first[1])
        fresh = [w for w in links(first[1]) if w not in visited]
        visited.update(fresh)
        W = sorted(W + [(dist[w], w) for w in fresh])[:ef]


def beam(dist, links, start, ef):
    """beam_literal without the rescans (test_builder_ref_cpu.py holds the two equal): the unexpanded entries wait
    in a heap. W's last entry only ever gets smaller once W is full, so an entry that fell off W is one greater than
    W's last, and it never comes back: it was visited."""
    W = [(dist[start], start)]
    visited = {start}
    waiting = [W[0]]
    while waiting:
        e = heapq.heappop(waiting)
        if len(W) == ef and e > W[-1]:
            continue  # fell off W before its turn
        for w in links(e[1]):
            if w in visited:
                continue
            visited.add(w)
            c = (dist[w], w)
            if len(W) == ef:
                if c > W[-1]:
                    continue
                W.pop()
            bisect.insort(W, c)
            heapq.heappush(waiting, c)
    return W, len(visited)


def heuristic(cand, sd, deg):
    """The neighbour heuristic over the HEURISTIC_WIDTH nearest candidates `cand` (sorted (d, id)): c is kept unless
    an already kept k has sd(k, c) < d(u, c), strictly; stop at deg kept. Returns the kept (d, id)."""
    kept = []
    for d, c in cand[:HEURISTIC_WIDTH]:
        if len(kept) == deg:
            break
        if any(sd(k, c) < d for _, k in kept):
            continue
        kept.append((d, c))
    return kept


# ------------------------------------------------------------------------------------------ the build
class Built:
    """levels (file convention: level + 1), offsets, entry_point, max_level, codes [n, 8], neighbors (faiss layout,
    -1 padded); lists[v][l] the sorted (d, id) of node v on level l; forward[(u, l)] the links u chose when it was
    inserted; visited[(u, l)] how many nodes u's beam on level l visited; batches [(start, count)]."""


def build(x, centroids, M_hnsw, efc, seed=0, beam_fn=beam):
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.shape[0]
    deg0, degU = 2 * M_hnsw, M_hnsw
    ef = max(min(efc, EF_CAP), deg0)
    lut = distance_tables(x, centroids)
    codes = codes_from_tables(lut)
    A = adc_matrix(lut, codes)
    S = sd_matrix(sdc_table(centroids), codes)
    del lut
    lev = assign_levels(n, M_hnsw, seed)
    order = insertion_order(lev, seed)
    entry, max_level = order[0], int(lev[order[0]])
    lists = [[[] for _ in range(int(lev[v]) + 1)] for v in range(n)]  # (d, id) pairs, unsorted until the end
    forward, visited, batches = {}, {}, []
    start = 1
    while start < n:
        count = min(start, MAX_BATCH, n - start)
        batches.append((start, count))
        chosen = []
        for u in order[start:start + count]:
            dist = A[u].tolist()
            ul = int(lev[u])
            cur = entry
            for l in range(max_level, ul, -1):
                cur = descend(dist, lambda v, l=l: [w for _, w in lists[v][l]], cur, l)
            for l in range(min(ul, max_level), -1, -1):
                W, nvis = beam_fn(dist, lambda v, l=l: [w for _, w in lists[v][l]], cur, ef)
                ids = [c for _, c in W[:HEURISTIC_WIDTH]]
                pos = {c: i for i, c in enumerate(ids)}
                sub = S[np.ix_(ids, ids)].tolist()
                kept = heuristic(W, lambda k, c: sub[pos[k]][pos[c]], deg0 if l == 0 else degU)
                chosen.append((u, l, kept))
                visited[(u, l)] = nvis
                cur = W[0][1]
        # nothing pointed to a batch member until here
        for u, l, kept in chosen:
            forward[(u, l)] = kept
            lists[u][l] = list(kept)
        for u, l, kept in chosen:
            deg = deg0 if l == 0 else degU
            for d, v in kept:
                L = lists[v][l]
                L.append((d, u))
                if len(L) > deg:
                    L.remove(max(L))
        start += count
    b = Built()
    b.n, b.M_hnsw, b.ef = n, M_hnsw, ef
    b.levels = (lev + 1).astype(np.int32)
    b.offsets = list_offsets(lev, M_hnsw)
    b.entry_point, b.max_level = int(entry), max_level
    b.codes = codes
    b.lists = [[sorted(L) for L in per] for per in lists]
    b.forward, b.visited, b.batches = forward, visited, batches
    nb = np.full(int(b.offsets[-1]), -1, dtype=np.int32)
    for v in range(n):
        for l, L in enumerate(b.lists[v]):
            at = int(b.offsets[v]) + (0 if l == 0 else deg0 + (l - 1) * degU)
            nb[at:at + len(L)] = [w for _, w in L]
    b.neighbors = nb
    return b


# ------------------------------------------------------------------------------------------ inputs the tests share
def gaussian_vectors(n, seed=0):
    return np.random.default_rng(seed).normal(size=(n, 128)).astype(np.float32)


def tied_vectors(groups, seed=1):
    """Small integer coordinates, every row present four times (interleaved, so the copies are `groups` apart): whole
    groups of nodes share one PQ code and every distance to them is equal."""
    rows = np.random.default_rng(seed).integers(0, 4, size=(groups, 128)).astype(np.float32)
    return np.ascontiguousarray(np.tile(rows, (4, 1)))


# ------------------------------------------------------------------------------------------ comparing with a file
def file_list(fx, v, l, M_hnsw):
    """The slots of node v on level l of a faiss IHNp file (oracle.faiss_file.read), -1 padding included."""
    at = int(fx.offsets[v]) + (0 if l == 0 else 2 * M_hnsw + (l - 1) * M_hnsw)
    return fx.neighbors[at:at + (2 * M_hnsw if l == 0 else M_hnsw)].tolist()


def first_difference(fx, b):
    """None when every list of the file equals the restatement's, else a message naming the first (node, level)
    that differs, with both lists. Also returns how many lists were compared."""
    nlists = 0
    for v in range(b.n):
        for l in range(int(b.levels[v])):
            nlists += 1
            got = file_list(fx, v, l, b.M_hnsw)
            want = file_list(b, v, l, b.M_hnsw)
            if got != want:
                return f"node {v} level {l}: file {got}, restatement {want} (with distances {b.lists[v][l]})", nlists
    return None, nlists
