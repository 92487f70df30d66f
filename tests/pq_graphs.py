"""IHNp + IxPq index files of any PQ and graph shape, for the HNSW-PQ kernel paths that no builder-made
d = 128 / 8 x 8 / M_hnsw = 16 index reaches -- TEST INFRASTRUCTURE ONLY. Like tests/tie_graphs.py (which stays as
it is: its 8 x 8, M_hnsw = 2 constants are imported by other tests) the writer restates the faiss on-disk layout
(impl/index_write.cpp) with its own struct packing, independent of the library's writer, and it
packs the centroid indices into faiss's generic bit layout itself (PQEncoderGeneric: least-significant bit first,
code_size = ceil(M * nbits / 8)), independent of builder.cpp's encoder.

Graph generators: fan_graph (one level, node i -> (deg0 * i + 1 + j) mod n: a walk that fans out over the whole
index, past the clear list of the visited set), random_graph (several levels, holes, a repeated link). PQ
generators: small-integer centroids (every fp32 sum exact, equal distances designed) or Gaussian ones."""
import math
import struct

import numpy as np


def default_levels(M_hnsw):
    """HNSW::set_default_probas(M, 1 / log(M)) [faiss impl/HNSW.cpp]: (assign_probas, cum_nneighbor_per_level)."""
    mult = 1.0 / math.log(float(M_hnsw))
    probas, cum, nn, level = [], [0], 0, 0
    while True:
        p = math.exp(-level / mult) * (1 - math.exp(-1 / mult))
        if p < 1e-9:
            break
        probas.append(p)
        nn += 2 * M_hnsw if level == 0 else M_hnsw
        cum.append(nn)
        level += 1
    return probas, cum


def code_size(M_pq, nbits):
    return (M_pq * nbits + 7) // 8


def pack_codes(codes_idx, nbits):
    """[n, M] centroid indices -> [n, code_size] bytes: index m occupies bits [m * nbits, (m + 1) * nbits) of the
    row read as one little-endian integer."""
    codes_idx = np.asarray(codes_idx)
    n, M = codes_idx.shape
    assert codes_idx.min(initial=0) >= 0 and codes_idx.max(initial=0) < (1 << nbits)
    cs = code_size(M, nbits)
    out = bytearray()
    for row in codes_idx.tolist():
        v = 0
        for m, c in enumerate(row):
            v |= c << (m * nbits)
        out += v.to_bytes(cs, "little")
    return np.frombuffer(bytes(out), dtype=np.uint8).reshape(n, cs)


def unpack_codes(codes, M_pq, nbits):
    """The inverse, by another route (numpy bit planes): [n * code_size] bytes -> [n, M] indices."""
    cs = code_size(M_pq, nbits)
    bits = np.unpackbits(np.asarray(codes, dtype=np.uint8).reshape(-1, cs), axis=1, bitorder="little")
    bits = bits[:, :M_pq * nbits].reshape(-1, M_pq, nbits).astype(np.int64)
    return (bits << np.arange(nbits)[None, None, :]).sum(axis=2)


def write_ihnp(path, d, M_pq, nbits, M_hnsw, centroids, codes_idx, rows, entry_point, max_level,
               ef_construction=40, ef_search=16, cum=None):
    """rows[i] = node i's link lists, level 0 first: 2 * M_hnsw slots, then M_hnsw per upper level, -1 padded.
    centroids: [M_pq, 2^nbits, d / M_pq] f32. codes_idx: [n, M_pq] centroid indices. `cum` replaces faiss's
    cum_nneighbor_per_level (for link tables that faiss itself would not lay out)."""
    n = len(rows)
    probas, cum_default = default_levels(M_hnsw)
    cum = list(cum_default if cum is None else cum)
    probas = probas[:len(cum) - 1]
    levels = [len(r) for r in rows]
    assert max(levels, default=1) <= len(probas)
    offsets = np.zeros(n + 1, dtype="<u8")
    nbrs = []
    for i, r in enumerate(rows):
        for l, lst in enumerate(r):
            assert len(lst) == cum[l + 1] - cum[l], (i, l, len(lst))
            nbrs.extend(lst)
        offsets[i + 1] = len(nbrs)
    centroids = np.ascontiguousarray(centroids, dtype="<f4")
    assert centroids.shape == (M_pq, 1 << nbits, d // M_pq) and d % M_pq == 0
    codes = pack_codes(np.asarray(codes_idx).reshape(n, M_pq), nbits)
    out = bytearray()

    def vec(a, dtype):
        a = np.ascontiguousarray(a, dtype=dtype)
        out.extend(struct.pack("<Q", a.size))
        out.extend(a.tobytes())

    def header():
        out.extend(struct.pack("<iqqqBi", d, n, 1 << 20, 1 << 20, 1, 1))  # ..., is_trained, METRIC_L2

    out.extend(b"IHNp")
    header()
    vec(probas, "<f8")
    vec(cum, "<i4")
    vec(levels, "<i4")
    vec(offsets, "<u8")
    vec(nbrs, "<i4")
    out.extend(struct.pack("<iiiii", entry_point, max_level, ef_construction, ef_search, 1))
    out.extend(b"IxPq")
    header()
    out.extend(struct.pack("<QQQ", d, M_pq, nbits))
    vec(centroids, "<f4")
    vec(codes, "<u1")
    out.extend(struct.pack("<iBi", 0, 0, 0))
    with open(path, "wb") as f:
        f.write(bytes(out))
    return path


def rows_of(fx):
    """The link lists of a read file (oracle.faiss_file) in write_ihnp's form."""
    cum = fx.cum_nneighbor_per_level
    rows = []
    for i in range(fx.ntotal):
        o = int(fx.offsets[i])
        rows.append([fx.neighbors[o + cum[l]:o + cum[l + 1]].tolist() for l in range(fx.levels[i])])
    return rows


def rewrite(fx, path):
    """write_ihnp from the unpacked fields of a read file."""
    M, nbits = int(fx.pq_M), int(fx.pq_nbits)
    return write_ihnp(path, fx.d, M, nbits, int(fx.cum_nneighbor_per_level[1]) // 2,
                      fx.centroids.reshape(M, 1 << nbits, fx.d // M), unpack_codes(fx.codes, M, nbits), rows_of(fx),
                      fx.entry_point, fx.max_level, fx.efConstruction, fx.efSearch)


# ------------------------------------------------------------------------------------------ graphs
def fan_graph(n, deg0, rng=None):
    """One level, every row full: node i links to (deg0 * i + 1 + j) mod n, j < deg0. From node 0 the walk reaches
    deg0^h new nodes at hop depth h, so a query computes about min(n, deg0 * ef) distances. Returns (rows, entry
    point, max_level); `rng` (optional) permutes each row."""
    assert deg0 % 2 == 0 and n > deg0
    rows = []
    for i in range(n):
        r = [(deg0 * i + 1 + j) % n for j in range(deg0)]
        if rng is not None:
            r = [r[j] for j in rng.permutation(deg0)]
        rows.append([r])
    return rows, 0, 0


def random_graph(n, M_hnsw, n_levels, rng, hole_p=0.2, dup=False):
    """Random links over up to n_levels levels. A row holds distinct ids; with probability hole_p it is cut short
    (-1 holes at its end), with hole_p = 0 every row is as full as its level's population allows (level 0: always
    full for n > 2 * M_hnsw). dup: the first level-0 row with two links lists its first link twice. Returns (rows,
    entry point, max_level)."""
    _, cum = default_levels(M_hnsw)
    levels = np.ones(n, dtype=np.int64)
    for l in range(1, n_levels):
        levels[rng.random(n) < 0.3 ** l] += 1
    entry = int(rng.choice(np.flatnonzero(levels == levels.max())))
    pools = [np.flatnonzero(levels > l) for l in range(int(levels.max()))]
    rows = []
    for i in range(n):
        r = []
        for l in range(levels[i]):
            width = cum[l + 1] - cum[l]
            pool = pools[l][pools[l] != i]
            k = min(width, len(pool))
            lst = [int(v) for v in rng.choice(pool, size=k, replace=False)] if k else []
            if lst and rng.random() < hole_p:
                lst = lst[:int(rng.integers(0, len(lst)))]
            r.append(lst + [-1] * (width - len(lst)))
        rows.append(r)
    if dup:
        i = next(i for i in range(n) if rows[i][0][1] >= 0)  # the first level-0 row with two links
        rows[i][0][1] = rows[i][0][0]
    return rows, entry, int(levels.max()) - 1


def chain_graph(n, M_hnsw):
    """One level, node i -> i + 1 .. i + 2 * M_hnsw (those below n): every node is reached from node 0."""
    rows = []
    for i in range(n):
        lst = [j for j in range(i + 1, min(n, i + 1 + 2 * M_hnsw))]
        rows.append([lst + [-1] * (2 * M_hnsw - len(lst))])
    return rows, (0 if n else -1), (0 if n else -1)


# ------------------------------------------------------------------------------------------ PQ
def int_centroids(d, M_pq, nbits):
    """Centroid c of every sub-quantizer is (c mod 16, 0, ..., 0): with integer queries every LUT entry and every
    sum of them is a small integer, exact in fp32 in any order."""
    c = np.zeros((M_pq, 1 << nbits, d // M_pq), dtype=np.float32)
    c[:, :, 0] = (np.arange(1 << nbits) % 16).astype(np.float32)[None, :]
    return c


def tie_codes(rng, n, M_pq, nbits, n_values=4):
    """Codes whose distances to an integer query take few distinct values: sub-quantizer 0 draws from n_values
    indices, sub-quantizer 1 (if any) from {0, 1}, the rest are 0."""
    codes = np.zeros((n, M_pq), dtype=np.int64)
    vals = rng.choice(np.arange(1, min(16, 1 << nbits)), size=min(n_values, min(16, 1 << nbits) - 1), replace=False)
    codes[:, 0] = rng.choice(vals, size=n)
    if M_pq > 1:
        codes[:, 1] = rng.integers(0, 2, size=n)
    return codes


def int_queries(rng, nq, d, M_pq):
    """Queries for int_centroids: zero, except a small integer in the first dimension of sub-vectors 0 and 1."""
    q = np.zeros((nq, d), dtype=np.float32)
    q[1:, 0] = rng.integers(0, 12, size=nq - 1)
    if M_pq > 1:
        q[2:, d // M_pq] = rng.integers(0, 3, size=nq - 2)
    return q


def gauss_centroids(rng, d, M_pq, nbits):
    return rng.standard_normal((M_pq, 1 << nbits, d // M_pq)).astype(np.float32)


def random_codes(rng, n, M_pq, nbits, n_sub=None):
    """Uniform indices in the first n_sub sub-quantizers (default: all), 0 in the rest."""
    codes = np.zeros((n, M_pq), dtype=np.int64)
    n_sub = M_pq if n_sub is None else n_sub
    codes[:, :n_sub] = rng.integers(0, 1 << nbits, size=(n, n_sub))
    return codes


def adc_reference(centroids, codes_idx, q):
    """ADC distances [nq, n] in numpy float32 with the documented order: a LUT entry is the
    sequential sum over t of (x_t - c_t)^2, a distance the sequential sum over m of the entries, each operation
    rounded to fp32 (no FMA). From the indices before packing: independent of every decoder."""
    M, ksub, dsub = centroids.shape
    codes_idx = np.asarray(codes_idx)
    out = np.zeros((len(q), len(codes_idx)), dtype=np.float32)
    for i, x in enumerate(np.asarray(q, dtype=np.float32)):
        for m in range(M):
            acc = np.zeros(ksub, dtype=np.float32)
            for t in range(dsub):
                diff = (x[m * dsub + t] - centroids[m, :, t]).astype(np.float32)
                acc = (acc + (diff * diff).astype(np.float32)).astype(np.float32)
            out[i] = (out[i] + acc[codes_idx[:, m]]).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------ built indices
def build(path, d, M_pq, nbits, M_hnsw, genome_len=1600, efc=40, seed=0):
    """A builder-made dense index over a `genome_len` bp genome (2,902 windows at 1,600 bp), single-threaded, of
    d-dimensional stand-in embeddings. Returns (read file, embeddings)."""
    from deepreadmapper_amd import synth
    from oracle import faiss_file
    g = synth.genome(genome_len, seed=17 + seed)
    x = synth.embed(synth.tag(synth.windows_lookup(g, 150, 1)), dim=d)
    synth.build_index(x, path, M_pq=M_pq, nbits=nbits, M_hnsw=M_hnsw, efc=efc, nthreads=1)
    return faiss_file.read(path), x


def queries_for(x, nq, seed=1):
    """nq / 2 Gaussian queries scaled like the embeddings + nq / 2 stored vectors (distance ties with their own
    codes' duplicates, as reads that match a window exactly)."""
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal((nq - nq // 2, x.shape[1])) * x.std() + x.mean()).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([g, x[rng.choice(len(x), size=nq // 2, replace=False)]]))


# ------------------------------------------------------------------------------------------ fixtures
# (shared by tests/test_pq_graphs_cpu.py, which proves what each reaches, and tests/test_gpu_pq_paths.py)
BUILT_SHAPES = {  # name: (d, M_pq, nbits, M_hnsw)
    "4x8d32": (32, 4, 8, 16),   # dsub 8: scalar LUT build
    "4x8d64": (64, 4, 8, 16),   # dsub 16: vector LUT build with M = 4
    "16x8": (128, 16, 8, 16),   # dsub 8, 16-byte codes
    "8x6": (128, 8, 6, 32),     # ksub 64, packed codes, deg0 = 64
    "8x5": (128, 8, 5, 4),      # an index straddles a byte boundary; deg0 = 8, many levels
    "8x10": (128, 8, 10, 16),   # a 10-bit index at shift 6 needs 3 bytes
}
LEAN_DEGREES = {"8x8m4": (128, 8, 8, 4), "8x8m12": (128, 8, 8, 12), "8x8m32": (128, 8, 8, 32)}
# (k, ef) per kernel. General: R = ceil(max(ef, k) / 64) = 1, 1, 2, 2, 5, 8 take the instantiations 1, 1, 2, 2, 8, 8;
# (150, 192) and (50, 200) are R = 3 and 4, the instantiation 4 that the first six leave out
GENERAL_KEF = [(1, 1), (10, 16), (100, 128), (64, 100), (200, 300), (300, 512), (150, 192), (50, 200)]
LDS_KEF = [(10, 600), (600, 600), (513, 16), (1024, 16), (10, 1024), (1024, 4096)]
LEAN_KEF = [(128, 128), (64, 64), (5, 128), (16, 100)]
FAN_N_LDS, FAN_N_GENERAL = 20000, 24000  # fan_graph sizes whose walks pass clear_cap at ef = 2048 / ef = 512
RAMP_N = 17000


def _fixture(path, d, M_pq, nbits, M_hnsw, centroids, codes_idx, graph, q):
    from oracle import faiss_file
    rows, entry, max_level = graph
    write_ihnp(path, d, M_pq, nbits, M_hnsw, centroids, codes_idx, rows, entry, max_level)
    return {"index": path, "fx": faiss_file.read(path), "q": q, "centroids": centroids, "codes_idx": codes_idx}


def make_built(directory, name):
    d, M_pq, nbits, M_hnsw = {**BUILT_SHAPES, **LEAN_DEGREES, "8x8": (128, 8, 8, 16)}[name]
    path = str(directory / f"{name}.index")
    fx, x = build(path, d, M_pq, nbits, M_hnsw)
    codes_idx = unpack_codes(fx.codes, M_pq, nbits)
    return {"index": path, "fx": fx, "q": queries_for(x, 64), "x": x, "codes_idx": codes_idx,
            "centroids": fx.centroids.reshape(M_pq, 1 << nbits, d // M_pq)}


def make_random(directory, name, d, M_pq, nbits, M_hnsw, n, n_levels=3, hole_p=0.2, dup=True, seed=0, nq=48):
    """Gaussian centroids, uniform codes, a random graph: the shapes the builder's k-means is too slow for."""
    rng = np.random.default_rng([seed, d, M_pq, nbits, M_hnsw, n])
    q = rng.standard_normal((nq, d)).astype(np.float32)
    return _fixture(str(directory / f"{name}.index"), d, M_pq, nbits, M_hnsw, gauss_centroids(rng, d, M_pq, nbits),
                    random_codes(rng, n, M_pq, nbits), random_graph(n, M_hnsw, n_levels, rng, hole_p, dup), q)


def make_tie(directory, name, d, M_pq, nbits, M_hnsw, n, n_levels=2, seed=0, nq=24):
    """Integer centroids, codes with few distinct distances, a random graph: equal distances everywhere."""
    rng = np.random.default_rng([seed, d, M_pq, nbits, M_hnsw, n, 7])
    return _fixture(str(directory / f"{name}.index"), d, M_pq, nbits, M_hnsw, int_centroids(d, M_pq, nbits),
                    tie_codes(rng, n, M_pq, nbits), random_graph(n, M_hnsw, n_levels, rng, 0.2, True),
                    int_queries(rng, nq, d, M_pq))


def make_chain(directory, name, d, M_pq, nbits, M_hnsw, n, nq=6):
    """n nodes, all reachable (chain_graph), tie codes: for ntotal < k and ntotal = 0."""
    rng = np.random.default_rng([n, d, M_pq, nbits])
    return _fixture(str(directory / f"{name}.index"), d, M_pq, nbits, M_hnsw, int_centroids(d, M_pq, nbits),
                    tie_codes(rng, n, M_pq, nbits), chain_graph(n, M_hnsw), int_queries(rng, nq, d, M_pq))


def make_fan(directory, n, nq=16):
    """fan_graph(n, 64) in 8 x 8: centroid c of a sub-quantizer is (c, 0, ..., 0), uniform codes in the first three
    sub-quantizers, integer queries in their first dimensions (exact distances, some ties)."""
    rng = np.random.default_rng(n)
    cen = np.zeros((8, 256, 16), dtype=np.float32)
    cen[:, :, 0] = np.arange(256, dtype=np.float32)[None, :]
    return _fixture(str(directory / f"fan{n}.index"), 128, 8, 8, 32, cen, random_codes(rng, n, 8, 8, 3),
                    fan_graph(n, 64), fan_queries(rng, nq))


def fan_queries(rng, nq):
    q = np.zeros((nq, 128), dtype=np.float32)
    q[:, [0, 16, 32]] = rng.integers(0, 256, size=(nq, 3))
    return q


def make_ramp(directory, n=RAMP_N, M_hnsw=32):
    """chain_graph whose distances fall along the chain: node i, r = n - 1 - i, has code (r mod 256, r / 256, 0, ...)
    under centroids (c, 0, ...) and (256 c, 0, ...), so to a query with x_0 <= 0 and x_16 <= 0 it is at
    (r mod 256 - x_0)^2 + (256 (r / 256) - x_16)^2 + const, increasing in r. Every hop then finds 2 * M_hnsw
    unseen, closer nodes: such a `sweep` query computes n - 1 distances at ANY ef (the only way past clear_cap at
    the lean kernel's ef <= 128). A `stall` query (x_16 = 256 * 255: the larger r / 256 the better) has its nearest
    nodes at the entry point and stops there."""
    rng = np.random.default_rng(n)
    r = n - 1 - np.arange(n)
    codes = np.zeros((n, 8), dtype=np.int64)
    codes[:, 0], codes[:, 1] = r % 256, r // 256
    cen = rng.standard_normal((8, 256, 16)).astype(np.float32)
    cen[:2] = 0
    cen[0, :, 0] = np.arange(256, dtype=np.float32)
    cen[1, :, 0] = 256.0 * np.arange(256, dtype=np.float32)
    return _fixture(str(directory / f"ramp{n}.index"), 128, 8, 8, M_hnsw, cen, codes, chain_graph(n, M_hnsw), None)


def ramp_queries(rng, nq, stall=False):
    q = np.zeros((nq, 128), dtype=np.float32)
    q[:, 32:] = rng.standard_normal((nq, 96))
    if stall:
        q[:, 0] = rng.integers(0, 256, size=nq)
        q[:, 16] = 256.0 * 255
    else:
        q[1:, 0] = -rng.integers(0, 64, size=nq - 1)
        q[2:, 16] = -256.0 * rng.integers(0, 4, size=nq - 2)
    return q
