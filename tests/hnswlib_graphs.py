"""Hand-made hnswlib index files for the fp32 search kernel (hnsw_flat_search.hip) -- TEST INFRASTRUCTURE ONLY.

write_hnswlib is the inverse of oracle/hnswlib_file.read, with its own struct packing (nothing of the library's
writer is called), so any graph can be put in front of the kernel and the oracle alike: rows that repeat an id,
rows wider than 128 links, labels past 2^32, one-node and empty indexes. The generators build the graphs the
builder never produces; tests/test_flat_graphs_cpu.py proves from oracle diagnostics that each of them reaches the
kernel path it is meant for, tests/test_gpu_flat_paths.py runs them on the GPU."""
import math
import struct

import numpy as np

def write_hnswlib(path, vec, l0_rows, up_rows, labels, ep, maxM, maxM0, M=None, mult=None, efc=128,
                  max_elements=None, maxlevel=None):
    """Write an hnswlib saveIndex file.

    vec [n, d] f32; labels [n] u64; ep the entry point (its level is the file's maxlevel unless one is given).
    l0_rows: per element its level-0 links (a sequence, at most maxM0 long), or an [n, 1 + maxM0] uint32 array of
    raw records (header word + link slots) taken as it is.
    up_rows: per element its upper levels: a list of link lists (entry l - 1 = level l, each at most maxM long),
    or a flat uint32 array of raw blocks [count | maxM links] taken as it is; empty for a level-0 element."""
    vec = np.ascontiguousarray(vec, dtype="<f4")
    n, d = vec.shape
    labels = np.ascontiguousarray(labels, dtype="<u8")
    assert labels.shape == (n,) and len(up_rows) == n
    if isinstance(l0_rows, np.ndarray) and l0_rows.ndim == 2:
        assert l0_rows.shape == (n, 1 + maxM0)
        l0 = np.ascontiguousarray(l0_rows, dtype="<u4")
    else:
        assert len(l0_rows) == n
        l0 = np.zeros((n, 1 + maxM0), dtype="<u4")
        for i, row in enumerate(l0_rows):
            assert len(row) <= maxM0
            l0[i, 0] = len(row)
            l0[i, 1:1 + len(row)] = np.asarray(row, dtype=np.uint32)
    blk = 1 + maxM
    ups = []
    for r in up_rows:
        if isinstance(r, np.ndarray):
            words = np.ascontiguousarray(r, dtype="<u4").ravel()
        else:
            words = np.zeros(len(r) * blk, dtype="<u4")
            for l, lst in enumerate(r):
                assert len(lst) <= maxM
                words[l * blk] = len(lst)
                words[l * blk + 1:l * blk + 1 + len(lst)] = np.asarray(lst, dtype=np.uint32)
        assert words.size % blk == 0
        ups.append(words)
    levels = [w.size // blk for w in ups]
    if maxlevel is None:  # an empty index has no entry point to take it from: hnswlib itself writes -1 there
        maxlevel = levels[ep] if n else 0
    M = maxM if M is None else M
    mult = 1.0 / math.log(M) if mult is None else mult
    off_data = 4 * (1 + maxM0)
    label_off = off_data + 4 * d
    size_el = label_off + 8
    out = bytearray()
    out += struct.pack("<6Q", 0, n if max_elements is None else max_elements, n, size_el, label_off, off_data)
    out += struct.pack("<iI", maxlevel, ep)
    out += struct.pack("<3Q", maxM, maxM0, M)
    out += struct.pack("<dQ", mult, efc)
    rec = np.zeros((n, size_el), dtype=np.uint8)
    rec[:, :off_data] = l0.view(np.uint8).reshape(n, off_data)
    rec[:, off_data:label_off] = vec.view(np.uint8).reshape(n, 4 * d)
    rec[:, label_off:] = labels.view(np.uint8).reshape(n, 8)
    out += rec.tobytes()
    for w in ups:
        out += struct.pack("<I", 4 * w.size)
        out += w.tobytes()
    with open(path, "wb") as f:
        f.write(bytes(out))
    return path


def rewrite(fx, path):
    """Write a parsed index (hnswlib_file.read) back: raw level-0 records and raw upper blocks."""
    blk = 1 + fx["maxM"]
    ups = [fx["up"][fx["up_off"][i]:fx["up_off"][i] + fx["levels"][i] * blk] if fx["levels"][i] else
           np.zeros(0, np.uint32) for i in range(fx["n"])]
    return write_hnswlib(path, fx["vec"], fx["l0"], ups, fx["labels"], fx["ep"], fx["maxM"], fx["maxM0"],
                         M=fx["M"], mult=fx["mult"], efc=fx["efc"], max_elements=fx["max_elements"])


def scaled_labels(rng, n):
    """Labels that need all 64 bits, from a permutation p of 0 .. n-1: (p // 2 + 1) * 2^33 + (p * 2654435761 mod 2^32).
    Two labels share each high word, so the low word decides between them; the low words are scattered, so their
    order is not the labels' order; and no label equals its node id. (p * (2^33 + c) + b with a small c would not
    do: both halves then grow with p, and a comparison of either half alone gives the right order.) All are
    distinct and below 2^63, because the oracle returns int64."""
    p = rng.permutation(n).astype(np.uint64)
    lab = (p // np.uint64(2) + np.uint64(1)) * np.uint64(2 ** 33) + (p * np.uint64(2654435761)) % np.uint64(2 ** 32)
    assert n == 0 or int(lab.max()) < 2 ** 63
    return lab


def random_tie_graph(rng, n, d, maxM, maxM0, dup, levels_max=3):
    """A random graph whose distances are small exact integers, so ties are everywhere: vectors are zero except
    the first four coordinates, integers in {0, 1, 2}. Level-0 rows hold 1 .. maxM0 random links, drawn with
    replacement (a row may list an id twice) when `dup` is set. A node on level l links only to nodes that reach
    level l, and the entry point sits on the top level (the product reader enforces both). Labels are
    scaled_labels. Returns the keyword arguments of write_hnswlib."""
    vec = np.zeros((n, d), dtype=np.float32)
    vec[:, :4] = rng.integers(0, 3, size=(n, 4))
    levels = np.zeros(n, dtype=np.int64)
    for l in range(1, levels_max):
        levels[rng.random(n) < 0.3 ** l] += 1
    levels[int(rng.integers(0, n))] = levels_max - 1  # the top level is never empty
    ep = int(rng.choice(np.flatnonzero(levels == levels.max())))

    def draw(pool, i, width):
        pool = pool[pool != i]
        cap = width if dup else min(width, len(pool))
        if cap == 0:
            return []
        return [int(v) for v in rng.choice(pool, size=int(rng.integers(1, cap + 1)), replace=dup)]

    everyone = np.arange(n)
    l0_rows = [draw(everyone, i, maxM0) for i in range(n)]
    if dup:  # whatever the draws gave, one row repeats an id right away and one at its far end
        l0_rows[0] = (l0_rows[0] + l0_rows[0][:1])[-maxM0:] if len(l0_rows[0]) > 1 else l0_rows[0] * 2
        l0_rows[ep][-1] = l0_rows[ep][0]
    up_rows = []
    for i in range(n):
        up_rows.append([draw(np.flatnonzero(levels >= l), i, maxM) for l in range(1, levels[i] + 1)])
    return {"vec": vec, "l0_rows": l0_rows, "up_rows": up_rows, "labels": scaled_labels(rng, n), "ep": ep,
            "maxM": maxM, "maxM0": maxM0}


def tiny_graph(rng, n, d, maxM, maxM0):
    """n <= maxM0 + 1 grid vectors on one level, everyone linked to everyone else, entry point 0; n = 0 gives the
    empty index."""
    assert n <= maxM0 + 1
    vec = np.zeros((n, d), dtype=np.float32)
    vec[:, :4] = rng.integers(0, 3, size=(n, 4))
    l0_rows = [[j for j in range(n) if j != i] for i in range(n)]
    return {"vec": vec, "l0_rows": l0_rows, "up_rows": [[] for _ in range(n)], "labels": scaled_labels(rng, n),
            "ep": 0, "maxM": maxM, "maxM0": maxM0}


def tie_queries(rng, nq, d):
    """Half on the graphs' integer grid (exact hits, integer distances), half offset by 0.5."""
    q = np.zeros((nq, d), dtype=np.float32)
    q[:, :4] = rng.integers(0, 3, size=(nq, 4))
    q[nq // 2:, :4] += 0.5
    return q


STAR_D, STAR_MAXM, STAR_MAXM0 = 16, 128, 256


def star_graph(hubs, seed=0):
    """One level, d = 16, maxM = 128, maxM0 = 256. Node 0 links to nodes 1 .. 256; the first `hubs` of those each
    link to 256 leaves of their own (which link back). Seen from queries near zero the hubs lie closest (squared
    norm <= 16), the leaves next (around 64), node 0's remaining children far away (around 900), and all
    coordinates are small integers, so an exhaustive search (ef > n) expands node 0, then every hub, and only then
    pops anything else: candidate_set peaks at 256 + 255 * hubs entries. With ef = 64 the hubs fill
    top_candidates and are all expanded, so every query computes 1 + 256 + 256 * hubs distances."""
    assert 0 <= hubs <= 256
    rng = np.random.default_rng(seed)
    n = 1 + 256 + 256 * hubs
    vec = rng.integers(-1, 2, size=(n, STAR_D)).astype(np.float32)
    vec[0] = 0.0
    vec[0, 0] = 5.0
    leaves = np.arange(257, n)
    vec[leaves, rng.integers(0, STAR_D, size=leaves.size)] = 8.0
    far = np.arange(1 + hubs, 257)
    vec[far, rng.integers(0, STAR_D, size=far.size)] = 30.0
    l0_rows = [list(range(1, 257))]
    for h in range(256):
        l0_rows.append(list(range(257 + 256 * h, 257 + 256 * (h + 1))) if h < hubs else [0])
    for h in range(hubs):
        l0_rows.extend([[1 + h]] * 256)
    return {"vec": vec, "l0_rows": l0_rows, "up_rows": [[] for _ in range(n)], "labels": scaled_labels(rng, n),
            "ep": 0, "maxM": STAR_MAXM, "maxM0": STAR_MAXM0}


def star_queries(rng, nq):
    """Near zero: every fourth query exactly zero (integer distances, ties everywhere), the others Gaussian with
    sigma 0.05, far inside the margins between the star's three shells."""
    q = (0.05 * rng.standard_normal((nq, STAR_D))).astype(np.float32)
    q[::4] = 0.0
    return q


def write_and_read(path, graph):
    """The graph as a file, and that file as the oracle's reader sees it."""
    from oracle import hnswlib_file
    write_hnswlib(path, **graph)
    return hnswlib_file.read(path)


def build_and_read(path, n, d, M, efc=64, seed=1):
    """A builder-made index over n Gaussian vectors (+ the vectors), parsed."""
    from deepreadmapper_amd import synth
    from oracle import hnswlib_file
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    synth.build_flat_index(x, path, M=M, efc=efc, nthreads=4)
    return hnswlib_file.read(path), x


def has_dup_row(fx):
    """Does some level-0 row list one id twice?"""
    for row in fx["l0"]:
        links = row[1:1 + (int(row[0]) & 0xFFFF)]
        if len(np.unique(links)) != len(links):
            return True
    return False
