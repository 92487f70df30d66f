"""Inputs for the exhaustive scans' slicing, chunking and selection paths (exact_scan.hip), and a
plain Python replay of the selection -- TEST INFRASTRUCTURE ONLY. Shared by tests/test_exact_cases_cpu.py, which
proves from the replay alone what each input does to a (query, slice), and tests/test_gpu_exact_paths.py, which runs
the inputs on the GPU.

Expected distances come from pq_graphs.adc_reference (from the centroid indices before packing: independent of every
decoder) and exact_ref.l2sqr8; the expected top-k is the (distance, id) sort of those. Every case is built once per
process and handed out read-only."""
import functools
from collections import namedtuple

import numpy as np

import exact_ref as R
import hnswlib_graphs as HG
import pq_graphs as PG

EMPTY = np.uint64(2 ** 64 - 1)  # the scans' kEmpty: no key equals it (ids are below 2^31)
STEP = {"pq8": 512, "pq": 256, "l2": 256}  # base rows per step: 256 threads x 2 codes (PQ 8 x 8), x 1 otherwise
QT = {"pq8": 8, "pq": 1, "l2": 8}
ORDERS = ("random", "descending", "ascending", "sawtooth")
N_ORDER = 8192  # rows of the arrival-order and the tie cases: one slice of 16 (PQ 8 x 8) or 32 steps
N_BIG = 65536   # rows of the chunked cases: 1,024 slices of 64 rows


def cap_of(kind, k):
    """The survivor buffer of a (query, slice), DESIGN.md sec. 4.9: the power of two >= k + rows per step."""
    cap = 64
    while cap < k + STEP[kind]:
        cap <<= 1
    return cap


def tight_ks(kind):
    """The k at which cap == k + step exactly: the buffer has no slack."""
    return [k for k in range(1, 1025) if cap_of(kind, k) == k + STEP[kind]]


# k per kernel for the arrival orders; each holds every tight k of its kernel
ORDER_KS = {"pq8": [1, 128, 512, 1024], "pq": [1, 128, 256, 768, 1024], "l2": [1, 128, 256, 768, 1024]}


def keys_of(dist):
    """The scans' 64-bit keys of one query's distances in row order: ord32(dist) << 32 | row. The distances here are
    sums of squares (>= +0.0, finite), for which the bit pattern itself is monotone."""
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    assert (dist >= 0).all() and np.isfinite(dist).all()
    return (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(dist), dtype=np.uint64)


def topk_of(dist, k):
    """(D [nq, k] f32, I [nq, k] int64) of a distance matrix [nq, n] under (distance, id), padded (+inf, -1)."""
    nq, n = dist.shape
    D = np.full((nq, k), np.inf, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for i in range(nq):
        order = np.lexsort((np.arange(n), dist[i]))[:k]
        D[i, :len(order)] = dist[i][order]
        I[i, :len(order)] = order
    return D, I


def arrange(items, dist0, order, step=256, seed=0):
    """`items` (codes or rows, one per base row) in another arrival order, by query 0's reference distance dist0.
    Returns (items[perm], perm). Ties keep their id order. "sawtooth": runs of `step` rows whose runs ascend and
    whose rows descend inside a run."""
    n = len(items)
    dist0 = np.asarray(dist0)
    assert dist0.shape == (n,)
    if order == "random":
        perm = np.random.default_rng(seed).permutation(n)
    elif order == "ascending":
        perm = np.argsort(dist0, kind="stable")
    elif order == "descending":
        perm = np.argsort(-dist0.astype(np.float64), kind="stable")
    elif order == "sawtooth":
        asc = np.argsort(dist0, kind="stable")
        perm = np.concatenate([run[np.argsort(-dist0[run].astype(np.float64), kind="stable")]
                               for run in (asc[b:b + step] for b in range(0, n, step))])
    else:
        raise ValueError(order)
    return np.ascontiguousarray(np.asarray(items)[perm]), perm


# ------------------------------------------------------------------------------------------ the selection, replayed
Trace = namedtuple("Trace", "compactions max_fill hit_cap appended passes first_compaction_step keys buf")


def selection_trace(keys, k, cap, step, r0, r1, le=False, trigger_ge=False, thr_at_k=False):
    """One (query, slice) of a scan kernel, replayed: rows [r0, r1) of `keys` (uint64, row order) arrive `step` at a
    time; a key below the threshold is appended to a buffer of `cap` entries; after a step, a buffer that could not
    take another (`fill + step > cap`) is cut to its k smallest, and the threshold becomes the k-th of them. At the
    end the buffer is cut once more and padded with EMPTY to k.

    How many keys pass in a step depends only on the keys and the threshold, not on the order in which the waves'
    atomics land, so the counts are those of the kernel; only the places inside the buffer differ (here: row order).

    Returns Trace: the compactions inside the loop, the largest fill, whether a fill equalled cap, the keys appended
    in all, the count per step, the step of the first compaction (None: there was none), the slice's k-list, and
    the whole buffer as the kernel leaves it (entries past k are stale).

    Variants of the kernel, for the tests to show what an input can tell apart: `le` appends `key <= threshold`,
    `trigger_ge` compacts at `fill + step >= cap`, `thr_at_k` takes sorted[k] (EMPTY beyond the fill) as threshold."""
    keys = np.asarray(keys, dtype=np.uint64)
    buf = np.full(cap, EMPTY, dtype=np.uint64)
    thr, fill = EMPTY, 0
    compactions, max_fill, hit_cap, appended, passes, first = 0, 0, False, 0, [], None

    def compact(final):
        nonlocal fill, thr
        srt = np.sort(buf[:fill])
        keep = min(fill, k)
        buf[:keep] = srt[:keep]
        if final:
            buf[keep:k] = EMPTY
        if fill >= k:
            at = k if thr_at_k else k - 1
            thr = srt[at] if at < fill else EMPTY
        fill = keep

    for s, b in enumerate(range(r0, r1, step)):
        rows = keys[b:min(b + step, r1)]
        passing = rows[rows <= thr] if le else rows[rows < thr]
        assert fill + len(passing) <= cap, "the step's room was checked before the step"
        buf[fill:fill + len(passing)] = passing
        fill += len(passing)
        appended += len(passing)
        passes.append(len(passing))
        max_fill = max(max_fill, fill)
        hit_cap |= fill == cap
        if (fill + step >= cap) if trigger_ge else (fill + step > cap):
            compact(False)
            compactions += 1
            first = s if first is None else first
    compact(True)
    return Trace(compactions, max_fill, bool(hit_cap), appended, tuple(passes), first, buf[:k].copy(), buf)


def merge_model(ws, slices, k, cap, stride=None):
    """exact_merge_kernel: the k smallest of the slices' k-lists, list s at ws[s * cap]. `stride` (a variant): the
    lists read at another stride."""
    stride = cap if stride is None else stride
    ws = np.asarray(ws, dtype=np.uint64).ravel()
    lists = [ws[s * stride:s * stride + k] for s in range(slices)]
    return np.sort(np.concatenate(lists))[:k]


def scan_model(keys, k, kind, slice_rows, merge_stride=None, **variant):
    """A whole scan of one query: every slice's selection_trace, then the merge. Returns (k keys, the traces)."""
    n, cap, step = len(keys), cap_of(kind, k), STEP[kind]
    slices = max(1, -(-n // slice_rows))
    traces = [selection_trace(keys, k, cap, step, s * slice_rows, min(n, (s + 1) * slice_rows), **variant)
              for s in range(slices)]
    ws = np.concatenate([t.buf for t in traces])
    return merge_model(ws, slices, k, cap, merge_stride), traces


def reference_keys(keys, k):
    """What any correct scan returns: the k smallest keys, padded with EMPTY."""
    out = np.full(k, EMPTY, dtype=np.uint64)
    srt = np.sort(np.asarray(keys, dtype=np.uint64))[:k]
    out[:len(srt)] = srt
    return out


# ------------------------------------------------------------------------------------------ inputs
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


PQ_SHAPES = {**PG.BUILT_SHAPES, "8x8": (128, 8, 8, 16)}  # name: (d, M_pq, nbits, M_hnsw of the built fixtures)


def write_pq_index(path, case):
    """The case as an IHNp file. The scan never reads the graph: chain_graph(n, 4) is the cheapest the loader takes
    (M_hnsw = 2 has more than the 24 levels of faiss's default table that drm_index_load accepts)."""
    rows, entry, max_level = PG.chain_graph(len(case["codes"]), 4)
    return PG.write_ihnp(str(path), case["d"], case["M"], case["nbits"], 4, case["centroids"], case["codes"], rows,
                         entry, max_level)


def _pq_case(d, M, nbits, centroids, codes, q):
    dist = PG.adc_reference(centroids, codes, q)
    _frozen(centroids, codes, q, dist)
    return {"d": d, "M": M, "nbits": nbits, "centroids": centroids, "codes": codes, "q": q, "dist": dist}


@functools.lru_cache(maxsize=None)
def pq_gauss(shape, n, nq=9, seed=0):
    """Gaussian centroids, uniform codes, Gaussian queries: real floats, distinct distances almost everywhere."""
    d, M, nbits, _ = PQ_SHAPES[shape]
    rng = np.random.default_rng([seed, d, M, nbits, n])
    return _pq_case(d, M, nbits, PG.gauss_centroids(rng, d, M, nbits), PG.random_codes(rng, n, M, nbits),
                    rng.standard_normal((nq, d)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def pq_lut(nbits, n=300, d=32, M=16, nq=9):
    """16 sub-quantizers of 2^nbits centroids over d = 32: a lookup table of 64 KB at nbits = 10 (the largest the
    scan takes) and 128 KB at 11. Gaussian centroids, uniform codes."""
    rng = np.random.default_rng([d, M, nbits, n])
    return _pq_case(d, M, nbits, PG.gauss_centroids(rng, d, M, nbits), PG.random_codes(rng, n, M, nbits),
                    rng.standard_normal((nq, d)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def pq_ties(shape, n, seed=0):
    """pq_graphs' integer centroids and tie codes: the n codes fall into 8 groups of equal codes (4 indices in
    sub-quantizer 0, 2 in sub-quantizer 1), about n / 8 each. Query 0 is zero; query 1 + g sits on group g (distance
    0), so every group is some query's nearest and holds that query's cut for any k below the group's size."""
    d, M, nbits, _ = PQ_SHAPES[shape]
    rng = np.random.default_rng([seed, d, M, nbits, n, 7])
    codes = PG.tie_codes(rng, n, M, nbits)
    groups = np.unique(codes[:, :2], axis=0)
    q = np.zeros((1 + len(groups), d), dtype=np.float32)
    q[1:, 0] = groups[:, 0] % 16  # int_centroids: centroid c is (c mod 16, 0, ...)
    q[1:, d // M] = groups[:, 1] % 16
    return _pq_case(d, M, nbits, PG.int_centroids(d, M, nbits), codes, q)


@functools.lru_cache(maxsize=None)
def pq8_big(n=N_BIG, nq=25):
    """The designed integer 8 x 8 index of the chunked cases: centroid c of every sub-quantizer is (c, 0, ..., 0),
    codes uniform over all 8 bytes, queries integers in the first dimension of every sub-vector: each distance is an
    exact integer below 2^24, and among 65,536 of them the first 1,024 hold many equal ones."""
    rng = np.random.default_rng(n)
    cen = np.zeros((8, 256, 16), dtype=np.float32)
    cen[:, :, 0] = np.arange(256, dtype=np.float32)[None, :]
    q = np.zeros((nq, 128), dtype=np.float32)
    q[:, ::16] = rng.integers(0, 256, size=(nq, 8))
    return _pq_case(128, 8, 8, cen, PG.random_codes(rng, n, 8, 8), q)


def _l2_case(base, q):
    dist = np.stack([R.l2sqr8(base, x) for x in q]) if len(base) else np.zeros((len(q), 0), np.float32)
    _frozen(base, q, dist)
    return {"base": base, "q": q, "dist": dist}


@functools.lru_cache(maxsize=None)
def l2_gauss(n, d, nq=9, seed=0):
    rng = np.random.default_rng([seed, n, d])
    return _l2_case(rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def l2_ties(n, d, groups=8, seed=0):
    """Duplicated rows: every base row is a copy of one of `groups` Gaussian rows, drawn at random, so a group holds
    about n / groups equal rows. Query 0 is Gaussian; query 1 + g is group g's row itself (distance 0)."""
    rng = np.random.default_rng([seed, n, d, groups])
    rows = rng.standard_normal((groups, d)).astype(np.float32)
    base = np.ascontiguousarray(rows[rng.integers(0, groups, size=n)])
    q = np.concatenate([rng.standard_normal((1, d)).astype(np.float32), rows])
    return _l2_case(base, np.ascontiguousarray(q))


def arranged(case, order, step):
    """The case with its base rows (codes or vectors) in `order` by query 0's distance; `dist` follows."""
    what = "codes" if "codes" in case else "base"
    items, perm = arrange(case[what], case["dist"][0], order, step)
    out = dict(case)
    out[what] = items
    out["dist"] = np.ascontiguousarray(case["dist"][:, perm])
    _frozen(out[what], out["dist"])
    return out


# the arrival-order inputs, one per scan kernel: 8,192 rows in one slice
ORDER_INPUTS = {"pq8": lambda: pq_gauss("8x8", N_ORDER), "pq": lambda: pq_gauss("8x6", N_ORDER),
                "l2": lambda: l2_gauss(N_ORDER, 16)}
# the tie inputs: equal distances everywhere, rows descending by query 0
TIE_INPUTS = {"pq8": lambda: pq_ties("8x8", N_ORDER), "pq": lambda: pq_ties("8x5", N_ORDER),
              "l2": lambda: l2_ties(N_ORDER, 32)}
TIE_SLICE_ROWS = (N_ORDER // 2, N_ORDER // 64)  # 2 and 64 slices


@functools.lru_cache(maxsize=None)
def order_case(kind, order):
    return arranged(ORDER_INPUTS[kind](), order, STEP[kind])


@functools.lru_cache(maxsize=None)
def tie_case(kind):
    return arranged(TIE_INPUTS[kind](), "descending", STEP[kind])


def tie_ks(dist, at_least=(70, 700), kmax=1024):
    """Per entry of `at_least` the first k >= it at which query 0's k-th and (k + 1)-th smallest distances are
    equal: the cut falls inside a group of equal distances and is decided by id."""
    srt = np.sort(dist[0])
    out = []
    for lo in at_least:
        k = next(k for k in range(lo, kmax + 1) if srt[k - 1] == srt[k])
        out.append(k)
    return out


# ------------------------------------------------------------------------------------------ flat handles
def write_flat_shuffled(path, built_path, seed=0):
    """A builder-made hnswlib file rewritten with hnswlib_graphs.scaled_labels (64-bit, in no order). Returns the
    parsed file."""
    from oracle import hnswlib_file
    fx = hnswlib_file.read(built_path)
    fx["labels"] = HG.scaled_labels(np.random.default_rng(seed), fx["n"])
    HG.rewrite(fx, str(path))
    return hnswlib_file.read(str(path))


def write_flat_empty(path, d=16):
    """An hnswlib file of no elements, as hnswlib writes it (entry point 2^32 - 1, maxlevel -1)."""
    g = HG.tiny_graph(np.random.default_rng(0), 0, d, 4, 8)
    g["ep"] = 0xFFFFFFFF
    return HG.write_hnswlib(str(path), **dict(g, maxlevel=-1))
