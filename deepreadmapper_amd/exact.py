"""Exhaustive k-nearest-neighbour scans on the GPU and recall@k of an approximate search against them.

`HnswPqIndex.exact_search` scores every PQ code of a loaded index, `HnswFlatIndex.exact_search` and
`exact_search_l2` every row of an fp32 matrix (include/drm_hip.h). The distances carry the bits
the graph searches report for the same pair, so an approximate result can be compared with the exact one by value."""
import ctypes as C

import numpy as np

from ._native import DRM_ERR_ARG, DrmError, check, lib, ptr
from .device import DeviceBuffer

QUERY_TILE = 8  # drm_exact_query_tile(): queries per workgroup of the PQ 8x8 scan
K_MAX = 1024


def set_slice_rows(rows):
    """drm_exact_set_slice_rows: base rows per slice of the scans' grid (0 = default). Results do not depend on it."""
    check(lib().drm_exact_set_slice_rows(int(rows)))


SCAN_KINDS = {"pq8": 0, "pq": 1, "l2": 2}  # drm_debug_exact_plan's `kind`
PLAN_FIELDS = ("qt", "step", "cap", "slice_rows", "slices", "chunk", "chunks")


def scan_plan(kind, n, n_base, k):
    """drm_debug_exact_plan: the plan a scan of `kind` ("pq8": PQ 8x8 with aligned queries, "pq": any other PQ scan,
    "l2": fp32) of n queries over n_base rows at k would run with under the current slice rows, as a dict of
    PLAN_FIELDS. From the function the scans use; launches nothing."""
    out = (C.c_int64 * 7)()
    check(lib().drm_debug_exact_plan(SCAN_KINDS[kind], int(n), int(n_base), int(k), out))
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def _queries(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("queries must be [n, d]")
    return x


def pq_exact_search(index, x, k, with_ms=False):
    """drm_exact_search on an HnswPqIndex: D [n,k] f32 ascending, I [n,k] int64, padding (+inf, -1)."""
    x = _queries(x)
    n, d = x.shape
    k = int(k)
    D = np.empty((n, max(k, 0)), dtype=np.float32)
    I = np.empty((n, max(k, 0)), dtype=np.int64)
    ms = C.c_double(0.0)
    check(lib().drm_exact_search(index.handle, ptr(x), n, d, k, ptr(D), ptr(I), C.byref(ms)))
    return (D, I, ms.value) if with_ms else (D, I)


def pq_exact_search_device(index, d_x, n, k, d_D, d_I, stream=None):
    """drm_exact_search_device on DeviceBuffers: enqueued on `stream` and synchronised."""
    check(lib().drm_exact_search_device(index.handle, d_x.ptr, int(n), int(k), d_D.ptr, d_I.ptr,
                                        stream.handle if stream is not None else None))


def flat_exact_search(index, x, k, with_ms=False):
    """drm_flat_exact_search on an HnswFlatIndex: D [n,k] f32, labels [n,k] u64 (ties by internal id, padding
    2^64-1)."""
    x = _queries(x)
    n, d = x.shape
    k = int(k)
    D = np.empty((n, max(k, 0)), dtype=np.float32)
    L = np.empty((n, max(k, 0)), dtype=np.uint64)
    ms = C.c_double(0.0)
    check(lib().drm_flat_exact_search(index.handle, ptr(x), n, d, k, ptr(D), ptr(L), C.byref(ms)))
    return (D, L, ms.value) if with_ms else (D, L)


def exact_search_l2(base, x, k, stream=None, with_ms=False):
    """The k nearest rows of `base` [n_base, d] for every row of `x` [n, d] under squared L2 in the flat search's
    summation order; ties by row number. numpy arrays (host entry point) or DeviceBuffers of float32 (device entry
    point, on `stream`). Returns (D [n,k] f32, I [n,k] int64), padding (+inf, -1)."""
    k = int(k)
    if isinstance(base, DeviceBuffer) or isinstance(x, DeviceBuffer):
        if not (isinstance(base, DeviceBuffer) and isinstance(x, DeviceBuffer)):
            raise ValueError("base and x must both be DeviceBuffers or both be arrays")
        (nb, d), (n, dx) = base.shape, x.shape
        if d != dx:
            raise DrmError(DRM_ERR_ARG, f"query dimension {dx} != base dimension {d}")
        d_D, d_I = DeviceBuffer((n, max(k, 0)), np.float32), DeviceBuffer((n, max(k, 0)), np.int64)
        try:
            check(lib().drm_exact_search_l2_device(base.ptr, nb, d, x.ptr, n, k, d_D.ptr, d_I.ptr,
                                                   stream.handle if stream is not None else None))
            return d_D.download(), d_I.download()
        finally:
            d_D.free()
            d_I.free()
    base = np.ascontiguousarray(base, dtype=np.float32)
    x = _queries(x)
    if base.ndim != 2:
        raise ValueError("base must be [n_base, d]")
    if base.shape[1] != x.shape[1]:
        raise DrmError(DRM_ERR_ARG, f"query dimension {x.shape[1]} != base dimension {base.shape[1]}")
    n, d = x.shape
    D = np.empty((n, max(k, 0)), dtype=np.float32)
    I = np.empty((n, max(k, 0)), dtype=np.int64)
    ms = C.c_double(0.0)
    check(lib().drm_exact_search_l2(ptr(base), base.shape[0], d, ptr(x), n, k, ptr(D), ptr(I), C.byref(ms)))
    return (D, I, ms.value) if with_ms else (D, I)


def recall_at_k(D_ann, I_ann, D_exact, I_exact, k=None):
    """Recall of an approximate result against the exact one, over the first k columns (default: the narrower of
    the two widths). Pure numpy. Per query:

      id_recall   = |I_ann[:k] & I_exact[:k]| / min(k, valid)   valid = exact rows that are not padding
      dist_recall = #{j < k : D_ann[j] <= D_exact[k-1]} / k

    dist_recall is robust to ties at the k-th distance (any member of the tie group counts), which is the figure to
    report where the two sides break ties differently; it needs both sides' distances to be bit-identical for the
    same pair, as the scans guarantee. Padded slots (id -1 or 2^64-1, distance +inf) never count as hits. A query
    whose exact result is all padding has id_recall 1.0. Returns a dict with the means `id_recall`, `dist_recall`
    and the per-query arrays `id_recall_per_query`, `dist_recall_per_query`."""
    D_ann, D_exact = np.asarray(D_ann, dtype=np.float32), np.asarray(D_exact, dtype=np.float32)
    I_ann, I_exact = np.asarray(I_ann), np.asarray(I_exact)
    if D_ann.ndim != 2 or D_ann.shape != I_ann.shape or D_exact.shape != I_exact.shape or \
            D_ann.shape[0] != D_exact.shape[0]:
        raise ValueError("D/I must be [n, width] with one row per query on both sides")
    width = min(D_ann.shape[1], D_exact.shape[1])
    k = width if k is None else int(k)
    if not 1 <= k <= width:
        raise ValueError(f"k = {k} outside [1, {width}]")
    n = D_ann.shape[0]
    # ids as int64 with one padding value (-1) on both sides: uint64 2^64-1 wraps to -1
    Ia = I_ann[:, :k].astype(np.int64, copy=True)
    Ie = I_exact[:, :k].astype(np.int64, copy=True)
    Da, De = D_ann[:, :k], D_exact[:, :k]
    pad_a = (Ia == -1) | np.isinf(Da)
    pad_e = (Ie == -1) | np.isinf(De)
    id_rec = np.ones(n, dtype=np.float64)
    for i in range(n):
        valid = int((~pad_e[i]).sum())
        if valid:
            hits = np.intersect1d(Ia[i][~pad_a[i]], Ie[i][~pad_e[i]]).size
            id_rec[i] = hits / min(k, valid)
    dist_rec = ((Da <= De[:, k - 1:k]) & ~pad_a).sum(axis=1) / float(k)
    return {"k": k, "id_recall": float(id_rec.mean()) if n else 1.0,
            "dist_recall": float(dist_rec.mean()) if n else 1.0,
            "id_recall_per_query": id_rec, "dist_recall_per_query": dist_rec}
