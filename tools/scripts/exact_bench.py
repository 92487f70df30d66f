"""Times the exhaustive scans (exact_scan.hip) with HIP events: the median kernel_ms of 9 runs
after a warm-up, one process at a time. Default: the C3 shape (1M windows, 1,024 sampled reads, k = 128), the PQ
scan over the index's codes and, with --fp32, the fp32 scan over the window-embedding table. --workload c5 runs the
PQ scan over the bench's 50M-code index. Prints one JSON line with each scan's bound and the fraction reached:

  PQ:   LDS lookups nq * ntotal * 8 at 32 ds_read_b32 lanes per clock per CU; code bytes
        ntotal * 8 * ceil(nq / QT) (each tile reads the stream once; tiles resident together share it in the caches)
  fp32: VALU operations nq * n_base * d * 3 (subtract, multiply, add; no FMA by definition) at 128 packed fp32
        operations per clock per CU
--cpu-ref N times tests/exact_ref.adc_topk (numpy, threads over queries) on the first N queries, for scale, and
records whether it equals the GPU scan bit for bit."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import bench  # noqa: E402
from deepreadmapper_amd import QUERY_TILE, HnswPqIndex, exact_search_l2, set_slice_rows, synth  # noqa: E402
from deepreadmapper_amd.device import device_props  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--workload", choices=["c3", "c5"], default="c3")
ap.add_argument("--queries", type=int, default=1024)
ap.add_argument("--k", type=int, default=128)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--fp32", action="store_true")
ap.add_argument("--slice-rows", type=int, default=0, help="drm_exact_set_slice_rows (0: the default split)")
ap.add_argument("--cpu-ref", type=int, default=0, metavar="N", help="time the numpy brute force on N queries")
ap.add_argument("--embed", default="gru", choices=["gru", "kmer3"], help="c5: the embedder of the bench's index")
ap.add_argument("--cache", default=bench.default_cache())
ap.add_argument("--out", default=None)
a = ap.parse_args()

if a.workload == "c3":
    w = synth.Workload("c3", 500_149, a.queries, seed=42, read_seed=7).generate(a.cache, gpu_build=True)
    index_path, q, refs = w.index_path, w.q_emb, w.refs
else:
    wl = bench.prepare_c5(argparse.Namespace(cache=a.cache, queries=a.queries, embed=a.embed), bench.Dist(), 0)
    index_path, q, refs = wl["index_path"], wl["q_emb"], wl["refs"]
q = np.ascontiguousarray(q[:a.queries])
props = device_props(0)
cus, hz = props["cu_count"], props["clock_hz"]


def median_ms(fn):
    fn()
    ts = [fn()[2] for _ in range(a.reps)]
    return float(np.median(ts)), [round(t, 4) for t in ts]


set_slice_rows(a.slice_rows)
out = {"workload": a.workload, "queries": len(q), "k": a.k, "slice_rows": a.slice_rows, "cu_count": cus, "clock_hz": hz, "query_tile": QUERY_TILE}
ix = HnswPqIndex(index_path, 0)
nt = int(ix.ntotal)
ms, all_ms = median_ms(lambda: ix.exact_search(q, a.k, with_ms=True))
D_gpu, I_gpu = ix.exact_search(q[:max(a.cpu_ref, 1)], a.k)
lds_ms = len(q) * nt * 8 / (cus * 32 * hz) * 1e3
code_bytes = nt * 8 * ((len(q) + QUERY_TILE - 1) // QUERY_TILE)
out["pq"] = {"ntotal": nt, "kernel_ms": round(ms, 4), "all_ms": all_ms, "lds_bound_ms": round(lds_ms, 4),
             "lds_frac": round(lds_ms / ms, 4), "code_bytes": code_bytes,
             "code_TBps": round(code_bytes / ms / 1e9, 3), "Gdist_per_s": round(len(q) * nt / ms / 1e6, 1)}
if a.cpu_ref:
    from concurrent.futures import ThreadPoolExecutor
    sys.path.insert(0, "tests")
    import exact_ref as R
    from oracle import faiss_file, oracle as O
    fx = faiss_file.read(index_path)
    s = O.make_index(fx)
    codes = fx.codes.reshape(fx.ntotal, -1)
    threads = min(16, os.cpu_count() or 1)
    t0 = time.time()
    with ThreadPoolExecutor(threads) as ex:
        ref = list(ex.map(lambda i: R.adc_topk(lambda v: O.pq_distance_table(s, v), codes, q[i:i + 1], a.k),
                          range(a.cpu_ref)))
    dt = time.time() - t0
    same = all(np.array_equal(r[0][0].view(np.uint32), D_gpu[i].view(np.uint32)) and np.array_equal(r[1][0], I_gpu[i])
               for i, r in enumerate(ref))
    out["cpu_ref"] = {"queries": a.cpu_ref, "threads": threads, "seconds": round(dt, 3), "equals_gpu_scan": bool(same),
                      "ms_per_1024_queries": round(dt / a.cpu_ref * 1024 * 1e3, 1)}
ix.free()
if a.fp32:
    x = synth.embed(synth.tag(np.asarray(refs)))
    ms, all_ms = median_ms(lambda: exact_search_l2(x, q, a.k, with_ms=True))
    valu_ms = len(q) * len(x) * x.shape[1] * 3 / (cus * 128 * hz) * 1e3
    out["fp32"] = {"n_base": len(x), "d": int(x.shape[1]), "kernel_ms": round(ms, 4), "all_ms": all_ms,
                   "valu_bound_ms": round(valu_ms, 4), "valu_frac": round(valu_ms / ms, 4),
                   "base_bytes": int(x.nbytes)}
line = json.dumps(out)
print(line, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
