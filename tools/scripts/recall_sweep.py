"""recall@k of the HNSW-PQ graph search against the exhaustive PQ-ADC scan on a
synth.Workload. Default: the C3 shape (1M windows, 1,024 sampled reads), on the host-built and the GPU-built IHNp
index (built here if absent); --workload c5 runs the bench's GPU-built 50M-code index. Per index: one scan at
k = 128, then drm_search at ef in {16, 32, 64, 128, 256} for k in {1, 10, 128} (as in faiss the candidate heap holds
max(ef, k) entries, a row's `heap`, while the level-0 walk still stops after ef steps), each with id_recall,
dist_recall, mean ndis and nhops. --fp32 (C3) also scans the window
embeddings in fp32 and reports the PQ loss: the id recall of the exhaustive ADC top-k against the exact fp32 top-k.
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
import bench  # noqa: E402
from deepreadmapper_amd import HnswPqIndex, exact_search_l2, recall_at_k, synth  # noqa: E402

EFS = (16, 32, 64, 128, 256)
KS = (1, 10, 128)

ap = argparse.ArgumentParser()
ap.add_argument("--workload", choices=["c3", "c5"], default="c3")
ap.add_argument("--queries", type=int, default=1024)
ap.add_argument("--builders", default="host,gpu", help="C3: which builders' indexes to sweep")
ap.add_argument("--fp32", action="store_true")
ap.add_argument("--build-threads", type=int, default=0)
ap.add_argument("--embed", default="gru", choices=["gru", "kmer3"], help="c5: the embedder of the bench's index")
ap.add_argument("--cache", default=bench.default_cache())
ap.add_argument("--out", default=None)
a = ap.parse_args()

indexes, refs = {}, None
if a.workload == "c3":
    for b in a.builders.split(","):
        w = synth.Workload("c3", 500_149, a.queries, seed=42, read_seed=7)
        w.generate(a.cache, nthreads=a.build_threads, log=bench.log, gpu_build=(b == "gpu"))
        indexes[b] = w.index_path
        q, refs = w.q_emb, w.refs
else:
    wl = bench.prepare_c5(argparse.Namespace(cache=a.cache, queries=a.queries, embed=a.embed), bench.Dist(), 0)
    indexes["gpu"], q = wl["index_path"], wl["q_emb"]
q = np.ascontiguousarray(q[:a.queries])

out = {"workload": a.workload, "queries": len(q), "indexes": {}}
exact = {}
for name, path in indexes.items():
    ix = HnswPqIndex(path, 0)
    De, Ie, scan_ms = ix.exact_search(q, 128, with_ms=True)
    exact[name] = (De, Ie)
    rows = []
    for ef in EFS:
        for k in KS:
            D, I, st = ix.search(q, k, ef)
            r = recall_at_k(D, I, De, Ie, k=k)
            rows.append({"ef": ef, "heap": max(ef, k), "k": k, "id_recall": round(r["id_recall"], 5),
                         "dist_recall": round(r["dist_recall"], 5), "ndis": round(st.ndis / len(q), 1),
                         "nhops": round(st.nhops / len(q), 1), "kernel_ms": round(st.kernel_ms, 3)})
    out["indexes"][name] = {"path": os.path.basename(path), "ntotal": int(ix.ntotal),
                            "scan_kernel_ms": round(scan_ms, 3), "rows": rows}
    ix.free()
if a.fp32 and refs is not None:
    x = synth.embed(synth.tag(refs))
    Df, If, l2_ms = exact_search_l2(x, q, 128, with_ms=True)
    out["fp32_scan_kernel_ms"] = round(l2_ms, 3)
    for name, (De, Ie) in exact.items():
        out["indexes"][name]["pq_loss_id_recall"] = {
            str(k): round(recall_at_k(De, Ie, Df, If, k=k)["id_recall"], 5) for k in KS}
line = json.dumps(out)
print(line, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
