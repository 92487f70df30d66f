"""Mapping-quality rate probe: drm_hit_mapq_device and drm_pair_mapq_device on --pairs synthetic
read pairs at k = 128 and at k = 1024, beside the SW rerank (drm_post_process_sw_static_device) of the same 2 x --pairs
reads at k = 128, whose device outputs the k = 128 kernels consume unchanged, and drm_pair_hits_device on the same
lists. HIP events, warm, median of --runs runs, the timed functions taking turns run by run. Before timing, a sample
of the k = 128 records is checked against the Python restatement of the definition (tests/mapq_ref.py).

The inputs are tools/scripts/pair_bench.py's: error-free 150-base mates of fragments of 200..500 bases with their true
window among 127 random candidates; the k = 1024 lists are random windows of a 200 kb genome on both strands with
random scores. The worst case of the locus scan is timed beside them: --worst reads whose k rows are k singleton loci
of one score, so that the scan takes k iterations."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mapq_ref  # noqa: E402
import pair_ref  # noqa: E402
from deepreadmapper_amd import (MAPQ_RESULT_DTYPE, PAIR_MAPQ_RESULT_DTYPE, PAIR_RESULT_DTYPE, WindowTable,  # noqa: E402
                                hit_mapq_device, pair_hits_device, pair_mapq_device, synth)
from deepreadmapper_amd._native import check, lib  # noqa: E402
from deepreadmapper_amd.device import DeviceBuffer, Event, Stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=65_536)
ap.add_argument("--runs", type=int, default=11)
ap.add_argument("--genome", type=int, default=200_000)
ap.add_argument("--worst", type=int, default=8_192)
a = ap.parse_args()
NP, K, K2, REF_LEN = a.pairs, 128, 1024, 150
NQ = 2 * NP

rng = np.random.default_rng(1)
g = synth.genome(a.genome, seed=3)
table = WindowTable(synth.windows_lookup(g, REF_LEN, 1))
n_win = 2 * (a.genome - REF_LEN + 1)
start = rng.integers(0, a.genome - 500, size=NP)
tlen = rng.integers(200, 501, size=NP)
reads = np.empty((NQ, REF_LEN), np.uint8)
truth = np.empty(NQ, np.int64)
for p in range(NP):
    e = start[p] + tlen[p]
    reads[2 * p] = g[start[p]:start[p] + REF_LEN]
    reads[2 * p + 1] = synth.revcomp(g[e - REF_LEN:e])
    truth[2 * p], truth[2 * p + 1] = 2 * start[p], 2 * (e - REF_LEN) + 1
q = synth.tag(reads)
nb = rng.integers(0, n_win, size=(NQ, K)).astype(np.int64)
nb[np.arange(NQ), rng.integers(0, K, size=NQ)] = truth

st = Stream()
d_q = DeviceBuffer.from_host(q)
d_ql = DeviceBuffer.from_host(np.full(NQ, q.shape[1], dtype=np.int32))
d_nb = DeviceBuffer.from_host(nb)
d_full = DeviceBuffer.from_host(np.full(NQ, REF_LEN, dtype=np.int32))
d_sc, d_ids, d_st = DeviceBuffer((NQ, K), np.int32), DeviceBuffer((NQ, K), np.uint64), DeviceBuffer(NQ, np.int32)
d_ids2 = DeviceBuffer.from_host(rng.integers(0, n_win, size=(NQ, K2)).astype(np.uint64))
d_sc2 = DeviceBuffer.from_host(rng.integers(1, REF_LEN + 1, size=(NQ, K2)).astype(np.int32))
d_st2 = DeviceBuffer.from_host(np.full(NQ, K2, dtype=np.int32))
d_pairs, d_pairs2 = DeviceBuffer((NP,), PAIR_RESULT_DTYPE), DeviceBuffer((NP,), PAIR_RESULT_DTYPE)
d_hit, d_hit2 = DeviceBuffer((NQ,), MAPQ_RESULT_DTYPE), DeviceBuffer((NQ,), MAPQ_RESULT_DTYPE)
d_pq, d_pq2 = DeviceBuffer((NP,), PAIR_MAPQ_RESULT_DTYPE), DeviceBuffer((NP,), PAIR_MAPQ_RESULT_DTYPE)
# the scan's worst case: k singleton loci (200 bases apart) of one score
NW = a.worst
worst = {}
for k in (K, K2):
    ids = np.broadcast_to((2 * 200 * np.arange(k)).astype(np.uint64), (NW, k)).copy()
    worst[k] = (DeviceBuffer.from_host(ids), DeviceBuffer.from_host(np.full((NW, k), 77, np.int32)),
                DeviceBuffer.from_host(np.full(NW, k, np.int32)), DeviceBuffer((NW,), MAPQ_RESULT_DTYPE))


def rerank():
    check(lib().drm_post_process_sw_static_device(table.handle, d_nb.ptr, NQ, K, d_q.ptr, d_ql.ptr, q.shape[1], 1, K, K,
                                                  d_sc.ptr, d_ids.ptr, d_st.ptr, st.handle))


def hit(d_i, d_s, d_c, n, k, out):
    return lambda: hit_mapq_device(d_i, d_s, d_c, d_full, n, k, REF_LEN, d_out=out, stream=st)


def pair(d_i, d_s, d_c, k, out):
    return lambda: pair_hits_device(d_i, d_s, d_c, d_i.ptr + 8 * k, d_s.ptr + 4 * k, d_c.ptr + 4, NP, k, REF_LEN,
                                    row_step=2, d_out=out, stream=st)


def pmapq(d_i, d_s, d_c, k, d_p, out):
    return lambda: pair_mapq_device(d_i, d_s, d_c, d_i.ptr + 8 * k, d_s.ptr + 4 * k, d_c.ptr + 4, d_full,
                                    d_full.ptr + 4, d_p, NP, k, REF_LEN, row_step=2, d_out=out, stream=st)


jobs = [(f"SW rerank, {NQ} reads x {K} candidates", rerank),
        (f"hit_mapq, {NQ} reads, k = {K}, on the rerank's outputs", hit(d_ids, d_sc, d_st, NQ, K, d_hit)),
        (f"pair_hits, {NP} pairs, k = {K}", pair(d_ids, d_sc, d_st, K, d_pairs)),
        (f"pair_mapq, {NP} pairs, k = {K}", pmapq(d_ids, d_sc, d_st, K, d_pairs, d_pq)),
        (f"hit_mapq, {NQ} reads, k = {K2}", hit(d_ids2, d_sc2, d_st2, NQ, K2, d_hit2)),
        (f"pair_hits, {NP} pairs, k = {K2}", pair(d_ids2, d_sc2, d_st2, K2, d_pairs2)),
        (f"pair_mapq, {NP} pairs, k = {K2}", pmapq(d_ids2, d_sc2, d_st2, K2, d_pairs2, d_pq2)),
        (f"hit_mapq worst case, {NW} reads of {K} singleton loci", hit(*worst[K][:3], NW, K, worst[K][3])),
        (f"hit_mapq worst case, {NW} reads of {K2} singleton loci", hit(*worst[K2][:3], NW, K2, worst[K2][3]))]
for _, f in jobs:
    f()
st.synchronize()
hits, pairs, pq = d_hit.download(), d_pairs.download(), d_pq.download()
ids, sc, cnt = d_ids.download(), d_sc.download(), d_st.download()
full = np.full(NQ, REF_LEN, np.int32)
sample = np.unique(np.concatenate([np.arange(min(NP, 64)), rng.integers(0, NP, size=64)]))
for p in sample:
    for r in (2 * p, 2 * p + 1):
        want = mapq_ref.hit_one(ids[r], sc[r], cnt[r], -1, REF_LEN, REF_LEN, 39, 2)
        assert {f: int(hits[f][r]) for f in mapq_ref.FIELDS} == want, (r, hits[r], want)
    want = mapq_ref.pair_one(ids[2 * p], sc[2 * p], cnt[2 * p], ids[2 * p + 1], sc[2 * p + 1], cnt[2 * p + 1], REF_LEN,
                             REF_LEN, {f: int(pairs[f][p]) for f in pair_ref.FIELDS}, REF_LEN, 0, 1000, 17, REF_LEN, 39, 2)
    assert {f: int(pq[f][p]) for f in mapq_ref.PAIR_FIELDS} == want, (p, pq[p], want)
for k in (K, K2):
    w = worst[k][3].download()
    assert (w["n_sub"] == k - 1).all() and (w["mapq"] == 0).all()
h2 = d_hit2.download()
print(f"{NP} pairs, k = {K}: mean n_sub {hits['n_sub'].mean():.2f}, mean locus_rows {hits['locus_rows'].mean():.2f}, "
      f"MAPQ mean {hits['mapq'].mean():.1f}; pair mapq1 mean {pq['mapq1'].mean():.1f}; {len(sample)} pairs equal the "
      f"restatement. k = {K2}: mean n_sub {h2['n_sub'].mean():.2f} (scan iterations per read)", flush=True)

ts = [[] for _ in jobs]
for _ in range(a.runs):
    for x, (_, f) in enumerate(jobs):
        e0, e1 = Event(), Event()
        e0.record(st)
        f()
        e1.record(st)
        st.synchronize()
        ts[x].append(e0.elapsed_ms(e1))
med = [statistics.median(t) for t in ts]
for (name, _), t, m in zip(jobs, ts, med):
    print(f"{name}: median {m:.3f} ms (min {min(t):.3f}, max {max(t):.3f}, {a.runs} runs)", flush=True)
print(f"k = {K}: hit_mapq / rerank {med[1] / med[0]:.4f}, pair_mapq / rerank {med[3] / med[0]:.4f}, pair_mapq / "
      f"pair_hits {med[3] / med[2]:.2f}; k = {K2}: pair_mapq / pair_hits {med[6] / med[5]:.2f}", flush=True)
