"""Mate-pairing rate probe: drm_pair_hits_device on --pairs synthetic read pairs at k = 128 and
at k = 1024, beside the SW rerank (drm_post_process_sw_static_device) of the same 2 x --pairs reads at k = 128, whose
device outputs the k = 128 pairing consumes unchanged (row_step 2). HIP events, warm, median of --runs runs, the timed
functions taking turns run by run. Before timing, a sample of the k = 128 records is checked against the Python
restatement of the definition (tests/pair_ref.py).

The reads are error-free 150-base mates of fragments of 200..500 bases (mate 1 forward, mate 2 the reverse
complement of the fragment's end) with their true window among 127 random candidates; the k = 1024 lists are random
windows of a 200 kb genome on both strands with random scores (nothing reranks 1024 candidates of 131,072 reads in
a probe's time), so most of their 2^20 combinations fail the strand or the distance test, as real lists do."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pair_ref  # noqa: E402
from deepreadmapper_amd import PAIR_RESULT_DTYPE, WindowTable, pair_hits_device, synth  # noqa: E402
from deepreadmapper_amd._native import check, lib  # noqa: E402
from deepreadmapper_amd.device import DeviceBuffer, Event, Stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=65_536)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--genome", type=int, default=200_000)
a = ap.parse_args()
NP, K, REF_LEN = a.pairs, 128, 150
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
d_sc, d_ids, d_st = DeviceBuffer((NQ, K), np.int32), DeviceBuffer((NQ, K), np.uint64), DeviceBuffer(NQ, np.int32)
d_out = DeviceBuffer((NP,), PAIR_RESULT_DTYPE)
K2 = 1024
d_ids2 = DeviceBuffer.from_host(rng.integers(0, n_win, size=(NQ, K2)).astype(np.uint64))
d_sc2 = DeviceBuffer.from_host(rng.integers(1, REF_LEN + 1, size=(NQ, K2)).astype(np.int32))
d_st2 = DeviceBuffer.from_host(np.full(NQ, K2, dtype=np.int32))
d_out2 = DeviceBuffer((NP,), PAIR_RESULT_DTYPE)


def rerank():
    check(lib().drm_post_process_sw_static_device(table.handle, d_nb.ptr, NQ, K, d_q.ptr, d_ql.ptr, q.shape[1], 1, K, K,
                                                  d_sc.ptr, d_ids.ptr, d_st.ptr, st.handle))


def pair(d_i, d_s, d_c, k, out):
    def f():
        pair_hits_device(d_i, d_s, d_c, d_i.ptr + 8 * k, d_s.ptr + 4 * k, d_c.ptr + 4, NP, k, REF_LEN, row_step=2,
                         d_out=out, stream=st)
    return f


pair128, pair1024 = pair(d_ids, d_sc, d_st, K, d_out), pair(d_ids2, d_sc2, d_st2, K2, d_out2)
rerank()
pair128()
st.synchronize()
res, ids, sc, cnt = d_out.download(), d_ids.download(), d_sc.download(), d_st.download()
sample = np.unique(np.concatenate([np.arange(min(NP, 64)), rng.integers(0, NP, size=64)]))
for p in sample:
    want = pair_ref.pair_one(ids[2 * p], sc[2 * p], cnt[2 * p], ids[2 * p + 1], sc[2 * p + 1], cnt[2 * p + 1], REF_LEN)
    assert {f: int(res[f][p]) for f in pair_ref.FIELDS} == want, (p, res[p], want)
proper = res["status"] == 0
assert (res["tlen"][proper] == tlen[proper]).mean() > 0.99, "the chosen pairs are not the simulated fragments"
print(f"{NP} pairs, k = {K}: {int(proper.sum())} proper (status 0), mean n_proper {res['n_proper'].mean():.2f}; "
      f"{len(sample)} records equal the restatement", flush=True)

jobs = [(f"SW rerank, {NQ} reads x {K} candidates", rerank), (f"pair_hits, {NP} pairs, k = {K}", pair128),
        (f"pair_hits, {NP} pairs, k = {K2}", pair1024)]
for _, f in jobs:
    f()
st.synchronize()
print(f"k = {K2}: mean n_proper {d_out2.download()['n_proper'].mean():.1f} of {K2 * K2} combinations", flush=True)
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
print(f"pairing / rerank at k = {K}: {med[1] / med[0]:.4f}; k = {K2} pairing / k = {K} rerank: {med[2] / med[0]:.3f}; "
      f"{NP * K * K / med[1] / 1e6:.1f} G combinations/s at k = {K}, {NP * K2 * K2 / med[2] / 1e6:.1f} G at k = {K2}",
      flush=True)
