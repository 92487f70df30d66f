"""Template-length rate probe: drm_tlen_scan_device on --pairs synthetic read pairs at k = 128 and
at k = 1024, beside drm_hit_mapq_device over the same 2 x --pairs lists (the scan does what two of its scans do, plus
one atomic) and beside the SW rerank (drm_post_process_sw_static_device) of those reads at k = 128, whose device outputs
the k = 128 kernels consume unchanged. Then the feature's payoff: drm_mate_rescue_device over --rescue tasks of a
simulated 300 +- 30 library with the default window 0,1000 and with the window drm_tlen_estimate reads off that
library's histogram. HIP events, warm, median of --runs runs, the timed functions taking turns run by run. Before
timing, a sample of the k = 128 records and the whole histogram's total are checked against the Python restatement
(tests/tlen_ref.py), and every rescue must find its mate in both windows.

The inputs are tools/scripts/mapq_bench.py's: error-free 150-base mates of fragments of 200..500 bases with their true
window among 127 random candidates; the k = 1024 lists are random windows of a 200 kb genome on both strands with
random scores."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tlen_ref  # noqa: E402
from deepreadmapper_amd import (MAPQ_RESULT_DTYPE, RESCUE_RESULT_DTYPE, TLEN_SAMPLE_DTYPE, GenomeTable,  # noqa: E402
                                WindowTable, hit_mapq_device, mate_rescue_device, synth, tlen_estimate,
                                tlen_scan_device)
from deepreadmapper_amd._native import check, lib  # noqa: E402
from deepreadmapper_amd.device import DeviceBuffer, Event, Stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=65_536)
ap.add_argument("--runs", type=int, default=11)
ap.add_argument("--genome", type=int, default=200_000)
ap.add_argument("--rescue", type=int, default=16_384)
a = ap.parse_args()
NP, K, K2, REF_LEN, MAX_SCAN = a.pairs, 128, 1024, 150, 10_000
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
d_hit, d_hit2 = DeviceBuffer((NQ,), MAPQ_RESULT_DTYPE), DeviceBuffer((NQ,), MAPQ_RESULT_DTYPE)
d_smp, d_smp2 = DeviceBuffer((NP,), TLEN_SAMPLE_DTYPE), DeviceBuffer((NP,), TLEN_SAMPLE_DTYPE)
zero = np.zeros((3, MAX_SCAN + 1), np.uint32)
d_hist, d_hist2 = DeviceBuffer.from_host(zero), DeviceBuffer.from_host(zero)

# the rescue's tasks: a 300 +- 30 library, mate 2 aligned over the window of mate 1's forward hit
NR = a.rescue
r_tlen = np.clip(np.rint(rng.normal(300, 30, size=NR)).astype(np.int64), REF_LEN, 1000)
r_start = rng.integers(0, a.genome - 1000, size=NR)
r_reads = np.stack([synth.revcomp(g[s + t - REF_LEN:s + t]) for s, t in zip(r_start, r_tlen)])
r_q = synth.tag(r_reads)
est = tlen_estimate(np.bincount(r_tlen, minlength=MAX_SCAN + 1).astype(np.uint32))
assert est["status"] == 0 and est["low"] <= r_tlen.min() and r_tlen.max() <= est["high"], est
genome = GenomeTable(g, REF_LEN)
d_anchor = DeviceBuffer.from_host((2 * r_start).astype(np.uint64))
d_tq = DeviceBuffer.from_host(np.arange(NR, dtype=np.int64))
d_rq = DeviceBuffer.from_host(r_q)
d_rql = DeviceBuffer.from_host(np.full(NR, r_q.shape[1], dtype=np.int32))
d_res = {w: DeviceBuffer((NR,), RESCUE_RESULT_DTYPE) for w in ("default", "estimated")}
windows = {"default": (0, 1000), "estimated": (est["low"], est["high"])}


def rerank():
    check(lib().drm_post_process_sw_static_device(table.handle, d_nb.ptr, NQ, K, d_q.ptr, d_ql.ptr, q.shape[1], 1, K, K,
                                                  d_sc.ptr, d_ids.ptr, d_st.ptr, st.handle))


def hit(d_i, d_s, d_c, k, out):
    return lambda: hit_mapq_device(d_i, d_s, d_c, d_full, NQ, k, REF_LEN, d_out=out, stream=st)


def scan(d_i, d_s, d_c, k, d_h, out):
    return lambda: tlen_scan_device(d_i, d_s, d_c, d_i.ptr + 8 * k, d_s.ptr + 4 * k, d_c.ptr + 4, d_full, d_full.ptr + 4,
                                    NP, k, REF_LEN, d_h, max_scan=MAX_SCAN, row_step=2, d_samples=out, stream=st)


def rescue(which):
    lo, hi = windows[which]
    return lambda: mate_rescue_device(genome, d_anchor, d_tq, NR, d_rq, d_rql, r_q.shape[1], NR, min_tlen=lo,
                                      max_tlen=hi, d_out=d_res[which], stream=st)


jobs = [(f"SW rerank, {NQ} reads x {K} candidates", rerank),
        (f"hit_mapq, {NQ} reads, k = {K}, on the rerank's outputs", hit(d_ids, d_sc, d_st, K, d_hit)),
        (f"tlen_scan, {NP} pairs, k = {K}, on the rerank's outputs", scan(d_ids, d_sc, d_st, K, d_hist, d_smp)),
        (f"hit_mapq, {NQ} reads, k = {K2}", hit(d_ids2, d_sc2, d_st2, K2, d_hit2)),
        (f"tlen_scan, {NP} pairs, k = {K2}", scan(d_ids2, d_sc2, d_st2, K2, d_hist2, d_smp2)),
        (f"mate_rescue, {NR} tasks, window 0,1000", rescue("default")),
        (f"mate_rescue, {NR} tasks, estimated window {est['low']},{est['high']}", rescue("estimated"))]
for _, f in jobs:
    f()
st.synchronize()
smp, hist = d_smp.download(), d_hist.download()
ids, sc, cnt = d_ids.download(), d_sc.download(), d_st.download()
sample = np.unique(np.concatenate([np.arange(min(NP, 64)), rng.integers(0, NP, size=64)]))
for p in sample:
    want = tlen_ref.scan_one(ids[2 * p], sc[2 * p], cnt[2 * p], ids[2 * p + 1], sc[2 * p + 1], cnt[2 * p + 1], REF_LEN,
                             REF_LEN, REF_LEN, 20, MAX_SCAN, REF_LEN, 39, 2)
    assert {f: int(smp[f][p]) for f in tlen_ref.SAMPLE_FIELDS} == want, (p, smp[p], want)
placed = (smp["cls"] >= 1) & (smp["cls"] <= 3)
assert int(hist.sum(dtype=np.int64)) == int(placed.sum())
fr = smp["cls"] == 1
assert (smp["tlen"][fr] == tlen[fr]).all()  # error-free reads: a sampled pair's T is its fragment's length
for which, d in d_res.items():
    res = d.download()
    assert (res["status"] == 0).all() and (res["score"] == REF_LEN).all(), which
e128 = tlen_estimate(hist[0])
smp2 = d_smp2.download()
print(f"{NP} pairs, k = {K}: classes 0..4 {np.bincount(smp['cls'], minlength=5).tolist()}, window {e128['low']},"
      f"{e128['high']} (mean {e128['mean']}, sd {e128['sd']}) from {e128['n']} FR pairs of fragments 200..500; "
      f"{len(sample)} pairs equal the restatement. k = {K2}: classes {np.bincount(smp2['cls'], minlength=5).tolist()}. "
      f"Rescue library 300 +- 30: window {est['low']},{est['high']}", flush=True)

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
print(f"k = {K}: tlen_scan / hit_mapq {med[2] / med[1]:.2f}, tlen_scan / rerank {med[2] / med[0]:.4f}; k = {K2}: "
      f"tlen_scan / hit_mapq {med[4] / med[3]:.2f}; mate_rescue estimated / default {med[6] / med[5]:.2f}", flush=True)
