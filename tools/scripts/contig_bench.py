"""Contig-stage rate probe: drm_contig_hits_device on --reads synthetic reads at k = 128, beside
the SW rerank (drm_post_process_sw_static_device) of the same reads, whose device outputs the stage consumes unchanged.
HIP events, warm, median of --runs runs, the timed functions taking turns run by run. The stage is timed on a table of
--contigs contigs (searched in LDS) and on one beyond drm_contig_lds_max() (searched in global memory). Before timing,
the outputs are checked against the plain restatement of the definition (tests/contig_ref.py).

The reads are error-free 150-base windows of a random genome with their true window among 127 random candidates. The
genome is cut into contigs of equal length with a 40-base gap in front of each but the first, so that about
(150 + 40) / contig length of the rows straddle a contig's end or touch a gap and are dropped.

The stage reads 12 bytes a row (id, score) and writes 32 (id, spread id, score, contig): its floor is 44 bytes a row at
the memory rate."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contig_ref  # noqa: E402
from deepreadmapper_amd import ContigTable, WindowTable, contig_hits_device, synth  # noqa: E402
from deepreadmapper_amd._native import check, lib  # noqa: E402
from deepreadmapper_amd.contigs import lds_max  # noqa: E402
from deepreadmapper_amd.device import DeviceBuffer, Event, Stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=131_072)
ap.add_argument("--runs", type=int, default=11)
ap.add_argument("--genome", type=int, default=200_000)
ap.add_argument("--contigs", type=int, default=25)
ap.add_argument("--hbm-gbs", type=float, default=6300.0, help="the memory rate the floor is computed with")
a = ap.parse_args()
NQ, K, REF_LEN, GAP = a.reads, 128, 150, 40

rng = np.random.default_rng(1)
g = synth.genome(a.genome, seed=3)
table = WindowTable(synth.windows_lookup(g, REF_LEN, 1))
n_win = 2 * (a.genome - REF_LEN + 1)
start = rng.integers(0, a.genome - REF_LEN, size=NQ)
reads = np.stack([g[s:s + REF_LEN] for s in start])
q = synth.tag(reads)
nb = rng.integers(0, n_win, size=(NQ, K)).astype(np.int64)
nb[np.arange(NQ), rng.integers(0, K, size=NQ)] = 2 * start


def contigs(n):
    """n contigs of equal length over the genome, a GAP-base gap in front of each but the first"""
    step = a.genome // n
    starts = np.arange(n, dtype=np.int64) * step
    starts[1:] += GAP
    lens = np.full(n, step, np.int64)
    lens[1:] -= GAP
    return ContigTable(starts, lens)


tables = [(f"{a.contigs} contigs (LDS)", contigs(a.contigs)),
          (f"{lds_max() + 1} contigs (global memory)", contigs(lds_max() + 1))]
st = Stream()
d_q = DeviceBuffer.from_host(q)
d_ql = DeviceBuffer.from_host(np.full(NQ, q.shape[1], dtype=np.int32))
d_nb = DeviceBuffer.from_host(nb)
d_sc, d_ids, d_st = DeviceBuffer((NQ, K), np.int32), DeviceBuffer((NQ, K), np.uint64), DeviceBuffer(NQ, np.int32)
d_out = (DeviceBuffer((NQ, K), np.uint64), DeviceBuffer((NQ, K), np.uint64), DeviceBuffer((NQ, K), np.int32),
         DeviceBuffer((NQ, K), np.int32), DeviceBuffer((NQ,), np.int32))


def rerank():
    check(lib().drm_post_process_sw_static_device(table.handle, d_nb.ptr, NQ, K, d_q.ptr, d_ql.ptr, q.shape[1], 1, K, K,
                                                  d_sc.ptr, d_ids.ptr, d_st.ptr, st.handle))


def stage(t):
    return lambda: contig_hits_device(t, d_ids, d_sc, d_st, NQ, K, REF_LEN, d_out=d_out, stream=st)


jobs = [(f"SW rerank, {NQ} reads x {K} candidates", rerank)]
jobs += [(f"contig_hits, {NQ} reads, k = {K}, {name}, on the rerank's outputs", stage(t)) for name, t in tables]
rerank()
st.synchronize()
ids, sc, cnt = d_ids.download(), d_sc.download(), d_st.download()
for name, t in tables:
    stage(t)()
    st.synchronize()
    want = contig_ref.contig_hits(t.starts, t.lens, ids, sc, cnt, REF_LEN)
    for b, w in zip(d_out, want):
        assert np.array_equal(b.download(), w), name
    print(f"{name}: {int(want[4].sum())} of {int(np.clip(cnt, 0, K).sum())} rows kept; equal to the restatement",
          flush=True)

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
floor = 44.0 * NQ * K / (a.hbm_gbs * 1e6)
for x in (1, 2):
    print(f"{jobs[x][0].split(', on')[0]}: {med[x] / med[0]:.4f} of the rerank; 44 B x {NQ * K} rows at "
          f"{a.hbm_gbs:.0f} GB/s = {floor:.3f} ms, measured / floor {med[x] / floor:.2f}", flush=True)
