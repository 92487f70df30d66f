"""Mate-rescue rate probe: drm_mate_rescue_device on --tasks tasks of 152-byte tagged reads over
1,000-row regions (the default 0..1000 template length), each read planted in its region at a random offset with 1 %
substitutions, on either strand. Beside it, in the same process and taking turns run by run, drm_sw_align_affine_device
at flank 8 on the same reads and their true windows, and the SW rerank of the same reads at k = 128
(drm_post_process_sw_static_device, the true window among 127 random ones). HIP events, warm, median of --runs runs.

The two alignment kernels run the same recurrence, the scan without packing or storing directions, so they are
compared as time per DP step: time / (tasks x steps), steps = n + ceil(m / C) - 1 (n rows, m query bytes, C = 3
columns per lane). Before timing, every record is checked: the region has 1,000 rows, and the rescue's score equals the
affine aligner's on the true window (the planted read is the best the region holds)."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from deepreadmapper_amd import (RESCUE_RESULT_DTYPE, GenomeTable, WindowTable, mate_rescue_device,  # noqa: E402
                                mate_rescue_window, synth)
from deepreadmapper_amd._native import check, lib  # noqa: E402
from deepreadmapper_amd.device import DeviceBuffer, Event, Stream  # noqa: E402
from deepreadmapper_amd.rerank import SW_ALIGNMENT_DTYPE, sw_scoring  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tasks", type=int, default=65_536)
ap.add_argument("--runs", type=int, default=11)
ap.add_argument("--genome", type=int, default=200_000)
ap.add_argument("--scoring", default="1,1,0,1", help="match,mismatch,open,extend of both alignment kernels")
ap.add_argument("--flank", type=int, default=8)
a = ap.parse_args()
T, K, REF_LEN, ROWS = a.tasks, 128, 150, 1000
GLEN = a.genome

rng = np.random.default_rng(1)
g = synth.genome(GLEN, seed=3)
genome = GenomeTable(g, REF_LEN)
table = WindowTable(synth.windows_lookup(g, REF_LEN, 1))
n_win = 2 * (GLEN - REF_LEN + 1)
reads, _, truth = synth.simulate_reads(g, T, seed=5)  # 1 % substitutions; truth = the read's window id
q = synth.tag(reads)
pos, rev = truth // 2, truth % 2
off = rng.integers(0, ROWS - REF_LEN + 1, size=T)
# a forward read is the mate of a reverse anchor to its right, a reverse read that of a forward anchor to its left;
# the anchor is moved inwards where the region would be cut at a genome end
anchor_pos = np.where(rev == 0, np.clip(pos + off, ROWS - REF_LEN, GLEN - REF_LEN), np.clip(pos - off, 0, GLEN - ROWS))
anchors = (2 * anchor_pos + (1 - rev)).astype(np.uint64)
nb = rng.integers(0, n_win, size=(T, K)).astype(np.int64)
nb[np.arange(T), rng.integers(0, K, size=T)] = truth

st = Stream()
scoring = sw_scoring(a.scoring.split(","))
d_q = DeviceBuffer.from_host(q)
d_ql = DeviceBuffer.from_host(np.full(T, q.shape[1], dtype=np.int32))
d_anchor = DeviceBuffer.from_host(anchors)
d_tq = DeviceBuffer.from_host(np.arange(T, dtype=np.int64))
d_res = DeviceBuffer((T,), RESCUE_RESULT_DTYPE)
d_wid = DeviceBuffer.from_host(truth.astype(np.uint64))
d_rec = DeviceBuffer(T, SW_ALIGNMENT_DTYPE)
d_ops = DeviceBuffer((T, 16), np.uint32)
d_nb = DeviceBuffer.from_host(nb)
d_sc, d_ids, d_st = DeviceBuffer((T, K), np.int32), DeviceBuffer((T, K), np.uint64), DeviceBuffer(T, np.int32)


def rescue():
    mate_rescue_device(genome, d_anchor, d_tq, T, d_q, d_ql, q.shape[1], T, 0, ROWS, [int(x) for x in scoring],
                       d_out=d_res, stream=st)


def affine():
    check(lib().drm_sw_align_affine_device(genome.handle, scoring.ctypes.data, a.flank, d_wid.ptr, d_tq.ptr, T, d_q.ptr,
                                           d_ql.ptr, q.shape[1], T, d_rec.ptr, d_ops.ptr, 16, st.handle))


def rerank():
    check(lib().drm_post_process_sw_static_device(table.handle, d_nb.ptr, T, K, d_q.ptr, d_ql.ptr, q.shape[1], 1, K, K,
                                                  d_sc.ptr, d_ids.ptr, d_st.ptr, st.handle))


rescue()
affine()
st.synchronize()
res, rec = d_res.download(), d_rec.download()
assert (res["region_len"] == ROWS).all() and (res["status"] == 0).all(), "a region is cut or a read found nothing"
assert (res["score"] >= rec["score"]).all(), "the scan scored below the aligner on a sub-region"
assert (res["score"] == rec["score"]).mean() > 0.99, "the scan does not find the planted reads"
back = [mate_rescue_window(res[t], REF_LEN, GLEN) for t in range(0, T, max(T // 256, 1))]
near = np.abs(np.array(back, dtype=np.int64) // 2 - pos[::max(T // 256, 1)]) <= 2
assert near.mean() > 0.99, "the rescued windows are not the reads' windows"
m, cols = int(q.shape[1]), 3
steps = {"rescue": ROWS + (m + cols - 1) // cols - 1, "affine": REF_LEN + 2 * a.flank + (m + cols - 1) // cols - 1}
print(f"{T} tasks, {ROWS}-row regions x {m} B reads, scoring {a.scoring}; mean score {res['score'].mean():.1f}; "
      f"scores equal the aligner's on the true windows", flush=True)

jobs = [(f"mate_rescue, {T} tasks x {ROWS} rows", rescue), (f"sw_align_affine flank {a.flank}, {T} pairs", affine),
        (f"SW rerank, {T} reads x {K} candidates", rerank)]
for _, f in jobs:
    f()
st.synchronize()
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
for (name, _), t, md in zip(jobs, ts, med):
    print(f"{name}: median {md:.3f} ms (min {min(t):.3f}, max {max(t):.3f}, {a.runs} runs)", flush=True)
per = {"rescue": med[0] * 1e6 / (T * steps["rescue"]), "affine": med[1] * 1e6 / (T * steps["affine"])}
print(f"per DP step: mate_rescue {per['rescue']:.4f} ns ({steps['rescue']} steps), sw_align_affine "
      f"{per['affine']:.4f} ns ({steps['affine']} steps): {per['rescue'] / per['affine']:.3f}x; "
      f"rescue / rerank at k = {K}: {med[0] / med[2]:.3f}; {T / med[0] / 1e3:.2f} M tasks/s", flush=True)
