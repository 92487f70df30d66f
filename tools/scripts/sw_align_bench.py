"""SW alignment rate probe (DESIGN.md "SW alignment"): drm_sw_align_device on P pairs of 150-byte windows against
152-byte tagged reads at 1 % substitutions, each read aligned to the window it was drawn from. HIP events, warm,
median of --runs runs. For scale it also times the score-only rerank (drm_post_process_sw_static_device) on the same
pairs (one candidate per read, which leaves most of that kernel's lanes idle) and on as many pairs in the shape it
is built for (P / 128 reads x 128 candidates). Checks the alignment scores against the rerank's before timing.
--scoring match,mismatch,open,extend adds the affine kernel (drm_sw_align_affine_device) on the same pairs in the same
process: at flank 0 on the same window table, and at --flank on a genome handle of the same genome (the same window
ids). --clip L (with --scoring) adds the end-aware kernel (drm_sw_align_affine_clip_device, tags 1 / 1) beside each of
the two, counts the records it changes and the clipped bases it recovers, and prints its time over the plain affine
kernel's per run pair. The timed functions take turns run by run, so that a drift of the machine meets all of them
alike."""
import argparse
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
from deepreadmapper_amd import GenomeTable, WindowTable, synth  # noqa: E402
from deepreadmapper_amd._native import check, lib  # noqa: E402
from deepreadmapper_amd.device import DeviceBuffer, Event, Stream  # noqa: E402
from deepreadmapper_amd.rerank import SW_ALIGNMENT_DTYPE, sw_scoring  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=65_536)
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--ops-stride", type=int, default=16)
ap.add_argument("--scoring", default=None, help="match,mismatch,open,extend: also time the affine kernel")
ap.add_argument("--flank", type=int, default=8, help="flank of the affine kernel's second timing (genome handle)")
ap.add_argument("--clip", type=int, default=None, help="clipping penalty: also time the end-aware affine kernel")
a = ap.parse_args()
if a.clip is not None and not a.scoring:
    ap.error("--clip needs --scoring")
P, K = a.pairs, 128

g = synth.genome(200_000, seed=3)
refs = synth.windows_lookup(g, 150, 1)
table = WindowTable(refs)
reads, _, truth = synth.simulate_reads(g, P, seed=5)
q = synth.tag(reads)
st = Stream()
d_q = DeviceBuffer.from_host(q)
d_ql = DeviceBuffer.from_host(np.full(P, q.shape[1], dtype=np.int32))
d_wid = DeviceBuffer.from_host(truth.astype(np.uint64))
d_pq = DeviceBuffer.from_host(np.arange(P, dtype=np.int64))
d_rec = DeviceBuffer(P, SW_ALIGNMENT_DTYPE)
d_ops = DeviceBuffer((P, a.ops_stride), np.uint32)
d_nb1 = DeviceBuffer.from_host(truth.reshape(P, 1).astype(np.int64))
d_sc1, d_id1, d_st1 = DeviceBuffer((P, 1), np.int32), DeviceBuffer((P, 1), np.uint64), DeviceBuffer(P, np.int32)
nq2 = P // K
rng = np.random.default_rng(1)
d_nb2 = DeviceBuffer.from_host(rng.integers(0, len(refs), size=(nq2, K)).astype(np.int64))
d_sc2, d_id2, d_st2 = DeviceBuffer((nq2, K), np.int32), DeviceBuffer((nq2, K), np.uint64), DeviceBuffer(nq2, np.int32)


def align():
    check(lib().drm_sw_align_device(table.handle, d_wid.ptr, d_pq.ptr, P, d_q.ptr, d_ql.ptr, q.shape[1], P, d_rec.ptr,
                                    d_ops.ptr, a.ops_stride, st.handle))


def rerank_same_pairs():
    check(lib().drm_post_process_sw_static_device(table.handle, d_nb1.ptr, P, 1, d_q.ptr, d_ql.ptr, q.shape[1], 1, 1, 1,
                                                  d_sc1.ptr, d_id1.ptr, d_st1.ptr, st.handle))


def rerank_native_shape():
    check(lib().drm_post_process_sw_static_device(table.handle, d_nb2.ptr, nq2, K, d_q.ptr, d_ql.ptr, q.shape[1], 1, K,
                                                  K, d_sc2.ptr, d_id2.ptr, d_st2.ptr, st.handle))


def affine(handle, flank):
    def f():
        check(lib().drm_sw_align_affine_device(handle, scoring.ctypes.data, flank, d_wid.ptr, d_pq.ptr, P, d_q.ptr,
                                               d_ql.ptr, q.shape[1], P, d_rec.ptr, d_ops.ptr, a.ops_stride, st.handle))
    return f


def affine_clip(handle, flank):
    def f():
        check(lib().drm_sw_align_affine_clip_device(handle, scoring.ctypes.data, clip.ctypes.data, flank, d_wid.ptr,
                                                    d_pq.ptr, P, d_q.ptr, d_ql.ptr, q.shape[1], P, d_rec.ptr, d_ops.ptr,
                                                    a.ops_stride, st.handle))
    return f


def timed(fs):
    """Median / min / max of --runs runs per function, warm, the functions taking turns."""
    for f in fs:
        f()
    st.synchronize()
    ts = [[] for _ in fs]
    for _ in range(a.runs):
        for x, f in enumerate(fs):
            e0, e1 = Event(), Event()
            e0.record(st)
            f()
            e1.record(st)
            st.synchronize()
            ts[x].append(e0.elapsed_ms(e1))
    times.extend(ts)
    return [(statistics.median(t), min(t), max(t)) for t in ts]


times = []  # every run of every timed function, in the order of `jobs`


align()
rerank_same_pairs()
st.synchronize()
rec = d_rec.download()
assert np.array_equal(rec["score"], d_sc1.download().reshape(-1)), "alignment score != rerank score"
assert (rec["status"] == 0).all(), "a read did not align (or needed more than --ops-stride operations)"
print(f"{P} pairs, 150 B windows x {q.shape[1]} B reads; scores equal the rerank's; mean score "
      f"{rec['score'].mean():.1f}, mean n_ops {rec['n_ops'].mean():.2f}", flush=True)
jobs = [("sw_align (DP + traceback)", align, P), ("score-only rerank, same pairs (1 candidate / read)",
                                                 rerank_same_pairs, P),
        (f"score-only rerank, {nq2} reads x {K} candidates", rerank_native_shape, nq2 * K)]
if a.scoring:
    scoring = sw_scoring(a.scoring.split(","))
    gtable = GenomeTable(g, 150)
    for handle, flank in ((table.handle, 0), (gtable.handle, a.flank)):
        affine(handle, flank)()
        st.synchronize()
        rec = d_rec.download()
        assert (rec["status"] == 0).all(), "a read did not align under the affine scoring"
        print(f"affine {a.scoring} flank {flank}: mean score {rec['score'].mean():.1f}, mean n_ops "
              f"{rec['n_ops'].mean():.2f}, {int((rec['q_end'] - rec['q_begin'] == 150).sum())} of {P} reads aligned "
              f"end to end", flush=True)
        jobs.append((f"sw_align_affine {a.scoring} flank {flank}", affine(handle, flank), P))
        if a.clip is None:
            continue
        clip = np.array([a.clip, 1, 1], dtype=np.int32)
        plain, plain_ops = rec, d_ops.download()
        affine_clip(handle, flank)()
        st.synchronize()
        rec, ops = d_rec.download(), d_ops.download()
        assert (rec["status"] == 0).all(), "a read did not align under the clipping penalty"
        live = np.arange(a.ops_stride)[None, :] < np.maximum(rec["n_ops"], plain["n_ops"])[:, None]  # the rest is stale
        changed = (rec != plain) | ((ops != plain_ops) & live).any(axis=1)
        span, span0 = rec["q_end"] - rec["q_begin"], plain["q_end"] - plain["q_begin"]
        print(f"affine {a.scoring} clip {a.clip} flank {flank}: {int(changed.sum())} of {P} records changed, "
              f"{int((span - span0).sum())} clipped bases recovered, {int((span == 150).sum())} of {P} reads aligned "
              f"end to end, mean score {rec['score'].mean():.1f}", flush=True)
        jobs.append((f"sw_align_affine_clip {a.scoring} clip {a.clip} flank {flank}", affine_clip(handle, flank), P))
res = timed([f for _, f, _ in jobs])
for (name, _, n), (med, lo, hi) in zip(jobs, res):
    print(f"{name}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}, {a.runs} runs) = {n / med / 1e3:.2f} M pairs/s",
          flush=True)
if a.scoring:
    at = {name: x for x, (name, _, _) in enumerate(jobs)}
    plain = [at[f"sw_align_affine {a.scoring} flank {flank}"] for flank in (0, a.flank)]
    print(f"affine / linear: flank 0 {res[plain[0]][0] / res[0][0]:.2f}x, flank {a.flank} "
          f"{res[plain[1]][0] / res[0][0]:.2f}x", flush=True)
    if a.clip is not None:
        for x, flank in zip(plain, (0, a.flank)):  # the end-aware kernel's job follows its plain one
            ratios = sorted(c / p for c, p in zip(times[x + 1], times[x]))
            print(f"end-aware / plain affine, flank {flank}: median of medians {res[x + 1][0] / res[x][0]:.3f}x; per "
                  f"run pair median {statistics.median(ratios):.3f}x (min {ratios[0]:.3f}, max {ratios[-1]:.3f}, "
                  f"{a.runs} pairs)", flush=True)
