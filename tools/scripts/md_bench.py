"""MD pass rate probe: drm_sw_align_md_device against the alignment it annotates,
drm_sw_align_affine_device, on the same rows in the same run. P simulated 150-base reads (substitutions, and a 2-base
deletion or insertion in every fourth read) are aligned over the flanked region of the window they were drawn from
(a genome handle, --flank, --scoring, 16 operation words a row); the MD pass then walks those records with --md-stride
words a row. HIP events around --reps back-to-back calls (one call of the MD pass is too short to time alone), warm,
median of --runs such windows, the two functions taking turns run by run so that a drift of the machine meets both
alike. Before timing, every MD record is checked against its alignment: n_mismatch + n_ins + n_del == nm."""
import argparse
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
from deepreadmapper_amd import GenomeTable, synth  # noqa: E402
from deepreadmapper_amd._native import check, lib  # noqa: E402
from deepreadmapper_amd.device import DeviceBuffer, Event, Stream  # noqa: E402
from deepreadmapper_amd.rerank import SW_ALIGNMENT_DTYPE, SW_MD_DTYPE, sw_scoring  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=131_072)
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--reps", type=int, default=20, help="calls inside one timed window")
ap.add_argument("--flank", type=int, default=32)
ap.add_argument("--scoring", default="1,4,6,1")
ap.add_argument("--ops-stride", type=int, default=16)
ap.add_argument("--md-stride", type=int, default=16)
ap.add_argument("--sub-rate", type=float, default=0.02)
a = ap.parse_args()
P = a.pairs

g = synth.genome(200_000, seed=3)
reads, _, truth = synth.simulate_reads(g, P, sub_rate=a.sub_rate, seed=5)
rng = np.random.default_rng(9)
reads = reads.copy()
# a few indels at a fixed read length: drop columns 60..61 of every eighth read and insert two bases at column 90 of
# every eighth other one; the tail is padded with random bases, or cut
pad = synth.genome(2 * P, seed=10).reshape(P, 2)
dele, ins = np.arange(0, P, 8), np.arange(4, P, 8)
reads[dele, 60:148] = reads[dele, 62:150]
reads[dele, 148:150] = pad[dele]
reads[ins, 92:150] = reads[ins, 90:148]
reads[ins, 90:92] = pad[ins]
q = synth.tag(reads)
table = GenomeTable(g, 150)
scoring = sw_scoring(a.scoring.split(","))
st = Stream()
d_q = DeviceBuffer.from_host(q)
d_ql = DeviceBuffer.from_host(np.full(P, q.shape[1], dtype=np.int32))
d_wid = DeviceBuffer.from_host(truth.astype(np.uint64))
d_pq = DeviceBuffer.from_host(np.arange(P, dtype=np.int64))
d_rec = DeviceBuffer(P, SW_ALIGNMENT_DTYPE)
d_ops = DeviceBuffer((P, a.ops_stride), np.uint32)
d_off = DeviceBuffer.from_host(np.arange(P, dtype=np.int64) * a.ops_stride)
d_h = DeviceBuffer(P, SW_MD_DTYPE)
d_md = DeviceBuffer((P, a.md_stride), np.uint32)


def align():
    check(lib().drm_sw_align_affine_device(table.handle, scoring.ctypes.data, a.flank, d_wid.ptr, d_pq.ptr, P, d_q.ptr,
                                           d_ql.ptr, q.shape[1], P, d_rec.ptr, d_ops.ptr, a.ops_stride, st.handle))


def md():
    check(lib().drm_sw_align_md_device(table.handle, a.flank, d_wid.ptr, d_pq.ptr, P, d_q.ptr, d_ql.ptr, q.shape[1], P,
                                       d_rec.ptr, d_ops.ptr, d_off.ptr, d_h.ptr, d_md.ptr, a.md_stride, st.handle))


def timed(fs):
    """Per-call median / min / max over --runs windows of --reps calls per function, warm, the functions taking turns."""
    for f in fs:
        f()
    st.synchronize()
    ts = [[] for _ in fs]
    for _ in range(a.runs):
        for x, f in enumerate(fs):
            e0, e1 = Event(), Event()
            e0.record(st)
            for _ in range(a.reps):
                f()
            e1.record(st)
            st.synchronize()
            ts[x].append(e0.elapsed_ms(e1) / a.reps)
    return [(statistics.median(t), min(t), max(t)) for t in ts]


align()
md()
st.synchronize()
rec, h = d_rec.download(), d_h.download()
assert (rec["status"] == 0).all(), "a read did not align (or needed more than --ops-stride operations)"
assert np.isin(h["status"], (0, 2)).all(), "an aligner's record did not walk"
assert np.array_equal(h["n_mismatch"] + h["n_ins"] + h["n_del"], rec["nm"]), "MD counts != the alignment's nm"
print(f"{P} pairs, flank {a.flank}, scoring {a.scoring}: mean n_ops {rec['n_ops'].mean():.2f}, mean nm "
      f"{rec['nm'].mean():.2f}, mean MD words {h['n_words'].mean():.2f}, {int((h['status'] == 2).sum())} rows with more "
      f"than {a.md_stride} words; counts equal nm on every row", flush=True)
# what the pass has to move a pair: ids, the record, its words, the region and query bytes it compares, its output
moved = P * (16 + 32 + 8 + 4 * rec["n_ops"].mean() + 2 * 150 + 24 + 4 * np.minimum(h["n_words"], a.md_stride).mean())
res = timed([align, md])
for name, (med, lo, hi) in zip((f"sw_align_affine {a.scoring} flank {a.flank}", "sw_align_md"), res):
    print(f"{name}: median {med:.4f} ms a call (min {lo:.4f}, max {hi:.4f}; {a.runs} windows of {a.reps} calls) = "
          f"{P / med / 1e3:.1f} M pairs/s", flush=True)
print(f"sw_align_md moves about {moved / 1e6:.1f} MB a call: {moved / res[1][0] / 1e6:.1f} GB/s", flush=True)
print(f"sw_align_md / sw_align_affine: {res[1][0] / res[0][0]:.4f}", flush=True)
