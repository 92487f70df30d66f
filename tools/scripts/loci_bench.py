"""Locus-list rate probe: drm_hit_loci_device at max_loci 1, 5 and 64 beside drm_hit_mapq_device,
the existing kernel, on the same lists -- 2 x --pairs synthetic reads at k = 128 (the device outputs of the SW rerank,
tools/scripts/mapq_bench.py's inputs), random lists at k = 1024, and the scan's worst case, --worst reads whose k rows
are k singleton loci of one score. drop_pct is the default 80; max_loci = 1 is timed at drop_pct 100 as well, where a
locus passes only at the head's score and the loop ends where hit_mapq's does: the same scan plus the stores. HIP
events around --calls back-to-back calls, warm, median of --runs such windows, the timed functions taking turns window
by window. Before timing, a sample of every
configuration is checked against the Python restatement of the definition (tests/loci_ref.py).
--pipeline READS times the single-read SAM stage of bin/pipeline instead (pipeline_stage below)."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loci_ref  # noqa: E402
from deepreadmapper_amd import MAPQ_RESULT_DTYPE, WindowTable, hit_loci_device, hit_mapq_device, synth  # noqa: E402
from deepreadmapper_amd._native import check, lib  # noqa: E402
from deepreadmapper_amd.device import DeviceBuffer, Event, Stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=65_536)
ap.add_argument("--runs", type=int, default=11)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--genome", type=int, default=200_000)
ap.add_argument("--worst", type=int, default=8_192)
ap.add_argument("--pipeline", type=int, default=0, metavar="READS",
                help="instead: the single-read SAM stage of bin/pipeline on READS reads, three ways")
a = ap.parse_args()


def pipeline_stage(n_reads, genome_len=100_000, k=32, reps=3):
    """bin/pipeline's single-read SAM stage (DRM_SAM_STATS=1) on one input: a random genome of genome_len bases with
    its first tenth appended once more (every read from there has two placements), n_reads 150-base reads with 1 %
    substitutions, k rerank rows a read; DRM_SAM_MAPQ=1 alone (a line and an alignment per rerank row), with
    DRM_SAM_LOCI=5, and with DRM_SAM_XA=1 beside it. Each way runs `reps` times, taking turns; the median is printed
    with the rows aligned and the file's size."""
    with tempfile.TemporaryDirectory() as wd:
        g = synth.genome(genome_len, seed=42)
        g = np.concatenate([g, g[:genome_len // 10]])
        fna, fq = os.path.join(wd, "g.fna"), os.path.join(wd, "reads.fastq")
        synth.write_fasta(fna, g)
        reads, names, _ = synth.simulate_reads(g, n_reads, seed=7)
        synth.write_fastq(fq, reads, names)
        t0 = time.time()
        subprocess.run([os.path.join(ROOT, "bin", "hnswpq_index"), fna, "idx", "150"], cwd=wd, check=True,
                       stdout=subprocess.DEVNULL)
        print(f"hnswpq_index on {len(g)} bases: {time.time() - t0:.1f} s", flush=True)
        ways = {"DRM_SAM_MAPQ=1": {}, "DRM_SAM_LOCI=5": dict(DRM_SAM_LOCI="5"),
                "DRM_SAM_LOCI=5 DRM_SAM_XA=1": dict(DRM_SAM_LOCI="5", DRM_SAM_XA="1")}
        seen = {w: [] for w in ways}
        for _ in range(reps):
            for way, more in ways.items():
                env = dict(os.environ, DRM_SAM_CIGAR="1", DRM_SAM_MAPQ="1", DRM_SAM_STATS="1", **more)
                t0 = time.time()
                r = subprocess.run([os.path.join(ROOT, "bin", "pipeline"), "idx", fq, fna, "128", str(k), str(k), "out",
                                    "1", "1"], cwd=wd, env=env, capture_output=True, text=True)
                wall = time.time() - t0
                if r.returncode != 0:
                    sys.exit(r.stdout + r.stderr)
                m = re.search(r"SAM stage: ([0-9.e+-]+) ms between the rerank and the writer, (\d+) rows aligned, "
                              r"([0-9.e+-]+) ms for the block loop", r.stdout)
                sam = os.path.join(wd, "out", "results.sam")
                with open(sam) as f:
                    lines = sum(1 for x in f if not x.startswith("@"))
                seen[way].append((float(m.group(1)), float(m.group(3)), wall, int(m.group(2)), os.path.getsize(sam), lines))
        for way, v in seen.items():
            med = [statistics.median(x[c] for x in v) for c in range(3)]
            print(f"{way}: SAM stage {med[0]:.1f} ms, block loop (search + rerank + SAM stage + writer) {med[1]:.1f} ms, "
                  f"process wall {med[2]:.2f} s (medians of {reps}); {v[0][3]} rows aligned, {v[0][5]} lines, "
                  f"{v[0][4]} bytes for {n_reads} reads at k = {k}", flush=True)


if a.pipeline:
    pipeline_stage(a.pipeline)
    sys.exit(0)
NP, K, K2, REF_LEN = a.pairs, 128, 1024, 150
NQ, NW = 2 * NP, a.worst

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
check(lib().drm_post_process_sw_static_device(table.handle, d_nb.ptr, NQ, K, d_q.ptr, d_ql.ptr, q.shape[1], 1, K, K,
                                              d_sc.ptr, d_ids.ptr, d_st.ptr, st.handle))
st.synchronize()
lists = {f"{NQ} reads, k = {K}, the rerank's outputs": (d_ids, d_sc, d_st, NQ, K),
         f"{NQ} reads, k = {K2}, random lists": (
             DeviceBuffer.from_host(rng.integers(0, n_win, size=(NQ, K2)).astype(np.uint64)),
             DeviceBuffer.from_host(rng.integers(1, REF_LEN + 1, size=(NQ, K2)).astype(np.int32)),
             DeviceBuffer.from_host(np.full(NQ, K2, dtype=np.int32)), NQ, K2)}
for k in (K, K2):  # the scan's worst case: k singleton loci (200 bases apart) of one score
    ids = np.broadcast_to((2 * 200 * np.arange(k)).astype(np.uint64), (NW, k)).copy()
    lists[f"worst case, {NW} reads of {k} singleton loci"] = (
        DeviceBuffer.from_host(ids), DeviceBuffer.from_host(np.full((NW, k), 77, np.int32)),
        DeviceBuffer.from_host(np.full(NW, k, np.int32)), NW, k)
CONFIGS = [(1, 100), (1, 80), (5, 80), (64, 80)]  # (max_loci, drop_pct)

jobs = []  # (list name, label, function, output buffers)
for name, (d_i, d_s, d_c, n, k) in lists.items():
    out = DeviceBuffer((n,), MAPQ_RESULT_DTYPE)
    jobs.append((name, "hit_mapq", lambda d_i=d_i, d_s=d_s, d_c=d_c, n=n, k=k, out=out: hit_mapq_device(
        d_i, d_s, d_c, d_full, n, k, REF_LEN, d_out=out, stream=st), (out,)))
    for ml, pct in CONFIGS:
        bufs = (DeviceBuffer((n,), MAPQ_RESULT_DTYPE), DeviceBuffer((n,), np.int32), DeviceBuffer((n,), np.int32),
                DeviceBuffer((n, ml), np.uint64), DeviceBuffer((n, ml), np.int32), DeviceBuffer((n, ml), np.int32),
                DeviceBuffer((n, ml), np.int32))
        jobs.append((name, f"hit_loci max_loci {ml} drop {pct}",
                     lambda d_i=d_i, d_s=d_s, d_c=d_c, n=n, k=k, ml=ml, pct=pct, b=bufs: hit_loci_device(
                         d_i, d_s, d_c, d_full, n, k, REF_LEN, ml, drop_pct=pct, d_out=b[0], d_n_loci=b[1],
                         d_n_pass=b[2], d_loci_ids=b[3], d_loci_scores=b[4], d_loci_rows=b[5], d_loci_size=b[6],
                         stream=st), bufs))

for _, _, f, _ in jobs:
    f()
st.synchronize()
# a sample of every configuration against the restatement; the MAPQ records against hit_mapq's, byte for byte
x = 0
for name, (d_i, d_s, d_c, n, k) in lists.items():
    ids, sc, cnt = d_i.download(), d_s.download(), d_c.download()
    if name.startswith("worst"):  # every read is the same list, and the restatement takes k^2 / 2 steps on it
        sample = np.array([0, n - 1])
    else:
        sample = np.unique(np.concatenate([np.arange(min(n, 8)), rng.integers(0, n, size=8 if k == K2 else 56)]))
    mapq = jobs[x][3][0].download()
    x += 1
    for ml, pct in CONFIGS:
        got = tuple(b.download() for b in jobs[x][3])
        x += 1
        assert got[0].tobytes() == mapq.tobytes(), (name, ml, pct)
        loci_ref.assert_equal(tuple(o[sample] for o in got),
                              loci_ref.loci_all(ids[sample], sc[sample], cnt[sample], np.full(len(sample), REF_LEN),
                                                REF_LEN, ml, drop_pct=pct), (name, ml, pct))
        print(f"{name}, max_loci {ml}, drop {pct}: mean n_loci {got[1].mean():.2f}, mean n_pass {got[2].mean():.2f}, "
              f"mean n_sub {got[0]['n_sub'].mean():.2f}; {len(sample)} reads equal the restatement", flush=True)

# a window is --calls back-to-back calls between two events: one call of the short lists takes about as long as the
# host needs to enqueue it, and a window of one would time the wrapper
ts = [[] for _ in jobs]
for _ in range(a.runs):
    for x, (_, _, f, _) in enumerate(jobs):
        e0, e1 = Event(), Event()
        e0.record(st)
        for _ in range(a.calls):
            f()
        e1.record(st)
        st.synchronize()
        ts[x].append(e0.elapsed_ms(e1) / a.calls)
base = None
for (name, label, _, _), t in zip(jobs, ts):
    m = statistics.median(t)
    base = m if label == "hit_mapq" else base
    print(f"{name}: {label}: median {m:.4f} ms a call (min {min(t):.4f}, max {max(t):.4f}, {a.runs} windows of "
          f"{a.calls} calls), {m / base:.3f} x hit_mapq", flush=True)
