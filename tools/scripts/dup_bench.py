"""Duplicate-set rate probe: drm_dupset_mark_device beside the SW rerank
(drm_post_process_sw_static_device) of the same number of reads at k = 128. HIP events, warm, median of --runs runs, the
timed functions taking turns run by run; every run marks into a fresh set (its creation, which zeroes the table, is not
timed). Before timing, the answers are checked against the plain restatement (tests/dup_ref.py).

  pairs   --pairs pairs in one call (the items of one SAM block of 2 x --pairs reads).
  reads   --reads single reads in blocks of --block, so that the set ends filled to its capacity: the time of every
          block of the run, first to last.
  big     a set of --big items (its table and keys far beyond the 256 MB Infinity Cache) filled to 3/4 in calls of 2^20
          items, then blocks of --block: the same kernels on a table that is not cache-resident.

One item in --dup-pct per cent repeats an earlier item's key. The three kernels must move per item: 16 B of end words in,
a 16 B key out and in again twice, one 8 B slot atomic or more, a 16 B key read per occupied slot probed, 8 B of answer out."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dup_ref  # noqa: E402
from deepreadmapper_amd import DupSet, WindowTable, synth  # noqa: E402
from deepreadmapper_amd._native import check, lib  # noqa: E402
from deepreadmapper_amd.device import DeviceBuffer, Event, Stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=65_536)
ap.add_argument("--reads", type=int, default=1_310_720)
ap.add_argument("--block", type=int, default=65_536)
ap.add_argument("--big", type=int, default=1 << 25)
ap.add_argument("--runs", type=int, default=11)
ap.add_argument("--dup-pct", type=int, default=10)
ap.add_argument("--genome", type=int, default=200_000)
a = ap.parse_args()
K, REF_LEN = 128, 150
rng = np.random.default_rng(1)


def words(n):
    """n end words of random ends on a 3 Gb genome, either strand"""
    e5 = rng.integers(-150, 3_000_000_000, size=n).astype(np.uint64)
    return (((e5 + np.uint64(1 << 20)) << np.uint64(1)) | rng.integers(0, 2, size=n).astype(np.uint64)) + np.uint64(1)


def items(n, paired):
    ends = np.stack([words(n), words(n) if paired else np.zeros(n, np.uint64)], axis=1)
    rep = np.flatnonzero(rng.integers(0, 100, size=n) < a.dup_pct)
    rep = rep[rep > 0]
    ends[rep] = ends[(rng.random(len(rep)) * rep).astype(np.int64)]  # an earlier item (or a repeat of one)
    return np.ascontiguousarray(ends)


st = Stream()


def timed(f):
    e0, e1 = Event(), Event()
    e0.record(st)
    f()
    e1.record(st)
    st.synchronize()
    return e0.elapsed_ms(e1)


def show(name, t):
    print(f"{name}: median {statistics.median(t):.4f} ms (min {min(t):.4f}, max {max(t):.4f}, {len(t)} runs)", flush=True)
    return statistics.median(t)


# ---- the rerank of one block of reads, the yardstick
NQ = a.block
g = synth.genome(a.genome, seed=3)
table = WindowTable(synth.windows_lookup(g, REF_LEN, 1))
start = rng.integers(0, a.genome - REF_LEN, size=NQ)
q = synth.tag(np.stack([g[s:s + REF_LEN] for s in start]))
nb = rng.integers(0, 2 * (a.genome - REF_LEN + 1), size=(NQ, K)).astype(np.int64)
nb[np.arange(NQ), rng.integers(0, K, size=NQ)] = 2 * start
d_q, d_ql = DeviceBuffer.from_host(q), DeviceBuffer.from_host(np.full(NQ, q.shape[1], dtype=np.int32))
d_nb = DeviceBuffer.from_host(nb)
d_sc, d_ids, d_st = DeviceBuffer((NQ, K), np.int32), DeviceBuffer((NQ, K), np.uint64), DeviceBuffer(NQ, np.int32)


def rerank():
    check(lib().drm_post_process_sw_static_device(table.handle, d_nb.ptr, NQ, K, d_q.ptr, d_ql.ptr, q.shape[1], 1, K, K,
                                                  d_sc.ptr, d_ids.ptr, d_st.ptr, st.handle))


# ---- pairs: one call
pe = items(a.pairs, True)
d_pe, d_pf = DeviceBuffer.from_host(pe), DeviceBuffer((a.pairs,), np.int64)
s = DupSet(a.pairs)
s.mark_device(d_pe, a.pairs, 0, d_pf, st)
st.synchronize()
want = dup_ref.FirstSeen(a.pairs).mark(pe)
assert np.array_equal(d_pf.download(), want)
print(f"{a.pairs} pairs: {int(((want >= 0) & (want != np.arange(a.pairs))).sum())} duplicates; equal to the restatement",
      flush=True)
s.free()

# ---- reads: blocks into one set
re_ = items(a.reads, False)
nblocks = a.reads // a.block
d_re, d_rf = DeviceBuffer.from_host(re_), DeviceBuffer((a.reads,), np.int64)
s = DupSet(a.reads)
for b in range(nblocks):
    s.mark_device(d_re.ptr + 16 * b * a.block, a.block, b * a.block, d_rf.ptr + 8 * b * a.block, st)
st.synchronize()
want = dup_ref.FirstSeen(a.reads).mark(re_)
assert np.array_equal(d_rf.download()[:nblocks * a.block], want[:nblocks * a.block])
info = s.info()
print(f"{a.reads} reads in {nblocks} blocks: {int(((want >= 0) & (want != np.arange(a.reads))).sum())} duplicates; equal "
      f"to the restatement; {info['slots']} slots ({info['slots'] * 8 >> 20} MiB) + {a.reads * 16 >> 20} MiB of keys",
      flush=True)
s.free()

t_rerank, t_pairs, t_blocks = [], [], [[] for _ in range(nblocks)]
rerank()
st.synchronize()
for _ in range(a.runs):
    t_rerank.append(timed(rerank))
    s = DupSet(a.pairs)
    t_pairs.append(timed(lambda: s.mark_device(d_pe, a.pairs, 0, d_pf, st)))
    s.free()
    s = DupSet(a.reads)
    for b in range(nblocks):
        t_blocks[b].append(timed(lambda: s.mark_device(d_re.ptr + 16 * b * a.block, a.block, b * a.block,
                                                       d_rf.ptr + 8 * b * a.block, st)))
    s.free()
m_rerank = show(f"SW rerank, {NQ} reads x {K} candidates", t_rerank)
m_pairs = show(f"dupset mark, {a.pairs} pairs in one call (fresh set of {a.pairs})", t_pairs)
print(f"  = {m_pairs / (2 * a.pairs / NQ * m_rerank):.5f} of the rerank of their {2 * a.pairs} reads "
      f"({2 * a.pairs / NQ:.0f} x the block's {m_rerank:.3f} ms); {m_pairs * 1e6 / a.pairs:.2f} ns an item", flush=True)
med = [statistics.median(t) for t in t_blocks]
for b in (0, nblocks // 2, nblocks - 1):
    show(f"dupset mark, block {b} of {nblocks} ({a.block} reads, set of {a.reads} filled to {b * a.block})", t_blocks[b])
total = sum(med)
print(f"dupset mark, all {nblocks} blocks: {total:.4f} ms (sum of the medians) = {total / (nblocks * m_rerank):.5f} of the "
      f"rerank of the {nblocks * a.block} reads ({nblocks} x {m_rerank:.3f} ms); {total * 1e6 / (nblocks * a.block):.2f} ns "
      f"an item", flush=True)

# ---- a table beyond the cache
if a.big:
    fill = a.big * 3 // 4 // (1 << 20) * (1 << 20)
    s = DupSet(a.big)
    chunk = items(1 << 20, False)
    d_chunk, d_cf = DeviceBuffer((1 << 20, 2), np.uint64), DeviceBuffer((1 << 20,), np.int64)
    for c in range(fill >> 20):
        chunk[:, 0] = words(1 << 20)
        d_chunk.upload(chunk)
        s.mark_device(d_chunk, 1 << 20, c << 20, d_cf, st)
        st.synchronize()
    info = s.info()
    t_big = []
    for r in range(min(a.runs, (a.big - fill) // a.block)):
        be = items(a.block, False)
        d_be = DeviceBuffer.from_host(be)
        t_big.append(timed(lambda: s.mark_device(d_be, a.block, fill + r * a.block, d_rf, st)))
    m_big = show(f"dupset mark, {a.block} reads into a set of {a.big} filled to {fill} ({info['slots'] * 8 >> 20} MiB of "
                 f"slots + {a.big * 16 >> 20} MiB of keys)", t_big)
    print(f"  = {m_big / m_rerank:.5f} of the rerank of the block; {m_big * 1e6 / a.block:.2f} ns an item", flush=True)
    s.free()
