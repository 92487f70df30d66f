"""Sort-order rate probe: drm_sort_order_device on the keys of a paired C5 run -- 2,621,440 lines,
positions uniform over 50 M, 2 % of the keys all-ones -- on one contig and on 25, beside three yardsticks on the same
keys: hipcub::DeviceRadixSort::SortPairs (tools/microbench/hipcub_sort.hip, built on demand with hipcc), numpy's stable
argsort on the host, and the SW rerank (drm_post_process_sw_static_device) of the same number of reads at k = 128, timed
on one block of --block reads and scaled. Device times are HIP events on one stream, warm, the median of --runs runs,
the timed functions taking turns run by run; the host time is a wall clock. Before timing, every order is checked
against np.argsort(keys, kind="stable"). Also timed: all-equal keys (every pass skipped) and random 64-bit keys (all
eight passes kept). The bytes a kept pass must move per key: 8 read by the count; 8 + 4 read and 8 + 4 written by the
scatter (the first kept pass reads no payload, the last writes no key); the histogram reads 8 once."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from deepreadmapper_amd import WindowTable, sort_order_device, sort_order_workspace, synth  # noqa: E402
from deepreadmapper_amd._native import check, lib  # noqa: E402
from deepreadmapper_amd.device import DeviceBuffer, Event, Stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=2_621_440)
ap.add_argument("--positions", type=int, default=50_000_000)
ap.add_argument("--block", type=int, default=65_536)
ap.add_argument("--runs", type=int, default=21)
ap.add_argument("--genome", type=int, default=200_000)
ap.add_argument("--no-rerank", action="store_true")
ap.add_argument("--no-hipcub", action="store_true")
a = ap.parse_args()
N, K, REF_LEN = a.keys, 128, 150
rng = np.random.default_rng(1)
ONES = np.uint64(2 ** 64 - 1)


def sam_keys(contigs):
    tid = rng.integers(0, contigs, N).astype(np.uint64)
    pos = rng.integers(1, a.positions // contigs + 1, N).astype(np.uint64)
    keys = (((tid << np.uint64(33)) | pos) << np.uint64(1)) | rng.integers(0, 2, N).astype(np.uint64)
    keys[rng.random(N) < 0.02] = ONES
    return keys


def kept_passes(keys):
    """The plan kernel's rule: a byte that is the same in every key is dropped, and so is one that only tells the
    all-ones keys from the rest when a lower byte that does the same is kept."""
    ones, kept, have = int((keys == ONES).sum()), [], False
    for p in range(8):
        v, c = np.unique((keys >> np.uint64(8 * p)) & np.uint64(255), return_counts=True)
        ones_only = ones > 0 and len(v) == 2 and int(v[-1]) == 255 and int(c[-1]) == ones
        if len(v) > 1 and not (ones_only and have):
            kept.append(p)
        have = have or ones_only
    return kept


def hipcub():
    """The yardstick's library, built beside its source when it is not there."""
    src = os.path.join(ROOT, "tools", "microbench", "hipcub_sort.hip")
    so = os.path.join(ROOT, "tools", "microbench", "libhipcub_sort.so")
    if not os.path.exists(so):
        hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
        subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-shared", "-fPIC", src, "-o", so], check=True)
    L = C.CDLL(so)
    L.hipcub_sort_pairs_bytes.argtypes = [C.c_int64, C.POINTER(C.c_size_t)]
    L.hipcub_sort_pairs.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                    C.c_void_p]
    return L


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


sets = {"1 contig": sam_keys(1), "25 contigs": sam_keys(25), "all equal": np.full(N, 12345, dtype=np.uint64),
        "random 64-bit": rng.integers(0, 2 ** 64, N, dtype=np.uint64)}
d_order, d_iota = DeviceBuffer((N,), np.uint32), DeviceBuffer.from_host(np.arange(N, dtype=np.uint32))
d_keys = {name: DeviceBuffer.from_host(k) for name, k in sets.items()}
print(f"{N} keys; workspace {sort_order_workspace(N) / 2 ** 20:.1f} MiB", flush=True)

H = None if a.no_hipcub else hipcub()
if H:
    nbytes = C.c_size_t(0)
    assert H.hipcub_sort_pairs_bytes(N, C.byref(nbytes)) == 0
    d_tmp = DeviceBuffer((max(nbytes.value, 1),), np.uint8)
    d_kout, d_vout = DeviceBuffer((N,), np.uint64), DeviceBuffer((N,), np.uint32)
    print(f"hipcub temporary storage {nbytes.value / 2 ** 20:.1f} MiB + {12 * N / 2 ** 20:.1f} MiB of output", flush=True)


def ours(name):
    sort_order_device(d_keys[name], N, d_order, st)


def theirs(name):
    assert H.hipcub_sort_pairs(d_tmp.ptr, nbytes.value, d_keys[name].ptr, d_kout.ptr, d_iota.ptr, d_vout.ptr, N,
                               st.handle) == 0


# ---- the answers first
want, host_ms = {}, {}
for name, keys in sets.items():
    t0 = time.perf_counter()
    want[name] = np.argsort(keys, kind="stable").astype(np.uint32)
    host_ms[name] = (time.perf_counter() - t0) * 1e3
    ours(name)
    st.synchronize()
    assert np.array_equal(d_order.download(), want[name]), name
    if H:
        theirs(name)
        st.synchronize()
        assert np.array_equal(d_vout.download(), want[name]), name  # an LSD radix sort is stable as well
    print(f"{name}: passes kept {kept_passes(keys)}; equal to numpy's stable argsort", flush=True)

# ---- the rerank of one block of reads
if not a.no_rerank:
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
        check(lib().drm_post_process_sw_static_device(table.handle, d_nb.ptr, NQ, K, d_q.ptr, d_ql.ptr, q.shape[1], 1, K,
                                                      K, d_sc.ptr, d_ids.ptr, d_st.ptr, st.handle))
    rerank()
    st.synchronize()

# ---- the times, in turns
t_ours, t_theirs, t_rerank = {n: [] for n in sets}, {n: [] for n in sets}, []
for name in sets:  # warm
    for _ in range(3):
        ours(name)
        if H:
            theirs(name)
st.synchronize()
for _ in range(a.runs):
    for name in sets:
        t_ours[name].append(timed(lambda: ours(name)))
        if H:
            t_theirs[name].append(timed(lambda: theirs(name)))
    if not a.no_rerank:
        t_rerank.append(timed(rerank))
m_rerank = show(f"SW rerank, {a.block} reads x {K} candidates", t_rerank) if t_rerank else None
for name, keys in sets.items():
    m = show(f"drm_sort_order_device, {name}", t_ours[name])
    kept = len(kept_passes(keys))
    moved = N * (8 + kept * 32 - 12) if kept else N * (8 + 4)
    print(f"  {m * 1e6 / N:.3f} ns a key; {kept} passes kept, {moved / 2 ** 20:.0f} MiB to move at the least = "
          f"{moved / (m * 1e-3) / 1e12:.3f} TB/s over the whole call", flush=True)
    if H:
        mh = show(f"hipcub SortPairs (64 bits), {name}", t_theirs[name])
        print(f"  ours / hipcub = {m / mh:.3f}", flush=True)
    print(f"  numpy stable argsort on the host: {host_ms[name]:.1f} ms (one run, wall clock) = {host_ms[name] / m:.0f} x ours",
          flush=True)
    if m_rerank:
        blocks = N / a.block
        print(f"  = {m / (blocks * m_rerank):.5f} of the rerank of {N} reads ({blocks:.0f} x {m_rerank:.3f} ms)", flush=True)
