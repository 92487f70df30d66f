"""Chunk plans of the SW rerank (drm_refs_set_sw_chunk, DESIGN.md sec. 4.4 "Round 8") on one window table, one
process: random 150 bp windows, random candidate ids, Q tagged 152-byte reads; per plan the mean and the minimum of
`--reps` event-timed calls, the plans interleaved over `--rounds` rounds. --check compares every plan's outputs with
the one-launch order's, byte for byte. --plans: queries per chunk (0 = one launch, -1 = the library's plan)."""
import argparse
import sys

import numpy as np

sys.path.insert(0, ".")
from deepreadmapper_amd import WindowTable, synth  # noqa: E402
from deepreadmapper_amd._native import check, lib  # noqa: E402
from deepreadmapper_amd.device import DeviceBuffer, Event, Stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--queries", type=int, default=1_250_000)
ap.add_argument("--windows", type=int, default=2_000_000)
ap.add_argument("--plans", default="0,-1")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--check", action="store_true")
a = ap.parse_args()
K, Q = 128, a.queries
g = synth.genome(a.windows // 2 + 149, seed=3)
refs = synth.windows_lookup(g, 150, 1)
table = WindowTable(refs)
rng = np.random.default_rng(1)
d_I = DeviceBuffer.from_host(rng.integers(0, len(refs), size=(Q, K)).astype(np.int64))
reads, _, _ = synth.simulate_reads(g, Q, read_len=150, seed=5)
q = synth.tag(reads)
d_q = DeviceBuffer.from_host(q)
d_ql = DeviceBuffer.from_host(np.full(Q, q.shape[1], dtype=np.int32))
d_sc, d_id, d_st = DeviceBuffer((Q, K), np.int32), DeviceBuffer((Q, K), np.uint64), DeviceBuffer(Q, np.int32)
st = Stream()


def run():
    check(lib().drm_post_process_sw_static_device(table.handle, d_I.ptr, Q, K, d_q.ptr, d_ql.ptr, q.shape[1], 1, K, K,
                                                  d_sc.ptr, d_id.ptr, d_st.ptr, st.handle))


plans = [int(p) for p in a.plans.split(",")]
base = None
for rnd in range(a.rounds):
    for p in plans:
        table.sw_chunk = p
        run()
        st.synchronize()
        if a.check and rnd == 0:
            out = (d_sc.download(), d_id.download(), d_st.download())
            if base is None:
                table.sw_chunk = 0
                run()
                st.synchronize()
                base = (d_sc.download(), d_id.download(), d_st.download())
                table.sw_chunk = p
            assert all(np.array_equal(x, y) for x, y in zip(out, base)), f"plan {p}: outputs differ from one launch"
        ts = []
        for _ in range(a.reps):
            e0, e1 = Event(), Event()
            e0.record(st)
            run()
            e1.record(st)
            st.synchronize()
            ts.append(e0.elapsed_ms(e1))
        print(f"round {rnd + 1} Q {Q} chunk {p:8d}: mean {np.mean(ts):8.3f} min {min(ts):8.3f} ms", flush=True)
