"""The fp32 HNSW builder under several threads: every node of the graph it writes can be reached from the entry
point. An exhaustive graph search (ef >= ntotal) then equals the exhaustive scan, which tests/test_gpu_exact.py
relies on."""
import numpy as np

import exact_ref as R
from oracle import hnswlib_file, oracle as O


def level0_unreachable(fx):
    n, l0 = fx["n"], fx["l0"]
    seen = np.zeros(n, dtype=bool)
    seen[fx["ep"]] = True
    stack = [int(fx["ep"])]
    while stack:
        u = stack.pop()
        for v in l0[u, 1:1 + (int(l0[u, 0]) & 0xFFFF)]:
            if not seen[v]:
                seen[v] = True
                stack.append(int(v))
    return int((~seen).sum())


def test_parallel_build_leaves_no_node_unreachable(c1, tmp_path):
    """C1's 1,702 windows at the fixture's parameters (M = 64, EFC = 128), 4 threads, three builds. A node inserted
    while the node it entered level 0 through was itself still being inserted used to lose its only in-link (14 to
    39 nodes per build). The oracle's searchKnn at ef = ntotal + 10 must return the fp32 restatement's distances."""
    from deepreadmapper_amd import synth
    q = c1["q"][:40]
    Dr, _ = R.l2sqr8_topk(c1["x"], q, 30)
    for r in range(3):
        path = str(tmp_path / f"b{r}.hnsw")
        synth.build_flat_index(c1["x"], path, M=64, efc=128, nthreads=4)
        fx = hnswlib_file.read(path)
        assert level0_unreachable(fx) == 0
        Do, _, _, _ = O.hnswlib_search(fx, q, 30, fx["n"] + 10)
        assert np.array_equal(Do.view(np.uint32), Dr.view(np.uint32))


def test_single_thread_build_unchanged_and_deterministic(c1, tmp_path):
    from deepreadmapper_amd import synth
    a, b = str(tmp_path / "a.hnsw"), str(tmp_path / "b.hnsw")
    synth.build_flat_index(c1["x"][:600], a, M=16, efc=64, nthreads=1)
    synth.build_flat_index(c1["x"][:600], b, M=16, efc=64, nthreads=1)
    assert open(a, "rb").read() == open(b, "rb").read()
    assert level0_unreachable(hnswlib_file.read(a)) == 0
