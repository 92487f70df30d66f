"""The SW rerank's bit-profile kernel on whole batches (`DRM_SW_BITPROFILE=1`).

The rerank launcher reads the variable once per process, so only a fresh process can switch every query to
`sw_score_kernel<64>` / `<152>` in full mode. `tests/test_gpu_rerank_dispatch.py` starts this script once as a child
with the variable set: it runs the fixed cases of `rerank_cases.cases()` and writes scores, ids and counts to an .npz,
which the parent compares with the oracle and with the default kernels' rows."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from rerank_cases import cases  # noqa: E402


def main(path):
    from deepreadmapper_amd import WindowTable, rerank_arrays
    res = {}
    for name, refs, nb, reads, stride, k, kc in cases():
        t = WindowTable(refs)
        sc, ids, cnt = rerank_arrays(t, nb, reads, stride, k, kc)
        t.free()
        res[name + ".scores"], res[name + ".ids"], res[name + ".counts"] = sc, ids, cnt
    np.savez(path, **res)


if __name__ == "__main__":
    main(sys.argv[1])
