"""Child of test_gpu_rerank_chunks.py: started with DRM_SW_BITPROFILE=1 (read once per process), it scores the
batches of the .npz given as argv[1] (refs, and per batch i nb<i>, q<i>, ql<i>; k = the list length) with the
bit-profile kernel alone and writes sc<i>, ids<i>, cnt<i> to argv[2]."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from deepreadmapper_amd import WindowTable, rerank_arrays  # noqa: E402

assert os.environ.get("DRM_SW_BITPROFILE") == "1"
src = np.load(sys.argv[1])
t = WindowTable(src["refs"])
out = {}
i = 0
while f"nb{i}" in src:
    nb = src[f"nb{i}"]
    out[f"sc{i}"], out[f"ids{i}"], out[f"cnt{i}"] = rerank_arrays(t, nb, (src[f"q{i}"], src[f"ql{i}"]), 1, nb.shape[1],
                                                                 nb.shape[1])
    i += 1
t.free()
np.savez(sys.argv[2], **out)
