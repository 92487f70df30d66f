"""Plain Python/numpy restatement of the alignment defined in include/drm_hip.h (drm_sw_align) -- a helper
for the tests, not a test. The reference has no traceback, so this file is what the GPU result must equal
on every pair; its DP is pinned to the reference's calc_sw_score by tests/test_sam_cigar_cpu.py."""
import numpy as np

M, I, D = 0, 1, 2  # BAM operation codes
FIELDS = ("score", "ref_begin", "ref_end", "q_begin", "q_end", "nm", "n_ops", "status")

_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ATCGN", b"TAGCN"):
    _COMP[_a] = _b


def revcomp(seq):
    """comp_table of the reference (src/utils/parse_inputs.cpp:5-14): anything but ACGTN becomes byte 0."""
    return bytes(_COMP[np.frombuffer(bytes(seq), dtype=np.uint8)[::-1]])


def window_bytes(genome, ref_len, wid):
    """find_sequence (src/utils/post_processor.cpp:47-64): genome[wid // 2 ..+ ref_len), reverse-complemented
    for odd wid, the empty string past the genome end."""
    g = bytes(genome)
    pos = wid // 2
    if pos + ref_len > len(g):
        return b""
    w = g[pos:pos + ref_len]
    return revcomp(w) if wid % 2 else w


def dp_matrix(w, q):
    w = np.frombuffer(bytes(w), dtype=np.uint8)
    q = np.frombuffer(bytes(q), dtype=np.uint8)
    n, m = len(w), len(q)
    H = np.zeros((n + 1, m + 1), dtype=np.int32)
    for i in range(1, n + 1):
        s = np.where(q == w[i - 1], 1, -1).astype(np.int32)
        base = np.maximum(np.maximum(H[i - 1, :-1] + s, H[i - 1, 1:] - 1), 0)  # without the left term
        # H[i][j] = max(base[j], H[i][j-1] - 1) = max_{k <= j} (base[k] - (j - k))
        idx = np.arange(1, m + 1, dtype=np.int32)
        H[i, 1:] = np.maximum.accumulate(base + idx) - idx
    return H


def align(w, q):
    """(record dict, ops list of BAM words in forward order) by the rules of include/drm_hip.h."""
    w, q = bytes(w), bytes(q)
    H = dp_matrix(w, q)
    score = int(H.max()) if H.size else 0
    if score == 0:
        return dict.fromkeys(FIELDS, 0) | {"status": 1}, []
    cells = np.argwhere(H == score)  # row-major: smallest i first, then smallest j
    i, j = int(cells[0][0]), int(cells[0][1])
    i_end, j_end = i, j
    steps, nm = [], 0
    while H[i, j] > 0:
        s = 1 if w[i - 1] == q[j - 1] else -1
        if H[i, j] == H[i - 1, j - 1] + s:
            steps.append(M)
            nm += s < 0
            i, j = i - 1, j - 1
        elif H[i, j] == H[i - 1, j] - 1:
            steps.append(D)
            nm += 1
            i -= 1
        else:
            assert H[i, j] == H[i, j - 1] - 1
            steps.append(I)
            nm += 1
            j -= 1
    steps.reverse()
    ops = []
    for op in steps:
        if ops and (ops[-1] & 15) == op:
            ops[-1] += 16
        else:
            ops.append((1 << 4) | op)
    rec = {"score": score, "ref_begin": i, "ref_end": i_end, "q_begin": j, "q_end": j_end, "nm": int(nm),
           "n_ops": len(ops), "status": 0}
    return rec, ops


def replay(w, q, record, ops):
    """(score, nm, first column is a match, last column is a match) recomputed from the operations alone."""
    w, q = bytes(w), bytes(q)
    i, j = int(record["ref_begin"]), int(record["q_begin"])
    score = nm = 0
    cols = []
    for word in ops:
        n, op = int(word) >> 4, int(word) & 15
        for _ in range(n):
            if op == M:
                eq = w[i] == q[j]
                score += 1 if eq else -1
                nm += not eq
                cols.append(bool(eq))
                i, j = i + 1, j + 1
            elif op == D:
                score, nm, i = score - 1, nm + 1, i + 1
                cols.append(False)
            else:
                assert op == I
                score, nm, j = score - 1, nm + 1, j + 1
                cols.append(False)
    assert i == int(record["ref_end"]) and j == int(record["q_end"]), "operations do not span the record"
    return score, nm, bool(cols and cols[0]), bool(cols and cols[-1])


def cigar_string(ops):
    return "".join(f"{int(x) >> 4}{'MID'[int(x) & 15]}" for x in ops)


def sam_fields(record, ops, q_len, ref_len, window_id, tags=(1, 1)):
    """(pos1, cigar) by drm_sam_cigar's rules."""
    lead = int(record["q_begin"]) - tags[0]
    trail = (q_len - tags[1]) - int(record["q_end"])
    assert lead >= 0 and trail >= 0
    parts = ([f"{lead}S"] if lead else []) + [cigar_string([x]) for x in ops] + ([f"{trail}S"] if trail else [])
    if window_id % 2:
        return window_id // 2 + (ref_len - int(record["ref_end"])) + 1, "".join(reversed(parts))
    return window_id // 2 + int(record["ref_begin"]) + 1, "".join(parts)


def cigar_query_length(cigar):
    """Query bases a CIGAR consumes (M, I, S)."""
    import re
    return sum(int(n) for n, op in re.findall(r"(\d+)([MIDS])", cigar) if op in "MIS")

