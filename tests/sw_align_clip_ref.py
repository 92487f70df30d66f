"""Plain Python/numpy restatement of the end-aware affine-gap alignment defined in include/drm_hip.h
(drm_sw_align_affine_clip) -- a helper for the tests, not a test. A scoring is (match, mismatch, gap_open, gap_extend),
L the clipping penalty, tags (tag_prefix, tag_postfix): the read is query columns a + 1 .. b with a = tag_prefix and
b = len(q) - tag_postfix. dp_matrices_plain is the text cell by cell; dp_matrices is the same a row at a time, which
tests/test_sw_align_clip_cpu.py pins to it, and align walks either."""
import numpy as np

from sw_align_affine_ref import NEG, replay  # noqa: F401  (replay: the score of the printed walk)
from sw_align_ref import D, FIELDS, I, M

NO_ALIGNMENT = dict.fromkeys(FIELDS, 0) | {"status": 1}


def floors(m, a, L):
    """floor(j) for j = 0..m."""
    return [0 if j <= a else -L for j in range(m + 1)]


def dp_matrices_plain(w, q, scoring, L, a):
    """(H, E, F) of the recurrence cell by cell, as written in the header, each (n + 1) x (m + 1)."""
    match, mismatch, gap_open, gap_extend = scoring
    w, q = bytes(w), bytes(q)
    n, m = len(w), len(q)
    fl = floors(m, a, L)
    H = [[0] * (m + 1) for _ in range(n + 1)]
    E = [[NEG] * (m + 1) for _ in range(n + 1)]
    F = [[NEG] * (m + 1) for _ in range(n + 1)]
    H[0] = list(fl)  # H[0][j] = floor(j); H[i][0] = 0 = floor(0)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            F[i][j] = max(H[i - 1][j] - gap_open - gap_extend, F[i - 1][j] - gap_extend)
            E[i][j] = max(H[i][j - 1] - gap_open - gap_extend, E[i][j - 1] - gap_extend)
            s = match if w[i - 1] == q[j - 1] else -mismatch
            H[i][j] = max(fl[j], H[i - 1][j - 1] + s, F[i][j], E[i][j])
    return np.array(H, dtype=np.int64), np.array(E, dtype=np.int64), np.array(F, dtype=np.int64)


def dp_matrices(w, q, scoring, L, a):
    """dp_matrices_plain a row at a time (sw_align_affine_ref.dp_matrices with the floor a vector)."""
    match, mismatch, gap_open, gap_extend = scoring
    w = np.frombuffer(bytes(w), dtype=np.uint8)
    q = np.frombuffer(bytes(q), dtype=np.uint8)
    n, m = len(w), len(q)
    fl = np.array(floors(m, a, L), dtype=np.int64)
    H = np.zeros((n + 1, m + 1), dtype=np.int64)
    H[0] = fl
    E = np.full((n + 1, m + 1), NEG, dtype=np.int64)
    F = np.full((n + 1, m + 1), NEG, dtype=np.int64)
    oe = gap_open + gap_extend
    idx = np.arange(m + 1, dtype=np.int64) * gap_extend
    base = np.zeros(m + 1, dtype=np.int64)  # H without the E term; base[0] = H[i][0] = 0
    for i in range(1, n + 1):
        s = np.where(q == w[i - 1], match, -mismatch).astype(np.int64)
        F[i, 1:] = np.maximum(H[i - 1, 1:] - oe, F[i - 1, 1:] - gap_extend)
        base[1:] = np.maximum(np.maximum(H[i - 1, :-1] + s, F[i, 1:]), fl[1:])
        # an H[i][k] that is itself E[i][k] never opens the winning gap, so base stands in for H
        E[i, 1:] = np.maximum.accumulate(base + idx)[:-1] - gap_open - idx[1:]
        H[i, 1:] = np.maximum(base[1:], E[i, 1:])
    return H, E, F


def adjusted(H, L, b):
    """adj(i, j) over i >= 1, j >= 1 (an (n x m) array), None when there is no cell."""
    if H.shape[0] < 2 or H.shape[1] < 2:
        return None
    adj = H[1:, 1:] - L
    if 1 <= b < H.shape[1]:
        adj[:, b - 1] += L
    return adj


def align(w, q, scoring, L, tags=(1, 1), matrices=dp_matrices):
    """(record dict, ops list of BAM words in forward order) by the rules of drm_sw_align_affine_clip."""
    match, mismatch, gap_open, gap_extend = scoring
    w, q = bytes(w), bytes(q)
    a, b = tags[0], len(q) - tags[1]
    if b < a:
        return dict(NO_ALIGNMENT), []
    H, E, F = matrices(w, q, scoring, L, a)
    fl = floors(len(q), a, L)
    adj = adjusted(H, L, b)
    if adj is None or int(adj.max()) <= 0:
        return dict(NO_ALIGNMENT), []
    best = int(adj.max())
    cells = np.argwhere(adj == best)  # row-major: smallest i first, then smallest j
    i, j = int(cells[0][0]) + 1, int(cells[0][1]) + 1
    i_end, j_end = i, j
    oe = gap_open + gap_extend
    steps, nm, state = [], 0, "H"
    while True:
        if state == "H":
            if i == 0 or j == 0 or H[i, j] == fl[j]:
                break
            s = match if w[i - 1] == q[j - 1] else -mismatch
            if H[i, j] == H[i - 1, j - 1] + s:
                steps.append(M)
                nm += s < 0
                i, j = i - 1, j - 1
            elif H[i, j] == F[i, j]:
                state = "F"
            else:
                assert H[i, j] == E[i, j]
                state = "E"
        elif state == "F":
            steps.append(D)
            nm += 1
            if F[i, j] == H[i - 1, j] - oe:  # closing the gap wins a tie against extending it
                state = "H"
            else:
                assert F[i, j] == F[i - 1, j] - gap_extend
            i -= 1
        else:
            steps.append(I)
            nm += 1
            if E[i, j] == H[i, j - 1] - oe:
                state = "H"
            else:
                assert E[i, j] == E[i, j - 1] - gap_extend
            j -= 1
    steps.reverse()
    ops = []
    for op in steps:
        if ops and (ops[-1] & 15) == op:
            ops[-1] += 16
        else:
            ops.append((1 << 4) | op)
    score = best + L * (j > a) + L * (j_end != b)
    rec = {"score": score, "ref_begin": i, "ref_end": i_end, "q_begin": j, "q_end": j_end, "nm": int(nm),
           "n_ops": len(ops), "status": 0}
    return rec, ops


def adjusted_score(record, L, tags, q_len):
    """What a record's walk is worth once it has paid for the ends it does not reach."""
    a, b = tags[0], q_len - tags[1]
    return int(record["score"]) - L * (int(record["q_begin"]) > a) - L * (int(record["q_end"]) != b)
