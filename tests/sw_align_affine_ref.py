"""Plain Python/numpy restatement of the affine-gap alignment defined in include/drm_hip.h (drm_sw_align_affine)
-- a helper for the tests, not a test. A scoring is (match, mismatch, gap_open, gap_extend), the last three being
penalties; at (1, 1, 0, 1) the definition equals drm_sw_align's (tests/sw_align_ref.py), which
tests/test_sam_cigar_region_cpu.py pins."""
import numpy as np

from sw_align_ref import D, FIELDS, I, M, cigar_string, revcomp

NEG = -(1 << 28)  # the borders' minus infinity


def region(genome, ref_len, wid, flank):
    """(start, length, reverse) of window id wid's target region on a genome: genome[wid // 2 ..+ ref_len) widened
    by flank bases on either side and clamped to the genome; length 0 when the window runs past the genome end."""
    glen, pos = len(genome), wid // 2
    if pos + ref_len > glen:
        return 0, 0, wid % 2
    s, e = max(0, pos - flank), min(glen, pos + ref_len + flank)
    return s, e - s, wid % 2


def region_bytes(genome, ref_len, wid, flank):
    g = bytes(genome)
    s, n, rev = region(g, ref_len, wid, flank)
    r = g[s:s + n]
    return revcomp(r) if rev else r


def dp_matrices(w, q, scoring):
    """(H, E, F) of the Gotoh recurrence, each (n + 1) x (m + 1)."""
    match, mismatch, gap_open, gap_extend = scoring
    w = np.frombuffer(bytes(w), dtype=np.uint8)
    q = np.frombuffer(bytes(q), dtype=np.uint8)
    n, m = len(w), len(q)
    H = np.zeros((n + 1, m + 1), dtype=np.int64)
    E = np.full((n + 1, m + 1), NEG, dtype=np.int64)
    F = np.full((n + 1, m + 1), NEG, dtype=np.int64)
    oe = gap_open + gap_extend
    idx = np.arange(m + 1, dtype=np.int64) * gap_extend
    base = np.zeros(m + 1, dtype=np.int64)  # H without the E term; base[0] = H[i][0] = 0
    for i in range(1, n + 1):
        s = np.where(q == w[i - 1], match, -mismatch).astype(np.int64)
        F[i, 1:] = np.maximum(H[i - 1, 1:] - oe, F[i - 1, 1:] - gap_extend)
        base[1:] = np.maximum(np.maximum(H[i - 1, :-1] + s, F[i, 1:]), 0)
        # E[i][j] = max_{k < j} (H[i][k] - open - (j - k) * ext), and an H[i][k] that is itself E[i][k] never wins
        # (opening costs at least what extending does), so base stands in for H (dp_matrices_plain is the loop)
        E[i, 1:] = np.maximum.accumulate(base + idx)[:-1] - gap_open - idx[1:]
        H[i, 1:] = np.maximum(base[1:], E[i, 1:])
    return H, E, F


def dp_matrices_plain(w, q, scoring):
    """The recurrence cell by cell, as written in the header: what dp_matrices must equal."""
    match, mismatch, gap_open, gap_extend = scoring
    w, q = bytes(w), bytes(q)
    n, m = len(w), len(q)
    H = [[0] * (m + 1) for _ in range(n + 1)]
    E = [[NEG] * (m + 1) for _ in range(n + 1)]
    F = [[NEG] * (m + 1) for _ in range(n + 1)]
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            F[i][j] = max(H[i - 1][j] - gap_open - gap_extend, F[i - 1][j] - gap_extend)
            E[i][j] = max(H[i][j - 1] - gap_open - gap_extend, E[i][j - 1] - gap_extend)
            s = match if w[i - 1] == q[j - 1] else -mismatch
            H[i][j] = max(0, H[i - 1][j - 1] + s, F[i][j], E[i][j])
    return np.array(H, dtype=np.int64), np.array(E, dtype=np.int64), np.array(F, dtype=np.int64)


def align(w, q, scoring):
    """(record dict, ops list of BAM words in forward order) by the rules of drm_sw_align_affine."""
    match, mismatch, gap_open, gap_extend = scoring
    w, q = bytes(w), bytes(q)
    H, E, F = dp_matrices(w, q, scoring)
    score = int(H.max()) if H.size else 0
    if score == 0:
        return dict.fromkeys(FIELDS, 0) | {"status": 1}, []
    cells = np.argwhere(H == score)  # row-major: smallest i first, then smallest j
    i, j = int(cells[0][0]), int(cells[0][1])
    i_end, j_end = i, j
    oe = gap_open + gap_extend
    steps, nm, state = [], 0, "H"
    while True:
        if state == "H":
            if H[i, j] == 0 or i == 0 or j == 0:
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
    rec = {"score": score, "ref_begin": i, "ref_end": i_end, "q_begin": j, "q_end": j_end, "nm": int(nm),
           "n_ops": len(ops), "status": 0}
    return rec, ops


def replay(w, q, record, ops, scoring):
    """(score, nm) recomputed from the operations alone: every run of I or D words is one gap of its length."""
    match, mismatch, gap_open, gap_extend = scoring
    w, q = bytes(w), bytes(q)
    i, j = int(record["ref_begin"]), int(record["q_begin"])
    score = nm = 0
    for word in ops:
        n, op = int(word) >> 4, int(word) & 15
        if op == M:
            for _ in range(n):
                eq = w[i] == q[j]
                score += match if eq else -mismatch
                nm += not eq
                i, j = i + 1, j + 1
        else:
            assert op in (I, D)
            score -= gap_open + n * gap_extend
            nm += n
            if op == D:
                i += n
            else:
                j += n
    assert i == int(record["ref_end"]) and j == int(record["q_end"]), "operations do not span the record"
    return score, nm


def sam_fields_region(record, ops, q_len, region_start, region_len, reverse, tags=(1, 1)):
    """(pos1, cigar) by drm_sam_cigar_region's rules."""
    lead = int(record["q_begin"]) - tags[0]
    trail = (q_len - tags[1]) - int(record["q_end"])
    assert lead >= 0 and trail >= 0
    parts = ([f"{lead}S"] if lead else []) + [cigar_string([x]) for x in ops] + ([f"{trail}S"] if trail else [])
    if reverse:
        return region_start + (region_len - int(record["ref_end"])) + 1, "".join(reversed(parts))
    return region_start + int(record["ref_begin"]) + 1, "".join(parts)
