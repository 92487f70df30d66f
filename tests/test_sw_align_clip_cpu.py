"""CPU tests of the restatement of the end-aware affine-gap alignment (tests/sw_align_clip_ref.py, the text of
drm_sw_align_affine_clip in include/drm_hip.h): at penalty 0 it is drm_sw_align_affine's restatement, its records
replay to their score and keep inside the read, a penalty never loses against the local alignment once both have paid
for their ends, and a substitution a few bases from a read's end is aligned instead of clipped."""
import numpy as np
import pytest

import sw_align_affine_ref as A
import sw_align_clip_ref as K
import sw_align_ref as R

ACGT = list(b"ACGT")
SCORINGS = [(1, 4, 6, 1), (2, 4, 4, 2), (1, 1, 1, 1), (1, 3, 5, 2), (1, 1, 0, 1)]
PENALTIES = [1, 5, 17, 63]


def _rand(rng, n, letters=ACGT):
    return bytes(rng.choice(letters, size=n).astype(np.uint8))


def _mutated(rng, w, n_edits):
    s = list(w)
    for _ in range(n_edits):
        kind, at = int(rng.integers(4)), int(rng.integers(len(s)))
        if kind <= 1:
            s[at] = int(rng.choice(ACGT))
        elif kind == 2:
            s.insert(at, int(rng.choice(ACGT)))
        elif len(s) > 1:
            del s[at]
    return bytes(s)


def _pairs(seed, count, tags):
    """(window, query) pairs: short random strings over two and four letters, and mutated copies of a window with
    edits near the ends, wrapped in tag bytes that match nothing."""
    rng = np.random.default_rng(seed)
    out = []
    for x in range(count):
        if x % 3 == 0:
            letters = list(b"AC") if x % 2 else ACGT
            w, read = _rand(rng, int(rng.integers(1, 25)), letters), _rand(rng, int(rng.integers(1, 25)), letters)
        else:
            w = _rand(rng, int(rng.integers(20, 61)))
            read = bytearray(_mutated(rng, w, int(rng.integers(0, 4))))
            for at in (int(rng.integers(0, 4)), len(read) - 1 - int(rng.integers(0, 4))):
                if rng.integers(2):
                    read[at] = ord("A") if read[at] != ord("A") else ord("C")
            read = bytes(read)
        out.append((w, b"<" * tags[0] + read + b">" * tags[1]))
    return out


def test_row_at_a_time_matrices_equal_the_cell_by_cell_text():
    for tags in ((0, 0), (1, 1), (3, 2)):
        for x, (w, q) in enumerate(_pairs(11, 60, tags)):
            scoring, L = SCORINGS[x % len(SCORINGS)], [0] + PENALTIES
            for pen in (L[x % 5], L[(x + 2) % 5]):
                for got, want in zip(K.dp_matrices(w, q, scoring, pen, tags[0]),
                                     K.dp_matrices_plain(w, q, scoring, pen, tags[0])):
                    assert np.array_equal(got[1:, 1:], want[1:, 1:]) and np.array_equal(got[0], want[0])
                assert K.align(w, q, scoring, pen, tags) == K.align(w, q, scoring, pen, tags, K.dp_matrices_plain)


@pytest.mark.parametrize("tags", [(0, 0), (1, 1), (3, 2)])
def test_penalty_0_is_the_affine_alignment(tags):
    mapped = 0
    for x, (w, q) in enumerate(_pairs(20 + tags[0], 150, tags)):
        scoring = SCORINGS[x % len(SCORINGS)]
        want = A.align(w, q, scoring)
        assert K.align(w, q, scoring, 0, tags) == want, (w, q, scoring)
        mapped += want[0]["status"] == 0
    assert mapped > 100
    # tags that leave no read: no alignment, whatever the bytes
    assert K.align(b"ACGT", b"ACGT", (1, 1, 1, 1), 0, (3, 2)) == (K.NO_ALIGNMENT, [])
    assert K.align(b"ACGT", b"<ACGT", (1, 1, 1, 1), 0, (3, 2))[0]["status"] == 0  # b == a: no column, still a floor
    assert K.align(b"", b"<A>", (1, 1, 1, 1), 0) == (K.NO_ALIGNMENT, [])


@pytest.mark.parametrize("L", PENALTIES)
def test_records_replay_and_never_lose_to_the_local_alignment(L):
    changed = mapped = 0
    for tags in ((1, 1), (0, 0)):
        for x, (w, q) in enumerate(_pairs(40 + L, 160, tags)):
            scoring = SCORINGS[x % len(SCORINGS)]
            rec, ops = K.align(w, q, scoring, L, tags)
            local, lops = A.align(w, q, scoring)
            if rec["status"] == 1:
                # nothing is worth its ends; then neither is the local alignment
                assert local["status"] == 1 or K.adjusted_score(local, L, tags, len(q)) <= 0
                continue
            mapped += 1
            assert rec["n_ops"] == len(ops) >= 1
            assert A.replay(w, q, rec, ops, scoring) == (rec["score"], rec["nm"]), (w, q, scoring, rec)
            assert rec["q_begin"] >= tags[0] and rec["q_end"] <= len(q) - tags[1]
            assert local["status"] == 0 and rec["score"] <= local["score"]
            assert K.adjusted_score(rec, L, tags, len(q)) >= K.adjusted_score(local, L, tags, len(q))
            assert K.adjusted_score(rec, L, tags, len(q)) > 0
            changed += (rec, ops) != (local, lops)
    assert mapped > 150 and changed > 20


@pytest.mark.parametrize("column", [0, 2, 147, 149])
def test_a_substitution_near_an_end_is_aligned_not_clipped(column):
    rng = np.random.default_rng(7)
    w = _rand(rng, 150)
    read = bytearray(w)
    read[column] = ord("A") if read[column] != ord("A") else ord("C")
    q = b"<" + bytes(read) + b">"
    scoring = (1, 4, 6, 1)
    local, lops = A.align(w, q, scoring)
    lead, trail = (column + 1, 0) if column < 75 else (0, 150 - column)
    assert A.sam_fields_region(local, lops, 152, 0, 150, 0) == \
        (lead + 1, (f"{lead}S" if lead else "") + f"{150 - lead - trail}M" + (f"{trail}S" if trail else ""))
    assert local["score"] == 150 - lead - trail
    rec, ops = K.align(w, q, scoring, 5)
    assert A.sam_fields_region(rec, ops, 152, 0, 150, 0) == (1, "150M")
    assert (rec["score"], rec["nm"], rec["status"]) == (145, 1, 0)
    assert K.align(w, q, scoring, 0) == (local, lops)
