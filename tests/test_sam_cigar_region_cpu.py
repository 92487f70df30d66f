"""CPU tests of the region form of the SAM CIGAR path: the host-only drm_sam_cigar_region, its agreement with
drm_sam_cigar on a window id's own region, and the Python restatement of the affine-gap alignment
(tests/sw_align_affine_ref.py), which at (1, 1, 0, 1) must equal the restatement of drm_sw_align."""
import ctypes as C

import numpy as np
import pytest

import sw_align_affine_ref as A
import sw_align_ref as R

SCORINGS = [(1, 4, 6, 1), (2, 4, 4, 2), (1, 1, 1, 1), (1, 3, 5, 2)]


def _rec(**kw):
    return dict(dict.fromkeys(R.FIELDS, 0), **kw)


def _w(n, op):
    return (n << 4) | op


def _random_pairs(seed, count, max_len):
    rng = np.random.default_rng(seed)
    for t in range(count):
        letters = list(b"AC" if t % 2 else b"ACGT")  # two letters: many ties
        w = bytes(rng.choice(letters, size=int(rng.integers(0, max_len + 1))).astype(np.uint8))
        q = bytes(rng.choice(letters, size=int(rng.integers(0, max_len + 1))).astype(np.uint8))
        yield w, q


# ------------------------------------------------------------------------------------------ the restatement
def test_restatement_at_1_1_0_1_equals_the_linear_definition():
    for w, q in _random_pairs(11, 4000, 14):
        assert A.align(w, q, (1, 1, 0, 1)) == R.align(w, q), (w, q)


def test_restatement_matrices_equal_the_cell_by_cell_recurrence():
    for w, q in _random_pairs(12, 300, 12):
        for sc in SCORINGS + [(1, 1, 0, 1)]:
            for got, want in zip(A.dp_matrices(w, q, sc), A.dp_matrices_plain(w, q, sc)):
                assert np.array_equal(got, want), (w, q, sc)


@pytest.mark.parametrize("scoring", SCORINGS)
def test_restatement_operations_replay_to_the_score(scoring):
    aligned = 0
    for w, q in _random_pairs(13, 1500, 16):
        rec, ops = A.align(w, q, scoring)
        if rec["status"] == 0:
            assert A.replay(w, q, rec, ops, scoring) == (rec["score"], rec["nm"]), (w, q)
            aligned += 1
    assert aligned > 1000


def test_restatement_known_affine_answers():
    x, y = b"ACGTACGTTAGACCAGTACC", b"GGATCCATTGCAAGCTTGCA"
    w, q = x + b"TGA" + y, x + y
    rec, ops = A.align(w, q, (1, 4, 6, 1))  # a gap of 3 costs 6 + 3 * 1
    assert R.cigar_string(ops) == "20M3D20M" and rec["score"] == 40 - 9 and rec["nm"] == 3
    rec, ops = A.align(q, w, (1, 4, 6, 1))
    assert R.cigar_string(ops) == "20M3I20M" and rec["score"] == 31
    assert (rec["ref_begin"], rec["ref_end"], rec["q_begin"], rec["q_end"]) == (0, 40, 0, 43)
    rec, ops = A.align(q, w, (1, 4, 20, 1))  # a gap dearer than either half is worth: one half alone, the upper
    assert R.cigar_string(ops) == "20M" and rec["score"] == 20 and rec["ref_end"] == 20  # one (smallest i)


def test_region_helper():
    g = bytes(range(65, 91)) * 4  # 104 bytes
    assert A.region(g, 10, 2 * 20, 3) == (17, 16, 0)
    assert A.region(g, 10, 2 * 20 + 1, 3) == (17, 16, 1)
    assert A.region(g, 10, 2 * 1, 3) == (0, 14, 0)
    assert A.region(g, 10, 2 * 94, 3) == (91, 13, 0)
    assert A.region(g, 10, 2 * 95, 3) == (0, 0, 0)
    assert A.region_bytes(g, 10, 2 * 20, 0) == R.window_bytes(g, 10, 2 * 20)
    assert A.region_bytes(b"ACGTTGCAAT", 4, 2 * 3 + 1, 2) == R.revcomp(b"CGTTGCAA")


# ------------------------------------------------------------------------------------------ drm_sam_cigar_region
def test_region_forward_with_both_clips():
    from deepreadmapper_amd import sam_cigar_region
    rec = _rec(score=15, ref_begin=5, ref_end=20, q_begin=4, q_end=19, n_ops=1)
    assert sam_cigar_region(rec, [_w(15, R.M)], 22, 92, 166, 0) == (92 + 5 + 1, "3S15M2S")
    assert sam_cigar_region(rec, [_w(15, R.M)], 22, 92, 166, 0) == A.sam_fields_region(rec, [_w(15, R.M)], 22, 92, 166, 0)


def test_region_forward_without_clips():
    from deepreadmapper_amd import sam_cigar_region
    rec = _rec(score=150, ref_begin=9, ref_end=159, q_begin=1, q_end=151, n_ops=1)
    assert sam_cigar_region(rec, [_w(150, R.M)], 152, 0, 158, 0) == (10, "150M")


def test_region_reverse_flips_pos_and_operations():
    from deepreadmapper_amd import sam_cigar_region
    ops = [_w(10, R.M), _w(2, R.I), _w(20, R.M), _w(5, R.D), _w(7, R.M)]
    rec = _rec(score=20, ref_begin=3, ref_end=45, q_begin=3, q_end=42, n_ops=5)
    pos1, cigar = sam_cigar_region(rec, ops, 47, 1000, 166, 1)
    assert cigar == "4S7M5D20M2I10M2S"
    assert pos1 == 1000 + (166 - 45) + 1
    assert (pos1, cigar) == A.sam_fields_region(rec, ops, 47, 1000, 166, 1)
    pos1, cigar = sam_cigar_region(rec, ops, 44, 1000, 166, 1, tags=(3, 2))  # the clips come from the tags given
    assert (pos1, cigar) == (1000 + 121 + 1, "7M5D20M2I10M")


def test_region_form_equals_window_form_on_the_windows_own_region():
    from deepreadmapper_amd import sam_cigar, sam_cigar_region
    rng = np.random.default_rng(21)
    for _ in range(48):
        ref_len = int(rng.integers(20, 200))
        wid = int(rng.integers(0, 10 ** 9))
        runs = [(int(rng.integers(1, 9)), int(op)) for op in rng.choice([R.M, R.I, R.D], size=int(rng.integers(1, 7)))]
        runs = [(n, op) for x, (n, op) in enumerate(runs) if x == 0 or runs[x - 1][1] != op]
        ref_span = sum(n for n, op in runs if op != R.I)
        q_span = sum(n for n, op in runs if op != R.D)
        if ref_span > ref_len:
            continue
        rb = int(rng.integers(0, ref_len - ref_span + 1))
        qb = int(rng.integers(1, 6))
        q_len = qb + q_span + int(rng.integers(1, 6))
        rec = _rec(score=1, ref_begin=rb, ref_end=rb + ref_span, q_begin=qb, q_end=qb + q_span, n_ops=len(runs))
        ops = [_w(n, op) for n, op in runs]
        assert sam_cigar_region(rec, ops, q_len, wid // 2, ref_len, wid & 1) == sam_cigar(rec, ops, q_len, ref_len, wid)
        assert sam_cigar(rec, ops, q_len, ref_len, wid) == R.sam_fields(rec, ops, q_len, ref_len, wid)


def test_region_errors():
    from deepreadmapper_amd import DrmError, sam_cigar_region
    from deepreadmapper_amd._native import DRM_ERR_ARG, lib
    ops = np.array([_w(15, R.M)], dtype=np.uint32)

    def raw(rec, cap, q_len=22):
        r = np.array([tuple(rec[f] for f in R.FIELDS)], dtype=[(f, np.int32) for f in R.FIELDS])
        pos, buf = C.c_int64(0), C.create_string_buffer(64)
        return lib().drm_sam_cigar_region(r.ctypes.data, ops.ctypes.data, q_len, 1, 1, 92, 166, 1, C.byref(pos), buf, cap)
    good = _rec(score=15, ref_begin=5, ref_end=20, q_begin=4, q_end=19, n_ops=1)
    assert raw(good, 64) == 0
    assert raw(good, len("2S15M3S") + 1) == 0
    assert raw(good, len("2S15M3S")) == DRM_ERR_ARG  # no room for the NUL
    assert raw(_rec(status=1), 64) == DRM_ERR_ARG
    assert raw(dict(good, status=2), 64) == DRM_ERR_ARG
    assert raw(dict(good, q_begin=0), 64) == DRM_ERR_ARG  # the alignment starts on the "<" tag
    assert raw(good, 64, q_len=19) == DRM_ERR_ARG  # ... or ends on the ">" tag
    with pytest.raises(DrmError) as e:
        sam_cigar_region(_rec(status=1), [], 22, 92, 166, 0)
    assert e.value.code == DRM_ERR_ARG
