"""CPU tests of the SAM CIGAR path: the Python restatement of the alignment (tests/sw_align_ref.py) is pinned to
the reference's calc_sw_score, its operations replay to its score, and the host-only drm_sam_cigar turns
hand-written records into POS / CIGAR by the rules of include/drm_hip.h."""
import ctypes as C

import numpy as np
import pytest

import sw_align_ref as R
from oracle import oracle as O

KNOWN = [(b"AAAAAAAA", b"<AAAA>"), (b"ACACACACAC", b"<ACAC>"), (b"AAAACCCC", b"<AAAATCCCC>"),
         (b"AAAATCCCC", b"<AAAACCCC>"), (b"GGGG", b"<TTTT>"), (b"A", b"A")]


def _edited(rng, w, edits=3):
    """w with `edits` random substitutions / insertions / deletions, tagged like format_fastq."""
    s = list(w)
    for _ in range(edits):
        kind, pos = int(rng.integers(3)), int(rng.integers(1, len(s) - 1))
        if kind == 0:
            s[pos] = int(rng.choice([c for c in b"ACGT" if c != s[pos]]))
        elif kind == 1:
            s.insert(pos, int(rng.choice(list(b"ACGT"))))
        else:
            del s[pos]
    return b"<" + bytes(s) + b">"


def _inputs():
    rng = np.random.default_rng(20)
    pairs = list(KNOWN)
    for n in (40, 150):
        for _ in range(6):
            w = bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))
            pairs.append((w, _edited(rng, w)))
    pairs.append((b"A" * 40, b"<" + b"A" * 37 + b">"))                   # homopolymer, deletion
    pairs.append((b"T" * 30, b"<" + b"T" * 12 + b"G" + b"T" * 20 + b">"))  # homopolymer, longer query
    pairs.append((b"ACG" * 14, b"<" + b"ACG" * 6 + b"AC" + b"ACG" * 7 + b">"))  # tandem repeat, one base lost
    pairs.append((b"CA" * 20, b"<" + b"CA" * 9 + b"CCA" + b"CA" * 10 + b">"))   # tandem repeat, one base added
    pairs.append((b"ACGTNNACGT", b"<ACGTNNACGT>"))                        # N matches N
    pairs.append((b"", b"<ACGT>"))
    return pairs


INPUTS = _inputs()


def test_restatement_score_is_calc_sw_score():
    for w, q in INPUTS:
        rec, _ = R.align(w, q)
        assert rec["score"] == O.calc_sw_score(w, q), (w, q)


def test_operations_replay_to_the_score():
    seen = set()
    for w, q in INPUTS:
        rec, ops = R.align(w, q)
        if rec["status"] == 1:
            assert rec["score"] == 0 and not ops
            continue
        score, nm, first, last = R.replay(w, q, rec, ops)
        assert (score, nm) == (rec["score"], rec["nm"]), (w, q)
        assert first and last, (w, q)  # so the tags are never inside the alignment
        seen |= {int(x) & 15 for x in ops}
    assert seen == {R.M, R.I, R.D}


def test_known_answers_of_the_restatement():
    want = [((0, 4, 1, 5), "4M", 4), ((0, 4, 1, 5), "4M", 4), ((0, 8, 1, 10), "4M1I4M", 7), ((0, 9, 1, 9), "4M1D4M", 7)]
    for (w, q), (span, cigar, score) in zip(KNOWN, want):
        rec, ops = R.align(w, q)
        assert (rec["ref_begin"], rec["ref_end"], rec["q_begin"], rec["q_end"]) == span
        assert R.cigar_string(ops) == cigar and rec["score"] == score
    assert R.align(*KNOWN[4])[0]["status"] == 1
    rec, ops = R.align(*KNOWN[5])
    assert rec["score"] == 1 and R.cigar_string(ops) == "1M" and rec["nm"] == 0


# ------------------------------------------------------------------------------------------ drm_sam_cigar
def _rec(score=0, ref_begin=0, ref_end=0, q_begin=0, q_end=0, nm=0, n_ops=0, status=0):
    return dict(score=score, ref_begin=ref_begin, ref_end=ref_end, q_begin=q_begin, q_end=q_end, nm=nm, n_ops=n_ops,
                status=status)


def _w(n, op):
    return (n << 4) | op


def test_sam_cigar_forward_with_both_clips():
    from deepreadmapper_amd import sam_cigar
    # read of 20 bases in a 22-byte tagged query: bases 3..17 align to window bytes 5..20 of window 2 * 100
    rec = _rec(score=15, ref_begin=5, ref_end=20, q_begin=4, q_end=19, n_ops=1)
    assert sam_cigar(rec, [_w(15, R.M)], 22, 150, 200) == (100 + 5 + 1, "3S15M2S")
    assert sam_cigar(rec, [_w(15, R.M)], 22, 150, 200) == R.sam_fields(rec, [_w(15, R.M)], 22, 150, 200)


def test_sam_cigar_no_clips():
    from deepreadmapper_amd import sam_cigar
    rec = _rec(score=150, ref_begin=0, ref_end=150, q_begin=1, q_end=151, n_ops=1)
    assert sam_cigar(rec, [_w(150, R.M)], 152, 150, 0) == (1, "150M")


def test_sam_cigar_insertion_and_deletion():
    from deepreadmapper_amd import sam_cigar
    ops = [_w(10, R.M), _w(2, R.I), _w(20, R.M), _w(1, R.D), _w(7, R.M)]
    rec = _rec(score=30, ref_begin=3, ref_end=41, q_begin=1, q_end=40, nm=3, n_ops=5)
    assert sam_cigar(rec, ops, 42, 150, 2 * 7) == (7 + 3 + 1, "10M2I20M1D7M1S")


def test_sam_cigar_odd_id_reverses_operations_and_flips_pos():
    from deepreadmapper_amd import sam_cigar
    ops = [_w(10, R.M), _w(2, R.I), _w(20, R.M), _w(1, R.D), _w(7, R.M)]
    rec = _rec(score=30, ref_begin=3, ref_end=41, q_begin=3, q_end=42, nm=3, n_ops=5)
    # the read is q[1:46]: leading clip 3 - 1 = 2, trailing clip 46 - 42 = 4; on the forward strand they swap
    pos1, cigar = sam_cigar(rec, ops, 47, 150, 2 * 7 + 1)
    assert cigar == "4S7M1D20M2I10M2S"
    assert pos1 == 7 + (150 - 41) + 1
    assert (pos1, cigar) == R.sam_fields(rec, ops, 47, 150, 15)


def test_sam_cigar_without_tags():
    from deepreadmapper_amd import sam_cigar
    rec = _rec(score=8, ref_begin=2, ref_end=10, q_begin=0, q_end=8, n_ops=1)
    assert sam_cigar(rec, [_w(8, R.M)], 8, 40, 6, tags=(0, 0)) == (3 + 2 + 1, "8M")
    assert sam_cigar(rec, [_w(8, R.M)], 10, 40, 6, tags=(0, 0)) == (6, "8M2S")


def test_sam_cigar_errors():
    from deepreadmapper_amd import DrmError, sam_cigar
    from deepreadmapper_amd._native import DRM_ERR_ARG, lib
    from deepreadmapper_amd.rerank import SW_ALIGNMENT_DTYPE
    r = np.zeros(1, dtype=SW_ALIGNMENT_DTYPE)
    r[0] = (15, 5, 20, 4, 19, 0, 1, 0)
    ops = np.array([_w(15, R.M)], dtype=np.uint32)
    pos, buf = C.c_int64(0), C.create_string_buffer(16)

    def call(cap):
        return lib().drm_sam_cigar(r.ctypes.data, ops.ctypes.data, 22, 1, 1, 150, 200, C.byref(pos), buf, cap)

    assert call(8) == 0 and buf.value == b"3S15M2S" and pos.value == 106  # 7 characters + NUL
    assert call(7) == DRM_ERR_ARG and b"cigar_cap" in lib().drm_last_error()
    with pytest.raises(DrmError) as e:  # status 1: there is no alignment to describe
        sam_cigar(_rec(status=1), [], 22, 150, 200)
    assert e.value.code == DRM_ERR_ARG


def test_version_minor_bumped():
    from deepreadmapper_amd._native import lib
    assert lib().drm_version() >= 200
