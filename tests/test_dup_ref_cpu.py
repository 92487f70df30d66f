"""CPU tests of the duplicate marking's host side and of its restatement (tests/dup_ref.py): the header's examples,
the reference's independence of how a run is cut into calls, drm_sam_end5 against the unclipped 5' end parsed back
from the printed POS and CIGAR, the error cases, the slot hash, and the proof that the small tables of
tests/test_gpu_dup.py hold a chain of three slots and a walk that wraps."""
import ctypes as C

import numpy as np
import pytest

import dup_ref as D
import sw_align_affine_ref as A
import sw_align_ref as R


def _rec(**kw):
    return dict(dict.fromkeys(R.FIELDS, 0), **kw)


# ------------------------------------------------------------------------------------------ the header's examples
def test_header_examples():
    from deepreadmapper_amd import dup_end_word, sam_end5
    rec = _rec(score=15, ref_begin=5, ref_end=20, q_begin=4, q_end=19, n_ops=1)
    assert sam_end5(rec, 1, 92, 166, 0) == D.end5(rec, 1, 92, 166, 0) == 94
    assert sam_end5(rec, 1, 92, 166, 1) == D.end5(rec, 1, 92, 166, 1) == 255
    assert sam_end5(_rec(ref_begin=0, q_begin=10), 1, 3, 150, 0) == -6  # a clip longer than the distance to the start
    assert dup_end_word(0, 0) == D.end_word(0, 0) == (1 << 21) + 1
    assert dup_end_word(-(1 << 20), 1) == D.end_word(-(1 << 20), 1) == 2
    assert dup_end_word(94, 1) == D.end_word(94, 1) == (((1 << 20) + 94) << 1) + 2
    assert dup_end_word((1 << 61) - 1, 1) == D.end_word((1 << 61) - 1, 1) < 1 << 64
    # the strand is part of the word, and no word is 0
    assert dup_end_word(7, 0) != dup_end_word(7, 1) and dup_end_word(-(1 << 20), 0) == 1


def test_key_is_the_unordered_pair():
    assert D.key(9, 5) == D.key(5, 9) == (5, 9)
    assert D.key(5, 0) == D.key(0, 5) == (0, 5)
    assert D.key(0, 0) is None


def test_reference_does_not_depend_on_the_cuts():
    ends = D.half_repeated(3, 500)
    whole = D.FirstSeen(500).mark(ends)
    dup = (whole >= 0) & (whole != np.arange(500))
    assert 150 < dup.sum() < 350 and (whole <= np.arange(500)).all()
    for cuts in ([250], [1, 2, 499], [7, 7, 100, 333, 334], list(range(1, 500))):
        s, got, lo = D.FirstSeen(500), [], 0
        for hi in cuts + [500]:
            got.append(s.mark(ends[lo:hi]))
            lo = hi
        assert np.array_equal(np.concatenate(got), whole), cuts
    # (e, 0) duplicates only (e, 0); (0, 0) never; swapped mates do
    s = D.FirstSeen(8)
    assert list(s.mark([(5, 9), (9, 5), (5, 0), (0, 5), (0, 0), (0, 0), (9, 0), (5, 9)])) == [0, 0, 2, 2, -1, -1, 6, 0]


# ------------------------------------------------------------------------------------------ drm_sam_end5
def _mutated_read(rng, src, kinds):
    """A read cut from src (already on the read's strand) with the named edits; returns the read."""
    s = bytearray(src)
    nxt = dict(zip(b"ACGT", b"CGTA"))
    n = len(s)
    if "lead" in kinds:   # substitutions at the 5' end: a leading clip
        for i in (0, 1, 2):
            s[i] = nxt[s[i]]
    if "trail" in kinds:  # ... and at the 3' end
        for i in (n - 1, n - 2):
            s[i] = nxt[s[i]]
    mid = n // 2
    if "del" in kinds:    # two reference bases the read lacks
        del s[mid:mid + 2]
    if "ins" in kinds:    # two bases the reference lacks
        s[mid // 2:mid // 2] = bytes(rng.choice(list(b"ACGT"), size=2).astype(np.uint8))
    return bytes(s)


def test_end5_equals_the_end_parsed_from_the_printed_line():
    from deepreadmapper_amd import sam_cigar, sam_cigar_region, sam_end5
    rng = np.random.default_rng(8)
    g = bytes(rng.choice(list(b"ACGT"), size=600).astype(np.uint8))
    ref_len = 60
    seen = dict(lead=0, trail=0, ins=0, dele=0, fwd=0, rev=0, flank=0, negative=0)
    kinds = [(), ("lead",), ("trail",), ("lead", "trail"), ("del",), ("ins",), ("lead", "del", "ins", "trail")]
    for t in range(56):
        kind = kinds[t % len(kinds)]
        pos = 0 if t % 11 == 0 or t in (1, 3) else int(rng.integers(0, len(g) - ref_len))  # a clip past the start
        wid = 2 * pos + (t // len(kinds)) % 2
        affine = t % 3 != 0
        flank = (0, 5, 12)[t % 3] if affine else 0
        start, length, rev = A.region(g, ref_len, wid, flank)
        w = A.region_bytes(g, ref_len, wid, flank)
        window = R.window_bytes(g, ref_len, wid)
        q = b"<" + _mutated_read(rng, window, kind) + b">"
        rec, ops = A.align(w, q, (1, 4, 6, 1)) if affine else R.align(w, q)
        assert rec["status"] == 0
        pos1, cigar = sam_cigar_region(rec, ops, len(q), start, length, rev)
        want = D.end5_from_line(pos1, cigar, rev)
        assert sam_end5(rec, 1, start, length, rev) == want == D.end5(rec, 1, start, length, rev), (t, cigar)
        if not affine:  # the window form: the region of the id
            assert (pos1, cigar) == sam_cigar(rec, ops, len(q), ref_len, wid)
            assert sam_end5(rec, 1, wid // 2, ref_len, wid & 1) == want
        lead, trail = rec["q_begin"] - 1, len(q) - 1 - rec["q_end"]
        seen["lead"] += lead > 0
        seen["trail"] += trail > 0
        seen["ins"] += "I" in cigar
        seen["dele"] += "D" in cigar
        seen["rev" if rev else "fwd"] += 1
        seen["flank"] += flank > 0
        seen["negative"] += want < 0
    assert all(v >= 3 for k, v in seen.items() if k != "negative") and seen["negative"] >= 1, seen


def test_end5_and_word_errors():
    from deepreadmapper_amd import DrmError, dup_end_word, dup_slot, sam_end5
    from deepreadmapper_amd._native import DRM_ERR_ARG, lib
    good = _rec(score=15, ref_begin=5, ref_end=20, q_begin=4, q_end=19, n_ops=1)

    def raw(rec, prefix=1, out=True):
        r = np.array([tuple(rec[f] for f in R.FIELDS)], dtype=[(f, np.int32) for f in R.FIELDS])
        e = C.c_int64(0)
        return lib().drm_sam_end5(r.ctypes.data, prefix, 92, 166, 0, C.byref(e) if out else None)
    assert raw(good) == 0
    assert raw(dict(good, status=1)) == DRM_ERR_ARG and raw(dict(good, status=2)) == DRM_ERR_ARG
    assert raw(good, prefix=5) == DRM_ERR_ARG  # the alignment starts inside the prefix tag
    assert raw(good, prefix=4) == 0 and raw(good, prefix=-1) == DRM_ERR_ARG
    assert raw(good, out=False) == DRM_ERR_ARG
    assert lib().drm_sam_end5(None, 1, 92, 166, 0, C.byref(C.c_int64(0))) == DRM_ERR_ARG
    with pytest.raises(DrmError) as e:
        sam_end5(_rec(status=1), 1, 0, 150, 0)
    assert e.value.code == DRM_ERR_ARG
    for bad in (-(1 << 20) - 1, 1 << 61, -(1 << 62)):
        with pytest.raises(DrmError) as e:
            dup_end_word(bad, 0)
        assert e.value.code == DRM_ERR_ARG
    assert lib().drm_dup_end_word(0, 0, None) == DRM_ERR_ARG
    for bad in (0, 3, -4, (1 << 32) + 1, 1 << 33):
        with pytest.raises(DrmError):
            dup_slot(1, 2, bad)


# ------------------------------------------------------------------------------------------ the hash and the seeds
def test_slot_hash_is_the_librarys():
    from deepreadmapper_amd import dup_slot
    rng = np.random.default_rng(5)
    for _ in range(400):
        lo, hi = (int(x) for x in rng.integers(0, 1 << 63, size=2, dtype=np.uint64))
        slots = 1 << int(rng.integers(0, 33))
        assert dup_slot(lo, hi, slots) == D.slot_hash(lo, hi) & (slots - 1)
    assert dup_slot(0, 0, 1 << 32) == 0 and dup_slot((1 << 64) - 1, (1 << 64) - 1, 1) == 0
    assert D.slot_hash(1, 2) != D.slot_hash(2, 1)  # hi is rotated: the hash is of the ordered (lo, hi)


def test_small_tables_hold_a_chain_of_three_and_a_wrap():
    sizes = (1, 2, 3, 7, 8, 33, 64)  # tests/test_gpu_dup.py fills a set of each size to capacity
    assert tuple(D.SMALL_SEEDS) == sizes
    chains, wraps = [], []
    for m in sizes:
        ends = D.distinct_ends(D.SMALL_SEEDS[m], m)
        keys = [D.key(*e) for e in ends]
        assert len(set(keys)) == m and None not in keys
        slots = D.slots_for(m)
        assert slots >= 2 * m > slots // 2
        home, chain, wrapped = D.probe(keys, slots)
        want_chain, want_wrap = D.small_case_wanted(m)
        assert max(chain) >= want_chain and (wrapped or not want_wrap), (m, chain, wrapped)
        assert (max(chain), wrapped) == D.small_case_property(m, D.SMALL_SEEDS[m])
        chains.append(max(chain))
        wraps.append(wrapped)
    assert max(chains) >= 3 and any(wraps)
    assert D.pick_seed(3) == D.SMALL_SEEDS[3] and D.pick_seed(64) == D.SMALL_SEEDS[64]
    # the simulator itself: three keys of one home slot at the table's end chain 1, 2, 3 and wrap
    by_home = {}
    for x in range(1, 4000):
        by_home.setdefault(D.slot_hash(0, x) & 7, []).append((0, x))
    home, chain, wrapped = D.probe(by_home[7][:3], 8)
    assert home == [7, 7, 7] and chain == [1, 2, 3] and wrapped
    assert D.probe(by_home[2][:2] + by_home[3][:1], 8) == ([2, 2, 3], [1, 2, 2], False)
