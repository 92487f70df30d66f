"""CPU tests of the MD tag's host side: drm_sam_md (through deepreadmapper_amd.sam_md) against the plain restatement
(tests/md_ref.py) on hand cases and on each of its argument errors, and a property test of the restatement itself:
read, CIGAR and MD together rebuild the genome bytes under the alignment, on both strands."""
import re

import numpy as np
import pytest

import md_ref as MD
import sw_align_affine_ref as A
import sw_align_ref as R

DRM_ERR_ARG = -1


def _w(n, op):
    return (n << 4) | op


def _case(region, query, ops, ref_begin=0, q_begin=0):
    """(md record, words) of the restatement for a hand-built walk."""
    rspan = sum(x >> 4 for x in ops if (x & 15) != R.I)
    qspan = sum(x >> 4 for x in ops if (x & 15) != R.D)
    rec = dict(dict.fromkeys(R.FIELDS, 0), ref_begin=ref_begin, ref_end=ref_begin + rspan, q_begin=q_begin,
               q_end=q_begin + qspan, n_ops=len(ops))
    h, words = MD.md_words(region, query, rec, ops)
    assert h["status"] == 0 and h["n_words"] == len(words)
    return h, words


def _both(h, words, reverse):
    from deepreadmapper_amd import sam_md
    want = MD.md_string(words, reverse)
    assert sam_md(h, words, reverse) == want
    assert re.fullmatch(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*", want)
    return want


READ = b"ACGTTGCAAGGCTTAACCGGATATCGCGTTAA" * 5  # 160 bases


def _hand_cases():
    r150 = READ[:150]
    yield "150", r150, r150, [_w(150, R.M)]
    sub = bytearray(r150)
    sub[10:12] = b"TT"  # the read differs in two adjacent columns: the reference holds GC there
    yield "10G0C138", r150, bytes(sub), [_w(150, R.M)]
    ends = bytearray(r150)
    ends[0], ends[-1] = ord("C"), ord("C")  # a leading and a trailing mismatch: the reference holds A and T
    yield "0A148T0", r150, bytes(ends), [_w(150, R.M)]
    # a deletion followed at once by a mismatch
    reg = b"ACGTACGTAC" + b"GGG" + b"TCAGTCAGTC"
    qry = b"ACGTACGTAC" + b"ACAGTCAGTC"
    yield "10^GGG0T9", reg, qry, [_w(10, R.M), _w(3, R.D), _w(10, R.M)]
    # D, I, D
    reg = b"TTTTT" + b"AC" + b"GT" + b"CCCCC"
    qry = b"TTTTT" + b"GGG" + b"CCCCC"
    yield "5^AC0^GT5", reg, qry, [_w(5, R.M), _w(2, R.D), _w(3, R.I), _w(2, R.D), _w(5, R.M)]
    # N against N matches, N against a base does not
    yield "3N1", b"ACNNA", b"ACNGA", [_w(5, R.M)]


CASES = list(_hand_cases())


@pytest.mark.parametrize("want,region,query,ops", CASES, ids=[c[0] for c in CASES])
def test_sam_md_hand_cases(want, region, query, ops):
    h, words = _case(region, query, ops)
    assert _both(h, words, 0) == want
    # the same alignment seen from a reverse-complemented region: the string of the forward strand
    rh, rwords = _case(R.revcomp(region), R.revcomp(query), ops[::-1])
    assert _both(rh, rwords, 1) == want


def test_sam_md_reversed_strings():
    h, words = _case(b"ACGTACGTAC" + b"GGG" + b"TCAGTCAGTC", b"ACGTACGTAC" + b"ACAGTCAGTC",
                     [_w(10, R.M), _w(3, R.D), _w(10, R.M)])
    assert _both(h, words, 1) == "9A0^CCC10"
    h, words = _case(b"TTTTT" + b"AC" + b"GT" + b"CCCCC", b"TTTTT" + b"GGG" + b"CCCCC",
                     [_w(5, R.M), _w(2, R.D), _w(3, R.I), _w(2, R.D), _w(5, R.M)])
    assert _both(h, words, 1) == "5^AC0^GT5"
    h, words = _case(b"ACNNA", b"ACNGA", [_w(5, R.M)])
    assert _both(h, words, 1) == "1N3"


def _md(n_words, status=0):
    return dict(dict.fromkeys(MD.MD_FIELDS, 0), n_words=n_words, status=status)


def _num(n):
    return n << 4


def _base(ch, kind):
    return (ord(ch) << 4) | kind


@pytest.mark.parametrize("name,h,words,reverse", [
    ("status 1", _md(1, 1), [_num(0)], 0),
    ("status 2", _md(3, 2), [_num(1), _base("A", 1), _num(1)], 0),
    ("status 3", _md(1, 3), [_num(0)], 0),
    ("kind above 2", _md(3), [_num(1), _base("A", 3), _num(1)], 0),
    ("a base that is no letter", _md(3), [_num(1), _base("<", 1), _num(1)], 0),
    ("a letter without a complement", _md(3), [_num(1), _base("R", 1), _num(1)], 1),
    ("starts with a base", _md(2), [_base("A", 1), _num(1)], 0),
    ("ends with a base", _md(2), [_num(1), _base("A", 2)], 0),
    ("two numbers", _md(3), [_num(1), _num(2), _num(3)], 0),
    ("no words", _md(0), [], 0),
])
def test_sam_md_argument_errors(name, h, words, reverse):
    from deepreadmapper_amd import DrmError, sam_md
    with pytest.raises(DrmError) as e:
        sam_md(h, words, reverse)
    assert e.value.code == DRM_ERR_ARG, name
    if h["status"] == 0:
        with pytest.raises(ValueError):
            MD.md_string(words, reverse)


def test_sam_md_cap_too_small():
    import ctypes as C
    from deepreadmapper_amd import SW_MD_DTYPE
    from deepreadmapper_amd._native import lib
    h = np.zeros(1, dtype=SW_MD_DTYPE)
    h["n_words"] = 3
    words = np.array([_num(120), _base("A", 1), _num(29)], dtype=np.uint32)
    buf = C.create_string_buffer(16)
    assert lib().drm_sam_md(h.ctypes.data, words.ctypes.data, 0, buf, 6) == DRM_ERR_ARG  # "120A29" + NUL is 7 bytes
    assert lib().drm_sam_md(h.ctypes.data, words.ctypes.data, 0, buf, 0) == DRM_ERR_ARG
    assert lib().drm_sam_md(h.ctypes.data, words.ctypes.data, 0, buf, 7) == 0 and buf.value == b"120A29"


def test_read_cigar_and_md_rebuild_the_genome_on_both_strands():
    """500 random alignments of the affine restatement on mutated slices of a random genome: the SAM fields of the
    pair (sam_fields_region's POS and CIGAR, md_string of md_words, the read as it is printed) give back the genome
    bytes at POS."""
    from deepreadmapper_amd import sam_md
    rng = np.random.default_rng(2024)
    g = bytes(rng.choice(list(b"ACGT"), size=3000).astype(np.uint8))
    ref_len, flank = 60, 12
    seen = set()
    for t in range(500):
        pos = int(rng.integers(0, len(g) - ref_len + 1))
        wid = 2 * pos + t % 2
        start, n, rev = A.region(g, ref_len, wid, flank)
        region = A.region_bytes(g, ref_len, wid, flank)
        s = list(R.window_bytes(g, ref_len, wid))
        for _ in range(int(rng.integers(0, 4))):
            s[int(rng.integers(len(s)))] = int(rng.choice(list(b"ACGT")))
        if t % 3 == 0:
            at = int(rng.integers(5, len(s) - 8))
            del s[at:at + int(rng.integers(1, 4))]
        if t % 4 == 0:
            at = int(rng.integers(5, len(s) - 5))
            s[at:at] = [int(x) for x in rng.choice(list(b"ACGT"), size=int(rng.integers(1, 3)))]
        q = b"<" + bytes(s) + b">"
        rec, ops = A.align(region, q, (1, 4, 6, 1))
        assert rec["status"] == 0
        h, words = MD.md_words(region, q, rec, ops)
        assert h["status"] == 0 and h["n_mismatch"] + h["n_ins"] + h["n_del"] == rec["nm"]
        assert h["n_words"] == len(words) == 2 * h["n_mismatch"] + h["n_del"] + sum((x & 15) == R.D for x in ops) + 1
        md = MD.md_string(words, rev)
        assert sam_md(h, words, rev) == md
        pos1, cigar = A.sam_fields_region(rec, ops, len(q), start, n, rev)
        seq = R.revcomp(q[1:-1]) if rev else q[1:-1]
        ref = MD.rebuild_reference(seq, cigar, md)
        assert ref == g[pos1 - 1:pos1 - 1 + len(ref)], (t, cigar, md)
        assert len(ref) == rec["ref_end"] - rec["ref_begin"]
        assert MD.nm_from_cigar_md(cigar, md) == rec["nm"]
        seen |= {rev, "D" in cigar and "d", "I" in cigar and "i"}
    assert {0, 1, "d", "i"} <= seen
