"""GPU tests of bin/pipeline's DRM_SAM_DUP=1 on test_gpu_mapq_cli's genome and index: a read set with pairs repeated
under other names, with the mates swapped between the two files, with a substitution beside the 5' end (soft-clipped, so
POS differs), with one unmappable mate and of all-N reads comes out -- as pairs (with and without the mate rescue) and as
single reads under DRM_SAM_LOCI -- as the composition of the package's wrappers plus DupSet byte for byte; exactly the
templates whose ends an earlier one had carry 1024; clearing that bit gives the file of the run without the switch; the
file does not depend on DRM_SAM_BLOCK; the switch without its companions, or a bad value, ends the run before the index
is loaded."""
import os

import numpy as np
import pytest

import sw_align_ref as R
from deepreadmapper_amd import DupSet, dup_end_word, sam_end5  # noqa: F401  (what this file is about)
from test_gpu_loci_cli import LOCI, _by_read, _composed_loci
from test_gpu_mapq_cli import REF_LEN, _lists, _sam, fixture  # noqa: F401
from test_gpu_pair_cli import _fastq
from test_gpu_rescue_cli import _composed, mutate

pytestmark = pytest.mark.gpu

LOST = -2  # the origin of a read the search may lose: its placement is the composition's business


def _sub(read, at):
    s = bytearray(read)
    s[at] = dict(zip(b"ACGT", b"CGTA"))[s[at]]
    return bytes(s)


@pytest.fixture(scope="module")
def dups(fixture):  # noqa: F811
    """The read set on the mapq fixture's genome and index: per pair its two (read, origin), an origin being the window
    id of the read's true placement (None: unmappable), and the unpaired run's rerank rows of the interleaved reads."""
    base = fixture
    g, tmp = base["g"], base["tmp"]
    n = b"N" * REF_LEN

    def frag(p, t):
        return (g[p:p + REF_LEN], 2 * p), (R.revcomp(g[p + t - REF_LEN:p + t]), 2 * (p + t - REF_LEN) + 1)
    a, b, c, d = frag(450, 300), frag(520, 260), frag(610, 350), frag(480, 400)
    x = frag(430, 377)
    x = (x[0], (mutate(x[1][0], 3), LOST))  # a mate the search loses and the rescue finds
    y = frag(640, 300)
    y = ((mutate(y[0][0], 3), LOST), y[1])  # ... and a lost mate 1
    pairs = [a, b, a, c, (b[1], b[0]),            # 2: a repeat under another name; 4: a repeat with the mates swapped
             ((_sub(a[0][0], 1), a[0][1]), a[1]),  # 5: a substitution at the second base of mate 1: 2S148M, POS + 2
             (a[0], (_sub(a[1][0], 1), a[1][1])),  # 6: ... of mate 2, the reverse strand: the clip is the line's last
             ((g[700:850], 1400), (n, None)), d, ((g[700:850], 1400), (n, None)),  # 9: one unmappable mate, repeated
             ((n, None), (n, None)), ((n, None), (n, None)),                      # all N: never marked
             (a[0], (n, None)),                    # 12: mate 1 of pair 0 alone: (e, 0) is no duplicate of (e1, e2)
             x, x,                                 # 14: a rescued mate is keyed like any other
             frag(120, 270), frag(120, 270),       # 16: both mates inside the genome's duplicated stretch: two loci
             y, y]
    names = [f"t{i}" for i in range(len(pairs))]
    m1, m2 = [p[0][0] for p in pairs], [p[1][0] for p in pairs]
    _fastq(tmp / "dup_m1.fastq", [s + "/1" for s in names], m1)
    _fastq(tmp / "dup_m2.fastq", [s + "/2" for s in names], m2)
    inter = [r for ab in zip(m1, m2) for r in ab]
    _fastq(tmp / "dup_inter.fastq", [s for s in names for _ in range(2)], inter)
    r = base["run"](tmp / "dup_inter.fastq", "dup_unpaired", ["1", "0"])
    assert r.returncode == 0, r.stdout + r.stderr
    ids = np.load(tmp / "dup_unpaired" / "sw_ids.npy")
    sc = np.load(tmp / "dup_unpaired" / "sw_scores.npy")
    assert ids.shape == sc.shape == (len(inter), 4)
    origins = [o for p in pairs for o in (p[0][1], p[1][1])]
    return dict(tmp=tmp, run=base["run"], g=g, names=names, reads=inter, truth=[], ids=ids, sc=sc, origins=origins)


def _run(fx, name, paired, **more):
    if paired:
        more = dict(DRM_MATES=str(fx["tmp"] / "dup_m2.fastq"), **more)
    r = fx["run"](fx["tmp"] / ("dup_m1.fastq" if paired else "dup_inter.fastq"), name, ["1", "1"], DRM_SAM_CIGAR="1",
                  **more)
    assert r.returncode == 0, r.stdout + r.stderr
    return _sam(fx, name)


def _flagged(line, bit):
    f = line.split("\t")
    f[1] = str(int(f[1]) | bit)
    return "\t".join(f)


def _cleared(lines):
    out = []
    for line in lines:
        f = line.split("\t")
        if not line.startswith("@"):
            f[1] = str(int(f[1]) & ~1024)
        out.append("\t".join(f))
    return out


def _marked(lines):
    return [bool(int(x.split("\t")[1]) & 1024) for x in lines if not x.startswith("@")]


def _end_words(fx, rows):
    """rows: {read: window id of its primary placement}; per read its end word through the package's wrappers (0 for a
    read without a row or without an alignment)."""
    from deepreadmapper_amd import GenomeTable, sw_align_arrays
    order = sorted(rows)
    queries = [b"<" + r + b">" for r in fx["reads"]]
    t = GenomeTable(np.frombuffer(fx["g"], dtype=np.uint8), REF_LEN)
    rec, _ = sw_align_arrays(t, np.array([rows[r] for r in order], dtype=np.uint64), np.array(order), queries)
    t.free()
    words = np.zeros(len(fx["reads"]), dtype=np.uint64)
    for x, r in enumerate(order):
        if int(rec["status"][x]) == 0:
            w = rows[r]
            words[r] = dup_end_word(sam_end5(rec[x], 1, w // 2, REF_LEN, w & 1), w & 1)
    return words


def _mark(ends, cuts):
    """DupSet over the items in calls that end at `cuts`: whether each item is a duplicate."""
    s, first, lo = DupSet(len(ends)), [], 0
    for hi in cuts:
        first.append(s.mark(ends[lo:hi]))
        lo = hi
    s.free()
    first = np.concatenate(first)
    return (first >= 0) & (first != np.arange(len(ends)))


def _expected_by_construction(keys):
    seen, out = set(), []
    for k in keys:
        out.append(k is not None and k in seen)
        seen.add(k)
    return out


@pytest.mark.parametrize("rescue", [False, True])
def test_paired_sam_equals_the_composition_plus_dupset(dups, rescue):
    fx = dups
    more = dict(DRM_PAIR_RESCUE="1") if rescue else {}
    plain, final = _composed(fx, rescue)
    ids = fx["ids"]
    rows = {}
    for p, (rec, wr) in enumerate(final):
        for m, j in enumerate((rec["j1"], rec["j2"])):
            if j >= 0:
                rows[2 * p + m] = int(ids[2 * p + m, j])
        if rec["status"] in (5, 6):
            rows[2 * p + (1 if rec["status"] == 5 else 0)] = wr
    npairs = len(final)
    ends = _end_words(fx, rows).reshape(npairs, 2)
    dup = _mark(ends, [npairs])
    assert np.array_equal(dup, _mark(ends, [1, 4, 5, 11, npairs]))
    want = plain[:2] + [_flagged(x, 1024) if dup[i // 2] else x for i, x in enumerate(plain[2:])]
    name = "dup_paired_rescue" if rescue else "dup_paired"
    got = _run(fx, name, True, DRM_SAM_DUP="1", **more)
    assert got == want
    # exactly the repeats: by name, whatever the composition says
    o = fx["origins"]
    keys = [None if o[2 * p] is None and o[2 * p + 1] is None else
            tuple(sorted((-1 if x is None else x) for x in (o[2 * p], o[2 * p + 1]))) for p in range(npairs)]
    by_name = _expected_by_construction(keys)
    assert [i for i, x in enumerate(by_name) if x] == [2, 4, 5, 6, 9, 14, 16, 18]
    assert _marked(got) == [by_name[i // 2] for i in range(2 * npairs)]
    # the clipped repeats print another POS than the pair they repeat, and are marked all the same
    f0, f5 = got[2].split("\t"), got[2 + 2 * 5].split("\t")
    assert f5[5] == "2S148M" and int(f5[3]) == int(f0[3]) + 2 and f0[5] == "150M"
    r0, r6 = got[3].split("\t"), got[2 + 2 * 6 + 1].split("\t")
    assert r6[5] == "148M2S" and r6[3] == r0[3] and int(r6[1]) & 16
    # without the switch: the parent's file, which is this one with the bit cleared
    without = _run(fx, name + "_off", True, **more)
    assert without == plain == _cleared(got) and not any(_marked(without))
    assert _run(fx, name + "_zero", True, DRM_SAM_DUP="0", **more) == plain
    if not rescue:
        for block in ("3", "1000"):
            assert _run(fx, name + "_b" + block, True, DRM_SAM_DUP="1", DRM_SAM_BLOCK=block) == want
    status = [rec["status"] for rec, _ in final]
    assert not rescue or any(x in (5, 6) for x in status), ("the fixture rescues no mate", status)


def test_single_read_sam_under_loci_equals_the_composition_plus_dupset(dups):
    fx = dups
    plain, places = _composed_loci(fx, 5)
    ids, _, cnt, _ = _lists(fx)
    rows = {i: int(ids[i, 0]) for i in range(len(places)) if places[i] > 0}
    ends = np.stack([_end_words(fx, rows), np.zeros(len(places), np.uint64)], axis=1)
    dup = _mark(ends, [len(ends)])
    assert np.array_equal(dup, _mark(ends, [3, 6, 7, 20, len(ends)]))
    groups = _by_read(plain)
    assert len(groups) == len(places)
    want = plain[:2] + [_flagged(x, 1024) if dup[i] else x for i, grp in enumerate(groups) for x in grp]
    got = _run(fx, "dup_single", False, DRM_SAM_DUP="1", **LOCI)
    assert got == want
    o = fx["origins"]
    by_name = _expected_by_construction([None if x is None else x for x in o])
    marked = [bool(int(grp[0].split("\t")[1]) & 1024) for grp in _by_read(got)]
    sure = [i for i, x in enumerate(o) if x != LOST]
    assert [marked[i] for i in sure] == [by_name[i] for i in sure] and sum(by_name) >= 10
    for grp in _by_read(got):  # every line of a read carries the read's answer
        assert len({int(x.split("\t")[1]) & 1024 for x in grp}) == 1
    assert any(len(grp) > 1 and int(grp[0].split("\t")[1]) & 1024 for grp in _by_read(got)), "no marked secondary line"
    without = _run(fx, "dup_single_off", False, **LOCI)
    assert without == plain == _cleared(got)
    for block in ("3", "1000"):
        assert _run(fx, "dup_single_b" + block, False, DRM_SAM_DUP="1", DRM_SAM_BLOCK=block, **LOCI) == want
    with_xa = _run(fx, "dup_single_xa", False, DRM_SAM_DUP="1", DRM_SAM_XA="1", **LOCI)
    assert _cleared(with_xa) == _run(fx, "dup_single_xa_off", False, DRM_SAM_XA="1", **LOCI)
    assert _marked(with_xa) == [bool(x) for x in dup]  # one line per read: XA entries carry no flag


def test_bad_dup_input_ends_before_the_index_is_loaded(dups):
    fx = dups
    m2 = str(fx["tmp"] / "dup_m2.fastq")
    cases = [(dict(DRM_SAM_DUP="1", DRM_SAM_CIGAR="1"), False),                      # neither pairs nor loci
             (dict(DRM_SAM_DUP="1", DRM_SAM_CIGAR="1", DRM_SAM_MAPQ="1"), False),    # MAPQ alone: a line per rerank row
             (dict(DRM_SAM_DUP="1"), False),                                         # no alignment at all
             (dict(DRM_SAM_DUP="2", DRM_SAM_CIGAR="1", DRM_MATES=m2), True),
             (dict(DRM_SAM_DUP="yes", DRM_SAM_CIGAR="1", DRM_MATES=m2), True),
             (dict(DRM_SAM_DUP="", DRM_SAM_CIGAR="1", DRM_MATES=m2), True),
             (dict(DRM_SAM_DUP="-1", DRM_SAM_CIGAR="1", **LOCI), False),
             (dict(DRM_SAM_DUP="1x", DRM_SAM_CIGAR="1", **LOCI), False)]
    for more, paired in cases:
        r = fx["run"](fx["tmp"] / ("dup_m1.fastq" if paired else "dup_inter.fastq"), "dup_bad", ["1", "1"], **more)
        assert r.returncode == 1 and r.stderr.startswith("Error:") and "DRM_SAM_DUP" in r.stderr, (more, r.stderr)
        assert "Index loaded" not in r.stdout and not os.path.exists(fx["tmp"] / "dup_bad" / "results.sam"), more
