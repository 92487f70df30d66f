"""GPU tests of bin/pipeline's DRM_SAM_LOCI=n (and DRM_SAM_XA=1, DRM_LOCI_DROP=pct): on the C1 genome with an exact
300-base duplicate appended (test_gpu_mapq_cli's fixture: reads from unique sequence, from the duplicate, with
substitutions, random and all-N) the file equals, byte for byte, the composition of the package's wrappers on the
unpaired run's rerank rows -- hit_loci with head 0, the alignment of the recorded loci's head rows, sam_cigar -- as
lines per locus, with the alternates folded into XA:Z, with MD, over a flanked region, and for pairs with and without
the mate rescue. The composition itself holds a read with two placements, one with exactly one and an unmapped one;
the primary line of a read that stays mapped is its line of the DRM_SAM_MAPQ=1 run; the paired file without its XA
tags is the file without the switch; no read has more than n lines; DRM_SAM_BLOCK changes nothing; without the switch
the file is the one of before; bad values and missing companions end the run before the index is loaded."""
import os
import re

import numpy as np
import pytest

import sw_align_ref as R
from deepreadmapper_amd import hit_loci  # noqa: F401  (what this file is about)
from test_gpu_mapq_cli import (REF_LEN, _composed_paired, _composed_single, _lists, _paired, _sam, _single,  # noqa: F401
                               fixture)

pytestmark = pytest.mark.gpu

HEADER = ["@HD\tVN:1.0\tSO:unsorted", "@SQ\tSN:ref\tLN:150"]
MIN_SCORE = 39
LOCI = dict(DRM_SAM_MAPQ="1", DRM_SAM_LOCI="5")


class _Aligner:
    """The alignments of (read, window id) rows through the package's wrappers: linear, or affine {1, 1, 0, 1} over a
    flank; the CIGAR, POS, NM, AS and MD of each row as the SAM prints them."""

    def __init__(self, fx, rows, flank=None, md=False):
        from deepreadmapper_amd import (GenomeTable, sam_cigar, sam_cigar_region, sam_md, sw_align_affine_arrays,
                                        sw_align_arrays, sw_align_md_arrays, sw_align_region)
        queries = [b"<" + r + b">" for r in fx["reads"]]
        wid = np.array([w for _, w in rows], dtype=np.uint64)
        q = np.array([i for i, _ in rows], dtype=np.int64)
        t = GenomeTable(np.frombuffer(fx["g"], dtype=np.uint8), REF_LEN)
        self.out = []
        if len(rows):
            if flank is None:
                rec, ops = sw_align_arrays(t, wid, q, queries)
            else:
                rec, ops = sw_align_affine_arrays(t, wid, q, queries, (1, 1, 0, 1), flank=flank)
            if md:
                mrec, words = sw_align_md_arrays(t, wid, q, queries, rec, ops, flank=flank or 0)
            for x, (_, w) in enumerate(rows):
                if int(rec["status"][x]) == 1:
                    self.out.append(None)
                    continue
                if flank is None:
                    pos1, cigar = sam_cigar(rec[x], ops[x], REF_LEN + 2, REF_LEN, w)
                else:
                    start, n, rev = sw_align_region(t, w, flank)
                    pos1, cigar = sam_cigar_region(rec[x], ops[x], REF_LEN + 2, start, n, rev)
                self.out.append(dict(pos1=pos1, cigar=cigar, nm=int(rec["nm"][x]), score=int(rec["score"][x]),
                                     md=sam_md(mrec[x], words[x], w & 1) if md else None))
        t.free()


def _xa(entries):
    """entries: [(window id, alignment or None)]; the tag, or nothing when no entry holds an alignment."""
    text = "".join(f"ref,{'-' if w & 1 else '+'}{a['pos1']},{a['cigar']},{a['nm']};" for w, a in entries if a)
    return "\tXA:Z:" + text if text else ""


def _composed_loci(fx, n, xa=False, md=False, flank=None, drop=80, min_score=MIN_SCORE):
    """The expected single-read file, and per read its number of placements (0 = unmapped)."""
    ids, sc, cnt, full = _lists(fx)
    reads = fx["reads"]
    rec, n_loci, n_pass, l_ids, l_sc, l_rows, l_size = hit_loci(ids, sc, cnt, full, REF_LEN, n, drop_pct=drop,
                                                                head=np.zeros(len(cnt), np.int32), min_score=min_score)
    mapped = (rec["status"] == 0) & (rec["best_score"] >= min_score)
    rows = []
    for i in range(len(reads)):
        for j in range(int(n_loci[i]) if mapped[i] else 0):
            w = int(ids[i, l_rows[i, j]])
            assert w == int(l_ids[i, j]) and int(sc[i, l_rows[i, j]]) == int(l_sc[i, j])
            rows.append((i, w))
    aln = _Aligner(fx, rows, flank, md).out
    want, places, x = list(HEADER), [], 0
    for i, read in enumerate(reads):
        name = fx["names"][i // 2]
        if not mapped[i]:
            want.append(f"{name}\t4\t*\t0\t0\t*\t*\t0\t0\t{read.decode()}\t*")
            places.append(0)
            continue
        mine = [(rows[x + j][1], aln[x + j]) for j in range(int(n_loci[i]))]
        x += len(mine)
        assert int(l_rows[i, 0]) == 0  # the primary is the rerank's first row, as without the switch
        places.append(len(mine))
        for j, (w, a) in enumerate(mine[:1] if xa else mine):
            flag = (0 if j == 0 else 256) | (16 if w & 1 else 0)
            seq = (R.revcomp(read) if w & 1 else read).decode()
            if a is None:
                want.append(f"{name}\t{flag | 4}\tref\t0\t0\t*\t*\t0\t0\t{seq}\t*")
                continue
            q = int(rec["mapq"][i]) if j == 0 else 0
            line = f"{name}\t{flag}\tref\t{a['pos1']}\t{q}\t{a['cigar']}\t*\t0\t0\t{seq}\t*\tAS:i:{a['score']}\tNM:i:{a['nm']}"
            line += f"\tMD:Z:{a['md']}" if md else ""
            want.append(line + (_xa(mine[1:]) if xa else ""))
    assert x == len(rows)
    return want, places


def _by_read(lines):
    """The body lines grouped per read: a line without flag 256 starts the next read."""
    groups = []
    for line in lines:
        if line.startswith("@"):
            continue
        if not int(line.split("\t")[1]) & 256:
            groups.append([])
        groups[-1].append(line)
    return groups


def _assert_spread(places):
    assert max(places) >= 2 and 1 in places and 0 in places, ("the fixture does not spread the placements", places)


def test_single_reads_one_line_per_locus(fixture):
    fx = fixture
    want, places = _composed_loci(fx, 5)
    _assert_spread(places)
    got = _single(fx, "loci", **LOCI)
    assert got == want
    assert _single(fx, "loci_b3", DRM_SAM_BLOCK="3", **LOCI) == want  # ten blocks of reads: the same file
    assert _single(fx, "loci_dflt", DRM_LOCI_DROP="80", DRM_SAM_XA="0", **LOCI) == want  # the defaults
    # the primary line of every read that stays mapped is its line in the run without the switch
    today, _ = _composed_single(fx)
    before = _single(fx, "loci_off", DRM_SAM_MAPQ="1", DRM_LOCI_DROP="garbage")  # read only with DRM_SAM_LOCI
    assert before == today  # without the switch the file is the one of before
    cnt = _lists(fx)[2]
    ends = np.cumsum(cnt)
    old = [before[2 + int(e - c):2 + int(e)] for c, e in zip(cnt, ends)]  # one line per rerank row there
    new = _by_read(got)
    assert len(new) == len(fx["reads"]) and 2 + int(ends[-1]) == len(before)
    for i, (a, b) in enumerate(zip(old, new)):
        if places[i]:
            assert len(b) == places[i] <= len(a) and b[0] == a[0], i
        else:
            assert len(b) == 1 and b[0].split("\t")[1:9] == ["4", "*", "0", "0", "*", "*", "0", "0"]
    # the reads from the duplicate have both copies as loci: two lines a genome apart, the second one secondary
    for read in (6, 9, 10, 11):
        f0, f1 = new[read][0].split("\t"), new[read][1].split("\t")
        assert places[read] == 2 and int(f1[1]) & 256 and f1[4] == "0" and f0[4] == "0"
        assert abs(int(f0[3]) - int(f1[3])) > len(fx["g"]) - 400 - 10
    # no read has more lines than n; n = 1 keeps the primaries only; DRM_LOCI_DROP is handed on as drop_pct
    for n in (1, 2):
        w, p = _composed_loci(fx, n)
        g = _single(fx, f"loci_n{n}", DRM_SAM_MAPQ="1", DRM_SAM_LOCI=str(n))
        assert g == w and max(len(x) for x in _by_read(g)) <= n and max(p) == n
    # with no chance level a random read's rows are loci of unequal scores: 0 lists them, 100 only the best ones
    w0, p0 = _composed_loci(fx, 5, drop=0, min_score=0)
    w100, p100 = _composed_loci(fx, 5, drop=100, min_score=0)
    assert sum(p0) > sum(p100)
    assert _single(fx, "loci_drop0", DRM_LOCI_DROP="0", DRM_MAPQ_MIN="0", **LOCI) == w0
    assert _single(fx, "loci_drop100", DRM_LOCI_DROP="100", DRM_MAPQ_MIN="0", **LOCI) == w100


def test_single_reads_with_xa(fixture):
    fx = fixture
    want, places = _composed_loci(fx, 5, xa=True)
    _assert_spread(places)
    got = _single(fx, "xa", DRM_SAM_XA="1", **LOCI)
    assert got == want
    assert _single(fx, "xa_b3", DRM_SAM_XA="1", DRM_SAM_BLOCK="3", **LOCI) == want
    lines, _ = _composed_loci(fx, 5)
    body = [x for x in got if not x.startswith("@")]
    assert len(body) == len(fx["reads"])  # one line per read
    # the tag comes last, holds one entry per alternate, and the entries are the secondary lines of the other form
    for i, (line, group) in enumerate(zip(body, _by_read(lines))):
        entries = re.findall(r"([^,;\t:]+),([+-])(\d+),([0-9MIDS]+),(\d+);", line.partition("\tXA:Z:")[2])
        assert len(entries) == max(places[i] - 1, 0) and ("XA:Z" in line) == (places[i] > 1)
        assert line.partition("\tXA:Z:")[0] == group[0]
        for e, sec in zip(entries, group[1:]):
            f = sec.split("\t")
            assert e == ("ref", "-" if int(f[1]) & 16 else "+", f[3], f[5], f[12][5:])


@pytest.mark.parametrize("mode", ["md", "flank"])
def test_single_reads_with_md_and_over_a_flank(fixture, mode):
    fx = fixture
    more, prm = (dict(DRM_SAM_MD="1"), dict(md=True)) if mode == "md" else (dict(DRM_SAM_FLANK="8"), dict(flank=8))
    for xa in (False, True):
        want, places = _composed_loci(fx, 5, xa=xa, **prm)
        _assert_spread(places)
        assert _single(fx, f"{mode}_{int(xa)}", DRM_SAM_XA=str(int(xa)), **LOCI, **more) == want
    if mode == "md":  # MD stands behind NM and in front of XA
        assert any(re.search(r"\tNM:i:\d+\tMD:Z:[0-9A-Z^]+\tXA:Z:", x) for x in want)


@pytest.mark.parametrize("rescue", [False, True])
def test_pairs_carry_the_alternates_as_xa(fixture, rescue):
    fx = fixture
    more = dict(DRM_PAIR_RESCUE="1") if rescue else {}
    today, _, final, _ = _composed_paired(fx, rescue)
    ids, sc, cnt, full = _lists(fx)
    head = np.full(len(cnt), -2, np.int32)  # -2 is no row: a rescued or unmapped mate has no list row behind its line
    for p, (rec, _) in enumerate(final):
        for m, j in enumerate((rec["j1"], rec["j2"])):
            if j >= 0 and rec["status"] != (6, 5)[m]:
                head[2 * p + m] = j
    _, n_loci, _, l_ids, _, l_rows, _ = hit_loci(ids, sc, cnt, full, REF_LEN, 5, head=head)
    rows = [(r, int(ids[r, l_rows[r, j]])) for r in range(len(cnt)) for j in range(1, int(n_loci[r]))]
    aln = _Aligner(fx, rows).out
    want, places, x = list(today[:2]), [], 0
    for r, line in enumerate(today[2:]):
        mine = [(rows[x + j][1], aln[x + j]) for j in range(max(int(n_loci[r]) - 1, 0))]
        x += len(mine)
        unmapped = int(line.split("\t")[1]) & 4
        want.append(line + ("" if unmapped else _xa(mine)))
        places.append(0 if unmapped else 1 + len(mine))
    assert x == len(rows) and (head >= 0).any() and (head == -2).any()
    _assert_spread(places)
    if rescue:
        assert any(rec["status"] in (5, 6) for rec, _ in final)
    name = "pair_loci_rescue" if rescue else "pair_loci"
    got = _paired(fx, name, **LOCI, **more)
    assert got == want
    assert _paired(fx, name + "_b3", DRM_SAM_BLOCK="3", **LOCI, **more) == want
    assert _paired(fx, name + "_xa", DRM_SAM_XA="1", **LOCI, **more) == want  # pairs take the XA form either way
    # without its tags the file is the one without the switch; n = 1 has no alternates at all
    before = _paired(fx, name + "_off", DRM_SAM_MAPQ="1", **more)
    assert before == today and [re.sub(r"\tXA:Z:[^\t]*$", "", x) for x in got] == before
    assert _paired(fx, name + "_n1", DRM_SAM_MAPQ="1", DRM_SAM_LOCI="1", **more) == before
    for line in got[2:]:
        assert line.count(";") <= 4 and ("XA:Z" not in line or line.split("\t")[-1].startswith("XA:Z:"))


def test_bad_values_and_missing_companions_end_before_the_index_is_loaded(fixture):
    fx = fixture
    on = dict(DRM_SAM_CIGAR="1", DRM_SAM_MAPQ="1")
    cases = [(dict(on, DRM_SAM_LOCI=v), "DRM_SAM_LOCI", ["1", "1"]) for v in ("0", "65", "-1", "5x", "", "1e1")]
    cases += [(dict(on, DRM_SAM_LOCI="5", DRM_LOCI_DROP=v), "DRM_LOCI_DROP", ["1", "1"]) for v in ("101", "-1", "x", "")]
    cases += [(dict(on, DRM_SAM_LOCI="5", DRM_SAM_XA=v), "DRM_SAM_XA", ["1", "1"]) for v in ("2", "yes", "")]
    cases += [(dict(on, DRM_SAM_XA="1"), "DRM_SAM_LOCI", ["1", "1"]),                      # XA without the loci
              (dict(DRM_SAM_CIGAR="1", DRM_SAM_LOCI="5"), "DRM_SAM_MAPQ", ["1", "1"]),      # no MAPQ
              (dict(DRM_SAM_MAPQ="1", DRM_SAM_LOCI="5"), "DRM_SAM_MAPQ", ["1", "1"]),       # no CIGAR
              (dict(on, DRM_SAM_LOCI="5"), "DRM_SAM_MAPQ", ["0", "1"]),                     # not dynamic
              (dict(on, DRM_SAM_LOCI="5"), "DRM_SAM_MAPQ", ["1", "0"]),                     # not streaming
              (dict(on, DRM_SAM_LOCI="5", DRM_DEVICES="0,0"), "DRM_DEVICES", ["1", "1"])]   # more than one device
    for more, word, mode in cases:
        r = fx["run"](fx["tmp"] / "inter.fastq", "bad_loci", mode, **more)
        assert r.returncode == 1 and r.stderr.startswith("Error:") and word in r.stderr, (more, r.stdout, r.stderr)
        assert "Index loaded" not in r.stdout and not os.path.exists(fx["tmp"] / "bad_loci" / "results.sam"), more
    m2 = str(fx["tmp"] / "m2.fastq")
    r = fx["run"](fx["tmp"] / "m1.fastq", "bad_loci", ["1", "1"], DRM_MATES=m2, DRM_SAM_CIGAR="1", DRM_SAM_LOCI="5")
    assert r.returncode == 1 and "DRM_SAM_MAPQ" in r.stderr and "Index loaded" not in r.stdout
    # the bounds themselves are accepted
    want, _ = _composed_loci(fx, 64, drop=100)
    assert _single(fx, "loci_edge", DRM_SAM_MAPQ="1", DRM_SAM_LOCI="64", DRM_LOCI_DROP="100") == want
