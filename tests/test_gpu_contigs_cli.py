"""GPU tests of DRM_CONTIGS=1 through the two tools: a FASTA of three random contigs, whose later headers carry letters,
and a fourth, chrD, that repeats chrC's last window, is indexed by bin/hnswpq_index and mapped by
bin/pipeline, single and paired. The header has one @SQ line per contig; the files equal, byte for byte, the
composition of the package's wrappers (contig_hits, pair_hits, hit_mapq / pair_mapq with DRM_SAM_MAPQ=1, sw_align_arrays
or with DRM_SAM_FLANK sw_align_affine_arrays, sam_cigar(_region), sam_pair_fields) on the plain run's sw_ids.npy /
sw_scores.npy; reads copied from a contig carry its name and local POS; no line leaves its contig; mates either side of
a contig boundary are no proper pair; a read whose best and second hit lie either side of the chrC / chrD seam gets the
MAPQ of two loci, not of one; the flank guard and the rescue guard are seen to fire; the files do not depend on
DRM_SAM_BLOCK or on DRM_PAIR_TLEN=auto's pre-pass; on a single-contig FASTA only the @SQ line and column 3 change; every
violated requirement ends the run with exit code 1 before the search.

tests/golden/ecoli_150.fna's header, "> Fake DNA sequence", has an empty name, which drm_fasta_contigs refuses as the
definition asks; the single-contig case therefore runs on a copy whose header names it."""
import os
import re
import subprocess

import numpy as np
import pytest

import sw_align_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_LEN = 150
K = 16          # rows per read
MAPQ_SPAN = 200  # chrC's last window and chrD's first lie 151 bases apart in the genome string
DROP = ("DRM_CONTIGS", "DRM_MATES", "DRM_PAIR_TLEN", "DRM_PAIR_PENALTY", "DRM_PAIR_RESCUE", "DRM_SAM_CIGAR",
        "DRM_SAM_SCORING", "DRM_SAM_FLANK", "DRM_SAM_BLOCK", "DRM_SAM_MAPQ", "DRM_SAM_L2_ROWS", "DRM_DEVICES", "DRM_MAPQ_SPAN",
        "DRM_MAPQ_MIN", "DRM_PAIR_RESCUE_MIN", "DRM_PAIR_TLEN_SAMPLE", "DRM_PAIR_TLEN_MAPQ")


def _fastq(path, names, reads):
    with open(path, "wb") as f:
        for n, r in zip(names, reads):
            f.write(b"@" + n.encode() + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")


def _sam(path):
    got = open(path).read().split("\n")
    assert got[-1] == ""
    return got[:-1]


def _ref_span(cigar):
    return sum(int(n) for n, op in re.findall(r"(\d+)([MIDS])", cigar) if op in "MD")


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    from deepreadmapper_amd import extract_fasta_sequence, fasta_contigs
    tmp = tmp_path_factory.mktemp("contigs_cli")
    env = dict(os.environ, DRM_BUILD_THREADS="1")
    for v in DROP:
        env.pop(v, None)
    rng = np.random.default_rng(77)
    rand = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))  # noqa: E731
    c = [rand(700), rand(150), rand(400)]
    c.append(c[2][250:400])  # chrD: chrC's last window once more, so that the search finds both for one read
    fa = tmp / "three.fa"
    fa.write_bytes(b">chrA first\n" + c[0][:300] + b"\n" + c[0][300:] + b"\n>chrB GATTACA cat\n" + c[1] +
                   b"\n>chrC tagged\n" + c[2] + b"\n>chrD\n" + c[3] + b"\n")
    names, starts, lens = fasta_contigs(str(fa))
    g = extract_fasta_sequence(str(fa))
    assert names == ["chrA", "chrB", "chrC", "chrD"] and lens.tolist() == [700, 150, 400, 150] and starts[1] == 711
    assert [g[s:s + n] for s, n in zip(starts, lens)] == c and starts[3] - (starts[2] + 250) == 151 < MAPQ_SPAN

    def index(ref, name, contigs, *more):
        e = dict(env, DRM_CONTIGS="1") if contigs else env
        r = subprocess.run([os.path.join(ROOT, "bin", "hnswpq_index"), str(ref), name, str(REF_LEN), *more], cwd=tmp,
                           env=e, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r
    r = index(fa, "ix", True)
    assert "4 contigs, 1400 bases" in r.stdout

    def run(ix, query, ref, name, extra, **more):
        return subprocess.run([os.path.join(ROOT, "bin", "pipeline"), ix, str(query), str(ref), "128", str(K), str(K), name] +
                              extra, cwd=tmp, env=dict(env, **more), capture_output=True, text=True)
    # single reads: (contig, local start, reverse) of exact windows, then a read cut across the chrA / chrB boundary, a
    # random read and one of N
    truth = [(0, 100, False), (0, 550, False), (1, 0, False), (2, 0, False), (2, 250, False), (2, 100, True),
             (0, 0, True)]
    reads = []
    for t, p, rev in truth:
        w = c[t][p:p + REF_LEN]
        reads.append(R.revcomp(w) if rev else w)
    # ... then a read that starts 4 bases in front of chrB, in the gap its header's letters make (the flank guard's case)
    reads += [c[0][-75:] + c[1][:75], g[707:711] + c[1][:146], rand(REF_LEN), b"N" * REF_LEN]
    _fastq(tmp / "reads.fastq", [f"read{i}" for i in range(len(reads))], reads)
    # pairs: proper on chrA; proper on chrC; mate 1 at the end of chrA with mate 2 at the start of chrB (close enough in
    # the genome string for the default 0,1000); mate 2 random; both N
    m1 = [c[0][50:200], c[2][20:170], c[0][550:700], c[2][200:350], b"N" * REF_LEN]
    m2 = [R.revcomp(c[0][250:400]), R.revcomp(c[2][230:380]), R.revcomp(c[1][0:150]), rand(REF_LEN), b"N" * REF_LEN]
    pnames = [f"pair{i}" for i in range(len(m1))]
    _fastq(tmp / "m1.fastq", [n + "/1" for n in pnames], m1)
    _fastq(tmp / "m2.fastq", [n + "/2" for n in pnames], m2)
    inter = [x for ab in zip(m1, m2) for x in ab]
    _fastq(tmp / "inter.fastq", [n for n in pnames for _ in range(2)], inter)
    rows = {}
    # the rescue guard's pair: mate 1 near the end of chrA; mate 2 from the start of chrB with every fourth base changed,
    # so that the rescue, scanning the genome string behind the anchor, finds it across the boundary; and a plain pair
    lost = bytearray(R.revcomp(c[1][0:150]))
    for i in range(0, REF_LEN, 4):
        lost[i] = ord("A") if lost[i] != ord("A") else ord("C")
    r1, r2 = [c[0][500:650], c[0][50:200]], [bytes(lost), R.revcomp(c[0][250:400])]
    _fastq(tmp / "r1.fastq", ["res0/1", "res1/1"], r1)
    _fastq(tmp / "r2.fastq", ["res0/2", "res1/2"], r2)
    for name, q in (("reads", "reads.fastq"), ("inter", "inter.fastq")):  # the plain runs: global ids of the rerank
        r = run("ix", tmp / q, fa, "plain_" + name, ["1", "0"])
        assert r.returncode == 0, r.stdout + r.stderr
        rows[name] = (np.load(tmp / ("plain_" + name) / "sw_ids.npy"), np.load(tmp / ("plain_" + name) / "sw_scores.npy"))
    return dict(tmp=tmp, env=env, run=run, index=index, fa=fa, g=g, contigs=(names, starts, lens), truth=truth,
                reads=reads, inter=inter, pnames=pnames, rows=rows, rand=rand, rescue=(r1, r2))


def _header(fx):
    names, _, lens = fx["contigs"]
    return ["@HD\tVN:1.0\tSO:unsorted"] + [f"@SQ\tSN:{n}\tLN:{int(x)}" for n, x in zip(names, lens)]


def _staged(fx, which):
    """contig_hits on the plain run's rows: (ids, spread, scores, contig, counts)."""
    from deepreadmapper_amd import ContigTable, contig_hits
    ids, sc = fx["rows"][which]
    cnt = (sc >= 0).sum(axis=1).astype(np.int32)  # rows past a query's status are written as -1
    table = ContigTable(fx["contigs"][1], fx["contigs"][2])
    out = contig_hits(table, ids, np.maximum(sc, 0), cnt, REF_LEN)
    table.free()
    return out


def _aligned(fx, wid, rows, queries, flank=None, contig=None):
    """(records, ops, regions): sw_align_arrays of the rows; with `flank` the affine alignment under the scoring 1,1,0,1,
    a row keeping its flank iff its clamped region lies inside its contig (the flank guard), else aligned with flank 0;
    regions[x] = (start, length, reverse) of the region row x was aligned over."""
    from deepreadmapper_amd import (ContigTable, GenomeTable, SW_ALIGNMENT_DTYPE, sw_align_affine_arrays, sw_align_arrays,
                                    sw_align_region)
    t = GenomeTable(np.frombuffer(fx["g"], dtype=np.uint8), REF_LEN)
    wid, rows = np.array(wid, dtype=np.uint64), np.array(rows, dtype=np.int64)
    if flank is None:
        rec, ops = sw_align_arrays(t, wid, rows, queries)
        t.free()
        return rec, ops, None
    table = ContigTable(fx["contigs"][1], fx["contigs"][2])
    regions, keep = [], []
    for w, ct in zip(wid, contig):
        start, n, rev = sw_align_region(t, int(w), flank)
        keep.append(table.find(start, n) == ct)
        regions.append((start, n, rev) if keep[-1] else sw_align_region(t, int(w), 0))
    keep = np.array(keep, dtype=bool)
    rec, ops = np.zeros(len(wid), dtype=SW_ALIGNMENT_DTYPE), [None] * len(wid)
    for sel, f in ((keep, flank), (~keep, 0)):
        idx = np.flatnonzero(sel)
        if len(idx):
            r, o = sw_align_affine_arrays(t, wid[idx], rows[idx], queries, (1, 1, 0, 1), flank=f)
            for x, y in enumerate(idx):
                rec[y], ops[y] = r[x], o[x]
    table.free()
    t.free()
    fx["flank_rows"] = (int(keep.sum()), int((~keep).sum()))
    return rec, ops, regions


def _cigar(rec, ops, w, region):
    from deepreadmapper_amd import sam_cigar, sam_cigar_region
    if region is None:
        return sam_cigar(rec, ops, REF_LEN + 2, REF_LEN, w)
    return sam_cigar_region(rec, ops, REF_LEN + 2, *region)


def _composed_single(fx, mapq=False, flank=None):
    from deepreadmapper_amd import hit_mapq
    names, starts, _ = fx["contigs"]
    oi, osp, osc, oc, ocnt = _staged(fx, "reads")
    reads = fx["reads"]
    pairs = [(i, j) for i in range(len(reads)) for j in range(int(ocnt[i]))]
    rec, ops, regions = _aligned(fx, [oi[i, j] for i, j in pairs], [i for i, _ in pairs], [b"<" + r + b">" for r in reads],
                                 flank, [oc[i, j] for i, j in pairs])
    q = None
    if mapq:  # the locus scan of the spread ids, head = the primary row; secondary lines print 0
        q = hit_mapq(osp, osc, ocnt, np.full(len(reads), REF_LEN), REF_LEN, head=np.zeros(len(reads)),
                     locus_span=MAPQ_SPAN)["mapq"]
    want, x = _header(fx), 0
    for i, read in enumerate(reads):
        if ocnt[i] == 0:
            want.append(f"read{i}\t4\t*\t0\t0\t*\t*\t0\t0\t{read.decode()}\t*")
        for j in range(int(ocnt[i])):
            w, t = int(oi[i, j]), int(oc[i, j])
            flag = (0 if j == 0 else 256) | (16 if w & 1 else 0)
            seq = (R.revcomp(read) if w & 1 else read).decode()
            dead = int(rec["status"][x]) == 1
            mq = 60 if q is None else 0 if dead or j > 0 else int(q[i])
            if dead:
                want.append(f"read{i}\t{flag | 4}\t{names[t]}\t0\t{mq}\t*\t*\t0\t0\t{seq}\t*")
            else:
                pos1, cigar = _cigar(rec[x], ops[x], w, regions[x] if regions else None)
                want.append(f"read{i}\t{flag}\t{names[t]}\t{pos1 - int(starts[t])}\t{mq}\t{cigar}\t*\t0\t0\t{seq}\t*\t"
                            f"AS:i:{int(rec['score'][x])}\tNM:i:{int(rec['nm'][x])}")
            x += 1
    return want


def _composed_pairs(fx, mapq=False):
    from deepreadmapper_amd import pair_hits, pair_mapq, sam_cigar, sam_pair_fields
    names, starts, _ = fx["contigs"]
    oi, osp, osc, oc, ocnt = _staged(fx, "inter")
    reads = fx["inter"]
    res = pair_hits(osp, osc, ocnt, osp[1:], osc[1:], ocnt[1:], REF_LEN, row_step=2)  # the spread ids
    chosen = {}
    for p in range(len(res)):
        for m, j in enumerate((int(res["j1"][p]), int(res["j2"][p]))):
            if j >= 0:
                chosen[2 * p + m] = (int(oi[2 * p + m, j]), int(oc[2 * p + m, j]))
    rows = sorted(chosen)
    rec, ops, _ = _aligned(fx, [chosen[r][0] for r in rows], rows, [b"<" + r + b">" for r in reads])
    pq = None
    if mapq:  # on the spread ids, as the pairing
        full = np.full(len(reads), REF_LEN)
        pq = pair_mapq(osp, osc, ocnt, osp[1:], osc[1:], ocnt[1:], full, full[1:], res, REF_LEN, row_step=2,
                       locus_span=MAPQ_SPAN)
    want = _header(fx)
    for p in range(len(res)):
        mates, text, ctg = [], [], []
        for m in range(2):
            r = 2 * p + m
            x = rows.index(r) if r in chosen else -1
            if x < 0 or int(rec["status"][x]) == 1:
                mates.append(None)
                text.append(None)
                ctg.append(None)
                continue
            w, t = chosen[r]
            pos1, cigar = sam_cigar(rec[x], ops[x], REF_LEN + 2, REF_LEN, w)
            mates.append((1, w & 1, pos1 - int(starts[t]), int(rec["ref_end"][x]) - int(rec["ref_begin"][x])))
            text.append((cigar, int(rec["score"][x]), int(rec["nm"][x])))
            ctg.append(t)
        split = None not in ctg and ctg[0] != ctg[1]
        f = sam_pair_fields(mates[0], mates[1], int(res["status"][p]) == 0 and not split)
        for m in range(2):
            read, o = reads[2 * p + m], f[m]
            own = ctg[m] if ctg[m] is not None else ctg[1 - m]
            rname = names[own] if o["has_rname"] else "*"
            rnext = "*" if not o["has_rname"] else names[ctg[1 - m]] if split else "="
            tlen = 0 if split else o["tlen"]
            mq = 60 if pq is None else 0 if mates[m] is None else int(pq["mapq1" if m == 0 else "mapq2"][p])
            if mates[m] is None:
                want.append(f"{fx['pnames'][p]}\t{o['flag']}\t{rname}\t{o['pos']}\t{mq}\t*\t{rnext}\t{o['pnext']}\t{tlen}\t"
                            f"{read.decode()}\t*")
                continue
            seq = (R.revcomp(read) if mates[m][1] else read).decode()
            cigar, score, nm = text[m]
            want.append(f"{fx['pnames'][p]}\t{o['flag']}\t{rname}\t{o['pos']}\t{mq}\t{cigar}\t{rnext}\t{o['pnext']}\t{tlen}\t"
                        f"{seq}\t*\tAS:i:{score}\tNM:i:{nm}")
    return want, res


def _inside_its_contig(fx, lines):
    """every mapped line: 1 <= POS and POS + reference span - 1 <= LN of its RNAME"""
    ln = dict(zip(fx["contigs"][0], fx["contigs"][2].tolist()))
    mapped = 0
    for line in lines:
        f = line.split("\t")
        if line.startswith("@") or int(f[1]) & 4:
            continue
        mapped += 1
        assert f[2] in ln and 1 <= int(f[3]) and int(f[3]) + _ref_span(f[5]) - 1 <= ln[f[2]], f[:9]
    return mapped


def test_single_reads(fixture):
    fx = fixture
    r = fx["run"]("ix", fx["tmp"] / "reads.fastq", fx["fa"], "single", ["1", "1"], DRM_CONTIGS="1", DRM_SAM_CIGAR="1")
    assert r.returncode == 0, r.stdout + r.stderr
    got = _sam(fx["tmp"] / "single" / "results.sam")
    H = len(_header(fx))
    assert got[:H] == _header(fx) and H == 5
    assert got == _composed_single(fx)
    r = fx["run"]("ix", fx["tmp"] / "reads.fastq", fx["fa"], "single_b3", ["1", "1"], DRM_CONTIGS="1", DRM_SAM_CIGAR="1",
                  DRM_SAM_BLOCK="3")
    assert r.returncode == 0, r.stdout + r.stderr
    assert _sam(fx["tmp"] / "single_b3" / "results.sam") == got  # blocks of three reads: the same file
    # independent of the composition: a read copied from a contig is there under the contig's name at its own position
    names = fx["contigs"][0]
    primary = {}
    for line in got[H:]:
        f = line.split("\t")
        if not int(f[1]) & 256:
            primary[f[0]] = f
    found = 0
    for i, (t, p, rev) in enumerate(fx["truth"]):
        f = primary[f"read{i}"]
        hit = f[2] == names[t] and int(f[3]) == p + 1 and f[5] == f"{REF_LEN}M" and bool(int(f[1]) & 16) == rev
        found += hit
    assert found >= len(fx["truth"]) - 1, (found, [primary[f"read{i}"][:6] for i in range(len(fx["truth"]))])
    assert _inside_its_contig(fx, got) >= found
    # the read cut across the chrA / chrB boundary: whatever it prints stays inside one contig (checked above), and the
    # window that holds all of it, which straddles the boundary, is not there as a full-length match
    cut = [l.split("\t") for l in got[H:] if l.startswith(f"read{len(fx['truth'])}\t")]
    assert cut and all(f[5] != f"{REF_LEN}M" for f in cut)
    assert int(primary[f"read{len(fx['reads']) - 1}"][1]) & 4  # the read of N: unmapped


def test_pairs(fixture):
    fx = fixture
    more = dict(DRM_CONTIGS="1", DRM_SAM_CIGAR="1", DRM_MATES=str(fx["tmp"] / "m2.fastq"))
    r = fx["run"]("ix", fx["tmp"] / "m1.fastq", fx["fa"], "paired", ["1", "1"], **more)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _sam(fx["tmp"] / "paired" / "results.sam")
    want, res = _composed_pairs(fx)
    assert got == want
    r = fx["run"]("ix", fx["tmp"] / "m1.fastq", fx["fa"], "paired_b2", ["1", "1"], DRM_SAM_BLOCK="2", **more)
    assert r.returncode == 0, r.stdout + r.stderr
    assert _sam(fx["tmp"] / "paired_b2" / "results.sam") == got
    H = len(_header(fx))
    assert len(got) == H + 2 * len(fx["pnames"])
    _inside_its_contig(fx, got)
    line = lambda p, m: got[H + 2 * p + m].split("\t")  # noqa: E731
    # the pairs inside chrA and chrC are proper, on their contig, at their local positions
    for p, (name, pos, t) in enumerate((("chrA", 51, 350), ("chrC", 21, 360))):
        a, b = line(p, 0), line(p, 1)
        assert a[2] == b[2] == name and a[6] == b[6] == "=" and int(a[1]) & 2 and int(b[1]) & 2, (a[:9], b[:9])
        assert int(a[3]) == pos and int(a[8]) == t == -int(b[8]) and a[7] == b[3] and b[7] == a[3]
    # mate 1 at the end of chrA, mate 2 at the start of chrB, 311 bases apart in the genome string: not a proper pair
    a, b = line(2, 0), line(2, 1)
    assert (a[2], a[3], a[6], a[7]) == ("chrA", "551", "chrB", "1") and (b[2], b[3], b[6], b[7]) == ("chrB", "1", "chrA", "551")
    assert a[8] == b[8] == "0" and not int(a[1]) & 2 and not int(b[1]) & 2 and int(res["n_proper"][2]) == 0
    # with the real ids the same two hits would have been a proper pair of T = 311: the stage is what prevents it
    from deepreadmapper_amd import pair_hits
    oi, _, osc, _, ocnt = _staged(fx, "inter")
    real = pair_hits(oi, osc, ocnt, oi[1:], osc[1:], ocnt[1:], REF_LEN, row_step=2)
    assert int(real["status"][2]) == 0 and int(real["tlen"][2]) == int(fx["contigs"][1][1]) + REF_LEN - 550 == 311
    assert [int(x.split("\t")[1]) & 0xC for x in got[-2:]] == [0xC, 0xC]  # the pair of N


def test_mapq_sees_two_loci_across_a_seam(fixture):
    """DRM_SAM_MAPQ=1: the locus scan and the pair MAPQ run on the spread ids. The read copied from chrC's last window
    has chrD's copy, 151 bases on in the genome string, as its second hit: with DRM_MAPQ_SPAN=200 the real ids would
    merge the two into one locus (MAPQ 60), the spread ids keep them apart."""
    from deepreadmapper_amd import hit_mapq
    fx = fixture
    more = dict(DRM_CONTIGS="1", DRM_SAM_CIGAR="1", DRM_SAM_MAPQ="1", DRM_MAPQ_SPAN=str(MAPQ_SPAN))
    r = fx["run"]("ix", fx["tmp"] / "reads.fastq", fx["fa"], "single_mapq", ["1", "1"], DRM_SAM_BLOCK="4", **more)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _sam(fx["tmp"] / "single_mapq" / "results.sam")
    assert got == _composed_single(fx, mapq=True)
    # the seam read is truth[4] = (chrC, 250): its list holds chrC's window and chrD's, both at 150
    oi, osp, osc, oc, ocnt = _staged(fx, "reads")
    i = fx["truth"].index((2, 250, False))
    starts = fx["contigs"][1]
    kept = {(int(oc[i, j]), int(oi[i, j])): int(osc[i, j]) for j in range(int(ocnt[i]))}
    assert kept.get((2, 2 * (int(starts[2]) + 250))) == REF_LEN and kept.get((3, 2 * int(starts[3]))) == REF_LEN, kept
    full, head = np.full(len(oi), REF_LEN), np.zeros(len(oi))
    real = hit_mapq(oi, osc, ocnt, full, REF_LEN, head=head, locus_span=MAPQ_SPAN)
    spread = hit_mapq(osp, osc, ocnt, full, REF_LEN, head=head, locus_span=MAPQ_SPAN)
    assert int(real["locus_rows"][i]) > int(spread["locus_rows"][i]) and int(real["sub_score"][i]) < REF_LEN
    assert int(spread["mapq"][i]) == 0 < 40 < int(real["mapq"][i]) and int(spread["sub_score"][i]) == REF_LEN
    line = [l.split("\t") for l in got if l.startswith(f"read{i}\t") and not int(l.split("\t")[1]) & 256]
    assert len(line) == 1 and (line[0][2], line[0][3]) in (("chrC", "251"), ("chrD", "1"))
    assert int(line[0][4]) == int(spread["mapq"][i])
    assert int(got[len(_header(fx))].split("\t")[4]) == 60  # read0, unique on chrA
    # pairs
    r = fx["run"]("ix", fx["tmp"] / "m1.fastq", fx["fa"], "paired_mapq", ["1", "1"], DRM_MATES=str(fx["tmp"] / "m2.fastq"),
                  **more)
    assert r.returncode == 0, r.stdout + r.stderr
    want, _ = _composed_pairs(fx, mapq=True)
    assert _sam(fx["tmp"] / "paired_mapq" / "results.sam") == want


def test_flank_guard_fires(fixture):
    """DRM_SAM_FLANK=8: a row whose flanked region leaves its contig is aligned without the flank. The read that starts 4
    bases in front of chrB would, with the flank, align over the gap to a position in front of its contig."""
    fx = fixture
    r = fx["run"]("ix", fx["tmp"] / "reads.fastq", fx["fa"], "single_flank", ["1", "1"], DRM_CONTIGS="1", DRM_SAM_CIGAR="1",
                  DRM_SAM_FLANK="8", DRM_SAM_BLOCK="3")
    assert r.returncode == 0, r.stdout + r.stderr
    got = _sam(fx["tmp"] / "single_flank" / "results.sam")
    assert got == _composed_single(fx, flank=8)
    with_flank, without = fx["flank_rows"]
    assert with_flank > 0 and without > 0  # both passes of the aligner ran
    _inside_its_contig(fx, got)
    i = len(fx["truth"]) + 1
    line = [l.split("\t") for l in got if l.startswith(f"read{i}\t") and l.split("\t")[2] == "chrB"]
    assert line and line[0][3] == "1" and line[0][5] == "4S146M", line
    # a read well inside chrA keeps its flank: aligned over 166 bases, it is still 150M at its place
    f = [l.split("\t") for l in got if l.startswith("read0\t")][0]
    assert (f[2], f[3], f[5]) == ("chrA", "101", f"{REF_LEN}M")


def test_rescue_guard_fires_and_tlen_auto_runs_the_chained_stage(fixture):
    from deepreadmapper_amd import ContigTable, GenomeTable, mate_rescue, mate_rescue_window
    fx = fixture
    tmp = fx["tmp"]
    r1, r2 = fx["rescue"]
    starts, lens = fx["contigs"][1], fx["contigs"][2]
    # what the rescue finds for mate 2 behind the anchor chrA:500: a hit good enough to be taken, on chrB
    t, table = GenomeTable(np.frombuffer(fx["g"], dtype=np.uint8), REF_LEN), ContigTable(starts, lens)
    rec = mate_rescue(t, [2 * 500], [1], [b"<" + r1[0] + b">", b"<" + r2[0] + b">"])
    assert int(rec["status"][0]) == 0 and int(rec["score"][0]) >= 49
    w = mate_rescue_window(rec[0], REF_LEN, len(fx["g"]))
    # ... or hanging over its end: either way not inside the anchor's contig
    assert w & 1 and abs((w >> 1) - int(starts[1])) <= 4 and table.find(w >> 1, REF_LEN) in (1, -1)
    assert table.find(500, REF_LEN) == 0
    t.free()
    table.free()
    more = dict(DRM_CONTIGS="1", DRM_SAM_CIGAR="1", DRM_MATES=str(tmp / "r2.fastq"))
    out = {}
    for name, extra in (("rescue_off", {}), ("rescue_on", dict(DRM_PAIR_RESCUE="1"))):
        r = fx["run"]("ix", tmp / "r1.fastq", fx["fa"], name, ["1", "1"], **more, **extra)
        assert r.returncode == 0, r.stdout + r.stderr
        out[name] = _sam(tmp / name / "results.sam")
    H = len(_header(fx))
    a, b = (x.split("\t") for x in out["rescue_on"][H:H + 2])
    assert a[2] == "chrA" and a[3] == "501" and not int(a[1]) & 2 and not int(b[1]) & 2 and b[2] != "chrB"
    _inside_its_contig(fx, out["rescue_on"])
    assert out["rescue_on"][H:H + 2] == out["rescue_off"][H:H + 2]  # the rescue across the boundary changed nothing
    assert all(int(x.split("\t")[1]) & 2 for x in out["rescue_on"][H + 2:H + 4])  # the plain pair is proper
    # DRM_PAIR_TLEN=auto: the pre-pass chains the stage on the device; too few pairs to estimate from, so the default
    # window stays and the file is the one of the run without it
    r = fx["run"]("ix", tmp / "m1.fastq", fx["fa"], "paired_auto", ["1", "1"], DRM_CONTIGS="1", DRM_SAM_CIGAR="1",
                  DRM_MATES=str(tmp / "m2.fastq"), DRM_PAIR_TLEN="auto")
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"FR/RF/same/far = (\d+)/(\d+)/(\d+)/(\d+)", r.stdout)
    assert "Template length (auto)" in r.stdout and m, r.stdout
    # the pair either side of the chrA / chrB boundary, 311 bases apart in the genome string, is "far" on the spread ids
    assert int(m.group(1)) >= 1 and int(m.group(4)) == 1, r.stdout
    want, _ = _composed_pairs(fx)
    assert _sam(tmp / "paired_auto" / "results.sam") == want


def test_single_contig_changes_only_sq_and_rname(fixture):
    """A single-contig FASTA with DRM_SAM_FLANK and DRM_PAIR_RESCUE=1 on: the guards never fire, and the paired file
    differs from the run without DRM_CONTIGS only in the @SQ line and column 3."""
    fx = fixture
    tmp = fx["tmp"]
    body = open(os.path.join(GOLDEN, "ecoli_150.fna"), "rb").read().split(b"\n", 1)[1]
    fna = tmp / "ecoli.fna"
    fna.write_bytes(b">ecoli Fake DNA sequence\n" + body)
    fx["index"](fna, "eco", True)
    from deepreadmapper_amd import extract_fasta_sequence
    g = extract_fasta_sequence(str(fna))
    frags = [(10, 200), (40, 260), (95, 330), (222, 500), (433, 377), (0, 300), (700, 300)]
    m1 = [g[p:p + REF_LEN] for p, t in frags] + [g[500:650], b"N" * REF_LEN]
    m2 = [R.revcomp(g[p + t - REF_LEN:p + t]) for p, t in frags] + [fx["rand"](REF_LEN), b"N" * REF_LEN]
    # a mate the search cannot find but the rescue can: mate 2 of the first pair with a third of its bases changed
    bad = bytearray(m2[0])
    for i in range(0, REF_LEN, 3):
        bad[i] = ord("A") if bad[i] != ord("A") else ord("C")
    m2[0] = bytes(bad)
    names = [f"e{i}" for i in range(len(m1))]
    _fastq(tmp / "e1.fastq", [n + "/1" for n in names], m1)
    _fastq(tmp / "e2.fastq", [n + "/2" for n in names], m2)
    more = dict(DRM_SAM_CIGAR="1", DRM_MATES=str(tmp / "e2.fastq"), DRM_SAM_FLANK="8", DRM_PAIR_RESCUE="1")
    out = {}
    for name, extra in (("eco_plain", {}), ("eco_contigs", dict(DRM_CONTIGS="1"))):
        r = fx["run"]("eco", tmp / "e1.fastq", fna, name, ["1", "1"], **more, **extra)
        assert r.returncode == 0, r.stdout + r.stderr
        out[name] = _sam(tmp / name / "results.sam")
    plain, got = out["eco_plain"], out["eco_contigs"]
    assert plain[1] == "@SQ\tSN:ref\tLN:150" and got[1] == f"@SQ\tSN:ecoli\tLN:{len(g)}" and plain[0] == got[0]
    assert len(plain) == len(got) == 2 + 2 * len(names)
    for a, b in zip(plain[2:], got[2:]):
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[2] in ("ref", "*") and fb[2] == ("ecoli" if fa[2] == "ref" else "*")
        assert fa[:2] + fa[3:] == fb[:2] + fb[3:]
    assert sum(int(x.split("\t")[1]) & 2 > 0 for x in got[2:]) >= 2 * (len(frags) - 1)


def test_violated_requirements_end_the_run_before_the_search(fixture):
    fx = fixture
    tmp = fx["tmp"]
    np.save(tmp / "q.npy", np.zeros((2, 128), np.float32))
    fx["index"](fx["fa"], "s2", False, "2")       # stride 2
    fx["index"](fx["fa"], "plainix", False)        # built without DRM_CONTIGS: windows per contig
    reads, ok = tmp / "reads.fastq", dict(DRM_CONTIGS="1", DRM_SAM_CIGAR="1")
    cases = [("ix", reads, ["1", "0"], ok, "use_streaming"),
             ("ix", reads, ["0", "1"], ok, "use_dynamic"),
             ("ix", reads, ["1", "1"], dict(DRM_CONTIGS="1"), "DRM_SAM_CIGAR"),
             ("ix", tmp / "q.npy", ["1", "1"], ok, "sequence queries"),
             ("ix", reads, ["1", "1"], dict(ok, DRM_DEVICES="0,1"), "one device"),
             ("s2", reads, ["1", "1"], ok, "stride 1"),
             ("ix", reads, ["1", "1"], dict(ok, DRM_SAM_L2_ROWS="1"), "DRM_SAM_L2_ROWS"),
             ("plainix", reads, ["1", "1"], ok, "rebuild the index with DRM_CONTIGS=1")]
    for ix, q, extra, more, word in cases:
        r = fx["run"](ix, q, fx["fa"], "bad", extra, **more)
        assert r.returncode == 1 and r.stderr.startswith("Error:") and word in r.stderr, (word, r.stdout, r.stderr)
        assert "Search" not in r.stdout and not os.path.exists(tmp / "bad" / "results.sam"), word
        if ix != "plainix":
            assert "Index loaded" not in r.stdout, word
