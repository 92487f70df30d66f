"""GPU tests of bin/pipeline's paired mode (DRM_MATES): read pairs simulated from the C1 genome come out as two SAM
lines per pair whose every byte is the composition of the package's wrappers (pair_hits, sw_align_arrays /
sw_align_affine_arrays, sam_cigar(_region), sam_pair_fields) on the unpaired run's rerank output; simulated pairs whose
true windows were found carry the proper-pair flag and their template length; the file does not depend on
DRM_SAM_BLOCK; bad input ends the run before the index is loaded; without DRM_MATES nothing changes."""
import os
import subprocess

import numpy as np
import pytest

import sw_align_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FNA = os.path.join(GOLDEN, "ecoli_150.fna")
REF_LEN = 150
PAIR_ENV = ("DRM_MATES", "DRM_PAIR_TLEN", "DRM_PAIR_PENALTY", "DRM_SAM_CIGAR", "DRM_SAM_SCORING", "DRM_SAM_FLANK",
            "DRM_SAM_BLOCK", "DRM_DEVICES")
# (fragment start, template length, mate roles swapped) of the simulated pairs
FRAGMENTS = [(10, 200, False), (40, 260, False), (95, 330, False), (150, 410, False), (222, 500, False),
             (301, 290, False), (433, 377, False), (60, 240, True), (180, 450, True), (350, 310, True)]


def _fastq(path, names, reads):
    with open(path, "wb") as f:
        for n, r in zip(names, reads):
            f.write(b"@" + n.encode() + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    """The C1 index, the two mate files, their interleaved file, and the unpaired run's rerank output."""
    from deepreadmapper_amd import extract_fasta_sequence
    tmp = tmp_path_factory.mktemp("pair_cli")
    env = dict(os.environ, DRM_BUILD_THREADS="1")
    for v in PAIR_ENV:
        env.pop(v, None)
    r = subprocess.run([os.path.join(ROOT, "bin", "hnswpq_index"), FNA, "c1", "150"], cwd=tmp, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = extract_fasta_sequence(FNA)
    rng = np.random.default_rng(42)
    rand = lambda: bytes(rng.choice(list(b"ACGT"), size=REF_LEN).astype(np.uint8))  # noqa: E731
    m1, m2, truth = [], [], []
    for p, t, swapped in FRAGMENTS:
        assert p + t <= len(g)
        a, b = g[p:p + REF_LEN], R.revcomp(g[p + t - REF_LEN:p + t])
        wa, wb = 2 * p, 2 * (p + t - REF_LEN) + 1
        if swapped:
            a, b, wa, wb = b, a, wb, wa
        m1.append(a)
        m2.append(b)
        truth.append((wa, wb, t))
    m1 += [g[500:650], rand(), g[700:850], b"N" * REF_LEN]  # mate 2 random; both random; mate 2 / both without a hit
    m2 += [rand(), rand(), b"N" * REF_LEN, b"N" * REF_LEN]
    names = [f"pair{i}" for i in range(len(m1))]
    _fastq(tmp / "m1.fastq", [n + "/1" for n in names], m1)
    _fastq(tmp / "m2.fastq", [n + "/2" for n in names], m2)
    inter = [x for ab in zip(m1, m2) for x in ab]
    _fastq(tmp / "inter.fastq", [n for n in names for _ in range(2)], inter)
    base = [os.path.join(ROOT, "bin", "pipeline"), "c1"]

    def run(query, name, extra, **more):
        return subprocess.run(base + [str(query), FNA, "128", "4", "4", name] + extra, cwd=tmp,
                              env=dict(env, **more), capture_output=True, text=True)
    r = run(tmp / "inter.fastq", "unpaired", ["1", "0"])
    assert r.returncode == 0, r.stdout + r.stderr
    ids = np.load(tmp / "unpaired" / "sw_ids.npy")
    sc = np.load(tmp / "unpaired" / "sw_scores.npy")
    assert ids.shape == sc.shape == (len(inter), 4)
    return dict(tmp=tmp, run=run, g=g, names=names, reads=inter, truth=truth, ids=ids, sc=sc)


def _composed(fx, affine=None, **pair):
    """The expected SAM lines, from the unpaired run's rows and the package's wrappers."""
    from deepreadmapper_amd import (GenomeTable, pair_hits, sam_cigar, sam_cigar_region, sam_pair_fields,
                                    sw_align_affine_arrays, sw_align_arrays, sw_align_region)
    ids, sc, reads = fx["ids"], fx["sc"], fx["reads"]
    cnt = (sc >= 0).sum(axis=1).astype(np.int32)  # rows past a query's status are written as -1
    sc = np.maximum(sc, 0)
    res = pair_hits(ids, sc, cnt, ids[1:], sc[1:], cnt[1:], REF_LEN, row_step=2, **pair)
    chosen = {}
    for p in range(len(res)):
        for m, j in enumerate((int(res["j1"][p]), int(res["j2"][p]))):
            if j >= 0:
                chosen[2 * p + m] = int(ids[2 * p + m, j])
    rows = sorted(chosen)
    queries = [b"<" + r + b">" for r in reads]
    t = GenomeTable(np.frombuffer(fx["g"], dtype=np.uint8), REF_LEN)
    wid = np.array([chosen[r] for r in rows], dtype=np.uint64)
    if affine:
        scoring, flank = affine
        rec, ops = sw_align_affine_arrays(t, wid, np.array(rows), queries, scoring, flank=flank)
    else:
        rec, ops = sw_align_arrays(t, wid, np.array(rows), queries)
    want = ["@HD\tVN:1.0\tSO:unsorted", "@SQ\tSN:ref\tLN:150"]
    for p in range(len(res)):
        mates, text = [], []
        for m in range(2):
            r = 2 * p + m
            x = rows.index(r) if r in chosen else -1
            if x < 0 or int(rec["status"][x]) == 1:
                mates.append(None)
                text.append(None)
                continue
            w = chosen[r]
            if affine:
                start, n, rev = sw_align_region(t, w, affine[1])
                pos1, cigar = sam_cigar_region(rec[x], ops[x], REF_LEN + 2, start, n, rev)
            else:
                pos1, cigar = sam_cigar(rec[x], ops[x], REF_LEN + 2, REF_LEN, w)
            mates.append((1, w & 1, pos1, int(rec["ref_end"][x]) - int(rec["ref_begin"][x])))
            text.append((cigar, int(rec["score"][x]), int(rec["nm"][x])))
        f = sam_pair_fields(mates[0], mates[1], int(res["status"][p]) == 0)
        for m in range(2):
            read, o = reads[2 * p + m], f[m]
            rname, rnext = ("ref", "=") if o["has_rname"] else ("*", "*")
            if mates[m] is None:
                want.append(f"{fx['names'][p]}\t{o['flag']}\t{rname}\t{o['pos']}\t60\t*\t{rnext}\t{o['pnext']}\t"
                            f"{o['tlen']}\t{read.decode()}\t*")
                continue
            seq = (R.revcomp(read) if mates[m][1] else read).decode()
            cigar, score, nm = text[m]
            assert R.cigar_query_length(cigar) == len(seq)
            want.append(f"{fx['names'][p]}\t{o['flag']}\tref\t{o['pos']}\t60\t{cigar}\t=\t{o['pnext']}\t{o['tlen']}\t"
                        f"{seq}\t*\tAS:i:{score}\tNM:i:{nm}")
    t.free()
    return want, res


def _sam(fx, name):
    got = open(fx["tmp"] / name / "results.sam").read().split("\n")
    assert got[-1] == ""
    return got[:-1]


def _paired(fx, name, **more):
    r = fx["run"](fx["tmp"] / "m1.fastq", name, ["1", "1"], DRM_MATES=str(fx["tmp"] / "m2.fastq"), DRM_SAM_CIGAR="1",
                  **more)
    assert r.returncode == 0, r.stdout + r.stderr
    return _sam(fx, name)


def test_paired_sam_equals_the_composition_and_flags_true_pairs(fixture):
    fx = fixture
    want, res = _composed(fx)
    got = _paired(fx, "paired")
    assert got == want
    assert _paired(fx, "paired_b3", DRM_SAM_BLOCK="3") == want  # five blocks of pairs: the same file
    assert len(got) == 2 + 2 * len(fx["names"])
    # independent of the composition: a simulated pair whose two true windows are among its reads' hits is a proper
    # pair with its template length
    found = 0
    for p, (wa, wb, t) in enumerate(fx["truth"]):
        if wa not in fx["ids"][2 * p].tolist() or wb not in fx["ids"][2 * p + 1].tolist():
            continue
        found += 1
        for m in range(2):
            f = got[2 + 2 * p + m].split("\t")
            assert int(f[1]) & 0x2 and int(f[1]) & 0x1 and f[6] == "=" and abs(int(f[8])) >= REF_LEN, (p, f)
            assert abs(int(f[8])) == t and int(f[1]) & (0x40 if m == 0 else 0x80), (p, f)
        a, b = got[2 + 2 * p].split("\t"), got[3 + 2 * p].split("\t")
        assert int(a[8]) == -int(b[8]) and a[3] == b[7] and a[7] == b[3]
    assert found >= 1, "no simulated pair has both true windows in its hit lists: the fixture positions are wrong"
    # the reads without any hit: mate 2 of the last but one pair, both mates of the last
    n = len(fx["names"])
    one, none = got[2 + 2 * (n - 2):2 + 2 * (n - 1)], got[2 + 2 * (n - 1):]
    assert [int(x.split("\t")[1]) & 0xC for x in one] == [0x8, 0x4] and one[1].split("\t")[2:9:4] == ["ref", "="]
    assert one[1].split("\t")[3] == one[0].split("\t")[3] and one[1].split("\t")[5] == "*"
    assert [x.split("\t")[1:9] for x in none] == [[str(0x1 | 0x4 | 0x8 | f), "*", "0", "60", "*", "*", "0", "0"]
                                                  for f in (0x40, 0x80)]
    assert res["status"].tolist()[-2:] == [2, 4]


def test_paired_sam_with_affine_scoring_and_flank(fixture):
    fx = fixture
    want, _ = _composed(fx, affine=((1, 4, 6, 1), 8))
    got = _paired(fx, "paired_affine", DRM_SAM_SCORING="1,4,6,1", DRM_SAM_FLANK="8", DRM_SAM_BLOCK="3")
    assert got == want
    # the pairing parameters reach the kernel: a template-length window that excludes every simulated pair
    want, res = _composed(fx, min_tlen=0, max_tlen=160, unpaired_penalty=0)
    assert (res["status"] != 0).all()
    assert _paired(fx, "paired_narrow", DRM_PAIR_TLEN="0,160", DRM_PAIR_PENALTY="0") == want
    assert not any(int(x.split("\t")[1]) & 0x2 for x in want[2:])


def test_bad_paired_input_ends_before_the_index_is_loaded(fixture):
    fx = fixture
    tmp = fx["tmp"]
    reads = fx["reads"]
    _fastq(tmp / "short.fastq", [f"pair{i}/2" for i in range(3)], reads[1:6:2])
    _fastq(tmp / "renamed.fastq", [("other" if i == 2 else f"pair{i}") + "/2" for i in range(len(fx["names"]))],
           reads[1::2])
    m2 = str(tmp / "m2.fastq")
    cases = [(["1", "1"], dict(DRM_MATES=str(tmp / "short.fastq"), DRM_SAM_CIGAR="1"), "record 3"),
             (["1", "1"], dict(DRM_MATES=str(tmp / "renamed.fastq"), DRM_SAM_CIGAR="1"), "record 2"),
             (["1", "0"], dict(DRM_MATES=m2, DRM_SAM_CIGAR="1"), "use_streaming"),
             (["0", "1"], dict(DRM_MATES=m2, DRM_SAM_CIGAR="1"), "use_dynamic"),
             (["1", "1"], dict(DRM_MATES=m2), "DRM_SAM_CIGAR"),
             (["1", "1"], dict(DRM_MATES=m2, DRM_SAM_CIGAR="1", DRM_PAIR_TLEN="100"), "DRM_PAIR_TLEN"),
             (["1", "1"], dict(DRM_MATES=m2, DRM_SAM_CIGAR="1", DRM_PAIR_TLEN="500,100"), "DRM_PAIR_TLEN"),
             (["1", "1"], dict(DRM_MATES=m2, DRM_SAM_CIGAR="1", DRM_PAIR_TLEN="0,1e3"), "DRM_PAIR_TLEN"),
             (["1", "1"], dict(DRM_MATES=m2, DRM_SAM_CIGAR="1", DRM_PAIR_PENALTY="-1"), "DRM_PAIR_PENALTY"),
             (["1", "1"], dict(DRM_MATES=str(tmp / "missing.fastq"), DRM_SAM_CIGAR="1"), "missing.fastq")]
    for extra, more, word in cases:
        r = fx["run"](tmp / "m1.fastq", "bad", extra, **more)
        assert r.returncode == 1 and r.stderr.startswith("Error:") and word in r.stderr, (more, r.stdout, r.stderr)
        assert "Index loaded" not in r.stdout and not os.path.exists(tmp / "bad" / "results.sam"), more


def test_pair_variables_without_mates_change_nothing(fixture):
    fx = fixture
    r = fx["run"](fx["tmp"] / "m1.fastq", "plain", ["1", "1"], DRM_SAM_CIGAR="1")
    assert r.returncode == 0, r.stdout + r.stderr
    r = fx["run"](fx["tmp"] / "m1.fastq", "ignored", ["1", "1"], DRM_SAM_CIGAR="1", DRM_PAIR_TLEN="garbage",
                  DRM_PAIR_PENALTY="x")
    assert r.returncode == 0, r.stdout + r.stderr
    plain = open(fx["tmp"] / "plain" / "results.sam", "rb").read()
    assert open(fx["tmp"] / "ignored" / "results.sam", "rb").read() == plain
    assert b"\t*\t0\t0\t" in plain and b"\t=\t" not in plain  # the unpaired lines, as before
