"""GPU tests of bin/pipeline's DRM_SAM_MAPQ=1: on the C1 genome with an exact 300-base duplicate appended, reads from
unique sequence, from the duplicate, with 10 substitutions and of random bases come out, as single reads and as pairs
(with and without DRM_PAIR_RESCUE=1), as the composition of the package's wrappers on the unpaired run's rerank rows
byte for byte -- the paired file being today's file with only column 5 replaced; the composition itself holds a MAPQ of
0, one strictly between 0 and 60 and one of 60; the file does not depend on DRM_SAM_BLOCK; bad input ends the run before
the index is loaded; without DRM_SAM_MAPQ every line says 60 as before."""
import os
import subprocess

import numpy as np
import pytest

import sw_align_ref as R
from deepreadmapper_amd import hit_mapq, pair_mapq, pair_mapq_rescued  # noqa: F401  (what this file is about)
from test_gpu_pair_cli import _fastq
from test_gpu_rescue_cli import _composed, mutate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNA = os.path.join(ROOT, "tests", "golden", "ecoli_150.fna")
REF_LEN = 150
DUP = (100, 400)  # the stretch of the C1 genome appended to it once more
ENV = ("DRM_MATES", "DRM_PAIR_TLEN", "DRM_PAIR_PENALTY", "DRM_PAIR_RESCUE", "DRM_PAIR_RESCUE_MIN", "DRM_SAM_CIGAR",
       "DRM_SAM_SCORING", "DRM_SAM_FLANK", "DRM_SAM_BLOCK", "DRM_DEVICES", "DRM_SAM_MAPQ", "DRM_MAPQ_MIN",
       "DRM_MAPQ_SPAN", "DRM_SAM_L2_ROWS")


def substitute10(read):
    """10 substitutions, every 15th base from the 8th."""
    nxt = dict(zip(b"ACGT", b"CGTA"))
    s = bytearray(read)
    for i in range(7, len(s), 15):
        s[i] = nxt[s[i]]
    assert sum(a != b for a, b in zip(s, read)) == 10
    return bytes(s)


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    """The duplicated genome and its index, the two mate files, their interleaved file (the single reads), and the
    unpaired run's rerank output."""
    from deepreadmapper_amd import extract_fasta_sequence
    tmp = tmp_path_factory.mktemp("mapq_cli")
    env = dict(os.environ, DRM_BUILD_THREADS="1")
    for v in ENV:
        env.pop(v, None)
    c1 = extract_fasta_sequence(FNA)
    g = c1 + c1[DUP[0]:DUP[1]]
    fna = tmp / "dup.fna"
    with open(fna, "wb") as f:
        f.write(b"> C1 with a 300-base duplicate\n" + b"\n".join(g[i:i + 80] for i in range(0, len(g), 80)) + b"\n")
    assert extract_fasta_sequence(str(fna)) == g
    r = subprocess.run([os.path.join(ROOT, "bin", "hnswpq_index"), str(fna), "c1dup", "150"], cwd=tmp, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(42)
    rand = lambda: bytes(rng.choice(list(b"ACGT"), size=REF_LEN).astype(np.uint8))  # noqa: E731
    frag = lambda p, t: (g[p:p + REF_LEN], R.revcomp(g[p + t - REF_LEN:p + t]))  # noqa: E731
    pairs = [frag(450, 300), frag(520, 260), frag(610, 350)]                # unique sequence
    pairs += [frag(150, 450), (frag(450, 300)[1], g[180:330])]               # one mate inside the duplicate
    pairs += [frag(120, 270)]                                                # both mates inside it
    a, b = frag(480, 400)
    pairs += [(substitute10(a), b), (a, substitute10(b))]                    # 10 substitutions
    a, b = frag(430, 377)
    pairs += [(a, mutate(b, 3))]                                             # a mate the search loses
    a, b = frag(640, 300)
    pairs += [(mutate(a, 3), b)]
    pairs += [(g[500:650], rand()), (rand(), rand()), (g[700:850], b"N" * REF_LEN), (b"N" * REF_LEN, b"N" * REF_LEN)]
    m1, m2 = [p[0] for p in pairs], [p[1] for p in pairs]
    names = [f"pair{i}" for i in range(len(m1))]
    _fastq(tmp / "m1.fastq", [n + "/1" for n in names], m1)
    _fastq(tmp / "m2.fastq", [n + "/2" for n in names], m2)
    inter = [x for ab in zip(m1, m2) for x in ab]
    _fastq(tmp / "inter.fastq", [n for n in names for _ in range(2)], inter)
    base = [os.path.join(ROOT, "bin", "pipeline"), "c1dup"]

    def run(query, name, extra, **more):
        return subprocess.run(base + [str(query), str(fna), "128", "4", "4", name] + extra, cwd=tmp,
                              env=dict(env, **more), capture_output=True, text=True)
    r = run(tmp / "inter.fastq", "unpaired", ["1", "0"])
    assert r.returncode == 0, r.stdout + r.stderr
    ids = np.load(tmp / "unpaired" / "sw_ids.npy")
    sc = np.load(tmp / "unpaired" / "sw_scores.npy")
    assert ids.shape == sc.shape == (len(inter), 4)
    return dict(tmp=tmp, run=run, g=g, names=names, reads=inter, truth=[], ids=ids, sc=sc)


def _lists(fx):
    sc = fx["sc"]
    cnt = (sc >= 0).sum(axis=1).astype(np.int32)  # rows past a query's status are written as -1
    return fx["ids"], np.maximum(sc, 0), cnt, np.array([len(r) for r in fx["reads"]], np.int32)


def _column5(lines):
    return [int(x.split("\t")[4]) for x in lines if not x.startswith("@")]


def _assert_spread(lines, what):
    q = _column5(lines)
    assert 0 in q and 60 in q and any(0 < x < 60 for x in q), (what, "the fixture does not spread the MAPQs", q)


def _composed_single(fx, **prm):
    """The expected single-read SAM: every rerank row of every read aligned (sw_align_arrays) and formatted
    (sam_cigar), the primary row's MAPQ from hit_mapq with head 0."""
    from deepreadmapper_amd import GenomeTable, sam_cigar, sw_align_arrays
    ids, sc, cnt, full = _lists(fx)
    reads = fx["reads"]
    res = hit_mapq(ids, sc, cnt, full, REF_LEN, head=np.zeros(len(cnt), np.int32), **prm)
    rows = [(i, j) for i in range(len(reads)) for j in range(int(cnt[i]))]
    queries = [b"<" + r + b">" for r in reads]
    t = GenomeTable(np.frombuffer(fx["g"], dtype=np.uint8), REF_LEN)
    rec, ops = sw_align_arrays(t, np.array([ids[i, j] for i, j in rows], dtype=np.uint64),
                               np.array([i for i, _ in rows]), queries)
    want = ["@HD\tVN:1.0\tSO:unsorted", "@SQ\tSN:ref\tLN:150"]
    for x, (i, j) in enumerate(rows):
        wid, read, name = int(ids[i, j]), reads[i], fx["names"][i // 2]
        flag = (0 if j == 0 else 256) | (16 if wid % 2 else 0)
        seq = (R.revcomp(read) if wid % 2 else read).decode()
        if int(rec["status"][x]) == 1:
            want.append(f"{name}\t{flag | 4}\tref\t0\t0\t*\t*\t0\t0\t{seq}\t*")
            continue
        pos1, cigar = sam_cigar(rec[x], ops[x], REF_LEN + 2, REF_LEN, wid)
        q = int(res["mapq"][i]) if j == 0 else 0
        want.append(f"{name}\t{flag}\tref\t{pos1}\t{q}\t{cigar}\t*\t0\t0\t{seq}\t*\tAS:i:{int(rec['score'][x])}"
                    f"\tNM:i:{int(rec['nm'][x])}")
    t.free()
    return want, res


def _composed_paired(fx, rescue, **prm):
    """Today's paired file (test_gpu_rescue_cli's composition, every line 60) with only column 5 replaced: pair_mapq on
    the lists pair_hits saw, pair_mapq_rescued on the pairs a rescue changed, 0 for an unmapped mate."""
    from deepreadmapper_amd import PAIR_RESULT_DTYPE, pair_hits
    today, final = _composed(fx, rescue)
    ids, sc, cnt, full = _lists(fx)
    res = pair_hits(ids, sc, cnt, ids[1:], sc[1:], cnt[1:], REF_LEN, row_step=2)
    pm = pair_mapq(ids, sc, cnt, ids[1:], sc[1:], cnt[1:], full, full[1:], res, REF_LEN, row_step=2, **prm)
    if rescue:
        after = np.zeros(len(final), dtype=PAIR_RESULT_DTYPE)
        rescue_score = np.zeros(len(final), np.int32)
        for p, (rec, _) in enumerate(final):
            after[p] = tuple(rec[f] for f in PAIR_RESULT_DTYPE.names)
            if rec["status"] == 5:  # mate 1 is the anchor: the sum less its score
                rescue_score[p] = rec["score"] - int(sc[2 * p, rec["j1"]])
            elif rec["status"] == 6:
                rescue_score[p] = rec["score"] - int(sc[2 * p + 1, rec["j2"]])
        pm = pair_mapq_rescued(after, pm, rescue_score, full, full[1:], REF_LEN, row_step=2, **prm)
    want = today[:2]
    for x, line in enumerate(today[2:]):
        f = line.split("\t")
        assert f[4] == "60"
        f[4] = "0" if int(f[1]) & 0x4 else str(int(pm["mapq1" if x % 2 == 0 else "mapq2"][x // 2]))
        want.append("\t".join(f))
    return want, today, final, pm


def _sam(fx, name):
    got = open(fx["tmp"] / name / "results.sam").read().split("\n")
    assert got[-1] == ""
    return got[:-1]


def _single(fx, name, **more):
    r = fx["run"](fx["tmp"] / "inter.fastq", name, ["1", "1"], DRM_SAM_CIGAR="1", **more)
    assert r.returncode == 0, r.stdout + r.stderr
    return _sam(fx, name)


def _paired(fx, name, **more):
    r = fx["run"](fx["tmp"] / "m1.fastq", name, ["1", "1"], DRM_MATES=str(fx["tmp"] / "m2.fastq"), DRM_SAM_CIGAR="1",
                  **more)
    assert r.returncode == 0, r.stdout + r.stderr
    return _sam(fx, name)


def test_single_read_sam_equals_the_composition(fixture):
    fx = fixture
    want, res = _composed_single(fx)
    _assert_spread(want, "single reads")
    got = _single(fx, "single", DRM_SAM_MAPQ="1")
    assert got == want
    assert _single(fx, "single_b3", DRM_SAM_MAPQ="1", DRM_SAM_BLOCK="3") == want  # ten blocks of reads: the same file
    assert _single(fx, "single_dflt", DRM_SAM_MAPQ="1", DRM_MAPQ_MIN="39", DRM_MAPQ_SPAN="150") == want  # the defaults
    # the reads from the duplicate have both copies among their rows (the same few bases beside the exact window where
    # the search missed it), score the same in both and map with MAPQ 0; secondary lines say 0
    ids = fx["ids"]
    for read in (6, 9, 10, 11):
        best, sub = int(ids[read, int(res["best"][read])]), int(ids[read, int(res["sub_row"][read])])
        assert int(res["best_score"][read]) == int(res["sub_score"][read]) > REF_LEN - 10
        assert abs((best >> 1) - (sub >> 1)) > len(fx["g"]) - DUP[1] - 10 and int(res["mapq"][read]) == 0
    for line in want[2:]:
        f = line.split("\t")
        assert not (int(f[1]) & (256 | 4)) or f[4] == "0", line
    # the parameters reach the kernel: a chance level above every score maps nothing, a span of one base makes the
    # stride-1 neighbours competitors
    for name, more, prm in (("single_min", dict(DRM_MAPQ_MIN="151"), dict(min_score=151)),
                            ("single_span", dict(DRM_MAPQ_SPAN="1"), dict(locus_span=1))):
        other, _ = _composed_single(fx, **prm)
        assert other != want and _single(fx, name, DRM_SAM_MAPQ="1", **more) == other
    assert set(_column5(_composed_single(fx, min_score=151)[0])) == {0}


def test_paired_sam_is_todays_file_with_column_five_replaced(fixture):
    fx = fixture
    for rescue, more in ((False, {}), (True, dict(DRM_PAIR_RESCUE="1"))):
        want, today, final, pm = _composed_paired(fx, rescue)
        _assert_spread(want, f"pairs, rescue {rescue}")
        name = "paired_rescue" if rescue else "paired"
        got = _paired(fx, name, DRM_SAM_MAPQ="1", **more)
        assert got == want
        assert _paired(fx, name + "_b3", DRM_SAM_MAPQ="1", DRM_SAM_BLOCK="3", **more) == want
        assert _paired(fx, name + "_60", **more) == today  # without DRM_SAM_MAPQ: the parent's file
        assert [x.split("\t")[:4] + x.split("\t")[5:] for x in got] == [x.split("\t")[:4] + x.split("\t")[5:] for x in today]
        status = [r["status"] for r, _ in final]
        if rescue:
            assert any(s in (5, 6) for s in status), status
            for p, s in enumerate(status):  # a rescued mate is never more certain than its anchor
                if s == 5:
                    assert int(pm["mapq2"][p]) <= int(pm["mapq1"][p])
                if s == 6:
                    assert int(pm["mapq1"][p]) <= int(pm["mapq2"][p])
        # pair 3: mate 1 lies in the duplicate, its mate in unique sequence lifts it from 0 to 40; pair 5 lies in the
        # duplicate with both mates and stays at 0
        assert (int(pm["q_se1"][3]), int(pm["mapq1"][3]), int(pm["q_pe"][3])) == (0, 40, 60)
        assert (int(pm["mapq1"][5]), int(pm["mapq2"][5]), int(pm["q_pe"][5])) == (0, 0, 0)


def test_bad_mapq_input_ends_before_the_index_is_loaded(fixture):
    fx = fixture
    m2 = str(fx["tmp"] / "m2.fastq")
    cases = [(dict(DRM_MAPQ_MIN="-1"), "DRM_MAPQ_MIN"), (dict(DRM_MAPQ_MIN="4x"), "DRM_MAPQ_MIN"),
             (dict(DRM_MAPQ_MIN=""), "DRM_MAPQ_MIN"), (dict(DRM_MAPQ_MIN="1048577"), "DRM_MAPQ_MIN"),
             (dict(DRM_MAPQ_SPAN="0"), "DRM_MAPQ_SPAN"), (dict(DRM_MAPQ_SPAN="1e2"), "DRM_MAPQ_SPAN"),
             (dict(DRM_MAPQ_SPAN="1048577"), "DRM_MAPQ_SPAN"), (dict(DRM_DEVICES="0,0"), "DRM_DEVICES"),
             (dict(DRM_SAM_L2_ROWS="1"), "DRM_SAM_L2_ROWS")]
    for x, (more, word) in enumerate(cases):
        for paired in (dict(), dict(DRM_MATES=m2))[:2 if x in (0, 4, 7) else 1]:
            r = fx["run"](fx["tmp"] / ("m1.fastq" if paired else "inter.fastq"), "bad", ["1", "1"], DRM_SAM_CIGAR="1",
                          DRM_SAM_MAPQ="1", **paired, **more)
            assert r.returncode == 1 and r.stderr.startswith("Error:") and word in r.stderr, (more, r.stdout, r.stderr)
            assert "Index loaded" not in r.stdout and not os.path.exists(fx["tmp"] / "bad" / "results.sam"), more
    # the bounds themselves are accepted
    r = fx["run"](fx["tmp"] / "inter.fastq", "edge", ["1", "1"], DRM_SAM_CIGAR="1", DRM_SAM_MAPQ="1",
                  DRM_MAPQ_MIN="1048576", DRM_MAPQ_SPAN="1048576")
    assert r.returncode == 0, r.stdout + r.stderr
    assert set(_column5(_sam(fx, "edge"))) == {0}


def test_without_the_switch_every_line_says_60(fixture):
    fx = fixture
    plain = _single(fx, "plain")
    assert set(_column5(plain)) == {60}
    # the MAPQ variables are read only with DRM_SAM_MAPQ=1, and DRM_SAM_MAPQ only in the streamed CIGAR mode
    assert _single(fx, "ignored", DRM_MAPQ_MIN="garbage", DRM_MAPQ_SPAN="-3") == plain
    assert _single(fx, "off", DRM_SAM_MAPQ="0", DRM_MAPQ_MIN="garbage") == plain
    outs = []
    for name, more in (("nocigar", {}), ("nocigar_mapq", dict(DRM_SAM_MAPQ="1", DRM_MAPQ_MIN="garbage"))):
        r = fx["run"](fx["tmp"] / "inter.fastq", name, ["1", "1"], **more)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(open(fx["tmp"] / name / "results.sam", "rb").read())
    assert outs[0] == outs[1] and set(_column5(outs[0].decode().split("\n")[:-1])) == {60}
