"""GPU tests of bin/pipeline's mate rescue (DRM_MATES with DRM_PAIR_RESCUE=1): pairs simulated from the C1 genome, some
with a mate so full of substitutions that the search loses its true window, come out as the composition of the
package's wrappers (pair_hits, mate_rescue, pair_rescue_choose, the aligners, sam_pair_fields) byte for byte; a
rescued pair carries the proper-pair flag and its template length; the file does not depend on DRM_SAM_BLOCK; without
DRM_PAIR_RESCUE the paired file is what it was; bad input ends the run before the index is loaded."""
import os
import subprocess

import numpy as np
import pytest

import sw_align_ref as R
from deepreadmapper_amd import mate_rescue, pair_rescue_choose  # noqa: F401  (what this file is about)
from test_gpu_mate_rescue import compose_wrappers
from test_gpu_pair_cli import _fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FNA = os.path.join(GOLDEN, "ecoli_150.fna")
REF_LEN = 150
STRIDE = 1  # of the C1 index: window ids are genome positions
RESCUE_MIN = 49  # bin/pipeline's default DRM_PAIR_RESCUE_MIN
ENV = ("DRM_MATES", "DRM_PAIR_TLEN", "DRM_PAIR_PENALTY", "DRM_PAIR_RESCUE", "DRM_PAIR_RESCUE_MIN", "DRM_SAM_CIGAR",
       "DRM_SAM_SCORING", "DRM_SAM_FLANK", "DRM_SAM_BLOCK", "DRM_DEVICES")
# (fragment start, template length, which mate carries the substitutions (None: neither), their period)
FRAGMENTS = [(10, 200, None, 0), (95, 330, None, 0), (222, 500, None, 0),
             (40, 260, 2, 3), (150, 410, 2, 3), (301, 290, 2, 4), (433, 377, 2, 3), (520, 300, 2, 4),
             (60, 240, 1, 3), (180, 450, 1, 3), (350, 310, 1, 4), (610, 350, 1, 3)]


def mutate(read, period):
    """Every period-th base of the read's inner 130 replaced: no 3-mer of that stretch survives at period 3, so the
    embedding search loses the window, while 10 clean bases at either end keep a local alignment from clipping."""
    nxt = dict(zip(b"ACGT", b"CGTA"))
    s = bytearray(read)
    for i in range(10, len(s) - 10, period):
        s[i] = nxt[s[i]]
    return bytes(s)


def simulate(g):
    """(mate 1 reads, mate 2 reads, truth): truth[p] = (true window of mate 1, of mate 2, template length) for the
    simulated fragments; four more pairs follow them (mate 2 random; both random; mate 2 / both all N)."""
    rng = np.random.default_rng(42)
    rand = lambda: bytes(rng.choice(list(b"ACGT"), size=REF_LEN).astype(np.uint8))  # noqa: E731
    m1, m2, truth = [], [], []
    for p, t, bad, period in FRAGMENTS:
        assert p + t <= len(g)
        a, b = g[p:p + REF_LEN], R.revcomp(g[p + t - REF_LEN:p + t])
        if bad == 1:
            a = mutate(a, period)
        if bad == 2:
            b = mutate(b, period)
        m1.append(a)
        m2.append(b)
        truth.append((2 * p, 2 * (p + t - REF_LEN) + 1, t))
    m1 += [g[500:650], rand(), g[700:850], b"N" * REF_LEN]
    m2 += [rand(), rand(), b"N" * REF_LEN, b"N" * REF_LEN]
    return m1, m2, truth


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    """The C1 index, the two mate files, their interleaved file, and the unpaired run's rerank output."""
    from deepreadmapper_amd import extract_fasta_sequence
    tmp = tmp_path_factory.mktemp("rescue_cli")
    env = dict(os.environ, DRM_BUILD_THREADS="1")
    for v in ENV:
        env.pop(v, None)
    r = subprocess.run([os.path.join(ROOT, "bin", "hnswpq_index"), FNA, "c1", "150"], cwd=tmp, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = extract_fasta_sequence(FNA)
    m1, m2, truth = simulate(g)
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


def _composed(fx, rescue, affine=None, min_score=RESCUE_MIN, **pair):
    """The expected SAM lines and the pairs' final records, from the unpaired run's rows and the package's wrappers."""
    from deepreadmapper_amd import (GenomeTable, pair_hits, sam_cigar, sam_cigar_region, sam_pair_fields,
                                    sw_align_affine_arrays, sw_align_arrays, sw_align_region)
    ids, sc, reads = fx["ids"], fx["sc"], fx["reads"]
    cnt = (sc >= 0).sum(axis=1).astype(np.int32)  # rows past a query's status are written as -1
    sc = np.maximum(sc, 0)
    res = pair_hits(ids, sc, cnt, ids[1:], sc[1:], cnt[1:], REF_LEN, row_step=2, **pair)
    queries = [b"<" + r + b">" for r in reads]
    t = GenomeTable(np.frombuffer(fx["g"], dtype=np.uint8), REF_LEN)
    prm = dict(ref_len=REF_LEN, min_tlen=pair.get("min_tlen", 0), max_tlen=pair.get("max_tlen", 1000),
               unpaired_penalty=pair.get("unpaired_penalty", 17))
    if rescue:
        final = compose_wrappers(t, len(fx["g"]), res, ids, sc, queries, prm, min_score)
    else:
        final = [({f: int(res[f][p]) for f in res.dtype.names}, 0) for p in range(len(res))]
    chosen = {}
    for p, (rec, wr) in enumerate(final):
        for m, j in enumerate((rec["j1"], rec["j2"])):
            if j >= 0:
                chosen[2 * p + m] = int(ids[2 * p + m, j])
        if rec["status"] in (5, 6):
            chosen[2 * p + (1 if rec["status"] == 5 else 0)] = wr
    rows = sorted(chosen)
    wid = np.array([chosen[r] for r in rows], dtype=np.uint64)
    if affine:
        scoring, flank = affine
        rec, ops = sw_align_affine_arrays(t, wid, np.array(rows), queries, scoring, flank=flank)
    else:
        rec, ops = sw_align_arrays(t, wid, np.array(rows), queries)
    want = ["@HD\tVN:1.0\tSO:unsorted", "@SQ\tSN:ref\tLN:150"]
    for p, (pr, _) in enumerate(final):
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
        f = sam_pair_fields(mates[0], mates[1], pr["status"] in (0, 5, 6))
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
    return want, final


def _sam(fx, name):
    got = open(fx["tmp"] / name / "results.sam").read().split("\n")
    assert got[-1] == ""
    return got[:-1]


def _paired(fx, name, **more):
    r = fx["run"](fx["tmp"] / "m1.fastq", name, ["1", "1"], DRM_MATES=str(fx["tmp"] / "m2.fastq"), DRM_SAM_CIGAR="1",
                  **more)
    assert r.returncode == 0, r.stdout + r.stderr
    return _sam(fx, name)


def test_rescued_sam_equals_the_composition(fixture):
    fx = fixture
    # the guard of this file: at least one simulated pair's mutated mate has its true window missing from the unpaired
    # run's rerank output, so that a rescue below is not a pair the search had found anyway
    lost = [p for p, (_, _, bad, _) in enumerate(FRAGMENTS)
            if bad and fx["truth"][p][bad - 1] not in fx["ids"][2 * p + bad - 1].tolist()]
    assert len(lost) >= 1, "every mutated mate's true window is among its hits: the fixture exercises no rescue"
    want, final = _composed(fx, True)
    got = _paired(fx, "rescue", DRM_PAIR_RESCUE="1")
    assert got == want
    assert len(got) == 2 + 2 * len(fx["names"])
    assert _paired(fx, "rescue_b3", DRM_PAIR_RESCUE="1", DRM_SAM_BLOCK="3") == want  # six blocks of pairs
    assert _paired(fx, "rescue_b1", DRM_PAIR_RESCUE="1", DRM_SAM_BLOCK="1") == want
    assert _paired(fx, "rescue_min", DRM_PAIR_RESCUE="1", DRM_PAIR_RESCUE_MIN=str(RESCUE_MIN)) == want  # the default
    status = [r["status"] for r, _ in final]
    rescued = [p for p, s in enumerate(status) if s in (5, 6)]
    assert len(rescued) >= 1 and 0 in status and any(s in (1, 2, 3) for s in status), status
    seen = 0
    for p in rescued:
        if p >= len(FRAGMENTS):
            continue
        _, _, bad, _ = FRAGMENTS[p]
        wa, wb, t = fx["truth"][p]
        # a rescue of the mutated mate whose true window the search had lost
        if not bad or status[p] != (5 if bad == 2 else 6) or (wa, wb)[bad - 1] in fx["ids"][2 * p + bad - 1].tolist():
            continue
        seen += 1
        a, b = got[2 + 2 * p].split("\t"), got[3 + 2 * p].split("\t")
        for m, f in enumerate((a, b)):
            assert int(f[1]) & 0x2 and int(f[1]) & 0x1 and f[6] == "=" and int(f[1]) & (0x40 if m == 0 else 0x80), (p, f)
            assert abs(abs(int(f[8])) - t) <= STRIDE, (p, f, t)
        assert int(a[8]) == -int(b[8]) and a[3] == b[7] and a[7] == b[3]
        assert abs(int(a[3]) - 1 - wa // 2) <= STRIDE and abs(int(b[3]) - 1 - wb // 2) <= STRIDE, (p, a[3], b[3])
    assert seen >= 1, "no lost mate was rescued at its true position"
    # a stricter minimum rescues nothing: the file without DRM_PAIR_RESCUE
    plain, _ = _composed(fx, False)
    assert _paired(fx, "rescue_never", DRM_PAIR_RESCUE="1", DRM_PAIR_RESCUE_MIN="1000") == plain
    assert plain != want


def test_rescue_honours_the_alignment_mode_and_the_pair_parameters(fixture):
    fx = fixture
    want, final = _composed(fx, True, affine=((1, 4, 6, 1), 8))
    assert any(r["status"] in (5, 6) for r, _ in final)
    got = _paired(fx, "rescue_affine", DRM_PAIR_RESCUE="1", DRM_SAM_SCORING="1,4,6,1", DRM_SAM_FLANK="8",
                  DRM_SAM_BLOCK="5")
    assert got == want
    want, final = _composed(fx, True, min_score=70, min_tlen=200, max_tlen=420, unpaired_penalty=5)
    got = _paired(fx, "rescue_prm", DRM_PAIR_RESCUE="1", DRM_PAIR_RESCUE_MIN="70", DRM_PAIR_TLEN="200,420",
                  DRM_PAIR_PENALTY="5")
    assert got == want


def test_without_rescue_the_paired_file_is_unchanged(fixture):
    fx = fixture
    want, _ = _composed(fx, False)
    assert _paired(fx, "norescue") == want
    assert _paired(fx, "rescue_0", DRM_PAIR_RESCUE="0") == want
    # DRM_PAIR_RESCUE_MIN is read only with DRM_PAIR_RESCUE=1, and a window beyond the cap matters only then
    assert _paired(fx, "min_alone", DRM_PAIR_RESCUE_MIN="garbage") == want
    wide, _ = _composed(fx, False, min_tlen=0, max_tlen=3000)
    assert _paired(fx, "wide", DRM_PAIR_TLEN="0,3000") == wide
    # without DRM_MATES neither variable is read
    r = fx["run"](fx["tmp"] / "m1.fastq", "plain", ["1", "1"], DRM_SAM_CIGAR="1")
    assert r.returncode == 0, r.stdout + r.stderr
    r = fx["run"](fx["tmp"] / "m1.fastq", "ignored", ["1", "1"], DRM_SAM_CIGAR="1", DRM_PAIR_RESCUE="1",
                  DRM_PAIR_RESCUE_MIN="x", DRM_PAIR_TLEN="0,3000")
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(fx["tmp"] / "ignored" / "results.sam", "rb").read() == open(fx["tmp"] / "plain" / "results.sam", "rb").read()


def test_bad_rescue_input_ends_before_the_index_is_loaded(fixture):
    fx = fixture
    m2 = str(fx["tmp"] / "m2.fastq")
    cases = [(dict(DRM_PAIR_RESCUE_MIN="-1"), "DRM_PAIR_RESCUE_MIN"), (dict(DRM_PAIR_RESCUE_MIN="4x"), "DRM_PAIR_RESCUE_MIN"),
             (dict(DRM_PAIR_RESCUE_MIN=""), "DRM_PAIR_RESCUE_MIN"), (dict(DRM_PAIR_RESCUE_MIN="1048577"), "DRM_PAIR_RESCUE_MIN"),
             (dict(DRM_PAIR_RESCUE_MIN="1e3"), "DRM_PAIR_RESCUE_MIN"), (dict(DRM_PAIR_TLEN="0,2049"), "2048"),
             (dict(DRM_PAIR_TLEN="400,2299"), "2048")]
    for more, word in cases:
        r = fx["run"](fx["tmp"] / "m1.fastq", "bad", ["1", "1"], DRM_MATES=m2, DRM_SAM_CIGAR="1", DRM_PAIR_RESCUE="1",
                      **more)
        assert r.returncode == 1 and r.stderr.startswith("Error:") and word in r.stderr, (more, r.stdout, r.stderr)
        assert "Index loaded" not in r.stdout and not os.path.exists(fx["tmp"] / "bad" / "results.sam"), more
    # the cap itself and the largest minimum are accepted
    r = fx["run"](fx["tmp"] / "m1.fastq", "edge", ["1", "1"], DRM_MATES=m2, DRM_SAM_CIGAR="1", DRM_PAIR_RESCUE="1",
                  DRM_PAIR_TLEN="0,2048", DRM_PAIR_RESCUE_MIN="1048576")
    assert r.returncode == 0, r.stdout + r.stderr
