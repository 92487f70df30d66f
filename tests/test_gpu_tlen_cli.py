"""GPU tests of bin/pipeline's DRM_PAIR_TLEN=auto: 40 error-free pairs simulated from the C1 genome with template lengths
from a fixed list between 250 and 400, two pairs with a random mate, one RF pair and one same-strand pair. The printed
window, its mean, sd, sample count and class counts are the composition rerank rows -> tlen_scan -> tlen_estimate of the
package's wrappers, number for number; results.sam is byte for byte the file of the run with DRM_PAIR_TLEN=<printed
min>,<printed max>, with and without DRM_PAIR_RESCUE=1 and DRM_SAM_MAPQ=1 and whatever DRM_SAM_BLOCK; every simulated FR
template length lies in the window; too few samples fall back to 0,1000; bad input ends the run before the index is
loaded; without DRM_PAIR_TLEN the paired file is what it was."""
import os
import re
import subprocess

import numpy as np
import pytest

import sw_align_ref as R
from deepreadmapper_amd import tlen_estimate, tlen_scan
from test_gpu_pair_cli import _composed, _fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNA = os.path.join(ROOT, "tests", "golden", "ecoli_150.fna")
REF_LEN = 150
ENV = ("DRM_MATES", "DRM_PAIR_TLEN", "DRM_PAIR_TLEN_SAMPLE", "DRM_PAIR_TLEN_MAPQ", "DRM_PAIR_PENALTY", "DRM_PAIR_RESCUE",
       "DRM_PAIR_RESCUE_MIN", "DRM_SAM_CIGAR", "DRM_SAM_SCORING", "DRM_SAM_FLANK", "DRM_SAM_BLOCK", "DRM_DEVICES",
       "DRM_SAM_MAPQ", "DRM_MAPQ_MIN", "DRM_MAPQ_SPAN", "DRM_SAM_L2_ROWS")
TLENS = [250, 262, 275, 281, 290, 296, 300, 300, 304, 310, 315, 322, 330, 338, 345, 352, 361, 377, 388, 400]
_LINE = (r"^\[MAIN\] Template length \(auto\): min=(\d+) max=(\d+) mean=(\d+) sd=(\d+) from (\d+) of (\d+) "
         r"pairs; FR/RF/same/far = (\d+)/(\d+)/(\d+)/(\d+)")
LINE = re.compile(_LINE + "$", re.M)
CUT = re.compile(_LINE + r" \(max cut from (\d+) to the mate rescue's 2048-row cap\)$", re.M)
FALLBACK = re.compile(r"^\[MAIN\] Template length \(auto\): (\d+) FR pairs among (\d+) sampled, fewer than 10: falling "
                      r"back to min=0 max=1000; FR/RF/same/far = (\d+)/(\d+)/(\d+)/(\d+)$", re.M)


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    """The C1 index, the two mate files, their interleaved file, and the unpaired run's rerank output."""
    from deepreadmapper_amd import extract_fasta_sequence
    tmp = tmp_path_factory.mktemp("tlen_cli")
    env = dict(os.environ, DRM_BUILD_THREADS="1")
    for v in ENV:
        env.pop(v, None)
    r = subprocess.run([os.path.join(ROOT, "bin", "hnswpq_index"), FNA, "c1", "150"], cwd=tmp, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = extract_fasta_sequence(FNA)
    rng = np.random.default_rng(77)
    rand = lambda: bytes(rng.choice(list(b"ACGT"), size=REF_LEN).astype(np.uint8))  # noqa: E731
    m1, m2, truth = [], [], []
    for x, t in enumerate(TLENS + TLENS[::-1]):
        p = (x * 53) % (len(g) - t + 1)
        a, b = g[p:p + REF_LEN], R.revcomp(g[p + t - REF_LEN:p + t])
        wa, wb = 2 * p, 2 * (p + t - REF_LEN) + 1
        if x % 3 == 2:  # mate 1 is the reverse read
            a, b, wa, wb = b, a, wb, wa
        m1.append(a)
        m2.append(b)
        truth.append((wa, wb, 1, t))
    m1 += [g[500:650], rand()]                                    # a random mate
    m2 += [rand(), R.revcomp(g[320:470])]
    m1 += [R.revcomp(g[100:250]), g[600:750]]                      # RF at 150 + 300; same strand at 150 + 380
    m2 += [g[400:550], g[220:370]]
    truth += [None, None, (2 * 100 + 1, 2 * 400, 2, 450), (2 * 600, 2 * 220, 3, 530)]
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


def _paired(fx, name, **more):
    """(stdout, results.sam's bytes) of a paired run."""
    r = fx["run"](fx["tmp"] / "m1.fastq", name, ["1", "1"], DRM_MATES=str(fx["tmp"] / "m2.fastq"), DRM_SAM_CIGAR="1",
                  **more)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout, open(fx["tmp"] / name / "results.sam", "rb").read()


def _composed_window(fx, npairs=None, **prm):
    """rerank rows -> tlen_scan -> tlen_estimate over the first npairs pairs: (estimate, class counts 0..4)."""
    sc = fx["sc"]
    cnt = (sc >= 0).sum(axis=1).astype(np.int32)  # rows past a query's status are written as -1
    ids, sc = fx["ids"], np.maximum(sc, 0)
    full = np.array([len(r) for r in fx["reads"]], np.int32)
    m = 2 * (len(fx["names"]) if npairs is None else npairs)
    samples, hist = tlen_scan(ids[:m], sc[:m], cnt[:m], ids[1:m], sc[1:m], cnt[1:m], full[:m], full[1:m], REF_LEN,
                              row_step=2, **prm)
    assert hist.shape == (3, 10001)
    return tlen_estimate(hist[0]), np.bincount(samples["cls"], minlength=5).tolist(), samples


def _assert_line(out, e, classes, sampled):
    """The one line the run printed says what the composition says, number for number; returns (min, max)."""
    got, fell = LINE.findall(out), FALLBACK.findall(out)
    assert len(got) + len(fell) == 1, out
    if e["status"] == 1:
        assert len(fell) == 1 and tuple(int(x) for x in fell[0]) == (classes[1], sampled) + tuple(classes[1:]), out
        return 0, 1000
    assert len(got) == 1, out
    assert tuple(int(x) for x in got[0]) == (e["low"], e["high"], e["mean"], e["sd"], e["n"], sampled) + tuple(classes[1:])
    return int(got[0][0]), int(got[0][1])


def test_printed_window_is_the_composition_and_holds_every_simulated_length(fixture):
    fx = fixture
    n = len(fx["names"])
    e, classes, samples = _composed_window(fx)
    out, _ = _paired(fx, "auto", DRM_PAIR_TLEN="auto")
    assert e["status"] == 0 and e["n"] == classes[1]
    lo, hi = _assert_line(out, e, classes, n)
    # every simulated FR template length lies in the window
    assert all(lo <= t[3] <= hi for t in fx["truth"] if t and t[2] == 1), (lo, hi)
    assert 250 <= e["p25"] <= e["p50"] <= e["p75"] <= 400 and hi < 1000
    # the reads are error-free and the index is at stride 1: a pair whose two true windows are among its reads' hits
    # is sampled with its true class and template length; a random mate is no sample
    found = 0
    for p, t in enumerate(fx["truth"]):
        if t is None:
            assert int(samples["cls"][p]) == 0, p
        elif t[0] in fx["ids"][2 * p].tolist() and t[1] in fx["ids"][2 * p + 1].tolist():
            found += 1
            assert (int(samples["cls"][p]), int(samples["tlen"][p])) == t[2:], (p, samples[p], t)
    assert found >= 20, "few simulated pairs have both true windows in their hit lists: the fixture is wrong"
    # the sample limit takes the first pairs; the thresholds and the MAPQ parameters reach the kernel: a threshold of 0
    # samples the random mates too, a chance level above every score samples nothing
    for more, prm, npairs in ((dict(DRM_PAIR_TLEN_SAMPLE="20"), {}, 20),
                              (dict(DRM_PAIR_TLEN_MAPQ="0", DRM_MAPQ_SPAN="1"), dict(min_mapq=0, locus_span=1), None),
                              (dict(DRM_PAIR_TLEN_MAPQ="1", DRM_MAPQ_MIN="151"), dict(min_mapq=1, min_score=151), None)):
        e2, classes2, _ = _composed_window(fx, npairs, **prm)
        out, _ = _paired(fx, "auto_prm", DRM_PAIR_TLEN="auto", **more)
        _assert_line(out, e2, classes2, n if npairs is None else npairs)
        assert classes2 != classes, more
    assert e2["status"] == 1 and classes2[1:] == [0, 0, 0, 0]


@pytest.mark.parametrize("more", [dict(), dict(DRM_PAIR_RESCUE="1"), dict(DRM_SAM_MAPQ="1"),
                                  dict(DRM_PAIR_RESCUE="1", DRM_SAM_MAPQ="1")], ids=["plain", "rescue", "mapq", "both"])
def test_sam_equals_the_run_with_the_printed_window(fixture, more):
    fx = fixture
    x = "".join(sorted(more))
    out, auto = _paired(fx, f"auto{x}", DRM_PAIR_TLEN="auto", DRM_SAM_BLOCK="3", **more)
    got = LINE.findall(out)
    assert len(got) == 1, out
    window = f"{got[0][0]},{got[0][1]}"
    out, fixed = _paired(fx, f"fixed{x}", DRM_PAIR_TLEN=window, **more)
    assert "Template length" not in out
    assert auto == fixed, (more, window)
    assert _paired(fx, f"auto{x}_b7", DRM_PAIR_TLEN="auto", DRM_SAM_BLOCK="7", **more)[1] == fixed
    assert fixed.count(b"\n") == 2 + 2 * len(fx["names"])
    if not more:  # the window matters to the file: one below every simulated length pairs nothing
        assert _paired(fx, "narrow", DRM_PAIR_TLEN="0,200")[1] != fixed


def test_too_few_samples_fall_back_to_the_default_window(fixture):
    fx = fixture
    _, default = _paired(fx, "default")
    out, sam = _paired(fx, "few", DRM_PAIR_TLEN="auto", DRM_PAIR_TLEN_SAMPLE="4")
    got = FALLBACK.findall(out)
    assert len(got) == 1 and not LINE.findall(out), out
    e, classes, _ = _composed_window(fx, 4)
    assert e["status"] == 1 and tuple(int(x) for x in got[0]) == (classes[1], 4) + tuple(classes[1:])
    assert sam == default
    out, sam = _paired(fx, "few_rescue", DRM_PAIR_TLEN="auto", DRM_PAIR_TLEN_SAMPLE="9", DRM_PAIR_RESCUE="1")
    assert len(FALLBACK.findall(out)) == 1
    assert sam == _paired(fx, "default_rescue", DRM_PAIR_RESCUE="1")[1]


def test_bad_input_ends_before_the_index_is_loaded(fixture):
    fx = fixture
    m2 = str(fx["tmp"] / "m2.fastq")
    auto = dict(DRM_MATES=m2, DRM_PAIR_TLEN="auto")
    cases = [(dict(DRM_PAIR_TLEN="auto"), "DRM_MATES")]
    cases += [(dict(auto, DRM_PAIR_TLEN_SAMPLE=v), "DRM_PAIR_TLEN_SAMPLE") for v in ("0", "", "abc", "-4", "1e3", "16777217")]
    cases += [(dict(auto, DRM_PAIR_TLEN_MAPQ=v), "DRM_PAIR_TLEN_MAPQ") for v in ("61", "", "x", "-1", "2.5")]
    cases += [(dict(auto, DRM_MAPQ_MIN="4x"), "DRM_MAPQ_MIN"), (dict(auto, DRM_MAPQ_SPAN="0"), "DRM_MAPQ_SPAN"),
              (dict(DRM_MATES=m2, DRM_PAIR_TLEN="Auto"), "DRM_PAIR_TLEN"), (dict(DRM_MATES=m2, DRM_PAIR_TLEN="auto,"), "DRM_PAIR_TLEN")]
    for more, word in cases:
        r = fx["run"](fx["tmp"] / "m1.fastq", "bad", ["1", "1"], DRM_SAM_CIGAR="1", **more)
        assert r.returncode == 1 and r.stderr.startswith("Error:") and word in r.stderr, (more, r.stdout, r.stderr)
        assert "Index loaded" not in r.stdout and not os.path.exists(fx["tmp"] / "bad" / "results.sam"), more
    # the bounds themselves are accepted, and the variables are read only under auto
    out, _ = _paired(fx, "edge", DRM_PAIR_TLEN="auto", DRM_PAIR_TLEN_SAMPLE="16777216", DRM_PAIR_TLEN_MAPQ="60")
    assert len(LINE.findall(out)) == 1
    _paired(fx, "ignored", DRM_PAIR_TLEN="0,1000", DRM_PAIR_TLEN_SAMPLE="garbage", DRM_PAIR_TLEN_MAPQ="-1")


def test_without_the_variable_the_paired_file_is_what_it_was(fixture):
    fx = fixture
    want, res = _composed(fx)
    out, sam = _paired(fx, "unset")
    assert "Template length" not in out
    assert sam.decode().split("\n")[:-1] == want
    assert _paired(fx, "unset_vars", DRM_PAIR_TLEN_SAMPLE="garbage", DRM_PAIR_TLEN_MAPQ="99")[1] == sam
    assert (res["status"] == 0).sum() >= 30


def test_rescue_cuts_a_window_wider_than_its_row_cap(tmp_path):
    """A library spread over 300 to 2,600 bases on a random 4,000-base genome: the estimated maximum lies beyond what
    drm_mate_rescue's 2,048 rows admit. Without the rescue it is printed as estimated; with it, it is cut to
    max(0, min - ref_len) + 2048, the line says so, and the file is that of the run with the cut window."""
    from deepreadmapper_amd import extract_fasta_sequence
    env = dict(os.environ, DRM_BUILD_THREADS="1")
    for v in ENV:
        env.pop(v, None)
    rng = np.random.default_rng(4000)
    g = bytes(rng.choice(list(b"ACGT"), size=4000).astype(np.uint8))
    fna = tmp_path / "wide.fna"
    with open(fna, "wb") as f:
        f.write(b"> random 4,000 bases\n" + b"\n".join(g[i:i + 80] for i in range(0, len(g), 80)) + b"\n")
    assert extract_fasta_sequence(str(fna)) == g
    r = subprocess.run([os.path.join(ROOT, "bin", "hnswpq_index"), str(fna), "wide", "150"], cwd=tmp_path, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tlens = [300, 450, 600, 800, 1000, 1200, 1400, 1600, 1800, 2000, 2200, 2400, 2600, 700, 1500, 2300]
    m1, m2 = [], []
    for x, t in enumerate(tlens):
        p = (x * 97) % (len(g) - t + 1)
        m1.append(g[p:p + REF_LEN])
        m2.append(R.revcomp(g[p + t - REF_LEN:p + t]))
    names = [f"pair{i}" for i in range(len(m1))]
    _fastq(tmp_path / "m1.fastq", [n + "/1" for n in names], m1)
    _fastq(tmp_path / "m2.fastq", [n + "/2" for n in names], m2)
    inter = [x for ab in zip(m1, m2) for x in ab]
    _fastq(tmp_path / "inter.fastq", [n for n in names for _ in range(2)], inter)

    def run(query, name, extra, **more):
        return subprocess.run([os.path.join(ROOT, "bin", "pipeline"), "wide", str(query), str(fna), "128", "4", "4", name]
                              + extra, cwd=tmp_path, env=dict(env, **more), capture_output=True, text=True)
    r = run(tmp_path / "inter.fastq", "unpaired", ["1", "0"])
    assert r.returncode == 0, r.stdout + r.stderr
    fx = dict(tmp=tmp_path, run=run, names=names, reads=inter, ids=np.load(tmp_path / "unpaired" / "sw_ids.npy"),
              sc=np.load(tmp_path / "unpaired" / "sw_scores.npy"))
    e, classes, _ = _composed_window(fx)
    widest = max(0, e["low"] - REF_LEN) + 2048
    assert e["status"] == 0 and e["high"] > widest, (e, "the fixture's library is not wide enough")
    out, _ = _paired(fx, "auto", DRM_PAIR_TLEN="auto")
    assert _assert_line(out, e, classes, len(names)) == (e["low"], e["high"]) and not CUT.findall(out)
    out, auto = _paired(fx, "auto_rescue", DRM_PAIR_TLEN="auto", DRM_PAIR_RESCUE="1")
    got = CUT.findall(out)
    assert len(got) == 1 and not LINE.findall(out), out
    assert tuple(int(x) for x in got[0]) == (e["low"], widest, e["mean"], e["sd"], e["n"], len(names)) + \
        tuple(classes[1:]) + (e["high"],)
    assert _paired(fx, "fixed_rescue", DRM_PAIR_TLEN=f"{e['low']},{widest}", DRM_PAIR_RESCUE="1")[1] == auto
    # one base wider is what the rescue refuses
    r = run(tmp_path / "m1.fastq", "bad", ["1", "1"], DRM_MATES=str(tmp_path / "m2.fastq"), DRM_SAM_CIGAR="1",
            DRM_PAIR_RESCUE="1", DRM_PAIR_TLEN=f"{e['low']},{widest + 1}")
    assert r.returncode == 1 and "Index loaded" not in r.stdout, r.stdout + r.stderr
