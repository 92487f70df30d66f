"""GPU tests of DRM_SAM_MD=1 and DRM_SAM_QUAL=1 through bin/pipeline: small FASTA and FASTQ fixtures are indexed by
bin/hnswpq_index and mapped single and paired, with the linear and the affine alignment, with and without DRM_CONTIGS
and with DRM_PAIR_RESCUE=1. Every mapped line's SEQ, CIGAR and MD rebuild the FASTA's bytes at RNAME:POS
(tests/md_ref.py, rebuild_reference), CIGAR and MD count to NM, unmapped lines carry no MD, and the file equals the run
without the switch once the MD tags are cut out, whatever DRM_SAM_BLOCK says. Column 11 is the FASTQ's quality line,
reversed under flag 16."""
import os
import re
import subprocess

import numpy as np
import pytest

import md_ref as MD
import sw_align_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LEN = 150
K = 8  # rows per read
DROP = ("DRM_CONTIGS", "DRM_MATES", "DRM_PAIR_TLEN", "DRM_PAIR_PENALTY", "DRM_PAIR_RESCUE", "DRM_SAM_CIGAR",
        "DRM_SAM_SCORING", "DRM_SAM_FLANK", "DRM_SAM_BLOCK", "DRM_SAM_MAPQ", "DRM_SAM_L2_ROWS", "DRM_DEVICES", "DRM_MAPQ_SPAN",
        "DRM_MAPQ_MIN", "DRM_PAIR_RESCUE_MIN", "DRM_PAIR_TLEN_SAMPLE", "DRM_PAIR_TLEN_MAPQ", "DRM_SAM_MD", "DRM_SAM_QUAL")
AFFINE = dict(DRM_SAM_FLANK="16", DRM_SAM_SCORING="1,4,6,1")
OTHER = {ord("A"): ord("C"), ord("C"): ord("G"), ord("G"): ord("T"), ord("T"): ord("A")}


def _qual(i, n):
    """A quality line that differs at every position from its neighbours and from its own reverse."""
    return bytes(33 + (7 * x + 3 * i) % 90 for x in range(n))


def _fastq(path, names, reads, quals=None):
    with open(path, "wb") as f:
        for i, (n, r) in enumerate(zip(names, reads)):
            f.write(b"@" + n.encode() + b"\n" + r + b"\n+\n" + (quals[i] if quals else _qual(i, len(r))) + b"\n")


def _sam(path):
    got = open(path).read().split("\n")
    assert got[-1] == ""
    return got[:-1]


def _substituted(seq, cols):
    s = bytearray(seq)
    for c in cols:
        s[c] = OTHER[s[c]]
    return bytes(s)


def _with_indels(g, at):
    """150 bases from g[at:]: a 3-base deletion after 70 bases and a 2-base insertion 50 bases later."""
    ins = bytes(OTHER[x] for x in g[at + 123:at + 125])  # differs from the bases it is put in front of
    read = g[at:at + 70] + g[at + 73:at + 123] + ins + g[at + 123:at + 151]
    assert len(read) == REF_LEN
    return read


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    from deepreadmapper_amd import extract_fasta_sequence, fasta_contigs
    tmp = tmp_path_factory.mktemp("md_cli")
    env = dict(os.environ, DRM_BUILD_THREADS="1")
    for v in DROP:
        env.pop(v, None)
    rng = np.random.default_rng(404)
    rand = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))  # noqa: E731
    a, b = rand(1000), rand(600)
    one, two = tmp / "one.fa", tmp / "two.fa"
    one.write_bytes(b">one\n" + a[:480] + b"\n" + a[480:] + b"\n")
    two.write_bytes(b">chrA\n" + a + b"\n>chrB\n" + b + b"\n")
    names, starts, lens = fasta_contigs(str(two))
    assert names == ["chrA", "chrB"] and extract_fasta_sequence(str(one)) == a

    def tool(*args, **more):
        return subprocess.run([os.path.join(ROOT, "bin", args[0]), *map(str, args[1:])], cwd=tmp, env=dict(env, **more),
                              capture_output=True, text=True)
    for ref, name, more in ((one, "ix1", {}), (two, "ix2", dict(DRM_CONTIGS="1"))):
        r = tool("hnswpq_index", ref, name, REF_LEN, **more)
        assert r.returncode == 0, r.stderr

    def run(contigs, query, name, **more):
        if contigs:
            more = dict(more, DRM_CONTIGS="1")
        return tool("pipeline", "ix2" if contigs else "ix1", query, two if contigs else one, 128, K, K, name, 1, 1, **more)
    # single reads: exact copies, substitutions (two of them adjacent, one in the first and one in the last column), ten
    # substitutions (more MD words than the first pass keeps), a 3-base deletion with a 2-base insertion, the same on the
    # reverse strand, a random read and one of N
    reads = [a[100:250], a[700:850], _substituted(a[300:450], [0, 40, 41, 100, 149]),
             _substituted(a[420:570], range(6, 150, 13)), _with_indels(a, 500), R.revcomp(a[600:750]),
             R.revcomp(_substituted(a[200:350], [10, 77])), R.revcomp(_with_indels(a, 30)), rand(REF_LEN), b"N" * REF_LEN]
    _fastq(tmp / "reads.fastq", [f"read{i}" for i in range(len(reads))], reads)
    # pairs (FR): mate 2 with ten substitutions, mate 2 with three, mate 1 with the indels, a mate 2 that only the
    # rescue finds (a third of its bases changed), mate 2 random, both N
    frags = [(50, 400), (300, 380), (520, 420), (610, 350)]
    m1 = [a[p:p + REF_LEN] for p, t in frags] + [a[20:170], b"N" * REF_LEN]
    m2 = [R.revcomp(a[p + t - REF_LEN:p + t]) for p, t in frags] + [rand(REF_LEN), b"N" * REF_LEN]
    m2[0] = R.revcomp(_substituted(R.revcomp(m2[0]), range(6, REF_LEN, 13)))  # more MD words than the first pass keeps
    m2[1] = R.revcomp(_substituted(R.revcomp(m2[1]), [3, 4, 90]))
    m1[2] = _with_indels(a, 520)
    m2[3] = _substituted(m2[3], range(0, REF_LEN, 3))
    pnames = [f"pair{i}" for i in range(len(m1))]
    _fastq(tmp / "m1.fastq", [n + "/1" for n in pnames], m1)
    _fastq(tmp / "m2.fastq", [n + "/2" for n in pnames], m2, [_qual(100 + i, REF_LEN) for i in range(len(m2))])
    return dict(tmp=tmp, run=run, refs={"ref": a, "chrA": a, "chrB": b}, reads=reads, m1=m1, m2=m2, pnames=pnames,
                rand=rand)


def _check_lines(fx, lines):
    """Every mapped line's SEQ, CIGAR and MD against the reference and NM; returns what the file was seen to hold."""
    seen = set()
    for line in lines:
        if line.startswith("@"):
            continue
        f = line.split("\t")
        flag, rname, pos, cigar, seq = int(f[1]), f[2], int(f[3]), f[5], f[9]
        tags = dict((t[:2], t[5:]) for t in f[11:])
        if flag & 4:
            assert "MD" not in tags and "MD:Z" not in line and cigar == "*"
            seen.add("unmapped")
            continue
        md = tags["MD"]
        ref = MD.rebuild_reference(seq, cigar, md)
        assert ref == fx["refs"][rname][pos - 1:pos - 1 + len(ref)], line
        assert MD.nm_from_cigar_md(cigar, md) == int(tags["NM"]), line
        assert list(tags) == ["AS", "NM", "MD"]
        seen |= {"reverse" if flag & 16 else "forward", "D" in cigar and "deletion", "I" in cigar and "insertion",
                 bool(re.search(r"[A-Z]0[A-Z]", md)) and "adjacent", md.isdigit() and "exact",
                 len(re.findall(r"[A-Z^]", md)) > 8 and "long", rname}
    return seen


CONFIGS = {
    "single-linear": dict(contigs=False, paired=False, more={}),
    "single-affine-contigs": dict(contigs=True, paired=False, more=AFFINE),
    "paired-linear-contigs-rescue": dict(contigs=True, paired=True, more=dict(DRM_PAIR_RESCUE="1")),
    "paired-affine-rescue": dict(contigs=False, paired=True, more=dict(AFFINE, DRM_PAIR_RESCUE="1")),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_md_on_every_mapped_line(fixture, name):
    fx, cfg = fixture, CONFIGS[name]
    tmp = fx["tmp"]
    more = dict(cfg["more"], DRM_SAM_CIGAR="1")
    query = tmp / "reads.fastq"
    if cfg["paired"]:
        more["DRM_MATES"] = str(tmp / "m2.fastq")
        query = tmp / "m1.fastq"
    out = {}
    for tag, extra in (("md", dict(DRM_SAM_MD="1")), ("plain", {}), ("md_b3", dict(DRM_SAM_MD="1", DRM_SAM_BLOCK="3"))):
        r = fx["run"](cfg["contigs"], query, f"{name}-{tag}", **more, **extra)
        assert r.returncode == 0, r.stdout + r.stderr
        out[tag] = open(tmp / f"{name}-{tag}" / "results.sam").read()
    assert "MD:Z" not in out["plain"]
    assert re.sub(r"\tMD:Z:[^\t\n]*", "", out["md"]) == out["plain"]
    assert out["md_b3"] == out["md"]
    seen = _check_lines(fx, _sam(tmp / f"{name}-md" / "results.sam"))
    want = {"forward", "reverse", "unmapped", "deletion", "insertion", "exact", "long", "chrA" if cfg["contigs"] else "ref"}
    if not cfg["paired"]:
        want.add("adjacent")
    assert want <= seen, want - seen


def test_md_needs_the_real_alignments(fixture):
    fx = fixture
    r = fx["run"](False, fx["tmp"] / "reads.fastq", "bad", DRM_SAM_MD="1")
    assert r.returncode == 1 and r.stderr.startswith("Error:") and "DRM_SAM_CIGAR" in r.stderr, r.stdout + r.stderr
    assert "Search" not in r.stdout and "Index loaded" not in r.stdout
    assert not os.path.exists(fx["tmp"] / "bad" / "results.sam")


def _columns(lines):
    return [x.split("\t") for x in lines if not x.startswith("@")]


def _check_qual(fields, read, qual):
    """Column 11 is the read's quality line, reversed where SEQ is the read's reverse complement; True when reversed."""
    seq, q = fields[9].encode(), qual.decode()
    assert q != q[::-1]
    if R.revcomp(read) == read:  # a read of N: either
        assert seq == read and fields[10] in (q, q[::-1])
        return False
    assert seq in (read, R.revcomp(read))
    assert fields[10] == (q if seq == read else q[::-1]), fields
    return seq != read


def test_qual_column_single_reads(fixture):
    fx = fixture
    tmp = fx["tmp"]
    out = {}
    for tag, extra in (("on", dict(DRM_SAM_QUAL="1")), ("off", {})):
        r = fx["run"](False, tmp / "reads.fastq", "qual-" + tag, DRM_SAM_CIGAR="1", **extra)
        assert r.returncode == 0, r.stdout + r.stderr
        out[tag] = _columns(_sam(tmp / ("qual-" + tag) / "results.sam"))
    assert len(out["on"]) == len(out["off"]) and {f[10] for f in out["off"]} == {"*"}
    flags = set()
    for on, off in zip(out["on"], out["off"]):
        assert on[:10] + on[11:] == off[:10] + off[11:]
        i = int(on[0][4:])
        flags.add(_check_qual(on, fx["reads"][i], _qual(i, REF_LEN)))
    assert flags == {False, True}
    # the reference's own SAM (no DRM_SAM_CIGAR) prints SEQ as read under every flag: so is the quality line
    r = fx["run"](False, tmp / "reads.fastq", "qual-ref", DRM_SAM_QUAL="1")
    assert r.returncode == 0, r.stdout + r.stderr
    for f in _columns(_sam(tmp / "qual-ref" / "results.sam")):
        assert f[10] == _qual(int(f[0][4:]), REF_LEN).decode() and f[9] == fx["reads"][int(f[0][4:])].decode()
    # .txt queries hold no quality line
    (tmp / "reads.txt").write_bytes(b"\n".join(fx["reads"][:3]) + b"\n")
    r = fx["run"](False, tmp / "reads.txt", "qual-txt", DRM_SAM_CIGAR="1", DRM_SAM_QUAL="1")
    assert r.returncode == 0, r.stdout + r.stderr
    assert {f[10] for f in _columns(_sam(tmp / "qual-txt" / "results.sam"))} == {"*"}


def test_qual_column_pairs_and_a_line_of_the_wrong_length(fixture):
    fx = fixture
    tmp = fx["tmp"]
    more = dict(DRM_SAM_CIGAR="1", DRM_MATES=str(tmp / "m2.fastq"), DRM_PAIR_RESCUE="1", DRM_SAM_MD="1")
    out = {}
    for tag, extra in (("on", dict(DRM_SAM_QUAL="1")), ("off", {})):
        r = fx["run"](False, tmp / "m1.fastq", "pqual-" + tag, **more, **extra)
        assert r.returncode == 0, r.stdout + r.stderr
        out[tag] = _columns(_sam(tmp / ("pqual-" + tag) / "results.sam"))
    assert len(out["on"]) == len(out["off"]) == 2 * len(fx["pnames"]) and {f[10] for f in out["off"]} == {"*"}
    reversed_lines = 0
    for x, (on, off) in enumerate(zip(out["on"], out["off"])):
        assert on[:10] + on[11:] == off[:10] + off[11:]
        p, mate = divmod(x, 2)
        reversed_lines += _check_qual(on, (fx["m1"], fx["m2"])[mate][p], _qual(p + 100 * mate, REF_LEN))
    assert reversed_lines >= 3
    # a quality line one character short, in the mates' file and in the reads' file
    quals = [_qual(i, REF_LEN) for i in range(len(fx["m2"]))]
    quals[2] = quals[2][:-1]
    _fastq(tmp / "short2.fastq", [n + "/2" for n in fx["pnames"]], fx["m2"], quals)
    _fastq(tmp / "short1.fastq", [n + "/1" for n in fx["pnames"]], fx["m1"], quals)
    for query, mates in ((tmp / "m1.fastq", tmp / "short2.fastq"), (tmp / "short1.fastq", tmp / "m2.fastq")):
        r = fx["run"](False, query, "qbad", DRM_SAM_CIGAR="1", DRM_MATES=str(mates), DRM_SAM_QUAL="1")
        assert r.returncode == 1 and r.stderr.startswith("Error:") and "pair2" in r.stderr, r.stdout + r.stderr
        assert "149 quality characters" in r.stderr and "Search" not in r.stdout
        r = fx["run"](False, query, "qok", DRM_SAM_CIGAR="1", DRM_MATES=str(mates))  # unread without the switch
        assert r.returncode == 0, r.stdout + r.stderr
