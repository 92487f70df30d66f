"""GPU tests of DRM_SAM_CLIP through bin/pipeline: small FASTA and FASTQ fixtures (those of test_gpu_md_cli.py in kind)
are indexed by bin/hnswpq_index and mapped single, paired, paired with rescue, with DRM_CONTIGS, and with DRM_SAM_LOCI
with and without DRM_SAM_XA. With DRM_SAM_CLIP=5 every mapped line's POS, CIGAR, AS, NM and MD are what the restatement
of drm_sw_align_affine_clip (tests/sw_align_clip_ref.py) gives over the line's region, reads with a substitution at an
end print 150M where the run without the variable prints a soft clip, lines whose restatement does not change are the
same bytes in both files, DRM_SAM_CLIP=0 is the unset variable, the file does not depend on DRM_SAM_BLOCK, and a
malformed value ends the run before the index is loaded."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import md_ref as MD
import sw_align_affine_ref as A
import sw_align_clip_ref as K
import sw_align_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LEN = 150
ROWS = 8  # rows per read
FLANK = 16
SCORING = (1, 4, 6, 1)
DROP = ("DRM_CONTIGS", "DRM_MATES", "DRM_PAIR_TLEN", "DRM_PAIR_PENALTY", "DRM_PAIR_RESCUE", "DRM_SAM_CIGAR",
        "DRM_SAM_SCORING", "DRM_SAM_FLANK", "DRM_SAM_BLOCK", "DRM_SAM_MAPQ", "DRM_SAM_L2_ROWS", "DRM_DEVICES", "DRM_MAPQ_SPAN",
        "DRM_MAPQ_MIN", "DRM_PAIR_RESCUE_MIN", "DRM_PAIR_TLEN_SAMPLE", "DRM_PAIR_TLEN_MAPQ", "DRM_SAM_MD", "DRM_SAM_QUAL",
        "DRM_SAM_CLIP", "DRM_SAM_LOCI", "DRM_SAM_XA", "DRM_LOCI_DROP")
AFFINE = dict(DRM_SAM_CIGAR="1", DRM_SAM_FLANK=str(FLANK), DRM_SAM_SCORING="1,4,6,1", DRM_SAM_MD="1")
OTHER = {ord("A"): ord("C"), ord("C"): ord("G"), ord("G"): ord("T"), ord("T"): ord("A")}


def _fastq(path, names, reads):
    with open(path, "wb") as f:
        for n, r in zip(names, reads):
            f.write(b"@" + n.encode() + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")


def _sam(path):
    got = open(path).read().split("\n")
    assert got[-1] == ""
    return got[:-1]


def _substituted(seq, cols):
    s = bytearray(seq)
    for c in cols:
        s[c] = OTHER[s[c]]
    return bytes(s)


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    from deepreadmapper_amd import extract_fasta_sequence, fasta_contigs
    tmp = tmp_path_factory.mktemp("clip_cli")
    env = dict(os.environ, DRM_BUILD_THREADS="1")
    for v in DROP:
        env.pop(v, None)
    rng = np.random.default_rng(505)
    rand = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))  # noqa: E731
    a, b = bytearray(rand(1300)), rand(600)
    # a second locus for the reads from there, so that DRM_SAM_LOCI has something to list; it lies far enough from the
    # contig's end for the per-contig flank guard to leave its windows their flank
    a[1040:1200] = a[100:260]
    a = bytes(a)
    one, two = tmp / "one.fa", tmp / "two.fa"
    one.write_bytes(b">one\n" + a[:480] + b"\n" + a[480:] + b"\n")
    two.write_bytes(b">chrA\n" + a + b"\n>chrB\n" + b + b"\n")
    names, starts, lens = fasta_contigs(str(two))
    assert names == ["chrA", "chrB"] and list(lens) == [1300, 600] and extract_fasta_sequence(str(one)) == a
    both, starts = extract_fasta_sequence(str(two)), [int(x) for x in starts]  # the genome the window ids count in
    assert both[starts[0]:starts[0] + 1300] == a and both[starts[1]:starts[1] + 600] == b

    def tool(*args, **more):
        return subprocess.run([os.path.join(ROOT, "bin", args[0]), *map(str, args[1:])], cwd=tmp, env=dict(env, **more),
                              capture_output=True, text=True)
    for ref, name, more in ((one, "ix1", {}), (two, "ix2", dict(DRM_CONTIGS="1"))):
        r = tool("hnswpq_index", ref, name, REF_LEN, **more)
        assert r.returncode == 0, r.stderr

    def run(contigs, query, name, **more):
        if contigs:
            more = dict(more, DRM_CONTIGS="1")
        return tool("pipeline", "ix2" if contigs else "ix1", query, two if contigs else one, 128, ROWS, ROWS, name, 1, 1,
                    **more)
    # single reads: exact copies; a substitution in the last base, in the first, in column 147 and in column 2; the same
    # on the reverse strand; an indel four bases from an end; a random read and one of N
    ends = [[149], [0], [147], [2]]
    reads = [a[100:250], a[700:850]] + [_substituted(a[300 + 40 * x:450 + 40 * x], c) for x, c in enumerate(ends)] + \
        [R.revcomp(_substituted(a[520 + 30 * x:670 + 30 * x], c)) for x, c in enumerate(ends)] + \
        [a[200:204] + a[205:351], a[400:546] + b"G" + a[546:549] if a[546] != ord("G") else a[400:546] + b"T" + a[546:549],
         rand(REF_LEN), b"N" * REF_LEN, _substituted(a[100:250], [148])]  # the last one has two loci
    assert {len(r) for r in reads} == {REF_LEN}
    end_reads = list(range(2, 10)) + [14]
    _fastq(tmp / "reads.fastq", [f"read{i}" for i in range(len(reads))], reads)
    # pairs (FR): an exact pair, mate 2 with its last base changed, mate 1 with its first, both with column 147 / column 2,
    # a mate 2 that only the rescue finds (a third of its bases changed, and its last), mate 2 random, both N
    frags = [(50, 400), (300, 380), (520, 420), (130, 390), (610, 350)]
    m1 = [a[p:p + REF_LEN] for p, t in frags] + [a[20:170], b"N" * REF_LEN]
    m2 = [R.revcomp(a[p + t - REF_LEN:p + t]) for p, t in frags] + [rand(REF_LEN), b"N" * REF_LEN]
    m2[1] = _substituted(m2[1], [149])
    m1[2] = _substituted(m1[2], [0])
    m1[3], m2[3] = _substituted(m1[3], [147]), _substituted(m2[3], [2])
    m2[4] = _substituted(m2[4], list(range(1, REF_LEN - 3, 3)) + [149])
    pnames = [f"pair{i}" for i in range(len(m1))]
    _fastq(tmp / "m1.fastq", [n + "/1" for n in pnames], m1)
    _fastq(tmp / "m2.fastq", [n + "/2" for n in pnames], m2)
    return dict(tmp=tmp, run=run, refs={"ref": (a, 0, a), "chrA": (both, starts[0], a), "chrB": (both, starts[1], b)}, reads=reads,
                end_reads=end_reads, m1=m1, m2=m2, pnames=pnames)


# ------------------------------------------------------------------------------------------ the restatement of a line
@functools.lru_cache(maxsize=None)
def _restated(genome, cstart, clen, pos, rev, flank, read, L):
    """(pos1 in the contig, cigar, AS, NM, MD) of `read` against window `pos` (0-based in the genome) of one strand, by
    the restatement; None where it finds no alignment. A flanked region that leaves the contig falls back to flank 0
    (the per-contig flank guard)."""
    wid = 2 * pos + rev
    s, n, _ = A.region(genome, REF_LEN, wid, flank)
    if flank and (s < cstart or s + n > cstart + clen):
        flank = 0
        s, n, _ = A.region(genome, REF_LEN, wid, 0)
    region = A.region_bytes(genome, REF_LEN, wid, flank)
    q = b"<" + read + b">"
    rec, ops = K.align(region, q, SCORING, L) if L else A.align(region, q, SCORING)
    if rec["status"]:
        return None
    pos1, cigar = A.sam_fields_region(rec, ops, len(q), s, n, rev)
    h, words = MD.md_words(region, q, rec, ops)
    assert h["status"] == 0
    return pos1 - cstart, cigar, rec["score"], rec["nm"], MD.md_string(words, rev)


def _line_fields(f):
    tags = dict((t[:2], t[5:]) for t in f[11:])
    return int(f[3]), f[5], int(tags["AS"]), int(tags["NM"]), tags["MD"]


def _windows_of(fx, f, L, every=False):
    """The windows (position, flank tried) whose restatement at penalty L gives the mapped line f: the search starts
    where the read's first base would lie and widens, for the SAM does not name the row's window; with `every` it goes
    through all the windows whose region can hold the alignment."""
    genome, cstart, contig = fx["refs"][f[2]]
    rev = 1 if int(f[1]) & 16 else 0
    read = R.revcomp(f[9].encode()) if rev else f[9].encode()
    want = _line_fields(f)
    lead = re.match(r"(\d+)S", f[5])
    first = cstart + want[0] - 1 - (int(lead.group(1)) if lead else 0)
    found = []
    for d in range(0, REF_LEN + FLANK + 1):
        for pos in ({first - d, first + d}):
            if cstart <= pos <= cstart + len(contig) - REF_LEN and \
                    _restated(genome, cstart, len(contig), pos, rev, FLANK, read, L) == want:
                found.append(pos)
        if found and d >= 3 and not every:  # the rows of a read are neighbouring windows: a few of them say the same
            break
    return genome, cstart, len(contig), rev, read, found


def _check_files(fx, clip_lines, plain_lines, L=5):
    """Every mapped line of the DRM_SAM_CLIP file against the restatement, and against the file without the variable;
    returns the lines that differ as (clip fields, plain fields)."""
    assert len(clip_lines) == len(plain_lines)
    differ, mapped = [], 0
    for got, plain in zip(clip_lines, plain_lines):
        if got.startswith("@"):
            assert got == plain
            continue
        f, g = got.split("\t"), plain.split("\t")
        assert f[0] == g[0]
        if int(f[1]) & 4:
            assert f[5] == "*" and "AS:i" not in got
            if not int(g[1]) & 4:
                assert f[9] in (g[9], R.revcomp(g[9].encode()).decode())  # an unmapped line prints the read as it came
                # an alignment that is not worth its two ends: the restatement finds none either, over one of the
                # windows that give the line without the variable (a few matching bases: many windows do)
                genome, cstart, clen, rev, read, found = _windows_of(fx, g, 0, every=True)
                assert found, plain
                assert None in {_restated(genome, cstart, clen, pos, rev, FLANK, read, L) for pos in found}, (got, plain)
                differ.append((f, g))
            elif got != plain:  # a pair's line whose mate's line changed
                differ.append((f, g))
            continue
        assert not int(g[1]) & 4 and f[9:11] == g[9:11], (got, plain)  # worth its ends: worth something without them
        mapped += 1
        genome, cstart, clen, rev, read, found = _windows_of(fx, f, L)
        assert found, got
        # nothing but POS, CIGAR, AS, NM, MD and, on a pair's lines, what follows from the mate's line (its flag bits,
        # PNEXT, TLEN) and an XA entry may differ
        assert int(f[1]) & ~0x2A == int(g[1]) & ~0x2A and f[2] == g[2] and f[4] == g[4], (got, plain)
        unchanged = {_restated(genome, cstart, clen, pos, rev, FLANK, read, 0) == _line_fields(f) for pos in found}
        if unchanged == {True}:
            assert (f[3], f[5], f[11:14]) == (g[3], g[5], g[11:14]), (got, plain)
        elif unchanged == {False}:
            assert got != plain
        if got != plain:
            differ.append((f, g))
    assert mapped >= 8
    return differ


CONFIGS = {
    "single": dict(contigs=False, paired=False, more={}),
    "single-contigs": dict(contigs=True, paired=False, more={}),
    "paired": dict(contigs=False, paired=True, more={}),
    "paired-rescue-contigs": dict(contigs=True, paired=True, more=dict(DRM_PAIR_RESCUE="1")),
    "loci": dict(contigs=False, paired=False, more=dict(DRM_SAM_MAPQ="1", DRM_SAM_LOCI="4")),
    "loci-xa": dict(contigs=False, paired=False, more=dict(DRM_SAM_MAPQ="1", DRM_SAM_LOCI="4", DRM_SAM_XA="1")),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_clip_on_every_mapped_line(fixture, name):
    fx, cfg = fixture, CONFIGS[name]
    tmp = fx["tmp"]
    more = dict(AFFINE, **cfg["more"])
    query = tmp / "reads.fastq"
    if cfg["paired"]:
        more["DRM_MATES"] = str(tmp / "m2.fastq")
        query = tmp / "m1.fastq"
    out = {}
    for tag, extra in (("clip", dict(DRM_SAM_CLIP="5")), ("plain", {}), ("zero", dict(DRM_SAM_CLIP="0")),
                       ("clip_b3", dict(DRM_SAM_CLIP="5", DRM_SAM_BLOCK="3"))):
        r = fx["run"](cfg["contigs"], query, f"{name}-{tag}", **more, **extra)
        assert r.returncode == 0, r.stdout + r.stderr
        out[tag] = open(tmp / f"{name}-{tag}" / "results.sam").read()
    assert out["zero"] == out["plain"] and out["clip_b3"] == out["clip"]
    clip, plain = _sam(tmp / f"{name}-clip" / "results.sam"), _sam(tmp / f"{name}-plain" / "results.sam")
    differ = _check_files(fx, clip, plain)
    # the reads with a substitution at an end: a soft clip without the variable, 150M and NM 1 with it
    full = [(f, g) for f, g in differ if f[5] == "150M" and "S" in g[5] and f[12] == "NM:i:1" and f[11] == "AS:i:145"]
    if cfg["paired"]:
        assert {f[0] for f, _ in full} >= {"pair1", "pair2", "pair3"}
        assert {int(f[1]) & 0xC0 for f, _ in full} == {0x40, 0x80}
        if "DRM_PAIR_RESCUE" in cfg["more"]:  # the rescued mate's line goes through the penalty too
            assert [f for f, g in differ if f[0] == "pair4" and int(f[1]) & 0x80]
    else:
        names = {f"read{i}" for i in fx["end_reads"]}
        assert {f[0] for f, _ in full if not int(f[1]) & 256} == names
        assert {int(f[1]) & 16 for f, _ in full} == {0, 16}
        indel = [f for f, g in differ if f[0] in ("read10", "read11") and not int(f[1]) & 256]
        assert len(indel) == 2 and all(re.fullmatch(r"\d+M1[ID]\d+M", f[5]) for f in indel), indel
    if "DRM_SAM_XA" in cfg["more"]:  # the last read's second locus: its entry goes through the penalty too
        assert re.search(r"^read14\t[^\n]*\tXA:Z:ref,\+(101|1041),150M,1;$", out["clip"], re.M), clip[-3:]
        assert re.search(r"^read14\t[^\n]*\tXA:Z:ref,\+(101|1041),148M2S,0;$", out["plain"], re.M), plain[-3:]
    if cfg["contigs"]:
        assert "\tchrA\t" in out["clip"]


def test_clip_alone_turns_the_affine_mode_on(fixture):
    """DRM_SAM_CLIP=5 beside DRM_SAM_CIGAR=1 alone: the scoring 1,1,0,1 and flank 0."""
    fx = fixture
    tmp = fx["tmp"]
    r = fx["run"](False, tmp / "reads.fastq", "alone", DRM_SAM_CIGAR="1", DRM_SAM_CLIP="5")
    assert r.returncode == 0, r.stdout + r.stderr
    r = fx["run"](False, tmp / "reads.fastq", "alone-plain", DRM_SAM_CIGAR="1")
    assert r.returncode == 0, r.stdout + r.stderr
    got, plain = _sam(tmp / "alone" / "results.sam"), _sam(tmp / "alone-plain" / "results.sam")
    assert len(got) == len(plain)
    a = fx["refs"]["ref"][2]
    checked = changed = 0
    for x, y in zip(got, plain):
        f = x.split("\t")
        if x.startswith("@") or int(f[1]) & 4:
            assert x == y
            continue
        # under 1,1,0,1 a substitution at an end costs 1 aligned and 5 clipped: every row of such a read over a window
        # that holds the whole read prints 150M
        rev = 1 if int(f[1]) & 16 else 0
        read = R.revcomp(f[9].encode()) if rev else f[9].encode()
        pos1, cigar = int(f[3]), f[5]
        if cigar == "150M":
            w = a[pos1 - 1:pos1 + 149]
            rec, ops = K.align(R.revcomp(w) if rev else w, b"<" + read + b">", (1, 1, 0, 1), 5)
            assert (R.cigar_string(ops), f"AS:i:{rec['score']}", f"NM:i:{rec['nm']}") == ("150M", f[11], f[12]), x
            checked += 1
        changed += x != y
    assert checked >= 5 and changed >= 1, (checked, changed)


def test_bad_values_end_before_the_index_is_loaded_and_the_variable_needs_the_real_alignments(fixture):
    fx = fixture
    tmp = fx["tmp"]
    for bad in ("64", "-1", "x", "", "5,5", "1000000000000"):
        r = fx["run"](False, tmp / "reads.fastq", "bad", DRM_SAM_CIGAR="1", DRM_SAM_CLIP=bad)
        assert r.returncode == 1 and r.stderr.startswith("Error:") and "DRM_SAM_CLIP" in r.stderr, (bad, r.stdout, r.stderr)
        assert "Index loaded" not in r.stdout and not os.path.exists(tmp / "bad" / "results.sam")
    # without DRM_SAM_CIGAR=1 the variable is not read: the reference's own SAM, whatever it says
    r = fx["run"](False, tmp / "reads.fastq", "ref-plain")
    assert r.returncode == 0, r.stdout + r.stderr
    for value in ("5", "x"):
        r = fx["run"](False, tmp / "reads.fastq", "ref-clip", DRM_SAM_CLIP=value)
        assert r.returncode == 0, r.stdout + r.stderr
        assert open(tmp / "ref-clip" / "results.sam", "rb").read() == open(tmp / "ref-plain" / "results.sam", "rb").read()
