"""GPU tests of bin/pipeline's SAM under the independent auditor (tests/sam_audit.py), every switch on together: three
contigs (an in-contig repeat, and the second contig's last window repeated as the third's first), some forty pairs
and the same reads as single reads, each with a truth record -- exact reads on both strands, reads at a contig's first
and last base, substitutions at base 2 and base 149, an indel each way, both copies of the repeats, all-N and random
reads, every pair shape (proper at several lengths, the TLEN tie, a contained mate, same-strand, RF, two contigs, one or
both mates unmappable, a mate only the rescue places) and the duplicate shapes (another name, the mates swapped, a
clipped 5' end, the all-N pair). The files of six runs are audited line by line against the FASTA and the FASTQ alone,
or compared byte for byte with an audited one; the files test_gpu_mapq_cli.py writes without contigs are audited too."""
import os
import subprocess

import numpy as np
import pytest

import sam_audit as A
from test_gpu_mapq_cli import _paired, _single, fixture as mapq_fixture  # noqa: F401
from test_gpu_rescue_cli import mutate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LEN = 150
ROWS = 8  # rows per read
FLANK = 16
CLIP = 5
AFFINE = (1, 4, 6, 1)
LEGACY = (1, 1, 0, 1)  # drm_sw_align's scoring, the reference's
WINDOW = (150, 500)
DROP = ("DRM_CONTIGS", "DRM_MATES", "DRM_PAIR_TLEN", "DRM_PAIR_PENALTY", "DRM_PAIR_RESCUE", "DRM_SAM_CIGAR",
        "DRM_SAM_SCORING", "DRM_SAM_FLANK", "DRM_SAM_BLOCK", "DRM_SAM_MAPQ", "DRM_SAM_L2_ROWS", "DRM_DEVICES", "DRM_MAPQ_SPAN",
        "DRM_MAPQ_MIN", "DRM_PAIR_RESCUE_MIN", "DRM_PAIR_TLEN_SAMPLE", "DRM_PAIR_TLEN_MAPQ", "DRM_SAM_MD", "DRM_SAM_QUAL",
        "DRM_SAM_CLIP", "DRM_SAM_LOCI", "DRM_SAM_XA", "DRM_LOCI_DROP", "DRM_SAM_DUP", "DRM_SAM_STATS")
OTHER = dict(zip(b"ACGT", b"CGTA"))
BASE = dict(DRM_CONTIGS="1", DRM_SAM_CIGAR="1", DRM_SAM_MAPQ="1", DRM_SAM_MD="1", DRM_SAM_QUAL="1", DRM_SAM_LOCI="5",
            DRM_SAM_DUP="1")
FULL = dict(BASE, DRM_SAM_XA="1", DRM_SAM_SCORING="1,4,6,1", DRM_SAM_FLANK=str(FLANK), DRM_SAM_CLIP=str(CLIP))
PAIRED = dict(DRM_PAIR_TLEN=f"{WINDOW[0]},{WINDOW[1]}", DRM_PAIR_PENALTY="17")


def _sub(read, offsets):
    s = bytearray(read)
    for o in offsets:
        s[o] = OTHER[s[o]]
    return bytes(s)


class Reads:
    """The read classes over the three contigs. A mate is (bases as the FASTQ holds them, truth(flank) -> A.Truth)."""

    def __init__(self, contigs, rng):
        self.contigs, self.rng = contigs, rng

    def mate(self, contig, start0, reverse, subs=(), deletion=0, insertion=0, places=None, mapq=None, lenient=False,
             damage=False):
        """The read of 150 bases whose first forward-strand base is contig[start0]; subs are offsets in the read as
        sequenced; an indel sits at the fragment's 75th base."""
        c = self.contigs[contig]
        frag = c[start0:start0 + REF_LEN + deletion - insertion]
        if deletion:
            frag = frag[:75] + frag[75 + deletion:]
        if insertion:
            extra = bytes(OTHER[x] for x in frag[75:75 + insertion])  # no inserted base repeats the base it precedes
            frag = frag[:75] + extra + frag[75:]
        assert len(frag) == REF_LEN and start0 >= 0, (contig, start0)
        read = _sub(A.revcomp(frag) if reverse else frag, subs)
        if damage:
            read = mutate(read, 3)

        def truth(flank):
            sim = None
            if deletion or insertion:
                # without a flank the region is the 150-base window (drm_sw_align), which cannot hold the 150 + deletion
                # reference bases of a read with a deletion: the best alignment inside it leaves `deletion` bases clipped
                lost = deletion if flank < deletion else 0
                sim = (REF_LEN - insertion - lost, 0, (deletion or insertion,))
            return A.Truth("lenient" if lenient else "map", contig, reverse, None if sim else start0 + 1, sim, places, mapq)
        return read, truth

    def unmappable(self, kind):
        read = b"N" * REF_LEN if kind == "n" else bytes(self.rng.choice(list(b"ACGT"), size=REF_LEN).astype(np.uint8))
        return read, lambda flank: A.Truth("unmapped" if kind == "n" else "chance")


def _pairs(R):
    """[(name, mate 1, mate 2)]. chrA[100:260] is repeated at chrA[1040:1200], chrB's last window is chrC's first."""
    f = lambda c, p, **kw: R.mate(c, p, False, **kw)  # noqa: E731
    r = lambda c, p, **kw: R.mate(c, p, True, **kw)  # noqa: E731
    n, rnd = (lambda: R.unmappable("n")), (lambda: R.unmappable("random"))
    rep = [("chrA", 106), ("chrA", 1046)]
    seam = [("chrB", 451), ("chrC", 1)]
    first = (f("chrA", 300, mapq=60), r("chrA", 450, mapq=60))
    pairs = [
        ("fr300", *first),
        ("fr400", f("chrA", 320, mapq=60), r("chrA", 570, mapq=60)),
        ("fr480", f("chrA", 500, mapq=60), r("chrA", 830, mapq=60)),
        ("tie", f("chrA", 700), r("chrA", 700)),
        ("contained", f("chrA", 860, deletion=3), r("chrA", 861)),
        ("same_strand", f("chrA", 310), f("chrA", 620)),
        ("rf", r("chrA", 330), f("chrA", 640)),
        ("two_contigs", f("chrA", 420, mapq=60), r("chrB", 200, mapq=60)),
        ("one_n", f("chrA", 650, mapq=60), n()),
        ("both_n", n(), n()),
        ("rescue", f("chrA", 335), r("chrA", 535, lenient=True, damage=True)),
        ("fr300_again", *first),
        ("fr300_swapped", first[1], first[0]),
        ("fr300_sub2", f("chrA", 300, subs=[1]), first[1]),
        ("both_n_again", n(), n()),
        ("sub2_sub149", f("chrA", 340, subs=[1]), r("chrA", 510, subs=[148])),
        ("sub149_sub2", f("chrB", 20, subs=[148]), r("chrB", 190, subs=[1])),
        ("subs_ins", f("chrB", 40, subs=[60, 90]), r("chrB", 260, insertion=2)),
        ("repeat_1", f("chrA", 105, places=rep, mapq=0), n()),
        ("repeat_2", n(), r("chrA", 1045, places=rep, mapq=0)),
        ("seam", f("chrB", 450, places=seam, mapq=0), n()),
        ("first_base", f("chrB", 0), r("chrB", 230)),
        ("last_base", f("chrC", 160), r("chrC", 300)),
        ("random", rnd(), rnd()),
        ("ten_subs", f("chrA", 560), r("chrA", 800, subs=range(7, REF_LEN, 15))),
        ("one_n_again", f("chrA", 650), n()),
    ]
    # more proper pairs over all three contigs, away from the repeats
    for x, (c, p, t) in enumerate((("chrA", 270, 300), ("chrA", 380, 450), ("chrA", 610, 410), ("chrA", 745, 280),
                                   ("chrB", 60, 330), ("chrB", 110, 340), ("chrC", 155, 290), ("chrC", 170, 275),
                                   ("chrA", 480, 500), ("chrA", 290, 150 + 37), ("chrB", 5, 440), ("chrA", 590, 365))):
        pairs.append((f"more{x}", f(c, p), r(c, p + t - REF_LEN)))
    return pairs


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    from deepreadmapper_amd import extract_fasta_sequence, fasta_contigs
    tmp = tmp_path_factory.mktemp("sam_audit_cli")
    env = dict(os.environ, DRM_BUILD_THREADS="1")
    for v in DROP:
        env.pop(v, None)
    rng = np.random.default_rng(1907)
    rand = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))  # noqa: E731
    a, b, c = bytearray(rand(1300)), rand(600), bytearray(rand(450))
    a[1040:1200] = a[100:260]  # far enough from the contig's end to keep its flank
    c[:REF_LEN] = b[-REF_LEN:]  # the seam: chrB's last window is chrC's first
    a, c = bytes(a), bytes(c)
    fa = tmp / "three.fa"
    fa.write_bytes(b">chrA\n" + a[:480] + b"\n" + a[480:] + b"\n>chrB\n" + b + b"\n>chrC\n" + c[:70] + b"\n" + c[70:] + b"\n")
    contigs = A.read_fasta(fa)
    # the headers are plain: the auditor's parser and the package's agree
    names, starts, lens = fasta_contigs(str(fa))
    genome = extract_fasta_sequence(str(fa))
    assert list(contigs) == list(names) == ["chrA", "chrB", "chrC"] and [len(s) for s in contigs.values()] == list(lens)
    assert contigs == {"chrA": a, "chrB": b, "chrC": c}
    assert all(genome[int(s):int(s) + int(n)] == contigs[k] for k, s, n in zip(names, starts, lens))

    def tool(*args, **more):
        return subprocess.run([os.path.join(ROOT, "bin", args[0]), *map(str, args[1:])], cwd=tmp, env=dict(env, **more),
                              capture_output=True, text=True)
    r = tool("hnswpq_index", fa, "ix", REF_LEN, DRM_CONTIGS="1")
    assert r.returncode == 0, r.stderr
    pairs = _pairs(Reads(contigs, rng))

    def fastq(path, names, reads):
        with open(path, "wb") as f:
            for name, read in zip(names, reads):
                q = bytes(rng.integers(35, 74, size=len(read)).astype(np.uint8))  # random Phred characters
                assert q != q[::-1]  # no palindrome: an unreversed quality line cannot pass for a reversed one
                f.write(b"@" + name.encode() + b"\n" + read + b"\n+\n" + q + b"\n")
    fastq(tmp / "m1.fastq", [n + "/1" for n, _, _ in pairs], [m[0] for _, m, _ in pairs])
    fastq(tmp / "m2.fastq", [n + "/2" for n, _, _ in pairs], [m[0] for _, _, m in pairs])
    fastq(tmp / "single.fastq", [f"{n}_{x}" for n, _, _ in pairs for x in (1, 2)], [m[0] for _, m1, m2 in pairs for m in (m1, m2)])
    single = A.templates_of(A.read_fastq(tmp / "single.fastq"))
    paired = A.templates_of(A.read_fastq(tmp / "m1.fastq"), A.read_fastq(tmp / "m2.fastq"))
    assert [n for n, _ in paired] == [n for n, _, _ in pairs] and len(single) == 2 * len(paired)

    def truth(is_paired, flank):
        out = {}
        for t, (_, m1, m2) in enumerate(pairs):
            for m, mate in enumerate((m1, m2)):
                out[(t, m) if is_paired else (2 * t + m, 0)] = mate[1](flank)
        return out

    def run(name, is_paired, **more):
        if is_paired:
            more = dict(more, DRM_MATES=str(tmp / "m2.fastq"))
        r = tool("pipeline", "ix", tmp / ("m1.fastq" if is_paired else "single.fastq"), fa, 128, ROWS, ROWS, name, 1, 1, **more)
        assert r.returncode == 0, r.stdout + r.stderr
        got = open(tmp / name / "results.sam").read().split("\n")
        assert got[-1] == ""
        return got[:-1]
    return dict(tmp=tmp, run=run, contigs=contigs, single=single, paired=paired, truth=truth, pairs=pairs, cache={})


def _file(fx, name):
    """The lines of one of the runs, made once."""
    runs = {"run1": (False, BASE), "run2": (False, FULL), "run3": (True, dict(FULL, DRM_PAIR_RESCUE="1", **PAIRED)),
            "run4": (True, dict(BASE, **PAIRED)), "run5": (True, dict(FULL, DRM_PAIR_RESCUE="1", DRM_SAM_BLOCK="4", **PAIRED)),
            "run6": (True, {k: v for k, v in dict(FULL, DRM_PAIR_RESCUE="1", **PAIRED).items() if k != "DRM_SAM_DUP"})}
    if name not in fx["cache"]:
        fx["cache"][name] = fx["run"](name, runs[name][0], **runs[name][1])
    return fx["cache"][name]


def _options(name):
    full = name in ("run2", "run3")
    is_paired = name in ("run3", "run4")
    return A.Options(scoring=AFFINE if full else LEGACY, clip=CLIP if full else 0, flank=FLANK if full else 0, md=True,
                     qual=True, mapq=True, xa=full or is_paired, paired=is_paired, dup=True, tlen=WINDOW if is_paired else None)


def _body(lines):
    return [x.split("\t") for x in lines if not x.startswith("@")]


def _audited(fx, name):
    lines, opt = _file(fx, name), _options(name)
    found = A.audit(lines, fx["contigs"], fx["paired" if opt.paired else "single"], opt, fx["truth"](opt.paired, opt.flank))
    assert not found, f"{name}: {len(found)} findings\n" + A.report(found)
    body = _body(lines)
    # so that a file that says nothing cannot pass: every must-map read is mapped, and the kinds of line are there
    truth = fx["truth"](opt.paired, opt.flank)
    primaries = [f for f in body if not int(f[1]) & 256]
    assert len(primaries) == len(truth)
    for key, f in zip(sorted(truth), primaries):
        assert truth[key].kind != "map" or not int(f[1]) & 4, f
    flags = [int(f[1]) for f in body]
    mapq = [int(f[4]) for f in body if not int(f[1]) & (4 | 256)]
    assert any(x & 16 and not x & 4 for x in flags) and any(x & 1024 for x in flags)
    assert 0 in mapq and 60 in mapq and any(0 < q < 60 for q in mapq), sorted(set(mapq))
    return body


def _lines_of(body, name):
    return [f for f in body if f[0].split("/")[0] == name]


def test_single_reads_with_the_references_scoring(fixture):
    body = _audited(fixture, "run1")
    assert any(int(f[1]) & 256 for f in body), "no secondary line"
    assert not any(t.startswith("XA:Z:") for f in body for t in f[11:])
    # a substitution at base 2 or base 149: a purely local alignment clips it
    for name in ("sub2_sub149_1", "sub2_sub149_2", "sub149_sub2_1", "sub149_sub2_2"):
        (f,) = [x for x in _lines_of(body, name) if not int(x[1]) & 256]
        assert f[5] in ("2S148M", "148M2S") and f[12] == "NM:i:0", f


def test_single_reads_with_every_switch_on(fixture):
    body = _audited(fixture, "run2")
    assert any(t.startswith("XA:Z:") for f in body for t in f[11:]), "no XA entry"
    assert not any(int(f[1]) & 256 for f in body)
    # the clipping penalty aligns what run 1 clips
    for name in ("sub2_sub149_1", "sub2_sub149_2", "sub149_sub2_1", "sub149_sub2_2"):
        (f,) = _lines_of(body, name)
        assert (f[5], f[12]) == ("150M", "NM:i:1"), f
    assert {int(f[1]) & 16 for name in ("sub2_sub149_1", "sub2_sub149_2") for f in _lines_of(body, name)} == {0, 16}


def test_pairs_with_every_switch_on_and_the_rescue(fixture):
    fx = fixture
    body = _audited(fx, "run3")
    assert any(t.startswith("XA:Z:") for f in body for t in f[11:]), "no XA entry"
    assert any(f[6] not in ("=", "*") for f in body), "no pair on two contigs"
    rescued = _lines_of(body, "rescue")[1]
    assert int(rescued[1]) & 0x2 and not int(rescued[1]) & 0x4, ("the rescue placed no mate", rescued)
    for name in ("sub2_sub149", "sub149_sub2"):
        assert [(f[5], f[12]) for f in _lines_of(body, name)] == [("150M", "NM:i:1")] * 2
    marked = {f[0] for f in body if int(f[1]) & 1024}
    assert marked == {"fr300_again", "fr300_swapped", "fr300_sub2", "one_n_again"}
    # run 5: the file does not depend on the block size; run 6: without DRM_SAM_DUP it is this file with 1024 cleared
    assert _file(fx, "run5") == _file(fx, "run3")
    cleared = ["\t".join([f[0], str(int(f[1]) & ~1024)] + f[2:]) for f in body]
    assert [x for x in _file(fx, "run6") if not x.startswith("@")] == cleared
    assert [x for x in _file(fx, "run6") if x.startswith("@")] == [x for x in _file(fx, "run3") if x.startswith("@")]


def test_pairs_with_the_references_scoring_and_no_rescue(fixture):
    body = _audited(fixture, "run4")
    assert any(f[6] not in ("=", "*") for f in body), "no pair on two contigs"
    f = _lines_of(body, "fr300_sub2")[0]
    assert f[5] == "2S148M" and int(f[1]) & 1024, f  # another POS than fr300's, the same unclipped 5' end


def test_the_files_without_contigs_pass_the_audit(mapq_fixture):  # noqa: F811
    """test_gpu_mapq_cli's genome, index and reads with DRM_SAM_CIGAR=1 alone: RNAME ref, the reference's @SQ line, a
    line per rerank row (single reads) and the pair fields over one sequence."""
    fx = mapq_fixture
    contigs = {"ref": fx["g"]}
    reads = [(n, r, b"I" * len(r)) for n, r in zip([n for n in fx["names"] for _ in range(2)], fx["reads"])]
    for is_paired in (False, True):
        lines = _paired(fx, "audit_paired") if is_paired else _single(fx, "audit_single")
        templates = A.templates_of(reads[0::2], reads[1::2]) if is_paired else A.templates_of(reads)
        opt = A.Options(scoring=LEGACY, paired=is_paired, reference_header=True, per_row=not is_paired,
                        tlen=(0, 1000) if is_paired else None)
        found = A.audit(lines, contigs, templates, opt)
        assert not found, f"paired {is_paired}: {len(found)} findings\n" + A.report(found)
        body = _body(lines)
        assert len(body) >= len(reads) and sum(not int(f[1]) & 4 for f in body) >= len(reads) // 2
        assert any(int(f[1]) & 16 for f in body) and (is_paired or any(int(f[1]) & 256 for f in body))
