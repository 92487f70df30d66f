"""GPU tests of bin/pipeline's DRM_SAM_FORMAT=bam on the fixtures of test_gpu_sort_cli.py: the paired fixture with
duplicates and rescue, the single reads under DRM_SAM_LOCI with and without DRM_SAM_XA, the four-contig fixture and the
audited three-contig fixture with every switch on, each unsorted and under DRM_SAM_SORT=coordinate. results.bam, taken
apart by the independent reader and decoder of tests/bam_ref.py, equals the results.sam of the same run without the
switch, header and every line, and passes the auditor where the SAM does; the fixtures do not let that pass vacuously;
the file itself does not depend on DRM_SAM_BLOCK; no results.sam appears; sam and the unset variable give the file of
before; bad values and the switch without its companions end the run before the index is loaded."""
import os
import subprocess

import pytest

import bam_ref as B
import sam_audit as A
from test_gpu_dup_cli import _run, dups  # noqa: F401
from test_gpu_loci_cli import LOCI
from test_gpu_loci_contigs_cli import _sam as _sam_file, fixture as contigs  # noqa: F401
from test_gpu_mapq_cli import fixture  # noqa: F401  (what `dups` is built on)
from test_gpu_sam_audit_cli import BASE, DROP, FULL, PAIRED, ROOT, ROWS, _options, fixture as audited  # noqa: F401

pytestmark = pytest.mark.gpu

ON = dict(DRM_SAM_DUP="1", DRM_SAM_MAPQ="1", DRM_SAM_MD="1", DRM_SAM_QUAL="1")
SORT = dict(DRM_SAM_SORT="coordinate")
BAM = dict(DRM_SAM_FORMAT="bam")


def _decoded(folder):
    """(the SAM lines results.bam decodes to, its bytes, the BTYPE of every member); no results.sam beside it."""
    assert sorted(os.listdir(folder)) == ["results.bam"], os.listdir(folder)
    data = open(os.path.join(folder, "results.bam"), "rb").read()
    raw, btypes, sizes = B.read_bgzf(data)
    assert all(s == B.BLOCK for s in sizes[:-2]) and 0 < sizes[-2] <= B.BLOCK  # whole blocks, the remainder, EOF
    return B.decode_bam(raw), data, btypes


def _bam(fx, name, paired, **more):
    """test_gpu_dup_cli._run for a run that writes results.bam."""
    if paired:
        more = dict(DRM_MATES=str(fx["tmp"] / "dup_m2.fastq"), **more)
    r = fx["run"](fx["tmp"] / ("dup_m1.fastq" if paired else "dup_inter.fastq"), name, ["1", "1"], DRM_SAM_CIGAR="1",
                  **more, **BAM)
    assert r.returncode == 0, r.stdout + r.stderr
    return _decoded(fx["tmp"] / name)


def _audited_bam(fx, name, paired, **more):
    """The audited fixture's run (its index, reads and arguments) for a run that writes results.bam."""
    tmp = fx["tmp"]
    env = {k: v for k, v in os.environ.items() if k not in DROP and k not in ("DRM_SAM_SORT", "DRM_SAM_FORMAT")}
    env.update(DRM_BUILD_THREADS="1", **more, **BAM)
    if paired:
        env["DRM_MATES"] = str(tmp / "m2.fastq")
    r = subprocess.run([os.path.join(ROOT, "bin", "pipeline"), "ix", str(tmp / ("m1.fastq" if paired else "single.fastq")),
                        str(tmp / "three.fa"), "128", str(ROWS), str(ROWS), name, "1", "1"], cwd=tmp, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return _decoded(tmp / name)


def _fields(lines):
    return [x.split("\t") for x in lines if not x.startswith("@")]


@pytest.mark.parametrize("rescue", [False, True])
def test_paired_bam_decodes_to_the_sam(dups, rescue):  # noqa: F811
    fx = dups
    more = dict(ON, DRM_PAIR_RESCUE="1") if rescue else dict(ON)
    name = "bam_paired_rescue" if rescue else "bam_paired"
    sam = _run(fx, name + "_sam", True, **more)
    body = _fields(sam)
    assert any(int(f[1]) & 16 for f in body), "no reverse line"
    assert any(f[2] == "*" and f[5] == "*" for f in body), "no unmapped line without RNAME"
    assert any(int(f[1]) & 4 and f[2] != "*" and int(f[3]) > 0 for f in body), "no unmapped mate carrying a position"
    assert any(int(f[1]) & 1024 for f in body), "no duplicate mark"
    assert any(int(f[8]) < 0 for f in body) and any(f[6] == "=" for f in body)
    got, data, btypes = _bam(fx, name, True, **more)
    assert got == sam
    assert 1 in btypes[:-1], "no member is fixed Huffman"
    want_sorted = _run(fx, name + "_sorted_sam", True, **more, **SORT)
    got_sorted, data_sorted, _ = _bam(fx, name + "_sorted", True, **more, **SORT)
    assert got_sorted == want_sorted and got_sorted[0] == "@HD\tVN:1.0\tSO:coordinate" and got_sorted != got
    if not rescue:
        for block in ("3", "1000"):
            assert _bam(fx, name + "_b" + block, True, DRM_SAM_BLOCK=block, **more)[1] == data
            assert _bam(fx, name + "_sorted_b" + block, True, DRM_SAM_BLOCK=block, **more, **SORT)[1] == data_sorted
        assert _run(fx, name + "_format_sam", True, DRM_SAM_FORMAT="sam", **more) == sam


@pytest.mark.parametrize("xa", [False, True])
def test_single_read_bam_under_loci_decodes_to_the_sam(dups, xa):  # noqa: F811
    fx = dups
    more = dict(ON, **LOCI, **(dict(DRM_SAM_XA="1") if xa else {}))
    name = "bam_single_xa" if xa else "bam_single"
    sam = _run(fx, name + "_sam", False, **more)
    body = _fields(sam)
    if xa:
        assert any(t.startswith("XA:Z:") for f in body for t in f[11:]), "no line with XA"
    else:
        assert any(int(f[1]) & 256 for f in body), "no secondary line"
    assert any(f[2] == "*" for f in body) and any(int(f[1]) & 16 for f in body)
    got, data, btypes = _bam(fx, name, False, **more)
    assert got == sam and 1 in btypes[:-1]
    assert _bam(fx, name + "_sorted", False, **more, **SORT)[0] == _run(fx, name + "_sorted_sam", False, **more, **SORT)
    if not xa:
        for block in ("3", "1000"):
            assert _bam(fx, name + "_b" + block, False, DRM_SAM_BLOCK=block, **more)[1] == data


def test_contig_bam_decodes_to_the_sam_and_the_compression_is_reported(contigs):  # noqa: F811
    fx = contigs
    more = dict(ON, DRM_CONTIGS="1", DRM_SAM_CIGAR="1", DRM_SAM_LOCI="5", DRM_MAPQ_SPAN="200")
    out = {}
    for name, extra in (("bam_off", {}), ("bam_on", dict(BAM, DRM_SAM_STATS="1")), ("bam_b4", dict(BAM, DRM_SAM_BLOCK="4")),
                        ("bam_sort_off", SORT), ("bam_sort_on", dict(SORT, **BAM))):
        r = fx["run"]("ix", fx["tmp"] / "reads.fastq", fx["fa"], name, ["1", "1"], **more, **extra)
        assert r.returncode == 0, r.stdout + r.stderr
        if "DRM_SAM_FORMAT" in extra:
            out[name] = _decoded(fx["tmp"] / name)
        else:
            out[name] = _sam_file(fx["tmp"] / name / "results.sam")
        if name == "bam_on":
            line = [x for x in r.stdout.split("\n") if x.startswith("[MAIN] BAM compression: ")]
            assert len(line) == 1 and " bytes in, " in line[0] and " bytes out, " in line[0] and " ms in " in line[0], r.stdout
            raw = B.read_bgzf(out[name][1])[0]
            assert f" {len(raw)} bytes in, {len(out[name][1])} bytes out" in line[0], (line, len(raw))
    head = [x for x in out["bam_off"] if x.startswith("@")]
    assert [x.split("\t")[1] for x in head[1:]] == ["SN:chrA", "SN:chrB", "SN:chrC", "SN:chrD"]
    assert len({f[2] for f in _fields(out["bam_off"]) if f[2] != "*"}) >= 2, "lines on fewer than two contigs"
    assert out["bam_on"][0] == out["bam_off"] and out["bam_b4"][1] == out["bam_on"][1]
    assert out["bam_sort_on"][0] == out["bam_sort_off"] != out["bam_off"]


@pytest.mark.parametrize("run", ["run1", "run3"])
def test_audited_bam_decodes_to_the_sam_and_passes_the_auditor(audited, run):  # noqa: F811
    """run1: single reads, a line per locus; run3: pairs with every switch on and the rescue (test_gpu_sam_audit_cli)."""
    fx = audited
    paired = run == "run3"
    env = dict(FULL, DRM_PAIR_RESCUE="1", **PAIRED) if paired else dict(BASE)
    sam = fx["run"]("bam_" + run + "_sam", paired, **env)
    got, _, btypes = _audited_bam(fx, "bam_" + run, paired, **env)
    assert got == sam and 1 in btypes[:-1]
    body = _fields(sam)
    assert any(int(f[1]) & 16 for f in body) and any(f[2] == "*" for f in body)
    if paired:
        assert any(t.startswith("XA:Z:") for f in body for t in f[11:]), "no line with XA"
        assert any(int(f[1]) & 4 and f[2] != "*" and int(f[3]) > 0 for f in body), "no unmapped mate with a position"
    opt = _options(run)
    found = A.audit(got, fx["contigs"], fx["paired" if paired else "single"], opt, fx["truth"](paired, opt.flank))
    assert not found, f"{run}: {len(found)} findings\n" + A.report(found)
    assert _audited_bam(fx, "bam_" + run + "_sorted", paired, **env, **SORT)[0] == \
        fx["run"]("bam_" + run + "_sorted_sam", paired, **env, **SORT)


def test_bad_values_end_the_run_before_the_index_is_loaded(dups):  # noqa: F811
    fx = dups
    m2 = str(fx["tmp"] / "dup_m2.fastq")
    good = dict(DRM_SAM_CIGAR="1", DRM_MATES=m2)
    cases = [(dict(good, DRM_SAM_FORMAT=""), ["1", "1"]),
             (dict(good, DRM_SAM_FORMAT="cram"), ["1", "1"]),
             (dict(good, DRM_SAM_FORMAT="1"), ["1", "1"]),
             (dict(good, DRM_SAM_FORMAT="BAM"), ["1", "1"]),
             (dict(DRM_SAM_FORMAT="bam"), ["1", "1"]),                      # without DRM_SAM_CIGAR=1
             (dict(DRM_SAM_FORMAT="bam", DRM_SAM_CIGAR="1"), ["1", "0"]),   # not streaming
             (dict(DRM_SAM_FORMAT="bam", DRM_SAM_CIGAR="1"), ["0", "1"])]   # not dynamic
    for more, extra in cases:
        paired = "DRM_MATES" in more
        r = fx["run"](fx["tmp"] / ("dup_m1.fastq" if paired else "dup_inter.fastq"), "bam_bad", extra, **more)
        assert r.returncode == 1 and r.stderr.startswith("Error:") and "DRM_SAM_FORMAT" in r.stderr, (more, r.stderr)
        assert "Index loaded" not in r.stdout and not os.path.exists(fx["tmp"] / "bam_bad"), more
