"""GPU tests of bin/pipeline's DRM_SAM_SORT=coordinate on the fixtures of test_gpu_dup_cli.py (repeated pairs, hence equal
keys; all-N reads; pairs with one unmappable mate; reads with two loci), of test_gpu_loci_contigs_cli.py (four contigs)
and of test_gpu_sam_audit_cli.py (three contigs, every switch): the file equals, byte for byte, the unsorted run's file
with @HD replaced and the body put through Python's stable sorted() under (RNAME == "*", index of RNAME among the @SQ
lines, POS, flag & 16); the fixtures do not let that pass vacuously; the file does not depend on DRM_SAM_BLOCK; unsorted
and the unset variable give the file of before; the sorted body, put back into the unsorted order under the old @HD,
passes the independent auditor; bad values and the switch without its companions end the run before the index is
loaded."""
import os

import pytest

import sam_audit as A
from test_gpu_dup_cli import _run, dups  # noqa: F401
from test_gpu_loci_cli import LOCI
from test_gpu_loci_contigs_cli import _sam as _sam_file, fixture as contigs  # noqa: F401
from test_gpu_mapq_cli import fixture  # noqa: F401  (what `dups` is built on)
from test_gpu_sam_audit_cli import BASE, FULL, PAIRED, _options, fixture as audited  # noqa: F401

pytestmark = pytest.mark.gpu

ON = dict(DRM_SAM_DUP="1", DRM_SAM_MAPQ="1", DRM_SAM_MD="1", DRM_SAM_QUAL="1")
SORT = dict(DRM_SAM_SORT="coordinate")
HD = "@HD\tVN:1.0\tSO:unsorted"


def _split(lines):
    head = [x for x in lines if x.startswith("@")]
    assert lines[:len(head)] == head and head[0].startswith("@HD") and all(x.startswith("@SQ") for x in head[1:])
    return head, lines[len(head):]


def _key(head):
    names = [x.split("\t")[1][3:] for x in head[1:]]

    def key(line):
        f = line.split("\t")
        return (f[2] == "*", 0 if f[2] == "*" else names.index(f[2]), int(f[3]), int(f[1]) & 16)
    return key


def _by_python(lines):
    """The unsorted file as DRM_SAM_SORT=coordinate is defined to write it."""
    head, body = _split(lines)
    assert head[0] == HD
    return ["@HD\tVN:1.0\tSO:coordinate"] + head[1:] + sorted(body, key=_key(head))


def _restored(unsorted, got):
    """The sorted file's body put back into the unsorted file's line order, under the old @HD."""
    head, body = _split(unsorted)
    key = _key(head)
    order = sorted(range(len(body)), key=lambda i: key(body[i]))
    ghead, gbody = _split(got)
    assert len(gbody) == len(body) and ghead[1:] == head[1:]
    back = [None] * len(body)
    for place, i in enumerate(order):
        back[i] = gbody[place]
    return [HD] + head[1:] + back


def _not_vacuous(lines, mate_position):
    head, body = _split(lines)
    key = _key(head)
    keys = [key(x) for x in body]
    assert keys != sorted(keys), "the unsorted body is in coordinate order already"
    assert len(set(keys)) < len(keys), "no two lines share a key"
    assert any(x.split("\t")[2] == "*" for x in body), "no line without RNAME"
    if mate_position:
        assert any(int(f[1]) & 4 and f[2] != "*" and int(f[3]) > 0 for f in (x.split("\t") for x in body)), \
            "no unmapped line carries its mate's position"


@pytest.mark.parametrize("rescue", [False, True])
def test_paired_file_is_the_unsorted_file_sorted(dups, rescue):  # noqa: F811
    fx = dups
    more = dict(ON, DRM_PAIR_RESCUE="1") if rescue else dict(ON)
    name = "sort_paired_rescue" if rescue else "sort_paired"
    unsorted = _run(fx, name + "_off", True, **more)
    _not_vacuous(unsorted, mate_position=True)
    want = _by_python(unsorted)
    got = _run(fx, name, True, **more, **SORT)
    assert got == want
    assert _restored(unsorted, got) == unsorted
    assert any(int(x.split("\t")[1]) & 1024 for x in got[2:])  # the marks travel with their lines
    if not rescue:
        for block in ("3", "1000"):
            assert _run(fx, name + "_b" + block, True, DRM_SAM_BLOCK=block, **more, **SORT) == want
        assert _run(fx, name + "_unsorted", True, DRM_SAM_SORT="unsorted", **more) == unsorted


@pytest.mark.parametrize("xa", [False, True])
def test_single_read_file_under_loci_is_the_unsorted_file_sorted(dups, xa):  # noqa: F811
    fx = dups
    more = dict(ON, **LOCI, **(dict(DRM_SAM_XA="1") if xa else {}))
    name = "sort_single_xa" if xa else "sort_single"
    unsorted = _run(fx, name + "_off", False, **more)
    _not_vacuous(unsorted, mate_position=False)
    if not xa:
        assert any(int(x.split("\t")[1]) & 256 for x in unsorted[2:]), "no secondary line"
    want = _by_python(unsorted)
    got = _run(fx, name, False, **more, **SORT)
    assert got == want
    if not xa:
        for block in ("3", "1000"):
            assert _run(fx, name + "_b" + block, False, DRM_SAM_BLOCK=block, **more, **SORT) == want
        assert _run(fx, name + "_unsorted", False, DRM_SAM_SORT="unsorted", **more) == unsorted


def test_contig_file_is_the_unsorted_file_sorted_and_the_times_are_printed(contigs):  # noqa: F811
    fx = contigs
    more = dict(ON, DRM_CONTIGS="1", DRM_SAM_CIGAR="1", DRM_SAM_LOCI="5", DRM_MAPQ_SPAN="200")
    out = {}
    for name, extra in (("sort_off", {}), ("sort_on", dict(SORT, DRM_SAM_STATS="1")), ("sort_b4", dict(SORT, DRM_SAM_BLOCK="4"))):
        r = fx["run"]("ix", fx["tmp"] / "reads.fastq", fx["fa"], name, ["1", "1"], **more, **extra)
        assert r.returncode == 0, r.stdout + r.stderr
        out[name] = _sam_file(fx["tmp"] / name / "results.sam")
        if name == "sort_on":
            assert "[MAIN] SAM sort: " in r.stdout and "ms for the final write" in r.stdout, r.stdout
    unsorted = out["sort_off"]
    head, body = _split(unsorted)
    assert [x.split("\t")[1] for x in head[1:]] == ["SN:chrA", "SN:chrB", "SN:chrC", "SN:chrD"]
    key = _key(head)
    keys = [key(x) for x in body]
    assert keys != sorted(keys) and any(k[0] for k in keys)
    assert len({k[1] for k in keys if not k[0]}) >= 2, "lines on fewer than two contigs"
    on_first = [k[2] for k in keys if not k[0] and k[1] == 0]
    assert keys[0][0] or keys[0][1] != 0 or keys[0][2] != min(on_first), "the first line is the sorted file's first already"
    assert out["sort_on"] == _by_python(unsorted) == out["sort_b4"]
    # the sorted body by itself: contigs in @SQ order, positions ascending inside each, the lines without RNAME last
    got = [key(x) for x in _split(out["sort_on"])[1]]
    assert got == sorted(got) and got[-1][0] and not got[0][0]


@pytest.mark.parametrize("run", ["run1", "run3"])
def test_sorted_body_in_the_old_order_passes_the_auditor(audited, run):  # noqa: F811
    """run1: single reads, a line per locus; run3: pairs with every switch on and the rescue (test_gpu_sam_audit_cli)."""
    fx = audited
    paired = run == "run3"
    env = dict(FULL, DRM_PAIR_RESCUE="1", **PAIRED) if paired else dict(BASE)
    unsorted = fx["run"]("sort_" + run + "_off", paired, **env)
    got = fx["run"]("sort_" + run, paired, **env, **SORT)
    assert got == _by_python(unsorted)
    _not_vacuous(unsorted, mate_position=paired)
    back = _restored(unsorted, got)
    assert back == unsorted
    opt = _options(run)
    found = A.audit(back, fx["contigs"], fx["paired" if paired else "single"], opt, fx["truth"](paired, opt.flank))
    assert not found, f"{run}: {len(found)} findings\n" + A.report(found)


def test_bad_values_end_the_run_before_the_index_is_loaded(dups):  # noqa: F811
    fx = dups
    m2 = str(fx["tmp"] / "dup_m2.fastq")
    good = dict(DRM_SAM_CIGAR="1", DRM_MATES=m2)
    cases = [(dict(good, DRM_SAM_SORT=""), ["1", "1"]),
             (dict(good, DRM_SAM_SORT="queryname"), ["1", "1"]),
             (dict(good, DRM_SAM_SORT="1"), ["1", "1"]),
             (dict(good, DRM_SAM_SORT="Coordinate"), ["1", "1"]),
             (dict(DRM_SAM_SORT="coordinate"), ["1", "1"]),               # without DRM_SAM_CIGAR=1
             (dict(DRM_SAM_SORT="coordinate", DRM_SAM_CIGAR="1"), ["1", "0"]),  # not streaming
             (dict(DRM_SAM_SORT="coordinate", DRM_SAM_CIGAR="1"), ["0", "1"])]  # not dynamic
    for more, extra in cases:
        paired = "DRM_MATES" in more
        r = fx["run"](fx["tmp"] / ("dup_m1.fastq" if paired else "dup_inter.fastq"), "sort_bad", extra, **more)
        assert r.returncode == 1 and r.stderr.startswith("Error:") and "DRM_SAM_SORT" in r.stderr, (more, r.stderr)
        assert "Index loaded" not in r.stdout and not os.path.exists(fx["tmp"] / "sort_bad" / "results.sam"), more
